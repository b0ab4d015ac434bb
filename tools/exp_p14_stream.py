#!/usr/bin/env python3
"""Kernel A/B of the p14 (14-bit packed bf16) stream GEMM against the bf16 stream GEMM, measured the way
profiles/r5_stream_gemm_vs_dma_only.jsonl was: back-to-back launches over rotating weight copies beyond the
256 MiB Infinity Cache, the first pass discarded, bf16 and p14 interleaved on one box, EPI_BF16.

    python tools/exp_p14_stream.py [--reps 3] [--out profiles/p14_stream_kernel_ab.jsonl]

One JSON line per (shape, M, kernel, repeat): us per launch, bf16-equivalent weights/s, bytes actually read.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from llm_map_reduce_summarizer_amd.ops import hip

    dev = "cuda:0"
    rows = []

    def b2b(fn, n):
        for _ in range(3):  # first pass over the copies: discarded
            fn()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(n):
            fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) * 1e-3 / n

    shapes = {"gate_up": (28672, 4096, 7), "lm_head": (128256, 4096, 4)}
    for name, (N, K, wpb) in shapes.items():
        nb = N * K * 2
        ncopy = max(3, int(1.2e9 // nb) + 1)
        ws = [(torch.randn(N, K, device=dev, dtype=torch.float32) * 0.02).to(torch.bfloat16) for _ in range(ncopy)]
        packed = []
        for w in ws:
            p, base7, bad = hip.p14_pack(w)
            assert bad == 0
            packed.append((p, base7))
        it = [0]
        stream = torch.cuda.current_stream().cuda_stream
        for M in (1, 40):
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            o = torch.empty(M, N, device=dev, dtype=torch.bfloat16)

            def run_bf16():
                it[0] += 1
                w = ws[it[0] % ncopy]
                rc = hip._fn("mrsum_stream_gemm")(x.data_ptr(), K, w.data_ptr(), N, K, M, o.data_ptr(), N, hip.EPI_BF16,
                                                  1, wpb, None, None, None, 0, 0.0, None, 0, None, 0, None, stream)
                assert rc == 0, rc

            def run_p14():
                it[0] += 1
                p, base7 = packed[it[0] % ncopy]
                rc = hip._fn("mrsum_stream_p14")(x.data_ptr(), K, p.data_ptr(), base7, N, K, M, o.data_ptr(), N,
                                                 hip.EPI_BF16, 1, wpb, None, None, None, 0, 0.0, None, 0, None, None,
                                                 stream)
                assert rc == 0, rc

            for rep in range(a.reps):
                for kind, fn, bytes_ in (("bf16", run_bf16, nb), ("p14", run_p14, nb * 7 // 8)):
                    t = b2b(fn, a.launches)
                    row = dict(op=name, N=N, K=K, wpb=wpb, M=M, kernel=kind, rep=rep, us=round(t * 1e6, 2),
                               Tweights_s=round(N * K / t / 1e12, 3), TBps=round(bytes_ / t / 1e12, 3))
                    rows.append(row)
                    print(json.dumps(row), flush=True)
            # bit identity on one copy, at the measured shape
            it[0] = 0
            run_bf16()
            ref = o.clone()
            it[0] = 0
            run_p14()
            torch.cuda.synchronize()
            print(json.dumps(dict(op=name, M=M, identical=bool(torch.equal(ref, o)))), flush=True)
        del ws, packed
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
