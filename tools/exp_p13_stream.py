#!/usr/bin/env python3
"""Kernel A/B of the p13 (13-bit packed bf16 + exception list) stream GEMM against the p14 and the bf16 stream
GEMM, measured as tools/exp_p14_stream.py does: back-to-back launches over rotating weight copies beyond the
256 MiB Infinity Cache, the first pass discarded, the forms interleaved on one box.  gate_up and the LM head run
unsplit (EPI_BF16); qkv, o and down at their decode split plans (fp32 partial slabs, 4 splits).  "p13x": the same
p13 kernel on copies with two planted exceptions each (the exception path must not show).

    python tools/exp_p13_stream.py [--reps 3] [--out profiles/p13_stream_kernel_ab.jsonl]

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

    # name: (N, K, wpb, splits)
    shapes = {"gate_up": (28672, 4096, 7, 1), "lm_head": (128256, 4096, 4, 1), "qkv": (6144, 4096, 6, 4),
              "o": (4096, 4096, 4, 4), "down": (4096, 14336, 4, 4)}
    for name, (N, K, wpb, S) in shapes.items():
        nb = N * K * 2
        ncopy = max(3, int(1.2e9 // nb) + 1)
        ws = [(torch.randn(N, K, device=dev, dtype=torch.float32) * 0.02).to(torch.bfloat16) for _ in range(ncopy)]
        p14s, p13s, p13x = [], [], []
        nex = 0
        for i, w in enumerate(ws):
            p, base7, bad = hip.p14_pack(w)
            assert bad == 0
            p14s.append((p, base7))
            t = hip.p13_pack(w)
            assert t[5] <= hip.P13_EXCAP
            nex += t[4]
            p13s.append(t)
            if name == "gate_up":
                wx = w.clone()
                wx[(977 * i + 5) % N, 300] = 1e-30
                wx[(977 * i + 5) % N, K - 3] = -1e-30
                t = hip.p13_pack(wx)
                assert t[5] <= hip.P13_EXCAP and t[4] >= 2
                p13x.append(t)
                del wx
        print(json.dumps(dict(op=name, copies=ncopy, natural_exceptions=nex)), flush=True)
        it = [0]
        stream = torch.cuda.current_stream().cuda_stream
        epi = hip.EPI_BF16 if S == 1 else hip.EPI_F32_PARTIAL
        for M in (1, 40):
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            o = torch.empty((M, N) if S == 1 else (S, M, N), device=dev,
                            dtype=torch.bfloat16 if S == 1 else torch.float32)

            def run_bf16():
                it[0] += 1
                w = ws[it[0] % ncopy]
                rc = hip._fn("mrsum_stream_gemm")(x.data_ptr(), K, w.data_ptr(), N, K, M, o.data_ptr(), N, epi,
                                                  S, wpb, None, None, None, 0, 0.0, None, 0, None, 0, None, stream)
                assert rc == 0, rc

            def run_p14():
                it[0] += 1
                p, base7 = p14s[it[0] % ncopy]
                rc = hip._fn("mrsum_stream_p14")(x.data_ptr(), K, p.data_ptr(), base7, N, K, M, o.data_ptr(), N, epi,
                                                 S, wpb, None, None, None, 0, 0.0, None, 0, None, None, stream)
                assert rc == 0, rc

            def run_p13(packs):
                def fn():
                    it[0] += 1
                    p, base7, exoff, exlist = packs[it[0] % ncopy][:4]
                    rc = hip._fn("mrsum_stream_p13")(x.data_ptr(), K, p.data_ptr(), base7, exoff.data_ptr(),
                                                     exlist.data_ptr(), N, K, M, o.data_ptr(), N, epi, S, wpb, None,
                                                     None, None, 0, 0.0, None, 0, None, None, stream)
                    assert rc == 0, rc
                return fn

            kinds = [("bf16", run_bf16, nb), ("p14", run_p14, nb * 7 // 8), ("p13", run_p13(p13s), nb * 13 // 16)]
            if p13x:
                kinds.append(("p13x", run_p13(p13x), nb * 13 // 16))
            for rep in range(a.reps):
                for kind, fn, bytes_ in kinds:
                    t = b2b(fn, a.launches)
                    row = dict(op=name, N=N, K=K, wpb=wpb, S=S, M=M, kernel=kind, rep=rep, us=round(t * 1e6, 2),
                               Tweights_s=round(N * K / t / 1e12, 3), TBps=round(bytes_ / t / 1e12, 3))
                    rows.append(row)
                    print(json.dumps(row), flush=True)
            # bit identity on one copy, at the measured shape
            it[0] = 0
            run_bf16()
            ref = o.clone()
            it[0] = 0
            run_p13(p13s)()
            torch.cuda.synchronize()
            print(json.dumps(dict(op=name, M=M, identical=bool(torch.equal(ref, o)))), flush=True)
        del ws, p14s, p13s, p13x
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
