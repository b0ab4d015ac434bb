"""p13 (lossless 13-bit packed bf16 decode weights with an exception list) on the GPU: the packer against the
bit-level reference (tiles and list), the packed stream GEMM bit-identical to the bf16 stream GEMM with the same
plan -- without exceptions and with exceptions planted at every position class the kernel distinguishes --, the
fallback chain p13 -> p14 -> bf16, the engine."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from llm_map_reduce_summarizer_amd.engine.config import get_model_config  # noqa: E402
from llm_map_reduce_summarizer_amd.engine.engine import LLMEngine, SamplingParams  # noqa: E402
from llm_map_reduce_summarizer_amd.ops import hip, reference  # noqa: E402

DEV = "cuda:0"
TINY = 1e-30  # bf16 e7 = 13: far below the 15-value window of weights of scale 0.05 (and below p14's)


def _rand(*shape, scale=1.0, seed=0):  # the generator of test_kernels_gpu.py (asymmetric random data)
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(DEV)


def _planted(N, K, S):
    """(row, k, sign) of the planted exceptions: first and last k block of a group, MFMA step 0 element 0 and step
    3 element 7, two in one tile in one lane and two in different lanes, one in the last wave of the second column
    tile, and (S = 4) one in the third split's k range."""
    kb1 = 128 * min(1, K // 128 - 1)
    far = min(128 * 25 + 5, K - 128 + 5)  # K = 5120, S = 4: k block 25 of 40 = split 2
    assert S == 1 or far // (K // S) == 2
    return [(0, 0, 1), (1, K - 1, -1), (17, kb1 + 8, -1), (17, kb1 + 9, 1), (18, kb1 + 40, 1), (19, kb1 + 100, -1),
            (N - 4, 64, 1), (33, far, -1)]


@pytest.mark.parametrize("N,K", [(64, 256), (224, 1280)])
def test_packer_matches_reference(N, K):
    w = _rand(N, K, scale=0.05, seed=70)
    w[1, 3] = 0.0   # the e7 = 0 class next to ordinary weights
    w[N - 1, K - 1] = -0.0
    for r, k, s in _planted(N, K, 1):
        w[r, k] = s * TINY
    w[40, 77] = 3e-10  # e7 = 47: one step below the window of a largest e7 of 62
    packed, base7, exoff, exlist, nex, worst = hip.p13_pack(w)
    rp, rb, roff, rlist, rworst = reference.p13_pack_ref(w.cpu())
    assert (base7, nex, worst) == (rb, rlist.numel(), rworst) and nex >= 9 and worst <= hip.P13_EXCAP
    assert torch.equal(packed.cpu(), rp)  # byte for byte: the format is pinned
    assert torch.equal(exoff.cpu(), roff) and torch.equal(exlist.cpu(), rlist)
    back = reference.p13_unpack_ref(packed.cpu(), base7, exoff.cpu(), exlist.cpu(), N, K)
    assert torch.equal(reference.p14_bits(back), reference.p14_bits(w.cpu()))
    for j in range(hip.P13_EXCAP - 3):  # group 1 already holds 4: the cap, then one above it
        w[20 + j, 200] = TINY
    assert hip.p13_pack(w)[5] == reference.p13_pack_ref(w.cpu())[4] == hip.P13_EXCAP + 1


class _Case:
    """One (M, wpb, K, S) plan: every epilogue of the stream GEMM on the bf16 weight (MRSUM_P14=0) and on its
    registered p13 form (MRSUM_P14=1, MRSUM_P13=1)."""

    def __init__(self, M, wpb, K, S, planted, monkeypatch):
        self.M, self.wpb, self.K, self.S, self.mp = M, wpb, K, S, monkeypatch
        self.N = N = 32 * wpb  # two column tiles
        self.x = _rand(M, K, seed=80)
        self.w = _rand(N, K, scale=0.05, seed=81)
        if planted:
            for r, k, s in _planted(N, K, S):
                self.w[r, k] = s * TINY
        self.resid0 = _rand(M, N, seed=82)
        g = torch.Generator(device="cpu").manual_seed(83)
        self.ssq = (torch.rand(M, 32, generator=g) * K / 16 + 0.5).to(DEV)
        self.cnt = torch.zeros(64, dtype=torch.int32, device=DEV)
        self.pw = hip.p13_attach(self.w, "gate_up")
        assert self.pw.packable and (self.pw.nex >= 8 if planted else True)

    def close(self):
        hip.p13_detach(self.w)

    def run(self, p13, epi, S, norm=False):
        """(results...) of one launch pair: split epilogues run twice on the same counters and scratch."""
        M, N, wpb = self.M, self.N, self.wpb
        self.mp.setenv("MRSUM_P14", "1" if p13 else "0")
        self.mp.setenv("MRSUM_P13", "1")
        before = dict(hip.STATS)
        nrm = (self.ssq, 1e-5) if norm else None
        outs = []
        if epi == hip.EPI_BF16:
            o = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
            outs.append(hip._stream_gemm(self.x, self.w, o, epi, 1, N, wpb, norm=nrm))
            launches = 1
        elif epi == hip.EPI_SWIGLU:
            o = torch.zeros(M, N // 2, dtype=torch.bfloat16, device=DEV)
            outs.append(hip._stream_gemm(self.x, self.w, o, epi, 1, N // 2, wpb, norm=nrm))
            launches = 1
        elif epi == hip.EPI_F32_PARTIAL:
            o = torch.zeros(S, M, N, dtype=torch.float32, device=DEV)
            outs.append(hip._stream_gemm(self.x, self.w, o, epi, S, N, wpb))
            launches = 1
        else:
            parts = torch.zeros(S, M, N, dtype=torch.float32, device=DEV)
            ssp = torch.zeros(M, 2, dtype=torch.float32, device=DEV)
            for _ in range(2):  # ticket re-arm: the second launch finds the counters at zero
                if epi == hip.EPI_SWIGLU_SPLIT:
                    o = torch.zeros(M, N // 2, dtype=torch.bfloat16, device=DEV)
                    hip._stream_gemm(self.x, self.w, o, epi, S, N // 2, wpb, parts=parts, counters=self.cnt)
                    outs.append(o)
                else:
                    r = self.resid0.clone()
                    hip._stream_gemm(self.x, self.w, None, epi, S, 0, wpb, parts=parts, counters=self.cnt, resid=r,
                                     ssp=ssp)
                    outs += [r, ssp.clone()]
            launches = 2
            assert int(self.cnt.abs().sum()) == 0
        d = {k: hip.STATS[k] - before[k] for k in ("stream_p13", "stream_p14", "stream_bf16")}
        want = dict(stream_p13=launches, stream_p14=launches, stream_bf16=0) if p13 else \
            dict(stream_p13=0, stream_p14=0, stream_bf16=launches)
        assert d == want
        return outs


@pytest.mark.parametrize("planted", [False, True])
@pytest.mark.parametrize("M", [1, 16, 17, 39, 64])
@pytest.mark.parametrize("wpb,K,S", [(4, 128, 1), (6, 1280, 1), (7, 1280, 1), (7, 5120, 4)])
def test_gemm_bit_identical_to_bf16_stream(M, wpb, K, S, planted, monkeypatch):
    """p14's grid (K = 128: one k block; K = 1280: 10 k blocks, the ring wraps; K = 5120 with 4 splits: the split
    path; every epilogue at every row-tile count), without and with planted exceptions."""
    c = _Case(M, wpb, K, S, planted, monkeypatch)
    try:
        runs = [(hip.EPI_BF16, 1, False), (hip.EPI_BF16, 1, True), (hip.EPI_SWIGLU, 1, False),
                (hip.EPI_SWIGLU, 1, True), (hip.EPI_F32_PARTIAL, S, False), (hip.EPI_SWIGLU_SPLIT, S, False),
                (hip.EPI_RESID_SPLIT, S, False)]
        for epi, s, norm in runs:
            a = c.run(False, epi, s, norm)
            b = c.run(True, epi, s, norm)
            assert len(a) == len(b)
            for i, (ta, tb) in enumerate(zip(a, b)):
                assert torch.equal(ta, tb), "epi %d S %d norm %s output %d differs" % (epi, s, norm, i)
            if epi in (hip.EPI_SWIGLU_SPLIT, hip.EPI_RESID_SPLIT):  # the repeat on the same tickets and scratch
                h = len(b) // 2
                assert all(torch.equal(p, q) for p, q in zip(b[:h], b[h:]))
        # and not vacuous: the product is the fp32 reference's, to bf16 accuracy
        ref = c.x.float() @ c.w.float().t()
        got = c.run(True, hip.EPI_BF16, 1)[0].float()
        assert float((got - ref).abs().max()) <= 2e-2 + 2e-2 * float(ref.abs().max())
    finally:
        c.close()


def test_exceptions_reach_the_product(monkeypatch):
    """The grid's x is random, so a lost 1e-30 would hide below bf16 rounding: with x = 2^100 on one column the
    restored exception IS the output (and 0 without the list)."""
    M, wpb, K = 3, 4, 256
    N = 32 * wpb
    w = _rand(N, K, scale=0.05, seed=84)
    w[:, 131] = 0.0
    w[18, 131], w[N - 1, 131] = TINY, -TINY
    x = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
    x[:, 131] = 2.0 ** 100
    monkeypatch.setenv("MRSUM_P14", "1")
    monkeypatch.setenv("MRSUM_P13", "1")
    pw = hip.p13_attach(w, "gate_up")
    try:
        assert pw.packable and pw.nex >= 2
        out = hip._stream_gemm(x, w, torch.zeros(M, N, dtype=torch.bfloat16, device=DEV), hip.EPI_BF16, 1, N, wpb)
        want = (x.float() @ w.float().t()).to(torch.bfloat16)
        assert torch.equal(out, want) and float(out[0, 18]) > 0 > float(out[0, N - 1])
    finally:
        hip.p13_detach(w)


def test_fallback_chain_p13_p14_bf16(monkeypatch, capsys):
    M, K, wpb = 5, 1280, 7
    N = 32 * wpb
    x = _rand(M, K, seed=90)
    w = _rand(N, K, scale=0.05, seed=91)
    monkeypatch.setenv("MRSUM_P14", "1")
    monkeypatch.setenv("MRSUM_P13", "1")

    def launch(env14="1"):
        monkeypatch.setenv("MRSUM_P14", env14)
        before = dict(hip.STATS)
        out = hip._stream_gemm(x, w, torch.zeros(M, N, dtype=torch.bfloat16, device=DEV), hip.EPI_BF16, 1, N, wpb)
        monkeypatch.setenv("MRSUM_P14", "1")
        return out, {k: hip.STATS[k] - before[k] for k in ("stream_p13", "stream_p14", "stream_bf16")}

    try:
        # cap exceptions in one group, inside p14's window (1e-14: e7 = 40): p13
        for j in range(hip.P13_EXCAP):
            w[32 + j, 130 + 100 * j] = 1e-14
        pw = hip.packed_attach(w, "gate_up")
        assert isinstance(pw, hip.Packed13Weight) and pw.packable and pw.nex >= hip.P13_EXCAP
        ref, d = launch("0")
        assert d == dict(stream_p13=0, stream_p14=0, stream_bf16=1)
        out, d = launch()
        assert torch.equal(out, ref) and d == dict(stream_p13=1, stream_p14=1, stream_bf16=0)
        hip.packed_detach(w)
        # cap + 1: the p14 kernel
        w[47, 5] = -1e-14
        pw = hip.packed_attach(w, "gate_up")
        assert isinstance(pw, hip.PackedWeight) and pw.packable and hip.p13_lookup(w) is None
        ref, _ = launch("0")
        out, d = launch()
        assert torch.equal(out, ref) and d == dict(stream_p13=0, stream_p14=1, stream_bf16=0)
        hip.packed_detach(w)
        # ... and an element that moves p14's window off the ordinary weights: bf16
        w[7, 130] = 1e20
        pw = hip.packed_attach(w, "gate_up")
        assert isinstance(pw, hip.PackedWeight) and not pw.packable
        assert "outside the exponent window" in capsys.readouterr().out
        ref, _ = launch("0")
        out, d = launch()
        assert torch.equal(out, ref) and d == dict(stream_p13=0, stream_p14=0, stream_bf16=1)
    finally:
        hip.packed_detach(w)


def _engine():
    return LLMEngine(get_model_config("tiny-gqa4", init_std=0.05), device="cuda:0", max_model_len=2048,
                     max_num_seqs=24, kv_pages=256, sync_every=8)


def test_engine_tokens_identical_with_and_without_p13(monkeypatch):
    """Batches of 1, 12 (the 10-16 row bucket) and 20 (> 16 rows): every M-dependent plan the engine selects."""
    batches = [[[128000] + [(i * 37 + j * 11) % 120000 + 5 for j in range(9 + 5 * i)] for i in range(n)]
               for n in (1, 12, 20)]
    monkeypatch.setenv("MRSUM_P14", "1")
    toks = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("MRSUM_P13", flag)
        before = dict(hip.STATS)
        eng = _engine()
        assert eng.model.p14
        assert any(isinstance(p, hip.Packed13Weight) for p in eng.model.p14) == (flag == "1")
        toks[flag] = [[o.token_ids for o in eng.generate(p, [SamplingParams(6, 0.3, 7 + i) for i in range(len(p))])]
                      for p in batches]
        assert hip.STATS["stream_p14"] > before["stream_p14"]
        assert (hip.STATS["stream_p13"] > before["stream_p13"]) == (flag == "1")
        del eng
    assert toks["1"] == toks["0"]
