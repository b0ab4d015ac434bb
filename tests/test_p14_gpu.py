"""p14 (lossless 14-bit packed bf16 decode weights) on the GPU: the packer against the bit-level reference, the
packed stream GEMM bit-identical to the bf16 stream GEMM with the same plan, the fallback, the engine."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from llm_map_reduce_summarizer_amd.engine.config import get_model_config  # noqa: E402
from llm_map_reduce_summarizer_amd.engine.engine import LLMEngine, SamplingParams  # noqa: E402
from llm_map_reduce_summarizer_amd.ops import hip, reference  # noqa: E402

DEV = "cuda:0"


def _rand(*shape, scale=1.0, seed=0):  # the generator of test_kernels_gpu.py (asymmetric random data)
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(DEV)


@pytest.mark.parametrize("N,K", [(64, 256), (224, 1280)])
def test_packer_matches_reference(N, K):
    w = _rand(N, K, scale=0.05, seed=70)
    w[1, 3] = 0.0   # the e7 = 0 class next to ordinary weights
    w[N - 1, K - 1] = -0.0
    packed, base7, bad = hip.p14_pack(w)
    rp, rb, rbad = reference.p14_pack_ref(w.cpu())
    assert (base7, bad) == (rb, rbad) == (rb, 0)
    assert torch.equal(packed.cpu(), rp)  # byte for byte: the format is pinned
    assert torch.equal(reference.p14_bits(reference.p14_unpack_ref(packed.cpu(), base7, N, K)),
                       reference.p14_bits(w.cpu()))
    w[N // 2, K // 2] = 1e-30  # far below the window
    assert hip.p14_pack(w)[2] == reference.p14_pack_ref(w.cpu())[2] == 1


class _Case:
    """One (M, wpb, K, S) plan: every epilogue of the stream GEMM on the bf16 weight (MRSUM_P14=0) and on its
    registered packed form (MRSUM_P14=1)."""

    def __init__(self, M, wpb, K, S, monkeypatch):
        self.M, self.wpb, self.K, self.S, self.mp = M, wpb, K, S, monkeypatch
        self.N = N = 32 * wpb  # two column tiles
        self.x = _rand(M, K, seed=80)
        self.w = _rand(N, K, scale=0.05, seed=81)
        self.resid0 = _rand(M, N, seed=82)
        g = torch.Generator(device="cpu").manual_seed(83)
        self.ssq = (torch.rand(M, 32, generator=g) * K / 16 + 0.5).to(DEV)
        self.cnt = torch.zeros(64, dtype=torch.int32, device=DEV)
        self.pw = hip.p14_attach(self.w, "gate_up")
        assert self.pw.packable

    def close(self):
        hip.p14_detach(self.w)

    def run(self, p14, epi, S, norm=False):
        """(results...) of one launch pair: split epilogues run twice on the same counters and scratch."""
        M, N, wpb = self.M, self.N, self.wpb
        self.mp.setenv("MRSUM_P14", "1" if p14 else "0")
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
        key = "stream_p14" if p14 else "stream_bf16"
        other = "stream_bf16" if p14 else "stream_p14"
        assert hip.STATS[key] - before[key] == launches and hip.STATS[other] == before[other]
        return outs


@pytest.mark.parametrize("M", [1, 16, 17, 39, 64])
@pytest.mark.parametrize("wpb,K,S", [(4, 128, 1), (6, 1280, 1), (7, 1280, 1), (7, 5120, 4)])
def test_gemm_bit_identical_to_bf16_stream(M, wpb, K, S, monkeypatch):
    """K = 128: one k block (clamped prologue); K = 1280 with one split: 10 k blocks > the deepest ring (8), so slots
    wrap; K = 5120 with 4 splits: the split path.  Every epilogue at every row-tile count."""
    c = _Case(M, wpb, K, S, monkeypatch)
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


def test_unpackable_weight_falls_back_to_bf16(monkeypatch, capsys):
    M, K, wpb = 5, 1280, 7
    N = 32 * wpb
    x = _rand(M, K, seed=90)
    w = _rand(N, K, scale=0.05, seed=91)
    w[7, 130] = 1e-30  # one element far below the exponent window
    monkeypatch.setenv("MRSUM_P14", "0")
    ref = hip._stream_gemm(x, w, torch.zeros(M, N, dtype=torch.bfloat16, device=DEV), hip.EPI_BF16, 1, N, wpb)
    monkeypatch.setenv("MRSUM_P14", "1")
    pw = hip.p14_attach(w, "down")
    try:
        assert not pw.packable and pw.packed is None and hip.p14_lookup(w) is None
        assert "outside the exponent window" in capsys.readouterr().out
        before = dict(hip.STATS)
        out = hip._stream_gemm(x, w, torch.zeros(M, N, dtype=torch.bfloat16, device=DEV), hip.EPI_BF16, 1, N, wpb)
        assert torch.equal(out, ref)
        assert hip.STATS["stream_bf16"] == before["stream_bf16"] + 1 and hip.STATS["stream_p14"] == before["stream_p14"]
    finally:
        hip.p14_detach(w)


def _engine():
    return LLMEngine(get_model_config("tiny-gqa4", init_std=0.05), device="cuda:0", max_model_len=2048,
                     max_num_seqs=24, kv_pages=256, sync_every=8)


def test_engine_tokens_identical_with_and_without_p14(monkeypatch):
    """Batches of 1, 12 (the 10-16 row bucket) and 20 (> 16 rows): every M-dependent plan the engine selects."""
    batches = [[[128000] + [(i * 37 + j * 11) % 120000 + 5 for j in range(9 + 5 * i)] for i in range(n)]
               for n in (1, 12, 20)]
    toks = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("MRSUM_P14", flag)
        before = hip.STATS["stream_p14"]
        eng = _engine()
        assert bool(eng.model.p14) == (flag == "1")
        toks[flag] = [[o.token_ids for o in eng.generate(p, [SamplingParams(6, 0.3, 7 + i) for i in range(len(p))])]
                      for p in batches]
        assert (hip.STATS["stream_p14"] > before) == (flag == "1")
        del eng
    assert toks["1"] == toks["0"]
