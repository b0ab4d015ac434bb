"""The attention kernels on the counting probes (tests/_probes.py): every valid key weighs exactly 1 and is
recognisable in the output, every slot that is no valid key holds a poison, so the output is known in closed
form and one key too many or too few -- at any context up to 2048 -- moves a dimension by 4x the bound.
tests/test_probes_cpu.py shows on the reference that the probes catch such mistakes.

Also the launcher's nontemporal-load instantiations (B x head groups >= 64: the production decode batch),
which no other kernel test reaches for G in {2, 4, 8, 16}, the RoPE variant or an fp8 cache, with an idle
bucket row (position 0, block table all scratch page 0) in the batch."""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import _probes as pr  # noqa: E402
from llm_map_reduce_summarizer_amd.ops import hip, reference  # noqa: E402

DEV = "cuda:0"
SC = 1.0 / math.sqrt(pr.D)
CTXS = [1, 2, 63, 64, 65, 127, 128, 129, 700, 1000, 2048]
BIG_CTXS = [1, 64, 65, 129, 700, 1000, 2048]
FMTS = ["bf16", "fp8", "fp8v"]
MAX_HQ = 64


@functools.lru_cache(maxsize=None)
def _cos_sin():
    return reference.rope_cos_sin(pr.MAX_CTX, pr.D, 500000.0, DEV)


@functools.lru_cache(maxsize=None)
def _decode_probe(ctxs, hkv, fmt, n_idle):
    """Shared by every head configuration over ``hkv`` kv heads (the plain decode never writes the cache): q
    rows are MAX_HQ heads wide, a launch reads the first hq of them."""
    return pr.decode_probe(list(ctxs), hkv, fmt, n_idle=n_idle, hq=MAX_HQ).to(DEV)


@functools.lru_cache(maxsize=None)
def _rope_probe(ctxs, hq, hkv, fmt, n_idle, sp):
    return pr.decode_rope_probe(list(ctxs), hq, hkv, fmt, n_idle=n_idle, sp=sp)  # on the CPU: a launch writes it


def _workspace(B, hq, hkv, splits, fused):
    ws = hip.DecodeWorkspace(B, hq, pr.D, splits, DEV, hip.decode_groups(hq, hkv), fused_combine=fused)
    # a reused allocation may hold NaN / inf: empty splits must publish zero slabs
    ws.part_o.fill_(float("nan"))
    ws.part_ml.fill_(float("nan"))
    return ws


def _run_decode(p, hq, hkv, splits, fused, launches=2):
    ws = _workspace(p.B, hq, hkv, splits, fused)
    for _ in range(launches):
        out = hip.attn_decode(p.q, p.kcache, p.vcache, p.block_tables, p.positions, hq, hkv, pr.D, pr.PAGE, SC,
                              workspace=ws)
        pr.check_counts(out[:p.live], p.expect)
    if fused:
        assert int(ws.counters.abs().sum()) == 0


def _run_rope(pc, hq, hkv, splits, fused, launches=3):
    p = pc.to(DEV)
    ws = _workspace(p.B, hq, hkv, splits, fused)
    for _ in range(launches):  # later launches rewrite the same K / V row
        out = hip.attn_decode_rope(p.parts, _cos_sin(), p.kcache, p.vcache, p.block_tables, p.positions, hq, hkv,
                                   pr.D, pr.PAGE, SC, workspace=ws)
        pr.check_counts(out[:p.live], p.expect)
    if fused:
        assert int(ws.counters.abs().sum()) == 0
    pr.check_new_rows(pc, pc.kcache, pc.vcache, p.kcache, p.vcache)


# splits 40 > 16: the per-head merge; 40 > the 32 pages of the longest context: empty splits
@pytest.mark.parametrize("hq,hkv", [(4, 4), (4, 2), (8, 2), (8, 1), (16, 1), (6, 2)])
@pytest.mark.parametrize("splits", [1, 3, 16, 40])
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("fmt", FMTS)
def test_decode_counts(hq, hkv, splits, fused, fmt):
    _run_decode(_decode_probe(tuple(CTXS), hkv, fmt, 2), hq, hkv, splits, fused)


@pytest.mark.parametrize("hq,hkv", [(4, 4), (4, 2), (8, 2), (8, 1), (6, 2), (32, 8)])
@pytest.mark.parametrize("sp", [1, 4])
@pytest.mark.parametrize("splits,fused", [(1, False), (3, True), (40, False)])
@pytest.mark.parametrize("fmt", FMTS)
def test_decode_rope_counts(hq, hkv, sp, splits, fused, fmt):
    _run_rope(_rope_probe(tuple(CTXS), hq, hkv, fmt, 2, sp), hq, hkv, splits, fused)


def _big_ctxs(B):
    return tuple(BIG_CTXS[i % len(BIG_CTXS)] for i in range(B - 1))  # + one idle row


# the smallest batches that reach B x head groups >= 64 (attn_decode.hip NT_MIN_GROUPS): G = 1, 2, 4, 8 over
# 8 kv heads x 8 rows, G = 16 over 2 kv heads x 32 rows
BIG = [(8, 8, 8), (16, 8, 8), (32, 8, 8), (64, 8, 8), (32, 2, 32)]


@pytest.mark.parametrize("hq,hkv,B", BIG)
@pytest.mark.parametrize("splits,fused", [(4, False), (3, True)])
@pytest.mark.parametrize("fmt", FMTS)
def test_decode_counts_large_batch(hq, hkv, B, splits, fused, fmt):
    assert B * hip.decode_groups(hq, hkv) >= 64
    _run_decode(_decode_probe(_big_ctxs(B), hkv, fmt, 1), hq, hkv, splits, fused)


@pytest.mark.parametrize("hq,hkv,B", BIG)
@pytest.mark.parametrize("splits,fused", [(4, False), (3, True)])
@pytest.mark.parametrize("fmt", FMTS)
def test_decode_rope_counts_large_batch(hq, hkv, B, splits, fused, fmt):
    assert B * hip.decode_groups(hq, hkv) >= 64
    _run_rope(_rope_probe(_big_ctxs(B), hq, hkv, fmt, 1, 2), hq, hkv, splits, fused)


# GQA ratios 1, 2, 4, 8 (all heads of a kv head in one workgroup) and 3 (one query head per workgroup)
RATIOS = [(2, 2), (4, 2), (8, 2), (8, 1), (6, 2)]


@pytest.mark.parametrize("hq,hkv", RATIOS)
def test_prefill_counts(hq, hkv):
    p = pr.prefill_probe([1, 63, 64, 65, 257, 700], hq, hkv).to(DEV)
    out = hip.attn_prefill(p.qkv, p.cu_seqlens, hq, hkv, pr.D, SC)
    pr.check_counts(out[:p.T], p.expect)


@pytest.mark.parametrize("hq,hkv", RATIOS)
@pytest.mark.parametrize("spans", [((0, 200),), ((130, 300), (0, 77), (1000, 1129)), ((64, 128), (2047, 2048))])
@pytest.mark.parametrize("fmt", FMTS)
def test_prefill_paged_counts(hq, hkv, spans, fmt):
    p = pr.paged_prefill_probe(list(spans), hq, hkv, fmt).to(DEV)
    out = hip.attn_prefill(p.qkv, p.cu_seqlens, hq, hkv, pr.D, SC, paged=pr.paged_args(p))
    pr.check_counts(out, p.expect)
