"""The GEMM probes (tests/_gemm_probes.py) proved on the CPU: the reference path reproduces every expectation
under the rule the GPU tests use, and that rule rejects every mutant -- the output of one specific kernel
mistake -- in every 16 x 16 output tile the mistake touches, at every probe shape.  No GPU needed.

The truncation mutant (a bf16 store that cuts instead of rounding to nearest even) changes only the elements
whose exact sum is not a bf16 value and rounds up: none at K = 128, where every |sum| <= 256, and a few per
thousand at K = 1024.  It is therefore required to be rejected somewhere in the output at K >= ROUNDING_K, not
in every tile, and asserted invisible at K = 128 so that nobody moves the rounding probe to a small K.
"""

import pytest
import torch

import _gemm_probes as P
from llm_map_reduce_summarizer_amd.ops import reference


def _rejected_in_every_tile(got, want, rule="exact", rows=None):
    """The rule flags ``got`` in every 16 x 16 tile (``rows``: only the tile rows holding these output rows)."""
    t = P.tile_any(P.mismatch(got, want, rule))
    if rows is not None:
        t = t[sorted({r // 16 for r in rows})]
    return bool(t.all())


# ------------------------------------------------------------------ the reference reproduces the expectations
@pytest.mark.parametrize("M,N,K", [(1, 128, 128), (17, 224, 384), (64, 128, 2304), (257, 272, 4096)])
def test_reference_linear_is_bit_exact(M, N, K):
    p = P.linear_probe(M, N, K)
    assert torch.equal(reference.linear(p.x, p.w), P.as_bf16(p.E))
    nkb = K // 128
    for S in sorted({1, 2 if nkb % 2 == 0 else 1, nkb}):
        slabs = reference.linear_parts(p.x, p.w, S)
        assert torch.equal(slabs, p.parts(M, S)) and torch.equal(slabs.double().sum(0), p.E)
    f = P.linear_probe(M, N, K, fp8=True)
    assert torch.equal(reference.linear(f.x, f.w), P.as_bf16(f.E))
    assert torch.equal(reference.linear_parts(f.x, f.w, 1)[0].double(), f.E)
    # residual epilogue: reference.add_rmsnorm_parts updates the residual with the same arithmetic
    res = p.resid.clone()
    reference.add_rmsnorm_parts(p.parts(M, 1), res, torch.ones(N, dtype=torch.bfloat16), P.EPS)
    assert torch.equal(res, P.resid_expected(p.resid, p.E, 16)[0])


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("K", [128, 1024, 2304])
def test_reference_swiglu_obeys_both_regimes(K, fp8):
    for regime in ("exact", "small"):
        p = P.swiglu_probe(64, 64, K, regime, fp8=fp8)
        gu = reference.linear_parts(p.x, p.w, 1)[0]  # the un-rounded fp32 gate_up product
        got = reference.swiglu(gu).to(torch.bfloat16)
        assert not bool(P.mismatch(got, p.want, p.rule).any()), (regime, K, fp8)
        if regime == "exact":  # g / (1 + exp(-g)) == g in fp32 from the lifted gates on
            g = p.G.float()
            assert torch.equal(g / (1.0 + torch.exp(-g)), g)


def test_reference_fp8_activations_are_exact():
    M, N, K = 33, 48, 256
    w = P.fp8_weight(P.int_w(N, K))
    xq, xs = P.fp8_rows(P.int_x(M, K))
    val = xq.double() * xs.double()[:, None]
    assert torch.equal(((xq.float() * xs[:, None]) @ w.dequant().t()).double(), P.expected(val, w))
    q2, s2, val2 = P.fp8_two_term(M, K)
    two = (q2[:, :K].float() + q2[:, K:].float() / 16) * s2[:, None]  # as tests/test_kernels_gpu.py reads it
    assert torch.equal(two.double(), val2) and torch.equal((two @ w.dequant().t()).double(), P.expected(val2, w))
    P.as_bf16(P.expected(val2, w))  # exact in fp32


def test_reference_deferred_norm_within_one_ulp():
    M, N, K = 39, 128, 384
    p = P.linear_probe(M, N, K)
    ssq = P.norm_ssq(M, K)
    got = (p.E.float() * torch.rsqrt(ssq.sum(1, keepdim=True) / K + P.EPS)).to(torch.bfloat16)
    assert not bool(P.mismatch(got, P.norm_expected(p.E, ssq, K), "ulp1").any())
    means = ssq.double().sum(1) / K
    ratio = means[1:] / means[:-1]
    assert bool(((ratio >= 4) | (ratio <= 0.25)).all())


# ------------------------------------------------------------------ every mutant, every tile, every shape
def _linear_shapes():
    """(family, Mmax, Ms, N, K, fp8, k block) of every linear probe of tests/test_gemm_probes_gpu.py."""
    out = []
    for wpb in (4, 5, 6, 7, 8):
        for K in P.STREAM_K:
            out.append(("stream", 200, P.STREAM_M + P.STREAM_TALL_M, 32 * wpb, K, False, 128))
        for K in P.STREAM_FP8_K:
            out.append(("stream_fp8", 64, P.STREAM_M, 32 * wpb, K, True, 256))
        for K in P.LDS_K:
            out.append(("lds", 64, P.STREAM_M, 32 * wpb, K, False, 128))
    for K in P.SKINNY_K:
        for fp8 in (False, True):
            out.append(("skinny", 64, P.SKINNY_M, 64, K, fp8, 128))
    for fp8 in (False, True):
        out.append(("skinny_global", 1, (1,), 64, P.SKINNY_GLOBAL_K, fp8, 128))
    for N in P.TILE_N:
        for K in P.TILE_K:
            out.append(("tile", 513, P.TILE_M, N, K, False, 64))
        for K in P.TILE_FP8_K:
            out.append(("tile_fp8", 513, P.TILE_M, N, K, True, 128))
    Md = max(P.DISPATCH_M)
    out += [("dispatch", Md, P.DISPATCH_M, 11520, 384, False, 128),
            ("dispatch", Md, P.DISPATCH_M, 128, 384, False, 128),
            ("dispatch", Md, P.DISPATCH_M, 128, 512, True, 128),
            ("dispatch", 64, (1, 16, 17, 64), 128, 512, "narrow", 128),
            ("tp_push", 39, (7, 39), 4096, 1024, False, 128),
            ("tp_push", 39, (7, 39), 4096, 512, "narrow", 256)]
    return out


@pytest.mark.parametrize("family", ["stream", "stream_fp8", "lds", "skinny", "skinny_global", "tile", "tile_fp8",
                                    "dispatch", "tp_push"])
def test_term_mutants_rejected_in_every_tile(family):
    """Dropped / doubled k element, stale k block, swapped 16-byte chunks, ragged-M clamp, shifted tile, shifted
    fp8 row scales and exchanged split-K slabs against the bit-exact rule."""
    for fam, Mmax, Ms, N, K, fp8, blk in _linear_shapes():
        if fam != family:
            continue
        p = P.linear_probe(Mmax, N, K, fp8=fp8)
        nb = K // blk
        chunk = 16 if fp8 else 8  # elements per 16 bytes
        ks = sorted({0, K // 2 + 3, K - 1})
        muts = {"drop k=%d" % k: P.mut_drop_k(p.x, p.w, k, E=p.E) for k in ks}
        muts.update({"double k=%d" % k: P.mut_double_k(p.x, p.w, k, E=p.E) for k in ks})
        for kb in sorted({0, nb - 2}) if nb >= 2 else ():
            muts["stale block %d" % kb] = P.mut_stale_block(p.x, p.w, kb, blk, E=p.E)
        for kb, c0, c1 in ((0, 0, 1), (nb - 1, blk // chunk - 2, blk // chunk - 1), (nb // 2, 1, blk // chunk - 1)):
            muts["swap chunks %d/%d of block %d" % (c0, c1, kb)] = P.mut_swap_chunks(p.x, p.w, kb, c0, c1, blk,
                                                                                    chunk, E=p.E)
        muts["tile shift"] = P.mut_tile_shift(p.E)
        if fp8:
            muts["row scales shifted"] = P.mut_scale_shift(p.x, p.w)
        for M in Ms:
            want = P.as_bf16(p.E[:M])
            for name, t in muts.items():
                assert _rejected_in_every_tile(P.as_bf16(t[:M]), want), (name, fam, M, N, K)
            if M >= 2:
                assert _rejected_in_every_tile(P.as_bf16(P.mut_ragged_clamp(p.E[:M])), want, rows=[M - 2]), \
                    ("ragged clamp", fam, M, N, K)
            if fam in ("stream", "stream_fp8", "lds", "skinny") and nb >= 2:
                S = nb if fam != "skinny" else 2
                slabs = p.parts(M, S)
                for s in sorted({0, S - 2}):
                    bad = P.mismatch(P.mut_swap_slabs(slabs, s), slabs)
                    assert all(bool(P.tile_any(bad[i]).all()) for i in (s, s + 1)), ("slabs", fam, M, N, K)


def test_residual_and_norm_mutants_rejected():
    """The last split left out of the residual sum (h and the per-tile sums of squares) and the deferred-norm
    row scale of the neighbouring row."""
    for wpb in (4, 5, 6, 7, 8):
        N, tile = 32 * wpb, 16 * wpb
        cases = [(K, False) for K in P.RESID_K if K >= 256] + [(K, "narrow") for K in P.RESID_FP8_K if K >= 512]
        for K, fp8 in cases:
            p = P.linear_probe(64, N, K, fp8=fp8)
            S = K // (256 if fp8 else 128)
            for M in P.STREAM_M:
                h, ssp = P.resid_expected(p.resid[:M], p.E[:M], tile)
                h2, ssp2 = P.mut_last_split_missing(p.resid[:M], p.parts(M, S), tile)
                assert _rejected_in_every_tile(h2, h) and bool((ssp2 != ssp).any()), (M, N, K, fp8)
                hp, _ = P.resid_expected(p.resid[:M], p.E[:M], tile, pushed=True)
                assert hp.shape == h.shape
        for K in P.STREAM_K:
            p = P.linear_probe(64, N, K)
            for M in P.STREAM_M[1:]:
                ssq = P.norm_ssq(M, K)
                assert _rejected_in_every_tile(P.mut_norm_neighbour(p.E[:M], ssq, K),
                                               P.norm_expected(p.E[:M], ssq, K), "ulp1"), (M, N, K)
    # every residual probe the GPU tests run satisfies the builder's preconditions (16-column skinny tiles too)
    for K in P.SKINNY_K:
        for fp8 in (False, "narrow"):
            p = P.linear_probe(16, 64, K, fp8=fp8)
            P.resid_expected(p.resid, p.E, 16)


@pytest.mark.parametrize("fp8", [False, True])
def test_gate_up_swap_rejected_in_every_tile(fp8):
    shapes = [(64, 16 * wpb, K) for wpb in (4, 7, 8) for K in (128, 384, 2304)] + [(513, 264, 1024), (64, 32, 512)]
    for Mmax, F, K in shapes:
        for regime in ("exact", "small"):
            p = P.swiglu_probe(Mmax, F, K, regime, fp8=fp8)
            for M in sorted({1, 17, Mmax}):
                assert _rejected_in_every_tile(P.mut_swap_gate_up(p, M), p.want[:M].contiguous(), p.rule), \
                    (regime, M, F, K)


# ------------------------------------------------------------------ the rounding probe
def test_truncation_visible_from_k_1024_and_invisible_at_128():
    for N in (128, 256):
        p = P.linear_probe(64, N, 128)
        assert float(p.E.abs().max()) <= 256 and torch.equal(P.trunc_bf16(p.E), P.as_bf16(p.E))
    for fam, Mmax, Ms, N, K, fp8, blk in _linear_shapes():
        if K < P.ROUNDING_K or fp8:
            continue
        p = P.linear_probe(Mmax, N, K)
        for M in Ms:
            if M * N >= 16 * 128:  # enough elements for a few per thousand to show
                assert bool(P.mismatch(P.trunc_bf16(p.E[:M]), P.as_bf16(p.E[:M])).any()), (fam, M, N, K)
    p = P.linear_probe(513, 528, 4096)  # the tile GEMM's rounding probe
    assert float(p.E.abs().max()) > 256


# ------------------------------------------------------------------ why the probes exist
@pytest.mark.parametrize("K", [1024, 2304, 4096])
def test_old_tolerance_passes_a_dropped_term(K):
    """The Gaussian operands and the ``_close(..., 2e-2)`` rule of tests/test_kernels_gpu.py on one decode row:
    for a share of the k columns (those whose activation is small) a kernel that drops the column passes in
    EVERY output element.  The integer probe of the same shape rejects the drop of every single column in
    every tile."""
    N = 96
    g = torch.Generator().manual_seed(60)
    x = torch.randn(1, K, generator=g).to(torch.bfloat16).double()
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).double()
    ref = x @ w.t()
    delta = x[0][:, None] * w.t()                                   # [K, N]: what dropping column k removes
    passes = ~P.old_rule_bad(ref - delta, ref.expand(K, N)).any(1)  # per k: no element flagged
    assert int(passes.sum()) >= K // 100, "the old rule should let one dropped column in a hundred pass"
    p = P.linear_probe(1, N, K)
    want = P.as_bf16(p.E)
    deltas = p.x[0].double()[:, None] * p.w.double().t()
    got = P.as_bf16((p.E - deltas).reshape(K, N))
    assert bool((got != want).view(K, N // 16, 16).any(2).all())


# ------------------------------------------------------------------ the one-hot probe
def test_onehot_probe_covers_the_borders_and_names_what_arrived():
    for K, blk in ((128, 128), (384, 128), (2304, 128), (1024, 64), (256, 256)):
        ks = P.onehot_ks(K, blk)
        nb = K // blk
        for b in {0, min(1, nb - 1), nb - 1}:
            assert b * blk in ks and b * blk + blk - 1 in ks
        b = min(1, nb - 1)
        assert all(b * blk + c - 1 in ks and b * blk + c in ks for c in range(8, blk, 8))
    o = P.OneHot(64, 128, 2304)
    assert o.covered
    assert torch.equal(reference.linear(o.x, o.w), o.want)
    o.check(o.want.clone())
    # two swapped chunks of the probed block: rows at those k see another column of w, and the message says so
    got = P.as_bf16(P.mut_swap_chunks(o.x, o.w, 1, 0, 1))
    with pytest.raises(AssertionError) as e:
        o.check(got, "swap")
    m = int((got != o.want).any(1).nonzero()[0])
    assert "out[m=%d" % m in str(e.value) and "k=%d" % (int(o.km[m]) + 8) in str(e.value)


def test_frames():
    x = P.int_x(5, 128)
    v = P.x_frame(x)
    assert torch.equal(v, x) and v.stride(0) == 192 and v.data_ptr() % 16 == 0
    for shape in ((5, 32), (3, 5, 32)):
        buf, view = P.out_frame(shape, torch.float32, "cpu")
        assert view.shape == shape and P.frame_untouched(buf, view)
        view.fill_(1.0)
        assert P.frame_untouched(buf, view)
        if len(shape) == 3:
            assert view.stride(0) == shape[1] * view.stride(1)
        buf.view(-1)[3] = 0.0
        assert not P.frame_untouched(buf, view)
