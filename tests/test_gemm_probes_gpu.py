"""Exact integer probes (tests/_gemm_probes.py) through the decode and prefill GEMM kernels: stream_gemm.hip
(bf16, p14 and fp8 weights), skinny_gemm.hip (register-streaming and x-in-LDS) and gemm.hip (the 256 x 256-tile
kernel, bf16 and fp8), every epilogue, and the dispatchers of ops/hip.py.

The expectation is known bit for bit (integer operands: every fp32 partial sum is exact in any order), so the
comparison is equality of every element.  Two expectations are not exact and are held to ONE bf16 ulp, a bound
derived in _gemm_probes.py and not measured: the small-gate SwiGLU regime and the deferred-norm consumer.  x is
a view into a wider and taller tensor padded with 2^60; outputs are views into sentinel-filled buffers whose
frame must stay untouched.  tests/test_gemm_probes_cpu.py proves that these rules reject every mutant (a
dropped or doubled k element, a stale k block, swapped 16-byte chunks, a truncating store, ...) in every tile.

The exact SwiGLU regime rests on g / (1 + 0) == g in the kernels' fp32 division (IEEE division: the kernel
library is built without fast-math flags).  It holds on the MI355X: every exact-regime case passes with bit
equality, no element differs.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

import _gemm_probes as P  # noqa: E402
from llm_map_reduce_summarizer_amd.ops import hip  # noqa: E402
from llm_map_reduce_summarizer_amd.ops.reference import Fp8Weight  # noqa: E402

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
WPBS = (4, 5, 6, 7, 8)


def _splits(nkb):
    return sorted({1, 2 if nkb % 2 == 0 else 1, nkb})


def _wdev(w):
    return Fp8Weight(w.q.to(DEV), w.scale.to(DEV)) if isinstance(w, Fp8Weight) else w.to(DEV)


def _framed(shape, dtype, off=8):
    return P.out_frame(shape, dtype, DEV, off)


def _done(buf, view, want, rule, what):
    P.check(view, want, rule, what)
    assert P.frame_untouched(buf, view), what + ": wrote outside the output view"


class _Stream:
    """The stream GEMM on bf16 weights, on their registered p14 tiles, or on fp8 weights, at one width."""

    def __init__(self, kind, wpb, monkeypatch):
        assert kind in ("bf16", "p14", "fp8")
        self.kind, self.wpb, self.attached, self.launches = kind, wpb, [], 0
        monkeypatch.setenv("MRSUM_P14", "1" if kind == "p14" else "0")
        self.before = dict(hip.STATS)

    def __enter__(self):
        return self

    def weight(self, w):
        d = _wdev(w)
        if self.kind == "p14":  # +-1, +-2, +-3 (two exponent values) and their power-of-two multiples pack
            assert hip.p14_attach(d, "gate_up").packable
            self.attached.append(d)
        return d

    def __call__(self, x, w, out, epi, S, ldo, **kw):
        f = hip._stream_fp8 if self.kind == "fp8" else hip._stream_gemm
        f(x, w, out, epi, S, ldo, self.wpb, **kw)
        self.launches += x.shape[0] <= hip.SKINNY_MAX_M

    def __exit__(self, *exc):
        for d in self.attached:
            hip.p14_detach(d)
        if self.kind == "p14" and exc[0] is None:  # every launch of up to 64 rows read the packed tiles
            assert self.launches > 0 and hip.STATS["stream_p14"] - self.before["stream_p14"] == self.launches
            assert hip.STATS["stream_bf16"] == self.before["stream_bf16"]
        return False


def _stream_k(kind):
    return P.STREAM_FP8_K if kind == "fp8" else P.STREAM_K


_STREAM_CASES = [(kind, wpb, K) for kind in ("bf16", "p14", "fp8") for wpb in WPBS for K in _stream_k(kind)]


# ------------------------------------------------------------------ stream GEMM: bf16 rows, fp32 slabs, deferred norm
@pytest.mark.parametrize("kind,wpb,K", _STREAM_CASES)
def test_stream_linear(kind, wpb, K, monkeypatch):
    """EPI_BF16, EPI_F32_PARTIAL at S in {1, 2, k blocks} (every slab compared) and the deferred-norm consumer
    on EPI_BF16 at M in {1, 15, 16, 17, 39, 64}; bf16 weights also on the tall tiles / row chunks of 65-200
    rows."""
    N, nkb = 32 * wpb, K // (256 if kind == "fp8" else 128)
    Ms = P.STREAM_M + (P.STREAM_TALL_M if kind == "bf16" else ())
    p = P.linear_probe(max(Ms), N, K, fp8=kind == "fp8")
    with _Stream(kind, wpb, monkeypatch) as run:
        w = run.weight(p.w)
        for M in Ms:
            tag = "%s wpb %d K %d M %d" % (kind, wpb, K, M)
            x = P.x_frame(p.x[:M], DEV)
            buf, o = _framed((M, N), BF16)
            run(x, w, o, hip.EPI_BF16, 1, o.stride(0))
            _done(buf, o, P.as_bf16(p.E[:M]), "exact", tag + " bf16")
            for S in _splits(nkb):
                buf, o = _framed((S, M, N), F32)
                run(x, w, o, hip.EPI_F32_PARTIAL, S, o.stride(1))
                _done(buf, o, p.parts(M, S), "exact", tag + " slabs S %d" % S)
            if M <= hip.SKINNY_MAX_M:
                ssq = P.norm_ssq(M, K)
                buf, o = _framed((M, N), BF16)
                run(x, w, o, hip.EPI_BF16, 1, o.stride(0), norm=(ssq.to(DEV), P.EPS))
                _done(buf, o, P.norm_expected(p.E[:M], ssq, K), "ulp1", tag + " deferred norm")


# ------------------------------------------------------------------ stream GEMM: SwiGLU epilogues
@pytest.mark.parametrize("kind,wpb,K", _STREAM_CASES)
def test_stream_swiglu(kind, wpb, K, monkeypatch):
    """EPI_SWIGLU in both gate regimes (+ the deferred norm on the small-gate one) and EPI_SWIGLU_SPLIT at
    S in {1, 2, k blocks}, launched twice on the same tickets, which must be zero afterwards (fp8: also with
    the deferred norm); bf16 weights also at 65-128 rows.

    Finding, not a defect: with a deferred norm the split-K epilogue scales every split's partial tile by the
    row scale before the last arriver sums them, so where the exact gate or up sum is zero it returns a
    residue of a few fp32 ulp of the partials (up to 3e-5 seen) instead of 0.  The probe of that case therefore
    holds no zero sum (SwigluProbe ``nonzero``, asserted by the builder); the one-ulp rule is unchanged."""
    F, nkb, fp8 = 16 * wpb, K // (256 if kind == "fp8" else 128), kind == "fp8"
    Ms = P.STREAM_M + (tuple(m for m in P.STREAM_TALL_M if m <= 128) if kind == "bf16" else ())
    cnt = torch.zeros(64, dtype=torch.int32, device=DEV)
    with _Stream(kind, wpb, monkeypatch) as run:
        for regime in ("exact", "small"):
            # fp8, small regime: the split-K SwiGLU consumes a deferred norm, which needs non-zero sums
            p = P.swiglu_probe(max(Ms), F, K, regime, fp8=fp8, nonzero=fp8 and regime == "small")
            w = run.weight(p.w)
            for M in Ms:
                tag = "%s wpb %d K %d M %d %s" % (kind, wpb, K, M, regime)
                x = P.x_frame(p.x[:M], DEV)
                want = p.want[:M]
                buf, o = _framed((M, F), BF16)
                run(x, w, o, hip.EPI_SWIGLU, 1, o.stride(0))
                _done(buf, o, want, p.rule, tag + " swiglu")
                if M > hip.SKINNY_MAX_M:
                    continue
                ssq = P.norm_ssq(M, K)
                nwant = p.norm_want(ssq)
                if regime == "small":
                    buf, o = _framed((M, F), BF16)
                    run(x, w, o, hip.EPI_SWIGLU, 1, o.stride(0), norm=(ssq.to(DEV), P.EPS))
                    _done(buf, o, nwant, "ulp1", tag + " swiglu + deferred norm")
                for S in _splits(nkb):
                    parts = torch.empty(S, M, 2 * F, dtype=F32, device=DEV)
                    for rep in range(2):
                        buf, o = _framed((M, F), BF16)
                        run(x, w, o, hip.EPI_SWIGLU_SPLIT, S, o.stride(0), parts=parts, counters=cnt)
                        _done(buf, o, want, p.rule, tag + " swiglu split S %d launch %d" % (S, rep))
                    if fp8 and regime == "small":
                        buf, o = _framed((M, F), BF16)
                        run(x, w, o, hip.EPI_SWIGLU_SPLIT, S, o.stride(0), parts=parts, counters=cnt,
                            norm=(ssq.to(DEV), P.EPS))
                        _done(buf, o, nwant, "ulp1", tag + " swiglu split S %d + deferred norm" % S)
                assert int(cnt.abs().sum()) == 0, tag + ": tickets not re-armed"


# ------------------------------------------------------------------ stream GEMM: split-K residual producer
@pytest.mark.parametrize("kind", ["bf16", "p14", "fp8"])
@pytest.mark.parametrize("wpb", WPBS)
def test_stream_resid_split(kind, wpb, monkeypatch):
    """EPI_RESID_SPLIT at S in {1, 2, k blocks}: h = bf16(resid + sum) and the exact per-tile sums of h^2,
    twice on the same tickets."""
    N, fp8 = 32 * wpb, kind == "fp8"
    cnt = torch.zeros(64, dtype=torch.int32, device=DEV)
    with _Stream(kind, wpb, monkeypatch) as run:
        for K in (P.RESID_FP8_K if fp8 else P.RESID_K):
            p = P.linear_probe(64, N, K, fp8="narrow" if fp8 else False)
            w = run.weight(p.w)
            for M in P.STREAM_M:
                x = P.x_frame(p.x[:M], DEV)
                h, ssp_want = P.resid_expected(p.resid[:M], p.E[:M], 16 * wpb)
                for S in _splits(K // (256 if fp8 else 128)):
                    tag = "%s wpb %d K %d M %d S %d" % (kind, wpb, K, M, S)
                    parts = torch.empty(S, M, N, dtype=F32, device=DEV)
                    for rep in range(2):
                        buf, r = _framed((M, N), BF16)
                        r.copy_(p.resid[:M])
                        ssp = torch.full((M, 2), P.SENTINEL, dtype=F32, device=DEV)
                        run(x, w, None, hip.EPI_RESID_SPLIT, S, 0, parts=parts, counters=cnt, resid=r, ssp=ssp)
                        _done(buf, r, h, "exact", tag + " residual, launch %d" % rep)
                        P.check(ssp, ssp_want, "exact", tag + " sums of squares")
                    assert int(cnt.abs().sum()) == 0, tag + ": tickets not re-armed"


@pytest.mark.parametrize("kind", ["bf16", "p14"])
@pytest.mark.parametrize("wpb", [4, 7])
def test_stream_onehot(kind, wpb, monkeypatch):
    """Row m of x is the unit vector at k_m (block and 16-byte chunk borders): the output is w[n, k_m]."""
    M, N, K = 64, 32 * wpb, 2304
    o1 = P.OneHot(M, N, K)
    assert o1.covered
    with _Stream(kind, wpb, monkeypatch) as run:
        w = run.weight(o1.w)
        buf, o = _framed((M, N), BF16)
        run(P.x_frame(o1.x, DEV), w, o, hip.EPI_BF16, 1, o.stride(0))
        o1.check(o, "%s wpb %d one-hot" % (kind, wpb))
        assert P.frame_untouched(buf, o)


# ------------------------------------------------------------------ register-streaming kernels
@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("K", P.SKINNY_K)
def test_skinny(waves, fp8, K, monkeypatch):
    """hip._skinny / hip._skinny_fp8 with 4- and 8-wave workgroups: EPI_BF16 at nt in {1, 2}, EPI_F32_PARTIAL at
    S in {1, 2, 4} (where it divides the k blocks), EPI_SWIGLU in both regimes and the residual producer
    (M <= 16)."""
    monkeypatch.setattr(hip, "SKINNY_WAVES_FORCE", waves)
    N, F, nkb = 64, 32, K // 128
    f = hip._skinny_fp8 if fp8 else hip._skinny
    p = P.linear_probe(64, N, K, fp8=fp8)
    pr = P.linear_probe(16, N, K, fp8="narrow") if fp8 else p
    w, wr = _wdev(p.w), _wdev(pr.w)
    sw = [P.swiglu_probe(64, F, K, regime, fp8=fp8) for regime in ("exact", "small")]
    sww = [_wdev(s.w) for s in sw]
    for M in P.SKINNY_M:
        tag = "waves %d fp8 %s K %d M %d" % (waves, fp8, K, M)
        x = P.x_frame(p.x[:M], DEV)
        for nt in (1, 2):
            buf, o = _framed((M, N), BF16)
            f(x, w, o, hip.EPI_BF16, nt, 1, o.stride(0))
            _done(buf, o, P.as_bf16(p.E[:M]), "exact", tag + " bf16 nt %d" % nt)
            for S in (1, 2, 4):
                if nkb % S == 0:
                    buf, o = _framed((S, M, N), F32)
                    f(x, w, o, hip.EPI_F32_PARTIAL, nt, S, o.stride(1))
                    _done(buf, o, p.parts(M, S), "exact", tag + " slabs nt %d S %d" % (nt, S))
        for s, wgu in zip(sw, sww):
            buf, o = _framed((M, F), BF16)
            f(P.x_frame(s.x[:M], DEV), wgu, o, hip.EPI_SWIGLU, 1, 1, o.stride(0))
            _done(buf, o, s.want[:M], s.rule, tag + " swiglu " + s.regime)
        if M <= 16:
            h, ssp_want = P.resid_expected(pr.resid[:M], pr.E[:M], 16)
            buf, r = _framed((M, N), BF16)
            r.copy_(pr.resid[:M])
            ssp = torch.full((M, N // 16), P.SENTINEL, dtype=F32, device=DEV)
            f(P.x_frame(pr.x[:M], DEV), wr, None, hip.EPI_SKINNY_RESID, 1, 1, 0, resid=r, ssp=ssp)
            _done(buf, r, h, "exact", tag + " residual")
            P.check(ssp, ssp_want, "exact", tag + " sums of squares")


@pytest.mark.parametrize("fp8", [False, True])
def test_skinny_one_row_x_in_lds_and_from_global(fp8):
    """One row at K = 32768: S = 1 leaves K / S > 28672, beyond the x slice the fp8 kernel keeps in LDS (x from
    global memory); S = 2 fits it."""
    N, K = 64, P.SKINNY_GLOBAL_K
    assert K // 1 > 28672 >= K // 2 and not hip.skinny_fp8_takes_norm(1, K, 1) and hip.skinny_fp8_takes_norm(1, K, 2)
    p = P.linear_probe(1, N, K, fp8=fp8)
    f = hip._skinny_fp8 if fp8 else hip._skinny
    x, w = P.x_frame(p.x, DEV), _wdev(p.w)
    buf, o = _framed((1, N), BF16)
    f(x, w, o, hip.EPI_BF16, 1, 1, o.stride(0))
    _done(buf, o, P.as_bf16(p.E), "exact", "one row, bf16")
    for S in (1, 2):
        buf, o = _framed((S, 1, N), F32)
        f(x, w, o, hip.EPI_F32_PARTIAL, 2, S, o.stride(1))
        _done(buf, o, p.parts(1, S), "exact", "one row, slabs S %d" % S)


@pytest.mark.parametrize("wpb", WPBS)
@pytest.mark.parametrize("K", P.LDS_K)
def test_skinny_lds(wpb, K):
    """hip._skinny_lds (x staged in LDS): EPI_BF16, EPI_F32_PARTIAL at S in {1, 2, k blocks} and EPI_SWIGLU."""
    N, F, nkb = 32 * wpb, 16 * wpb, K // 128
    p = P.linear_probe(64, N, K)
    w = _wdev(p.w)
    sw = [P.swiglu_probe(64, F, K, regime) for regime in ("exact", "small")]
    sww = [_wdev(s.w) for s in sw]
    for M in P.STREAM_M:
        tag = "wpb %d K %d M %d" % (wpb, K, M)
        x = P.x_frame(p.x[:M], DEV)
        buf, o = _framed((M, N), BF16)
        hip._skinny_lds(x, w, o, hip.EPI_BF16, 1, o.stride(0), wpb)
        _done(buf, o, P.as_bf16(p.E[:M]), "exact", tag + " bf16")
        for S in _splits(nkb):
            buf, o = _framed((S, M, N), F32)
            hip._skinny_lds(x, w, o, hip.EPI_F32_PARTIAL, S, o.stride(1), wpb)
            _done(buf, o, p.parts(M, S), "exact", tag + " slabs S %d" % S)
        for s, wgu in zip(sw, sww):
            buf, o = _framed((M, F), BF16)
            hip._skinny_lds(P.x_frame(s.x[:M], DEV), wgu, o, hip.EPI_SWIGLU, 1, o.stride(0), wpb)
            _done(buf, o, s.want[:M], s.rule, tag + " swiglu " + s.regime)


# ------------------------------------------------------------------ the 256 x 256-tile GEMM
@pytest.mark.parametrize("K", P.TILE_K)
@pytest.mark.parametrize("mfma32", [False, True])
def test_tile_gemm_bf16(K, mfma32):
    """hip.gemm on strided x at M in {1, 255, 256, 257, 513} x N in {16, 256, 272, 528}, both store epilogues
    (a 16-byte and an 8-byte aligned output view), 16x16 and 32x32 MFMA tiles.  K = 4096 is the rounding probe:
    sums beyond 256, where bf16 no longer holds every integer."""
    gm = hip.GEMM_GROUP_M | (hip.GEMM_MFMA32 if mfma32 else 0)
    for N in P.TILE_N:
        p = P.linear_probe(max(P.TILE_M), N, K)
        w = _wdev(p.w)
        if K == 4096 and N >= 256:
            assert float(p.E.abs().max()) > 256 and bool((P.trunc_bf16(p.E) != P.as_bf16(p.E)).any())
        for M in P.TILE_M:
            x = P.x_frame(p.x[:M], DEV)
            for off in (8, 4):
                buf, o = _framed((M, N), BF16, off)
                assert (o.data_ptr() % 16 == 0) == (off == 8)
                hip.gemm(x, w, out=o, group_m=gm)
                _done(buf, o, P.as_bf16(p.E[:M]), "exact", "K %d N %d M %d off %d mfma32 %s" % (K, N, M, off, mfma32))


@pytest.mark.parametrize("K", P.TILE_FP8_K)
@pytest.mark.parametrize("mfma32", [False, True])
def test_tile_gemm_fp8(K, mfma32):
    """hip.gemm_fp8: integer e4m3fn activations and weights with power-of-two row scales on both, and the
    two-term [hi | lo] activation, whose value is (hi + lo) xs."""
    gm = hip.GEMM_GROUP_M | (hip.GEMM_MFMA32 if mfma32 else 0)
    Mmax = max(P.TILE_M)
    xq, xs = P.fp8_rows(P.int_x(Mmax, K))
    val = xq.double() * xs.double()[:, None]
    q2, s2, val2 = P.fp8_two_term(Mmax, K)
    for N in P.TILE_N:
        w = P.fp8_weight(P.int_w(N, K))
        E, E2 = P.expected(val, w), P.expected(val2, w)
        wd = _wdev(w)
        for M in P.TILE_M:
            for off in (8, 4):
                tag = "K %d N %d M %d off %d mfma32 %s" % (K, N, M, off, mfma32)
                buf, o = _framed((M, N), BF16, off)
                hip.gemm_fp8(P.x_frame(xq[:M], DEV), xs[:M].to(DEV), wd, out=o, group_m=gm)
                _done(buf, o, P.as_bf16(E[:M]), "exact", tag)
            buf, o = _framed((M, N), BF16)
            hip.gemm_fp8(P.x_frame(q2[:M], DEV), s2[:M].to(DEV), wd, out=o, group_m=gm)
            _done(buf, o, P.as_bf16(E2[:M]), "exact", tag + " two-term")


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("mfma32", [False, True])
def test_tile_gemm_swiglu(fp8, mfma32):
    """The fused SwiGLU epilogue of hip.gemm / hip.gemm_fp8 in both gate regimes, N % 32 == 0."""
    gm = hip.GEMM_GROUP_M | (hip.GEMM_MFMA32 if mfma32 else 0)
    for K in (128, 1024):
        for F in (16, 128, 144, 272):
            for regime in ("exact", "small"):
                p = P.swiglu_probe(max(P.TILE_M), F, K, regime, fp8=fp8, xfp8=fp8)
                w = _wdev(p.w)
                for M in P.TILE_M:
                    for off in (8, 4):
                        buf, o = _framed((M, F), BF16, off)
                        if fp8:
                            xs = torch.ones(M, dtype=F32, device=DEV)
                            hip.gemm_fp8(P.x_frame(P.to_fp8(p.x[:M]), DEV), xs, w, out=o, swiglu=True, group_m=gm)
                        else:
                            hip.gemm(P.x_frame(p.x[:M], DEV), w, out=o, swiglu=True, group_m=gm)
                        _done(buf, o, p.want[:M], p.rule, "fp8 %s mfma32 %s K %d F %d M %d off %d %s"
                              % (fp8, mfma32, K, F, M, off, regime))


def test_tile_gemm_onehot():
    M, N, K = 256, 272, 1024
    o1 = P.OneHot(M, N, K, blk=64)  # the kernel's k tile: 128 bytes
    assert o1.covered
    w = _wdev(o1.w)
    for off in (8, 4):
        buf, o = _framed((M, N), BF16, off)
        hip.gemm(P.x_frame(o1.x, DEV), w, out=o)
        o1.check(o, "tile GEMM one-hot, off %d" % off)
        assert P.frame_untouched(buf, o)


# ------------------------------------------------------------------ dispatchers: the hand-off between kernels
def test_dispatch_linear():
    """hip.linear: a stream shape (the stream kernel up to 64 rows, its tall tiles up to 128, the tile GEMM above)
    and a narrow one (register-streaming kernel, tile GEMM above 64 rows)."""
    for N, K in ((11520, 384), (128, 384)):
        assert (hip.stream_config(N, K, splits=1) is not None) == (N == 11520)
        p = P.linear_probe(max(P.DISPATCH_M), N, K)
        w = _wdev(p.w)
        for M in P.DISPATCH_M:
            P.check(hip.linear(p.x[:M].to(DEV), w), P.as_bf16(p.E[:M]), "exact", "linear N %d M %d" % (N, M))


def test_dispatch_linear_parts():
    N, K, S = 128, 384, 3
    p = P.linear_probe(max(P.DISPATCH_M), N, K)
    w = _wdev(p.w)
    for M in P.DISPATCH_M:
        x = p.x[:M].to(DEV)
        P.check(hip.linear_parts(x, w, S, nt=4, kernel="stream"), p.parts(M, S), "exact", "stream parts M %d" % M)
        if M <= hip.SKINNY_MAX_M:
            for kernel in ("skinny", "lds"):
                P.check(hip.linear_parts(x, w, S, kernel=kernel), p.parts(M, S), "exact", "%s parts M %d" % (kernel, M))


def test_dispatch_linear_swiglu():
    F, K = 64, 384
    for regime in ("exact", "small"):
        p = P.swiglu_probe(max(P.DISPATCH_M), F, K, regime)
        w = _wdev(p.w)
        for M in P.DISPATCH_M:
            x = p.x[:M].to(DEV)
            small = M <= hip.SKINNY_MAX_M  # above: the stream kernel up to 128 rows, else the tile GEMM
            for kernel in ("stream", "skinny", "lds", "stream_split", "gemm") if small else ("stream", "skinny"):
                out = hip.linear_swiglu(x, w, kernel=kernel, wpb=4, splits=3)
                P.check(out, p.want[:M], p.rule, "linear_swiglu %s M %d %s" % (kernel, M, regime))


def _quantiser_rows(x):
    """x with one element per row set to 3.5 or 7: the row maximum at which the dynamic e4m3fn row quantiser's
    scale max / 448 is a power of two and every element stays exact."""
    x = x.clone()
    x[:, 7] = torch.where(torch.arange(x.shape[0]) % 2 == 0, 3.5, 7.0).to(x.dtype)
    return x


def test_dispatch_fp8_linear():
    """hip.fp8_linear: W8A16 streaming kernels up to 256 rows (64-row chunks above 64), above that the dynamic
    row quantiser and the fp8 tile GEMM."""
    N, K = 128, 512
    w = P.fp8_weight(P.int_w(N, K))
    x = _quantiser_rows(P.int_x(max(P.DISPATCH_M), K))
    P.check_exact(x, w.q.to(BF16))
    E = P.expected(x, w)
    wd = _wdev(w)
    for M in P.DISPATCH_M:
        P.check(hip.fp8_linear(x[:M].to(DEV), wd), P.as_bf16(E[:M]), "exact", "fp8_linear M %d" % M)


def test_dispatch_fp8_linear_swiglu():
    """hip.fp8_linear_swiglu; the lift of the exact regime is 448, the row maximum at which the quantiser's scale
    is 1 (above 128 rows the rows go through it)."""
    F, K = 64, 512
    for regime in ("exact", "small"):
        p = P.swiglu_probe(max(P.DISPATCH_M), F, K, regime, fp8=True, xfp8=True, lift=448.0)
        x = p.x if regime == "exact" else None
        w = _wdev(p.w)
        for M in P.DISPATCH_M:
            if x is None and M > hip.STREAM_MAX_M_SWIGLU:
                continue  # small regime: rows whose maximum is 2 do not quantise exactly
            out = hip.fp8_linear_swiglu(p.x[:M].to(DEV), w)
            P.check(out, p.want[:M], p.rule, "fp8_linear_swiglu M %d %s" % (M, regime))


@pytest.mark.parametrize("fp8", [False, True])
def test_dispatch_resid_producers(fp8):
    """hip.stream_resid and hip.skinny_resid."""
    N, K, wpb, S = 128, 512, 4, 2
    p = P.linear_probe(64, N, K, fp8="narrow" if fp8 else False)
    w = _wdev(p.w)
    for M in (1, 16, 17, 64):
        for producer, tile in (("stream", 16 * wpb), ("skinny", 16)):
            if producer == "skinny" and M > 16:
                continue
            h, ssp_want = P.resid_expected(p.resid[:M], p.E[:M], tile)
            r = p.resid[:M].to(DEV)
            x = p.x[:M].to(DEV)
            ssp = hip.stream_resid(x, w, r, wpb, S) if producer == "stream" else hip.skinny_resid(x, w, r)
            P.check(r, h, "exact", "%s_resid M %d" % (producer, M))
            P.check(ssp, ssp_want, "exact", "%s_resid sums of squares M %d" % (producer, M))
    assert all(int(t.abs().sum()) == 0 for t in hip._TILE_COUNTERS.values())


# ------------------------------------------------------------------ TP push over a group of one
@pytest.mark.parametrize("M", [7, 39])
@pytest.mark.parametrize("fp8", [False, True])
def test_stream_resid_tp_push_group_of_one_exact(fp8, M):
    """The TP-push producer over a group of one rank (as test_stream_resid_tp_push_group_of_one): the pushed
    partial is rounded to bf16 before the residual is added, so h = bf16(resid + bf16(sum))."""
    from llm_map_reduce_summarizer_amd.parallel.custom_ar import LocalPush
    N, K = 4096, 512 if fp8 else 1024
    wpb, S = (8, 2) if fp8 else (4, 4)
    p = P.linear_probe(M, N, K, fp8="narrow" if fp8 else False)
    h, ssp_want = P.resid_expected(p.resid, p.E, 16 * wpb, pushed=True)
    hl, _ = P.resid_expected(p.resid, p.E, 16 * wpb)
    assert not torch.equal(h, hl) or K < P.ROUNDING_K  # the extra rounding is visible in the expectation
    push = LocalPush(max_bytes=1 << 20)
    try:
        x, w = p.x.to(DEV), _wdev(p.w)
        for rep in range(2):  # the push epochs advance
            r = p.resid.to(DEV)
            ssp = hip.stream_resid(x, w, r, wpb, S, tp=push.push_handle())
            P.check(r, h, "exact", "TP push residual, call %d" % rep)
            P.check(ssp, ssp_want, "exact", "TP push sums of squares, call %d" % rep)
        assert push.error() == 0
    finally:
        push.close()
