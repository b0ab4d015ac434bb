"""Exact integer probes for the GEMM kernels: operands whose output is known bit for bit.

Gaussian operands and a tolerance of a few percent of the output cannot show one dropped or doubled k element,
a ring slot consumed one k block stale, two swapped 16-byte chunks or a truncating bf16 store.  With small
integer operands every product and every fp32 partial sum is an integer below 2^24, so the fp32 accumulator is
exact in ANY summation order, split-K and wave reduction.  What remains is the final fp32 -> bf16 cast, round to
nearest even by contract (csrc/kernels/common.h): the expected output is known bit for bit and any change in
the set of (m, n, k) terms changes an integer.

* ``LinearProbe``: x in {+-1, +-2}, w in {+-1, +-2, +-3} (never zero: a dropped term always changes the sum;
  two exponent values: packable as p14), optionally as an Fp8Weight with power-of-two row scales 2^(n % 7 - 3),
  distinct over any seven consecutive rows.  Built for the tallest M of a test; a test of M rows takes the
  first M rows, so the weights (and a packed copy of them) are shared by every M.
* ``OneHot``: row m of x is the unit vector at k_m, w[n, k] = ((131 n + 7 k) % 251) - 125; the output must be
  w[n, k_m] and a failure names what arrived instead.
* ``SwigluProbe``: [8 gate | 8 up]-interleaved weights in two regimes.  "exact": one k column with x = L > 0
  and gate weight 3 lifts every gate sum to >= 32, where g / (1 + exp(-g)) == g in fp32, so the output is
  bf16(G U) bit for bit.  "small": the gate rows scaled by a power of two to |G| <= 64, compared with fp64
  silu(G) U rounded to bf16 to within ONE bf16 ulp.
* residual (``resid`` / ``resid_expected``) and deferred-norm (``norm_ssq`` / ``norm_expected``) operands.
* frames: ``x_frame`` puts x into a wider and taller tensor padded with 2^60, ``out_frame`` makes an output
  view inside a sentinel-filled buffer, ``frame_untouched`` checks every element outside the view.
* mutants: the output a specific kernel mistake would produce, computed on the CPU.
  tests/test_gemm_probes_cpu.py proves that the rules below reject each of them.

Rules.  ``exact``: equality of every element.  ``ulp1``: at most one bf16 ulp from the fp64 expectation
rounded to bf16.  ulp1 is derived, not measured: the kernels' fp32 silu (|g| <= 64) and rsqrt row scale are a
few fp32 ulp (<= ~2^-18 relative) from the fp64 value, far below half a bf16 ulp (2^-9), so only a value next
to a rounding tie can land on the other neighbour -- one ulp.  No other tolerance exists in these probes.

Everything here is plain torch on the CPU.
"""

from __future__ import annotations

import functools

import torch

from llm_map_reduce_summarizer_amd.ops import reference
from llm_map_reduce_summarizer_amd.ops.reference import Fp8Weight

LIMIT = float(2 ** 24)       # fp32 holds every integer below it
POISON = 2.0 ** 60           # padding of the x backing tensor: one leaked element swamps any sum
SENTINEL = -3.0 * 2.0 ** 100  # output frames (exact in bf16 and fp32; no probe output comes near it)
KB = 128                     # the kernels' k block (bf16 elements)
X_VALUES = (-2.0, -1.0, 1.0, 2.0)
W_VALUES = (-3.0, -2.0, -1.0, 1.0, 2.0, 3.0)
LIFT_K = 5                   # the k column that lifts the gates of the exact SwiGLU regime
GATE_MIN, GATE_SMALL = 32.0, 64.0
EPS = 1e-5

# probe shapes, shared by the CPU proof (every mutant at every shape) and the GPU tests
STREAM_K = (128, 256, 384, 1024, 2304)       # 1, 2, 3, 8, 18 k blocks: ring shallower / equal / deeper than D
STREAM_M = (1, 15, 16, 17, 39, 64)
STREAM_TALL_M = (65, 96, 97, 128, 129, 200)
STREAM_FP8_K = (256, 768, 1024, 2304)
RESID_K = STREAM_K                           # the residual probes' K: per-tile sums of h^2 stay below 2^24 ...
RESID_FP8_K = (256, 512, 768)                # ... which with row scales (0.5, 1, 2: "narrow") needs a smaller K
SKINNY_M = (1, 5, 16, 17, 48, 64)
SKINNY_K = (512, 1792)                       # 4 and 14 k blocks (14: not a multiple of the wave count)
SKINNY_GLOBAL_K = 32768                      # M = 1 with K / S > 28672: x from global memory
LDS_K = (128, 640, 1024)
TILE_M = (1, 255, 256, 257, 513)
TILE_N = (16, 256, 272, 528)
TILE_K = (64, 128, 192, 1024, 4096)
TILE_FP8_K = (128, 256, 1024)
ROUNDING_K = 1024                            # from here on truncation instead of RNE is visible
DISPATCH_M = (1, 16, 17, 64, 65, 128, 129, 256, 257)


class Probe:
    """A bag of named tensors and values."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _choice(values, shape, g: torch.Generator) -> torch.Tensor:
    return torch.tensor(values, dtype=torch.float64)[torch.randint(len(values), shape, generator=g)]


def _gen(*seed) -> torch.Generator:
    s = 0
    for v in seed:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _pow2(e: torch.Tensor) -> torch.Tensor:
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double())


def row_scales(n: int, lo: int = -3, shift: int = 0) -> torch.Tensor:
    """fp64 [n] power-of-two row scales 2^((i + shift) % 7 + lo): seven consecutive rows are distinct, so no
    two rows of a 16-row block that are less than 7 apart share one and a shift by one row always shows."""
    return _pow2((torch.arange(n) + shift) % 7 + lo)


# ------------------------------------------------------------------ number formats and rules
def as_bf16(table: torch.Tensor) -> torch.Tensor:
    """The fp64 table of exact results rounded to bf16 with RNE (asserts that fp32 holds it exactly first)."""
    f = table.float()
    assert torch.equal(f.double(), table.double()), "the table is not exact in fp32"
    return f.to(torch.bfloat16)


def near_bf16(table: torch.Tensor) -> torch.Tensor:
    """fp64 -> bf16 for the ulp1 rule (through fp32: a double rounding can only pick the other neighbour of a
    tie, which the one-ulp rule covers)."""
    return table.float().to(torch.bfloat16)


def trunc_bf16(table: torch.Tensor) -> torch.Tensor:
    """The truncating store: the fp32 value with its low 16 bits cut off."""
    f = table.float()
    assert torch.equal(f.double(), table.double())
    return (f.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def bf16_ord(t: torch.Tensor) -> torch.Tensor:
    """bf16 -> int32 that orders the values, adjacent values one apart (+-0 both 0)."""
    i = t.contiguous().view(torch.int16).to(torch.int32) & 0xffff
    mag = i & 0x7fff
    return torch.where((i & 0x8000) != 0, -mag, mag)


def mismatch(got: torch.Tensor, want: torch.Tensor, rule: str = "exact") -> torch.Tensor:
    """bool, shaped like ``want``: the elements of ``got`` that break ``rule`` ("exact" or "ulp1")."""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if rule == "exact":
        return got != want  # NaN != anything: a NaN output is a mismatch
    assert rule == "ulp1" and got.dtype == torch.bfloat16
    return ((bf16_ord(got) - bf16_ord(want)).abs() > 1) | ~torch.isfinite(got.float())


def tile_any(bad: torch.Tensor) -> torch.Tensor:
    """bool [ceil(M / 16), ceil(N / 16)]: the 16 x 16 output tiles of ``bad`` [M, N] that hold a True."""
    M, N = bad.shape
    mt, nt = -(-M // 16), -(-N // 16)
    p = torch.zeros(mt * 16, nt * 16, dtype=torch.bool)
    p[:M, :N] = bad
    return p.view(mt, 16, nt, 16).any(3).any(1)


def check(got: torch.Tensor, want: torch.Tensor, rule: str = "exact", what: str = "") -> None:
    """Every element of ``got`` obeys ``rule`` against ``want`` (moved to got's device)."""
    want = want.to(got.device)
    bad = mismatch(got, want, rule)
    if bool(bad.any()):
        idx = [int(v) for v in bad.nonzero()[0]]
        raise AssertionError("%s: %d of %d elements break the %s rule; first at %s: got %r, expected %r"
                             % (what, int(bad.sum()), bad.numel(), rule, idx, float(got[tuple(idx)]),
                                float(want[tuple(idx)])))


# ------------------------------------------------------------------ frames
def x_frame(x: torch.Tensor, device=None) -> torch.Tensor:
    """``x`` [M, K] as a view (16-byte aligned rows, row stride K + 64) into a [M + 3, K + 64] tensor whose
    padding -- 32 columns on either side and 3 rows after M -- holds 2^60 (e4m3 tensors: 448, the largest)."""
    M, K = x.shape
    fp8 = x.dtype == torch.float8_e4m3fn
    back = torch.full((M + 3, K + 64), 448.0 if fp8 else POISON, dtype=torch.float32).to(x.dtype)
    back[:M, 32:32 + K] = x
    if device is not None:
        back = back.to(device)
    return back[:M, 32:32 + K]


def out_frame(shape, dtype, device, off: int = 8):
    """(buffer, view): an output view of ``shape`` ([M, N] or slabs [S, M, N]) ``off`` elements into the rows
    of a wider sentinel-filled buffer with one row (2-D) or one slab (3-D) before and after.  Slab s of a 3-D
    view starts M rows after slab s - 1, as the kernels' slab layout requires."""
    if len(shape) == 2:
        M, N = shape
        buf = torch.full((M + 2, N + 16), SENTINEL, dtype=dtype, device=device)
        return buf, buf[1:1 + M, off:off + N]
    S, M, N = shape
    buf = torch.full((S + 2, M, N + 16), SENTINEL, dtype=dtype, device=device)
    return buf, buf[1:1 + S, :, off:off + N]


def frame_untouched(buf: torch.Tensor, view: torch.Tensor) -> bool:
    """Every element of ``buf`` outside ``view`` still holds the sentinel."""
    outside = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    outside.as_strided(view.shape, view.stride(), view.storage_offset() - buf.storage_offset()).fill_(False)
    return int(outside.sum()) == buf.numel() - view.numel() and bool((buf[outside] == SENTINEL).all())


# ------------------------------------------------------------------ integer operands
def check_exact(x: torch.Tensor, w: torch.Tensor) -> None:
    """Every partial sum of x @ w^T, over any subset of k in any order, stays below 2^24 in magnitude."""
    assert float((x.double().abs() @ w.double().abs().t()).max()) < LIMIT, "partial sums may reach 2^24"


@functools.lru_cache(maxsize=None)
def int_x(M: int, K: int, seed: int = 0) -> torch.Tensor:
    return _choice(X_VALUES, (M, K), _gen(seed, 1, M, K)).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def int_w(N: int, K: int, seed: int = 0) -> torch.Tensor:
    return _choice(W_VALUES, (N, K), _gen(seed, 2, N, K)).to(torch.bfloat16)


def int_operands(M: int, N: int, K: int, seed: int = 0):
    """bf16 x [M, K] in {+-1, +-2} and w [N, K] in {+-1, +-2, +-3} from a seeded CPU generator."""
    x, w = int_x(M, K, seed), int_w(N, K, seed)
    check_exact(x, w)
    return x, w


def wd(w) -> torch.Tensor:
    """The fp64 value of a weight (bf16 tensor or Fp8Weight)."""
    return w.q.double() * w.scale.double()[:, None] if isinstance(w, Fp8Weight) else w.double()


def expected(x: torch.Tensor, w) -> torch.Tensor:
    """The fp64 table x @ w^T (integers, or integers times the power-of-two row scales of an Fp8Weight)."""
    return x.double() @ wd(w).t()


def parts(x: torch.Tensor, w, S: int) -> torch.Tensor:
    """The exact fp32 split-K slabs [S, M, N]: slab s covers k in [s K / S, (s + 1) K / S)."""
    K = x.shape[1]
    ks = K // S
    assert ks * S == K
    xd, w64 = x.double(), wd(w)
    t = torch.stack([xd[:, s * ks:(s + 1) * ks] @ w64[:, s * ks:(s + 1) * ks].t() for s in range(S)])
    f = t.float()
    assert torch.equal(f.double(), t)
    return f


def to_fp8(t: torch.Tensor) -> torch.Tensor:
    q = t.float().to(torch.float8_e4m3fn)
    assert torch.equal(q.double(), t.double()), "value not exact in e4m3fn"
    return q


def fp8_weight(w: torch.Tensor, lo: int = -3, narrow: bool = False) -> Fp8Weight:
    """``w`` (integers) as an Fp8Weight built directly: q holds the same integers, row n's scale is
    2^(n % 7 + lo) -- ``narrow``: 2^(n % 3 - 1), for the residual probes."""
    sc = _pow2(torch.arange(w.shape[0]) % 3 - 1) if narrow else row_scales(w.shape[0], lo)
    return Fp8Weight(to_fp8(w).contiguous(), sc.float().contiguous())


class LinearProbe:
    """x [Mmax, K] and w [N, K] (bf16, or Fp8Weight when ``fp8``) with the exact table ``E`` [Mmax, N];
    ``resid`` [Mmax, N] is the integer residual in +-[1, 64].  ``fp8`` "narrow": the row scales 0.5, 1, 2."""

    def __init__(self, Mmax: int, N: int, K: int, seed: int = 0, fp8=False):
        self.M, self.N, self.K, self.fp8 = Mmax, N, K, fp8
        self.x, wi = int_operands(Mmax, N, K, seed)
        self.w = fp8_weight(wi, narrow=fp8 == "narrow") if fp8 else wi
        self.E = expected(self.x, self.w)
        assert float(self.E.abs().max()) < LIMIT
        g = _gen(seed, 3, Mmax, N)
        self.resid = (torch.randint(1, 65, (Mmax, N), generator=g) *
                      (torch.randint(2, (Mmax, N), generator=g) * 2 - 1)).to(torch.bfloat16)

    def parts(self, M: int, S: int) -> torch.Tensor:
        return parts(self.x[:M], self.w, S)


@functools.lru_cache(maxsize=None)
def linear_probe(Mmax: int, N: int, K: int, seed: int = 0, fp8=False) -> LinearProbe:
    return LinearProbe(Mmax, N, K, seed, fp8)


# ------------------------------------------------------------------ residual epilogue
def resid_expected(resid: torch.Tensor, total: torch.Tensor, tile: int, pushed: bool = False):
    """(h, ssp) of residual += x @ w^T: h = bf16(resid + sum) -- ``pushed`` (TP push): bf16(resid +
    bf16(sum)), the pushed partial is rounded first -- and ssp [M, N / tile] the exact per-tile row sums of
    h^2.  Asserts that every h is a multiple of 0.5 and every sum of squares, in units of 0.25, stays below
    2^24, so the fp32 reduction is exact in any order."""
    if pushed:
        total = as_bf16(total).double()
    h = as_bf16(resid.double() + total)
    M, N = h.shape
    u = 1.0 if torch.equal(h.double().round(), h.double()) else 2.0  # h in units of 1 / u
    assert torch.equal((u * h.double()).round(), u * h.double())
    ssp = h.double().pow(2).view(M, N // tile, tile).sum(-1)
    assert u * u * float(ssp.max()) < LIMIT, "a per-tile row sum of squares reaches 2^24: use a smaller K"
    return h, ssp.float()


# ------------------------------------------------------------------ deferred-norm consumer
def norm_ssq(M: int, K: int, tiles: int = 32) -> torch.Tensor:
    """fp32 [M, tiles], integer valued (the fp32 reduction is exact in any order) and uneven over the tiles;
    row m's mean of squares sum / K is 4^(m % 5): neighbouring rows differ by factors of 4 (or 256)."""
    assert K % tiles == 0 and K // tiles >= 4 and tiles % 4 == 0
    mean = _pow2(2 * (torch.arange(M) % 5))
    t = torch.arange(tiles)
    wobble = ((t % 2) * 2 - 1) * ((t // 2) % 2 + 1)  # -1 +1 -2 +2 ...: sums to zero over every 4 tiles
    ssq = (mean * (K // tiles))[:, None] + wobble[None, :].double()
    assert bool((ssq > 0).all()) and torch.equal(ssq.sum(1), mean * K) and float(ssq.sum(1).max()) < LIMIT
    return ssq.float()


def norm_scale(ssq: torch.Tensor, K: int, eps: float = EPS) -> torch.Tensor:
    """fp64 [M, 1]: rsqrt(mean + eps) of every row."""
    return torch.rsqrt(ssq.double().sum(1, keepdim=True) / K + eps)


def norm_expected(E: torch.Tensor, ssq: torch.Tensor, K: int) -> torch.Tensor:
    """bf16(sum * rsqrt(mean + eps)) from fp64 (ulp1 rule)."""
    return near_bf16(E * norm_scale(ssq, K))


# ------------------------------------------------------------------ SwiGLU
def silu64(g: torch.Tensor) -> torch.Tensor:
    return g / (1.0 + torch.exp(-g))


def _no_zero_sums(x: torch.Tensor, w: torch.Tensor, g: torch.Generator) -> None:
    """Redraw single elements of w (in place, from W_VALUES) until no element of x @ w^T is zero."""
    xd, K = x.double(), x.shape[1]
    for n in range(w.shape[0]):
        tries = 0
        while bool((xd @ w[n].double() == 0).any()):
            k = int(torch.randint(K, (1,), generator=g))
            others = [v for v in W_VALUES if v != float(w[n, k])]
            w[n, k] = others[int(torch.randint(len(others), (1,), generator=g))]
            tries += 1
            assert tries < 200


class SwigluProbe:
    """x [Mmax, K], the [8 gate | 8 up]-interleaved weight ``w`` [2 F, K] (bf16 or Fp8Weight), the fp64 gate /
    up tables ``G`` / ``U`` (with the row scales) and ``want`` (bf16) under ``rule``.  ``xfp8``: x must be exact
    in e4m3fn too (the tile GEMM's fp8 path); ``lift``: a fixed lift value instead of the smallest power of two
    (448: the row maximum at which the dynamic row quantiser's scale is exactly 1).

    ``nonzero`` (small regime): no gate or up sum is exactly zero -- the precondition of the split-K SwiGLU
    that consumes a deferred norm.  That kernel multiplies every split's partial tile by the fp32 row scale
    BEFORE the last arriver sums them, so its error is a few fp32 ulp of the PARTIALS: relative to a sum >= 1
    unit that is at most S max|partial| 2^-24 < 2^-12 at these shapes, still below half a bf16 ulp, but where
    the exact sum is zero a residue of that size remains and no relative bound exists.  Single weights are
    redrawn from the same value set until no sum is zero."""

    def __init__(self, Mmax: int, F: int, K: int, regime: str, seed: int = 0, fp8: bool = False,
                 xfp8: bool = False, lift: float = 0.0, nonzero: bool = False):
        assert regime in ("exact", "small") and F % 8 == 0
        self.M, self.F, self.K, self.regime, self.fp8 = Mmax, F, K, regime, fp8
        x = int_x(Mmax, K, seed + 10).clone()
        wg, wu = int_w(F, K, seed + 11).clone(), int_w(F, K, seed + 12).clone()
        if nonzero:
            assert regime == "small"
            g = _gen(seed, 4, Mmax, F, K)
            _no_zero_sums(x, wg, g)
            _no_zero_sums(x, wu, g)
        wg0 = wg.clone()
        lo = 0 if regime == "exact" else -3  # exact regime: scales >= 1 keep the scaled gate >= 32
        sg = row_scales(F, lo) if fp8 else torch.ones(F, dtype=torch.float64)
        su = row_scales(F, lo, 3) if fp8 else torch.ones(F, dtype=torch.float64)
        if regime == "exact":
            x[:, LIFT_K] = 0.0
            need = float((x.double() @ wg.double().t()).abs().max()) + GATE_MIN
            L = lift if lift else 1.0
            while 3.0 * L < need and not lift:
                L *= 2.0
            assert 3.0 * L >= need
            assert L <= 256.0 or L == lift or not xfp8, "the lift of an e4m3fn activation must stay exact"
            x[:, LIFT_K] = L      # the same sign in every row of x ...
            wg[:, LIFT_K] = 3.0   # ... and of the gate weight
        check_exact(x, wg)
        check_exact(x, wu)
        G, U = x.double() @ wg.double().t(), x.double() @ wu.double().t()
        if regime == "exact":
            assert float(G.min()) >= GATE_MIN and float((G * U).abs().max()) < LIMIT
            self.rule = "exact"
        else:
            p = 0
            while float((G * sg).abs().max()) * 2.0 ** -p > GATE_SMALL:
                p += 1
            if fp8:
                sg = sg * 2.0 ** -p
            else:
                wg = (wg.double() * 2.0 ** -p).to(torch.bfloat16)
                assert torch.equal(wg.double() * 2.0 ** p, wg0.double())
                G = G * 2.0 ** -p
            self.rule = "ulp1"
        self.x = x
        self.G, self.U = G * sg, U * su
        assert regime == "exact" or float(self.G.abs().max()) <= GATE_SMALL
        assert not nonzero or (bool((self.G != 0).all()) and bool((self.U != 0).all()))
        wq = reference.interleave_gate_up(wg, wu).contiguous()
        if fp8:
            sc = reference.interleave_gate_up(sg[:, None], su[:, None])[:, 0]
            self.w = Fp8Weight(to_fp8(wq).contiguous(), sc.float().contiguous())
            assert torch.equal(self.w.scale.double(), sc)
        else:
            self.w = wq
        g2, u2 = reference.split_gate_up(expected(x, self.w))
        assert torch.equal(g2, self.G) and torch.equal(u2, self.U)
        self.want = self.expect(self.G, self.U)

    def expect(self, G: torch.Tensor, U: torch.Tensor) -> torch.Tensor:
        """bf16 output of gate / up tables under this probe's regime."""
        return as_bf16(G * U) if self.regime == "exact" else near_bf16(silu64(G) * U)

    def norm_want(self, ssq: torch.Tensor) -> torch.Tensor:
        """The first len(ssq) rows through a deferred norm: silu(G s) (U s) with the fp64 row scale s <= 1 (ulp1)."""
        s = norm_scale(ssq, self.K)
        M = ssq.shape[0]
        assert float(s.max()) <= 1.0
        return near_bf16(silu64(self.G[:M] * s) * (self.U[:M] * s))


@functools.lru_cache(maxsize=None)
def swiglu_probe(Mmax: int, F: int, K: int, regime: str, seed: int = 0, fp8: bool = False,
                 xfp8: bool = False, lift: float = 0.0, nonzero: bool = False) -> SwigluProbe:
    return SwigluProbe(Mmax, F, K, regime, seed, fp8, xfp8, lift, nonzero)


# ------------------------------------------------------------------ fp8 activations (the tile GEMM's fp8 path)
def fp8_rows(x: torch.Tensor):
    """(xq e4m3fn [M, K], xs fp32 [M]): integer rows with the power-of-two row scales 2^(m % 5 - 2)."""
    return to_fp8(x), _pow2(torch.arange(x.shape[0]) % 5 - 2).float()


def fp8_two_term(M: int, K: int, seed: int = 0):
    """(xq [M, 2 K] = [hi | 16 lo], xs [M], value fp64 [M, K] = (hi + lo) xs): the two-term activation, whose
    lo half the GEMM scales by 2^-4; hi and lo are integers in {+-1, +-2}."""
    hi, lo = int_x(M, K, seed + 20), int_x(M, K, seed + 21)
    xq, xs = fp8_rows(torch.cat([hi.double(), 16.0 * lo.double()], 1))
    return xq, xs, (hi.double() + lo.double()) * xs.double()[:, None]


# ------------------------------------------------------------------ one-hot probe
def onehot_ks(K: int, blk: int = KB):
    """The probed k: first and last element of the first, second and last k block, and both sides of every
    8-element (16-byte) chunk border of one block (the second, or the only one)."""
    nb = K // blk
    ks = []
    for b in sorted({0, min(1, nb - 1), nb - 1}):
        ks += [b * blk, b * blk + blk - 1]
    b = min(1, nb - 1)
    for c in range(8, blk, 8):
        ks += [b * blk + c - 1, b * blk + c]
    return ks


class OneHot:
    """Row m of x is the unit vector at k_m = ks[m % len(ks)]; the output must be w[n, k_m] exactly."""

    def __init__(self, M: int, N: int, K: int, blk: int = KB):
        self.M, self.N, self.K = M, N, K
        ks = onehot_ks(K, blk)
        self.km = torch.tensor([ks[m % len(ks)] for m in range(M)])
        self.covered = len(set(self.km.tolist())) == len(set(ks))
        self.x = torch.zeros(M, K, dtype=torch.bfloat16)
        self.x[torch.arange(M), self.km] = 1.0
        n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
        self.wi = (131 * n + 7 * k) % 251 - 125
        self.w = self.wi.to(torch.bfloat16)
        assert torch.equal(self.w.double(), self.wi.double())
        self.want = self.w[:, self.km].t().contiguous()

    def check(self, got: torch.Tensor, what: str = "") -> None:
        got = got.cpu()
        bad = mismatch(got, self.want)
        if not bool(bad.any()):
            return
        m, n = [int(v) for v in bad.nonzero()[0]]
        v, km = float(got[m, n]), int(self.km[m])
        same_row = (self.wi[n].double() == v).nonzero().flatten()
        same_col = (self.wi[:, km].double() == v).nonzero().flatten()
        k_near = int(same_row[(same_row - km).abs().argmin()]) if same_row.numel() else None
        n_near = int(same_col[(same_col - n).abs().argmin()]) if same_col.numel() else None
        raise AssertionError(
            "%s: %d of %d one-hot outputs are wrong; first: out[m=%d, n=%d] = %r, expected w[n=%d, k=%d] = %r; "
            "the value is w[n=%d, k=%s] (nearest k in the same weight row) and w[n=%s, k=%d] (nearest row at "
            "the same k)" % (what, int(bad.sum()), bad.numel(), m, n, v, n, km, float(self.want[m, n]), n,
                             k_near, n_near, km))


# ------------------------------------------------------------------ mutants: what a specific mistake would output
def mut_drop_k(x, w, k: int, E=None) -> torch.Tensor:
    """k element ``k`` dropped (``E``: the precomputed exact table of x and w)."""
    return (expected(x, w) if E is None else E) - torch.outer(x[:, k].double(), wd(w)[:, k])


def mut_double_k(x, w, k: int, E=None) -> torch.Tensor:
    """k element ``k`` counted twice."""
    return (expected(x, w) if E is None else E) + torch.outer(x[:, k].double(), wd(w)[:, k])


def mut_stale_block(x, w, kb: int, blk: int = KB, E=None) -> torch.Tensor:
    """k block ``kb`` of x paired with block kb + 1 of w (a ring slot consumed one block off)."""
    xd, w64 = x.double(), wd(w)
    a, b = slice(kb * blk, (kb + 1) * blk), slice((kb + 1) * blk, (kb + 2) * blk)
    return (expected(x, w) if E is None else E) + xd[:, a] @ (w64[:, b] - w64[:, a]).t()


def mut_swap_chunks(x, w, kb: int, c0: int, c1: int, blk: int = KB, chunk: int = 8, E=None) -> torch.Tensor:
    """Two 16-byte chunks (``chunk`` elements) of every W row swapped inside k block ``kb`` (a wrong swizzle)."""
    xd, w64 = x.double(), wd(w)
    a = slice(kb * blk + c0 * chunk, kb * blk + (c0 + 1) * chunk)
    b = slice(kb * blk + c1 * chunk, kb * blk + (c1 + 1) * chunk)
    d = w64[:, b] - w64[:, a]
    return (expected(x, w) if E is None else E) + xd[:, a] @ d.t() - xd[:, b] @ d.t()


def mut_ragged_clamp(E: torch.Tensor) -> torch.Tensor:
    """Row M - 1 replicated into row M - 2 (a ragged-M clamp one row early); applies to the tile of row M - 2."""
    out = E.clone()
    out[-2] = E[-1]
    return out


def mut_tile_shift(E: torch.Tensor, by: int = 4) -> torch.Tensor:
    """Every 16-column output tile rotated by ``by`` columns."""
    M, N = E.shape
    return torch.roll(E.view(M, N // 16, 16), by, dims=2).reshape(M, N)


def mut_swap_slabs(p: torch.Tensor, s: int = 0) -> torch.Tensor:
    """Slabs s and s + 1 of the split-K output exchanged."""
    out = p.clone()
    out[s], out[s + 1] = p[s + 1], p[s]
    return out


def mut_scale_shift(x, w: Fp8Weight) -> torch.Tensor:
    """fp8 weight row scales shifted by one row."""
    return x.double() @ (w.q.double() * torch.roll(w.scale.double(), 1)[:, None]).t()


def mut_norm_neighbour(E: torch.Tensor, ssq: torch.Tensor, K: int) -> torch.Tensor:
    """The deferred-norm row scale taken from the neighbouring row."""
    return near_bf16(E * torch.roll(norm_scale(ssq, K), 1, 0))


def mut_swap_gate_up(p: SwigluProbe, M: int) -> torch.Tensor:
    """Gate and up exchanged within every 16-row weight block."""
    return near_bf16(silu64(p.U[:M]) * p.G[:M])


def mut_last_split_missing(resid, slabs: torch.Tensor, tile: int):
    """The last split left out of the residual sum."""
    return resid_expected(resid, slabs[:-1].double().sum(0), tile)


def old_rule_bad(got: torch.Tensor, want: torch.Tensor, atol: float = 2e-2, rtol: float = 2e-2) -> torch.Tensor:
    """The tolerance of the Gaussian-data tests (tests/test_kernels_gpu.py ``_close(..., 2e-2)``): the elements
    with |got - want| > atol + rtol |want|."""
    return (got.double() - want.double()).abs() > atol + rtol * want.double().abs()
