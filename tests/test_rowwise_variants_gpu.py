"""The row-wise kernels (norm.hip, rope_kv.hip, act.hip, the plain sampler) at the instantiations and edges
the launchers can select but no other kernel test runs: every VPT of the norms (D up to 16384, partial last
vector passes, full and partial VPT = 1 rows), strided x / out, a row where eps dominates, more than four
split-K slabs; the D = 64 RoPE kernel, a bf16 cache with P != 64, write_cache = 0, padded rows, seq_idx < 0;
swiglu beyond one shape, the embed id clamp, kv_scatter's skipped rows; the sampler's V % 8 tail, ld > V, ties
and the two-shard path.

The reference is fp64 on the CPU from the same bf16 inputs.  Bounds: a bf16 output is within 2^-8 |y| of the
fp64 value y (round-to-nearest is within half a unit in the last place, at most 2^-8 / (1 + 2^-8) relative;
the fp32 arithmetic before it adds about 1e-6 relative, inside the remaining 2^-16); an e4m3 output within
half a step, 2^-4 |y| (normal) + 2^-10 s (subnormal), with 2 % slack for the kernel's fp32 y."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from llm_map_reduce_summarizer_amd.ops import hip, reference  # noqa: E402

DEV = "cuda:0"
EPS = 1e-5
BF16 = 2.0 ** -8


def _randn(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _bf(t):
    return t.to(torch.bfloat16).to(DEV)


def _grid(*shape, seed, scale=0.7):
    """fp32 multiples of 2^-6 below 2^5: sums of a few dozen of them are exact in fp32 in any order."""
    return torch.round(_randn(*shape, seed=seed, scale=scale) * 64) / 64


def _within(out, y64, rel, absolute=0.0, what=""):
    o = out.detach().double().cpu()
    err = (o - y64).abs()
    tol = rel * y64.abs() + absolute
    bad = (err > tol) | ~torch.isfinite(o)
    assert not bool(bad.any()), "%s: %d of %d beyond the bound, worst err / tol %.3f" % (
        what, int(bad.sum()), bad.numel(), float((err / tol.clamp_min(1e-300)).max()))


def _rms64(h, w, eps=EPS):
    h, w = h.double().cpu(), w.double().cpu()
    return h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps) * w


def _strided(t, fill):
    """(buffer, view): ``t`` copied into the middle of rows 16 elements longer (row stride D + 16, the view
    16 bytes into the row), the 8 columns on either side filled with ``fill``."""
    buf = torch.full((t.shape[0], t.shape[1] + 16), fill, dtype=t.dtype, device=t.device)
    view = buf[:, 8:8 + t.shape[1]]
    view.copy_(t)
    return buf, view


def _sentinels_intact(buf, fill):
    return bool((buf[:, :8] == fill).all()) and bool((buf[:, -8:] == fill).all())


# VPT 1 (partial 16 / 264 / 272, full 2048), 2 (3072: partial last pass), 4 (5120: partial), 8 (12288: partial;
# 16384: full)
NORM_D = [16, 272, 2048, 3072, 5120, 12288, 16384]
NORM_MODES = ["plain", "strided", "small"]


def _norm_inputs(T, D, mode):
    x = _randn(T, D, seed=100 + D) * (1e-3 if mode == "small" else 1.0)  # small: eps = 1e-5 dominates mean(x^2)
    return _bf(x), _bf(_randn(T, D, seed=200 + D)), _bf(_randn(D, seed=300 + D) + 1)


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("D", [8, 264] + NORM_D)
@pytest.mark.parametrize("mode", NORM_MODES)
def test_rmsnorm_variants(T, D, mode):
    x, _, w = _norm_inputs(T, D, mode)
    if mode == "strided":
        _, xv = _strided(x, 7.0)
        obuf, ov = _strided(torch.zeros_like(x), -3.0)
        out = hip.rmsnorm(xv, w, EPS, out=ov)
        assert _sentinels_intact(obuf, -3.0)
    else:
        out = hip.rmsnorm(x, w, EPS)
    _within(out, _rms64(x, w), BF16, what="rmsnorm")


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("D", [8, 264] + NORM_D)
@pytest.mark.parametrize("mode", NORM_MODES)
def test_add_rmsnorm_variants(T, D, mode):
    x, r, w = _norm_inputs(T, D, mode)
    if mode == "small":
        r = (r.float() * 1e-3).to(torch.bfloat16)
    want_r = (x.float() + r.float()).to(torch.bfloat16)
    r1 = r.clone()
    if mode == "strided":
        _, xv = _strided(x, 7.0)
        obuf, ov = _strided(torch.zeros_like(x), -3.0)
        out = hip.add_rmsnorm(xv, r1, w, EPS, out=ov)
        assert _sentinels_intact(obuf, -3.0)
    else:
        out = hip.add_rmsnorm(x, r1, w, EPS)
    assert torch.equal(r1, want_r)  # one correctly rounded fp32 add, then round-to-nearest-even, on both sides
    _within(out, _rms64(r1, w), BF16, what="add_rmsnorm")


def _check_fp8(q, s, y64, split):
    """q e4m3 [T, D] (or two-term [T, 2 D]) with row scales s against the fp64 rows y64."""
    T, D = y64.shape
    s64 = s.double().cpu()
    want_s = y64.abs().amax(-1).clamp_min(1e-12) / 448.0
    assert bool(torch.isfinite(s64).all()) and bool(((s64 - want_s).abs() <= 1e-3 * want_s).all()), (s64, want_s)
    qf = q.float().double().cpu()
    sc = s64[:, None]
    if split:
        _within(sc * (qf[:, :D] + qf[:, D:] / 16.0), y64, 1.02 * 2.0 ** -8, 1.02 * 2.0 ** -14 * sc, "two-term e4m3")
    _within(sc * qf[:, :D], y64, 1.02 * 2.0 ** -4, 1.02 * 2.0 ** -10 * sc, "e4m3")


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("D", NORM_D)
@pytest.mark.parametrize("mode", NORM_MODES)
@pytest.mark.parametrize("variant", ["plain", "residual", "split"])
def test_rmsnorm_fp8_variants(T, D, mode, variant):
    x, r, w = _norm_inputs(T, D, mode)
    if mode == "small":
        r = (r.float() * 1e-3).to(torch.bfloat16)
    xin = _strided(x, 7.0)[1] if mode == "strided" else x
    if variant == "residual":
        r1 = r.clone()
        q, s = hip.rmsnorm_fp8(xin, w, EPS, residual=r1)
        assert torch.equal(r1, (x.float() + r.float()).to(torch.bfloat16))
        h = r1
    else:
        q, s = hip.rmsnorm_fp8(xin, w, EPS, split=variant == "split")
        h = x
    assert q.shape == (T, 2 * D if variant == "split" else D) and s.shape == (T,)
    _check_fp8(q, s, _rms64(h, w), variant == "split")


@pytest.mark.parametrize("split", [False, True])
def test_rmsnorm_fp8_zero_row(split):
    """An all-zero row: a finite scale (the 1e-12 floor) and all-zero bytes -- also under the negative weights
    among these (0 x w = -0 would be the byte 0x80)."""
    T, D = 3, 272
    x, _, w = _norm_inputs(T, D, "plain")
    x[1] = 0
    assert bool((w < 0).any())
    q, s = hip.rmsnorm_fp8(x, w, EPS, split=split)
    assert bool(torch.isfinite(s).all()) and float(s[1]) > 0
    zero_row = q[1].view(torch.uint8).cpu()
    print("non-zero bytes of the zero row:", sorted(set(zero_row[zero_row != 0].tolist())))
    assert int(zero_row.count_nonzero()) == 0
    _check_fp8(q, s, _rms64(x, w), split)


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("D", [264, 4096, 12288])
@pytest.mark.parametrize("S", [1, 4, 5, 8, 9, 16])  # > 4: the batched second loop (one, two, three more batches)
def test_add_rmsnorm_parts_variants(S, T, D):
    parts = _grid(S, T, D, seed=400 + S).to(DEV)
    r = _bf(_grid(T, D, seed=401, scale=1.0))
    w = _bf(_randn(D, seed=402) + 1)
    r1 = r.clone()
    out = hip.add_rmsnorm_parts(parts, r1, w, EPS)
    want = (parts.double().cpu().sum(0) + r.double().cpu())
    rounded = want.to(torch.bfloat16).double()
    ulp = 2.0 ** (torch.floor(torch.log2(rounded.abs().clamp_min(2.0 ** -126))) - 7)
    assert bool(((r1.double().cpu() - rounded).abs() <= ulp).all())
    _within(out, _rms64(r1, w), BF16, what="add_rmsnorm_parts")


def test_norm_host_checks():
    """A bad call raises ValueError before any launch."""
    T = 2
    w = torch.ones(2 * 4096, dtype=torch.bfloat16, device=DEV)
    parts = torch.zeros(2, T, 4096, device=DEV)
    r = torch.zeros(T, 4096, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError):
        hip.add_rmsnorm_parts(parts, r, w[::2], EPS)                         # w not contiguous
    with pytest.raises(ValueError):
        hip.add_rmsnorm_parts(parts, r, w[:4096], EPS, out=torch.empty(T + 1, 4096, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(ValueError):
        hip.add_rmsnorm_parts(parts, r, w[:4096], EPS, out=torch.empty(T, 4096 + 8, dtype=torch.bfloat16, device=DEV))
    big = 16384 + 8
    with pytest.raises(ValueError):
        hip.add_rmsnorm_parts(torch.zeros(1, T, big, device=DEV), torch.zeros(T, big, dtype=torch.bfloat16, device=DEV),
                              torch.ones(big, dtype=torch.bfloat16, device=DEV), EPS)
    with pytest.raises(ValueError):
        hip.add_rmsnorm(r.clone(), r, w[::2], EPS)                            # w not contiguous
    torch.cuda.synchronize()
    assert float(r.abs().sum()) == 0  # nothing ran


# ------------------------------------------------------------------ rope_kv / rope_kv_parts
def _rope_case(hq, hkv, d, page, S=None, write_cache=True, pad=0, neg=True):
    """Runs rope_kv (S None) or rope_kv_parts (S slabs) over 7 tokens of 2 sequences (one token with
    seq_idx < 0 when ``neg``) on sentinel-filled bf16 caches and checks everything it wrote or left alone."""
    W = (hq + 2 * hkv) * d
    half = d // 2
    pos = torch.tensor([0, page - 1, page, 2 * page + 3, 5, 3 * page - 1, 7], dtype=torch.int32)
    sidx = torch.tensor([0, 0, 0, 0, 1, 1, -1 if neg else 1], dtype=torch.int32)
    T = pos.numel()
    bt = torch.tensor([[3, 5, 1, 7], [2, 6, 4, 0]], dtype=torch.int32)
    cs = reference.rope_cos_sin(4 * page, d, 500000.0)
    k0 = torch.full((8, hkv, page, d), 0.5, dtype=torch.bfloat16, device=DEV)
    v0 = torch.full((8, hkv, page, d), -0.25, dtype=torch.bfloat16, device=DEV)
    k1, v1 = k0.clone(), v0.clone()
    dev = lambda t: t.to(DEV)  # noqa: E731
    if S is None:
        src = _randn(T, W, seed=500 + d + page).to(torch.bfloat16)
        buf = torch.full((T, W + pad), 9.0, dtype=torch.bfloat16, device=DEV)
        out = buf[:, :W]
        out.copy_(src)
        x64 = src.double()
        # the whole buffer: rows W + pad long (row_stride > width), the pad columns must stay
        hip.rope_kv(buf, dev(pos), dev(sidx), dev(bt), k1 if write_cache else None, v1 if write_cache else None,
                    dev(cs), hq, hkv, d, page, write_cache=write_cache)
    else:
        parts = _grid(S, T, W, seed=600 + S)
        x64 = parts.double().sum(0)  # exact, and exact in fp32 in any order
        buf = torch.full((T, W + pad), 9.0, dtype=torch.bfloat16, device=DEV)
        out = buf[:, :W]
        hip.rope_kv_parts(dev(parts), dev(pos), dev(sidx), dev(bt), k1, v1, dev(cs), hq, hkv, d, page, out=out)
    torch.cuda.synchronize()
    if pad:
        assert bool((buf[:, W:] == 9.0).all())  # the pad columns of the rows
    o = out.cpu()
    # rotated Q and K heads against fp64 (the table's fp32 cos / sin are the kernel's inputs too)
    c = cs[pos.long()].double()
    cos, sin = c[..., 0][:, None, :], c[..., 1][:, None, :]
    qk = x64[:, : (hq + hkv) * d].view(T, hq + hkv, d)
    a, b = qk[..., :half], qk[..., half:]
    got = o[:, : (hq + hkv) * d].view(T, hq + hkv, d).double()
    for g_, want, mag in ((got[..., :half], a * cos - b * sin, (a * cos).abs() + (b * sin).abs()),
                          (got[..., half:], b * cos + a * sin, (b * cos).abs() + (a * sin).abs())):
        assert bool(((g_ - want).abs() <= BF16 * mag).all()), float(((g_ - want).abs() / mag.clamp_min(1e-30)).max())
    # V columns: the input rows (parts: the bf16 rounding of the exact slab sum), bit for bit
    assert torch.equal(o[:, (hq + hkv) * d:], x64[:, (hq + hkv) * d:].to(torch.bfloat16))
    # the cache: every cached row is the row's K / V columns bit for bit (the kernel stores the same packed
    # vector to both places); rows with seq_idx < 0 and every other slot keep the sentinel
    want_k, want_v = k0.cpu(), v0.cpu()
    if write_cache:
        keep = sidx >= 0
        pg = bt[sidx[keep].long(), (pos[keep] // page).long()].long()
        sl = (pos[keep] % page).long()
        want_k[pg, :, sl] = o[keep][:, hq * d: (hq + hkv) * d].reshape(-1, hkv, d)
        want_v[pg, :, sl] = o[keep][:, (hq + hkv) * d:].reshape(-1, hkv, d)
    assert torch.equal(k1.cpu(), want_k) and torch.equal(v1.cpu(), want_v)


@pytest.mark.parametrize("page", [16, 64])
@pytest.mark.parametrize("pad", [0, 24])
def test_rope_kv_d64(page, pad):
    _rope_case(4, 2, 64, page, pad=pad)


@pytest.mark.parametrize("d", [64, 128])
def test_rope_kv_small_page_bf16_cache(d):
    _rope_case(8, 2, d, 16, pad=8)


@pytest.mark.parametrize("d", [64, 128])
def test_rope_kv_without_cache_write(d):
    _rope_case(4, 2, d, 64, write_cache=False, pad=16)


@pytest.mark.parametrize("S", [5, 8, 16])
@pytest.mark.parametrize("d,page", [(128, 64), (64, 16)])
def test_rope_kv_parts_many_slabs(S, d, page):
    _rope_case(4, 2, d, page, S=S, pad=8 if S == 8 else 0)


def test_kv_scatter_skips_and_small_page():
    hkv, d, P, n = 2, 128, 16, 9
    rows = _bf(_randn(n, 2, hkv, d, seed=700))
    page = torch.tensor([3, -1, 1, 1, -1, 5, -1, 2, 3], dtype=torch.int32)
    slot = torch.tensor([0, 4, 15, 7, 0, 8, 9, 1, 15], dtype=torch.int32)
    k0 = torch.full((7, hkv, P, d), 0.5, dtype=torch.bfloat16, device=DEV)
    v0 = torch.full((7, hkv, P, d), -0.25, dtype=torch.bfloat16, device=DEV)
    k1, v1 = k0.clone(), v0.clone()
    hip.kv_scatter(rows, page.to(DEV), slot.to(DEV), k1, v1)
    keep = page >= 0
    want_k, want_v = k0.cpu(), v0.cpu()
    want_k[page[keep].long(), :, slot[keep].long()] = rows.cpu()[keep][:, 0]
    want_v[page[keep].long(), :, slot[keep].long()] = rows.cpu()[keep][:, 1]
    assert torch.equal(k1.cpu(), want_k) and torch.equal(v1.cpu(), want_v)


# ------------------------------------------------------------------ swiglu, embed
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("F", [16, 2064, 14336])  # 2064 = 258 vectors: past one block; 14336: Llama-3-8B
def test_swiglu_variants(T, F):
    gu = _bf(_randn(T, 2 * F, seed=800 + F, scale=2.0))
    g, u = reference.split_gate_up(gu.double().cpu())
    y64 = g * torch.sigmoid(g) * u
    out = hip.swiglu(gu)
    err = (out.double().cpu() - y64).abs() / (BF16 * y64.abs() + 1e-6)
    print("swiglu T=%d F=%d: worst err / bound %.3f" % (T, F, float(err.max())))
    _within(out, y64, BF16, 1e-6, "swiglu")


@pytest.mark.parametrize("D", [8, 4104])  # 4104 = 513 vectors: a third pass of the 256 threads, one lane wide
def test_embed_clamps_ids(D):
    V = 50
    table = _bf(_randn(V, D, seed=900 + D))
    ids = torch.tensor([3, -5, V, 2 ** 31 - 1, 0, V - 1, -2 ** 31], dtype=torch.int32, device=DEV)
    rows = torch.tensor([3, 0, V - 1, V - 1, 0, V - 1, 0], device=DEV)
    assert torch.equal(hip.embed(ids, table), table[rows])


# ------------------------------------------------------------------ plain sampler
class _St:
    def __init__(self, B, temps, seeds, positions):
        i32 = dict(dtype=torch.int32, device=DEV)
        self.next_ids = torch.zeros(B, **i32)
        self.positions = torch.tensor(positions, **i32)
        self.gen_count = torch.zeros(B, **i32)
        self.max_new = torch.full((B,), 100, **i32)
        self.out_tokens = torch.zeros(B, 8, **i32)
        self.done = torch.zeros(B, **i32)
        self.result = torch.zeros(B, dtype=torch.int64, device=DEV)
        self.temps = torch.tensor(temps, dtype=torch.float32, device=DEV)
        self.seeds = torch.tensor(seeds, dtype=torch.int64, device=DEV)
        self.eos = torch.full((4,), -1, **i32)


TEMPS, SEEDS, POS0 = [0.0, 0.0, 0.0, 0.3, 1.0], [1, 2, 3, 4, 5], [5, 0, 17, 4000, 9]
TRAP = 30000.0  # in the ld - V columns past the row: reading one would win every argmax


def _sampler_logits(V, ld):
    """bf16 [5, V] view of a [5, ld] buffer.  Row 1: the maximum twice, at V // 3 and in the last column (the
    V % 8 tail where there is one) -- the lower index must win; row 2: the maximum only in the last column."""
    buf = torch.full((5, ld), TRAP, dtype=torch.bfloat16)
    logits = buf[:, :V]
    logits.copy_(_randn(5, V, seed=1000 + V, scale=2.0).to(torch.bfloat16))
    top = float(logits.float().max()) + 1.0
    logits[1, V // 3] = top
    logits[1, V - 1] = top
    logits[2, V - 1] = top
    buf = buf.to(DEV)
    return buf, buf[:, :V]


def _check_tokens(got, logits, pos):
    V = logits.shape[1]
    for b in range(5):
        row = logits[b].float().cpu()
        if TEMPS[b] > 0:  # Gumbel rows: the same winner, or a near-tie within the fast log's rounding
            row = row / TEMPS[b] + reference.gumbel_noise(SEEDS[b], pos[b], V)
            assert int(got[b]) == int(torch.argmax(row)) or row[int(got[b])] >= row.max() - 1e-3
        else:  # greedy rows: the lowest index of the exact maximum
            assert int(got[b]) == int((row == row.max()).nonzero()[0])


SAMPLER_SHAPES = [(7, 8), (1000, 1000), (1001, 1008), (128256, 128264)]


@pytest.mark.parametrize("V,ld", SAMPLER_SHAPES)
def test_sampler_plain_tail_stride_and_ties(V, ld):
    buf, logits = _sampler_logits(V, ld)
    assert logits.stride(0) == ld
    st = _St(5, TEMPS, SEEDS, POS0)
    for step in range(2):  # the second launch needs the first to have re-zeroed ``result``
        pos = st.positions.cpu().tolist()
        assert pos == [p + step for p in POS0]
        hip.sample(logits, st)
        _check_tokens(st.out_tokens[:, step].cpu(), logits, pos)
        assert int(st.result.abs().sum()) == 0
    assert st.gen_count.cpu().tolist() == [2] * 5
    assert int(st.out_tokens[1, 0]) == V // 3 and int(st.out_tokens[2, 0]) == V - 1


def _umax_(keys, other):
    """In place unsigned max of two int64 key tensors (what the TP group's max-reduce does)."""
    flip = -2 ** 63
    keys.copy_(torch.maximum(keys ^ flip, other ^ flip) ^ flip)


@pytest.mark.parametrize("V,ld", SAMPLER_SHAPES)
def test_sampler_two_shards_match_whole_row(V, ld):
    """sample_tp over two vocabulary shards (tok_offset, keys max-reduced here) == sample over the whole row."""
    buf, logits = _sampler_logits(V, ld)
    whole = _St(5, TEMPS, SEEDS, POS0)
    hip.sample(logits, whole)
    cut = V // 2  # 3, 500, 500, 64128: shard 1 starts at an odd column for V = 7
    shards = []
    for lo, hi in ((0, cut), (cut, V)):
        sb = torch.full((5, (hi - lo + 7) // 8 * 8 + 8), TRAP, dtype=torch.bfloat16, device=DEV)
        sb[:, : hi - lo].copy_(logits[:, lo:hi])
        shards.append((sb[:, : hi - lo], lo))
    other = {}
    hip.sample_tp(shards[1][0], _St(5, TEMPS, SEEDS, POS0), shards[1][1], lambda k: other.update(keys=k.clone()))
    st = _St(5, TEMPS, SEEDS, POS0)
    hip.sample_tp(shards[0][0], st, shards[0][1], lambda k: _umax_(k, other["keys"]))
    assert torch.equal(st.out_tokens[:, 0], whole.out_tokens[:, 0])
    assert torch.equal(st.next_ids, whole.next_ids) and torch.equal(st.positions, whole.positions)
    assert int(st.result.abs().sum()) == 0
    _check_tokens(st.out_tokens[:, 0].cpu(), logits, POS0)
