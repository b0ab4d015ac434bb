"""Plain-PyTorch reference implementations of every engine op.

These are (1) the numerics oracle the HIP kernels are tested against
(fp32 math, same data layouts, same masking rules) and (2) the compute path
on CPU-only hosts, where the tiny test models run.  On a GPU the engine uses
``ops.hip`` exclusively (see ``ops/__init__.py``).

Layouts shared with the kernels (``csrc/kernels/*.hip``):

* ``qkv`` [T, (Hq + 2 Hkv) * D]: Q heads, then K heads, then V heads.
* KV cache per layer: ``kcache``/``vcache`` [num_pages, Hkv, P, D];
  token at position ``p`` of a sequence lives in page
  ``block_tables[row, p // P]`` at offset ``p % P``.
* ``cos_sin`` [max_pos, D/2, 2] fp32 (cos, sin), HF rotate-half pairing.
* fp8 KV cache (``--kv-dtype fp8``: K and V; ``fp8v``: V only, K stays bf16; csrc/kernels/kv8.h): per layer uint8 [num_pages, Hkv, SLAB],
  SLAB = P * D + 4 * P -- a (page, head) slab holds P rows of D e4m3fn bytes, then P fp32 row scales;
  a row is quantised whole with the power-of-two scale >= max|x| / 448.
"""

from __future__ import annotations

import math
from typing import Optional

import torch

LOG2E = 1.4426950408889634


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    xf = x.float()
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * w.float()
    y = y.to(x.dtype)
    if out is not None:
        out.copy_(y)
        return out
    return y


def add_rmsnorm(x: torch.Tensor, residual: torch.Tensor, w: torch.Tensor, eps: float,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    residual.copy_((x.float() + residual.float()).to(residual.dtype))
    return rmsnorm(residual, w, eps, out)


def rope_inv_freq(head_dim: int, theta: float, scaling=None) -> torch.Tensor:
    """RoPE inverse frequencies (float64); ``scaling`` = (factor, low_freq_factor, high_freq_factor,
    original_max_position) applies Llama-3.1's "llama3" rule: wavelengths longer than
    orig / low_freq_factor are divided by ``factor``, shorter than orig / high_freq_factor kept, and the
    band between interpolated smoothly."""
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    if scaling is None:
        return inv
    factor, low, high, orig = scaling
    wavelen = 2 * math.pi / inv
    low_wl, high_wl = orig / low, orig / high
    smooth = ((orig / wavelen) - low) / (high - low)
    mid = (1 - smooth) * inv / factor + smooth * inv
    out = torch.where(wavelen > low_wl, inv / factor, inv)
    band = (wavelen <= low_wl) & (wavelen >= high_wl)
    return torch.where(band, mid, out)


def rope_cos_sin(max_pos: int, head_dim: int, theta: float, device=None, scaling=None) -> torch.Tensor:
    inv = rope_inv_freq(head_dim, theta, scaling)
    t = torch.arange(max_pos, dtype=torch.float64)
    ang = torch.outer(t, inv)
    return torch.stack([ang.cos(), ang.sin()], dim=-1).float().contiguous().to(device)


def kv8_slab(page: int, d: int) -> int:
    return page * d + 4 * page


def kv8_quant_rows(x: torch.Tensor):
    """Rows [..., d] -> (e4m3fn bytes [..., d] uint8, fp32 scales [...]): scale = the power of two >= max|x| / 448
    (1 for a zero row) and at least 2^-126 (a normal number: 1 / scale stays finite), q = RNE e4m3(x / scale) --
    kv8.h's row rule."""
    xf = x.float()
    amax = xf.abs().amax(-1)
    m, e = torch.frexp(amax / 448.0)
    e = torch.clamp(torch.where(m == 0.5, e - 1, e), min=-126)
    sc = torch.where(amax > 0, torch.ldexp(torch.ones_like(amax), e), torch.ones_like(amax))
    q = (xf / sc[..., None]).to(torch.float8_e4m3fn).view(torch.uint8)
    return q, sc


def kv8_from_bf16(cache: torch.Tensor) -> torch.Tensor:
    """A bf16 cache [pages, Hkv, P, d] in the fp8 slab layout [pages, Hkv, P * d + 4 P] (every row quantised)."""
    n, hkv, page, d = cache.shape
    q, sc = kv8_quant_rows(cache)
    return torch.cat([q.reshape(n, hkv, page * d), sc.contiguous().view(torch.uint8).reshape(n, hkv, 4 * page)], -1)


def cache_pages(cache: torch.Tensor, pages: torch.Tensor, page: int, d: int) -> torch.Tensor:
    """fp32 [len(pages), Hkv, P, d] of a bf16 or fp8-slab cache."""
    c = cache.index_select(0, pages)
    if cache.dtype != torch.uint8:
        return c.float()
    q = c[..., : page * d].reshape(*c.shape[:2], page, d).contiguous().view(torch.float8_e4m3fn).float()
    sc = c[..., page * d:].contiguous().view(torch.float32)
    return q * sc[..., None]


def cache_write(cache: torch.Tensor, pages: torch.Tensor, offs: torch.Tensor, rows: torch.Tensor, page: int,
                d: int) -> None:
    """cache[pages[i], :, offs[i]] = rows[i] ([n, Hkv, d]) for a bf16 or fp8-slab cache."""
    if cache.dtype != torch.uint8:
        cache[pages, :, offs] = rows.to(cache.dtype)
        return
    q, sc = kv8_quant_rows(rows)  # [n, Hkv, d] bytes, [n, Hkv]
    n, hkv = rows.shape[0], rows.shape[1]
    col = offs[:, None] * d + torch.arange(d, device=offs.device)[None, :]  # [n, d] byte columns
    for h in range(hkv):
        cache[pages[:, None], h, col] = q[:, h]
        sb = page * d + 4 * offs[:, None] + torch.arange(4, device=offs.device)[None, :]
        cache[pages[:, None], h, sb] = sc[:, h].contiguous().view(torch.uint8).view(n, 4)


def rope_kv(qkv: torch.Tensor, positions: torch.Tensor, seq_idx: torch.Tensor, block_tables: torch.Tensor,
            kcache: Optional[torch.Tensor], vcache: Optional[torch.Tensor], cos_sin: torch.Tensor,
            hq: int, hkv: int, d: int, page: int, write_cache: bool = True) -> None:
    T = qkv.shape[0]
    if T == 0:
        return
    half = d // 2
    pos = positions[:T].long()
    cs = cos_sin[pos]  # [T, half, 2]
    cos, sin = cs[..., 0][:, None, :], cs[..., 1][:, None, :]
    qk = qkv[:, : (hq + hkv) * d].view(T, hq + hkv, d).float()
    a, b = qk[..., :half], qk[..., half:]
    ra = a * cos - b * sin
    rb = b * cos + a * sin
    rot = torch.cat([ra, rb], dim=-1).to(qkv.dtype)
    qkv[:, : (hq + hkv) * d] = rot.reshape(T, -1)
    if write_cache:
        rows = seq_idx[:T].long()
        keep = rows >= 0  # seq_idx < 0: prefill padding token, never cached
        rows, p_, k = rows[keep], pos[keep], rot[:, hq:][keep]
        pages = block_tables[rows, p_ // page].long()
        offs = p_ % page
        v = qkv[:, (hq + hkv) * d: (hq + 2 * hkv) * d].view(T, hkv, d)[keep]
        cache_write(kcache, pages, offs, k, page, d)
        cache_write(vcache, pages, offs, v, page, d)


def rope_kv_parts(parts: torch.Tensor, positions, seq_idx, block_tables, kcache, vcache, cos_sin, hq, hkv, d, page,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    qkv = parts.float().sum(0).to(torch.bfloat16)
    rope_kv(qkv, positions, seq_idx, block_tables, kcache, vcache, cos_sin, hq, hkv, d, page)
    if out is not None:
        out.copy_(qkv)
        return out
    return qkv


def kv_scatter(rows: torch.Tensor, page: torch.Tensor, slot: torch.Tensor, kcache: torch.Tensor,
               vcache: torch.Tensor) -> None:
    """Reference of ops.hip.kv_scatter: cache[page[i], :, slot[i], :] = rows[i, 0 | 1] (page < 0 skipped)."""
    if kcache.dtype == torch.uint8 or vcache.dtype == torch.uint8:
        raise ValueError("kv_scatter: the context-parallel K/V exchange takes bf16 caches only")
    keep = page[: rows.shape[0]].long() >= 0
    pg, sl, r = page[: rows.shape[0]].long()[keep], slot[: rows.shape[0]].long()[keep], rows[keep]
    kcache[pg, :, sl, :] = r[:, 0].to(kcache.dtype)
    vcache[pg, :, sl, :] = r[:, 1].to(vcache.dtype)


def interleave_gate_up(wg: torch.Tensor, wu: torch.Tensor) -> torch.Tensor:
    """[F, H] gate + [F, H] up -> [2F, H] rows in blocks of 16 = [8 gate | 8 up]."""
    f, h = wg.shape
    return torch.stack([wg.reshape(f // 8, 8, h), wu.reshape(f // 8, 8, h)], dim=1).reshape(2 * f, h)


def split_gate_up(gu: torch.Tensor):
    """Inverse of the blocked column layout of a gate_up GEMM output."""
    f = gu.shape[-1] // 2
    v = gu.reshape(*gu.shape[:-1], f // 8, 2, 8)
    return v[..., 0, :].reshape(*gu.shape[:-1], f), v[..., 1, :].reshape(*gu.shape[:-1], f)


def swiglu(gu: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    g, u = split_gate_up(gu)
    g, u = g.float(), u.float()
    y = (g * torch.sigmoid(g) * u).to(gu.dtype)
    if out is not None:
        out.copy_(y)
        return out
    return y


class Fp8Weight:
    """OCP e4m3fn weight [N, K] with one fp32 scale per output row (W = scale[:, None] * float(q))."""

    def __init__(self, q: torch.Tensor, scale: torch.Tensor):
        self.q, self.scale = q, scale

    @property
    def shape(self):
        return self.q.shape

    def numel(self) -> int:
        return self.q.numel()

    def nbytes(self) -> int:
        return self.q.numel() + 4 * self.scale.numel()

    def dequant(self, dtype=torch.float32) -> torch.Tensor:
        return (self.q.float() * self.scale.float()[:, None]).to(dtype)

    @staticmethod
    def quantize(w: torch.Tensor) -> "Fp8Weight":
        wf = w.float()
        scale = wf.abs().amax(dim=1).clamp_min(1e-12) / 448.0
        q = (wf / scale[:, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
        return Fp8Weight(q.contiguous(), scale.contiguous())


def _w(w):
    return w.dequant(torch.bfloat16) if isinstance(w, Fp8Weight) else w


# ------------------------------------------------------------------ p14: lossless 14-bit bf16 weights
# Bit-level reference of the format of csrc/kernels/stream_gemm.hip ("p14"): lo = w & 0xff verbatim,
# hi = w >> 8 as the 6-bit code (sign << 5) | c5 with e7 = hi & 0x7f: c5 = 0 for e7 = 0 (zeros, subnormals,
# the smallest normals), else c5 = e7 - base7 + 1 in 1..31, base7 = max(max e7 - 30, 1).
# One 3584-byte tile per (16-row group, 128-wide k block); lane l = 16 g + r of the tile owns
# W[16 G + r][128 kb + 32 i + 8 g + e] (i < 4 MFMA steps, e < 8).
P14_TILE = 3584
P14_WINDOW = 31  # e7 values of the window [base7, base7 + 30]; e7 = 0 has a code of its own
_P14_SIGN_SHIFT = (0, 1, 2, 7)  # sign bit of byte b at 8 b + 7 - shift[q], q = 2 (i & 1) + (e >> 2)


def p14_bits(w: torch.Tensor) -> torch.Tensor:
    """The 16 bits of every bf16 element as int64."""
    return w.contiguous().view(torch.int16).to(torch.int64) & 0xffff


def p14_base7(w: torch.Tensor) -> int:
    return max(int(((p14_bits(w) >> 8) & 0x7f).max()) - (P14_WINDOW - 1), 1)


def _p14_lanes(u: torch.Tensor) -> torch.Tensor:
    """[N, K] -> [tiles, 64 lanes, 4 steps, 8] in the tile order (group-major, k blocks consecutive)."""
    N, K = u.shape
    t = u.reshape(N // 16, 16, K // 128, 4, 4, 8)  # G, r, kb, i, g, e
    return t.permute(0, 2, 4, 1, 3, 5).reshape(-1, 64, 4, 8)


def p14_pack_ref(w: torch.Tensor):
    """bf16 [N, K] (N % 16 == 0, K % 128 == 0) -> (uint8 [N * K * 7 / 4] tiles, base7, out-of-window count).
    The matrix is packable iff the count is zero (an out-of-window element's code keeps only its low 5 bits)."""
    N, K = w.shape
    assert w.dtype == torch.bfloat16 and N % 16 == 0 and K % 128 == 0
    u = _p14_lanes(p14_bits(w))
    base7 = p14_base7(w)
    e7 = (u >> 8) & 0x7f
    c = torch.where(e7 == 0, e7, e7 - base7 + 1)
    bad = int(((e7 != 0) & ((c < 1) | (c > P14_WINDOW))).sum())
    c5, sg = c & 31, u >> 15
    T = u.shape[0]
    lo = (u & 0xff).reshape(T, 64, 2, 16).permute(0, 2, 1, 3).reshape(T, 2048)
    q4 = c5 & 15
    nib = (q4[..., :4] | q4[..., 4:] << 4).reshape(T, 1024)
    two = torch.zeros(T, 64, 2, dtype=torch.int64, device=u.device)
    for i in range(4):
        for e in range(8):
            b, q = e & 3, 2 * (i & 1) + (e >> 2)
            two[:, :, i >> 1] |= (c5[:, :, i, e] >> 4) << (8 * b + 4 - q)
            two[:, :, i >> 1] |= sg[:, :, i, e] << (8 * b + 7 - _P14_SIGN_SHIFT[q])
    two = torch.stack([(two >> (8 * k)) & 0xff for k in range(4)], dim=-1).reshape(T, 512)
    return torch.cat([lo, nib, two], dim=1).to(torch.uint8).reshape(-1), base7, bad


def p14_unpack_ref(packed: torch.Tensor, base7: int, N: int, K: int) -> torch.Tensor:
    """Inverse of p14_pack_ref for a packable matrix: the original bf16 [N, K], bit for bit."""
    t = packed.reshape(-1, P14_TILE).to(torch.int64)
    T = t.shape[0]
    lo = t[:, :2048].reshape(T, 2, 64, 2, 8).permute(0, 2, 1, 3, 4).reshape(T, 64, 4, 8)
    nb = t[:, 2048:3072].reshape(T, 64, 4, 4)
    q4 = torch.cat([nb & 15, nb >> 4], dim=-1)
    tb = t[:, 3072:].reshape(T, 64, 2, 4)
    two = sum(tb[..., k] << (8 * k) for k in range(4))
    hi = torch.zeros_like(lo)
    for i in range(4):
        for e in range(8):
            b, q = e & 3, 2 * (i & 1) + (e >> 2)
            s = two[:, :, i >> 1]
            c5 = q4[:, :, i, e] | ((s >> (8 * b + 4 - q)) & 1) << 4
            e7 = torch.where(c5 == 0, c5, c5 + base7 - 1)
            hi[:, :, i, e] = ((s >> (8 * b + 7 - _P14_SIGN_SHIFT[q])) & 1) << 7 | e7
    u = (hi << 8 | lo).reshape(N // 16, K // 128, 4, 16, 4, 8).permute(0, 3, 1, 4, 2, 5).reshape(N, K)
    u = torch.where(u >= 0x8000, u - 0x10000, u)
    return u.to(torch.int16).view(torch.bfloat16)


# ------------------------------------------------------------------ p13: 13 bits and an exception list
# Bit-level reference of stream_gemm.hip "p13": hi as the 5-bit code (sign << 4) | c4, c4 = 0 for e7 = 0, else
# e7 - base7 + 1 in 1..15, base7 = max(max e7 - 14, 1).  An element with 0 < e7 < base7 is an exception: c4 = 0 in
# the tile and the word kb << 18 | lane << 12 | (8 i + e) << 7 | e7 in the list, which is sorted by (16-row
# group, word) with offsets per group.  One 3328-byte tile per (group, k block), lanes as p14:
# [0, 2048) lo plane, [2048, 3072) c4 nibbles (both as p14), [3072, 3328) one sign dword per lane, the sign of
# (i, e) at bit 8 (e & 3) + 2 i + (e >> 2).
P13_TILE = 3328
P13_WINDOW = 15
P13_EXCAP = 8  # a matrix is packable iff no 16-row group holds more exceptions


def p13_base7(w: torch.Tensor) -> int:
    return max(int(((p14_bits(w) >> 8) & 0x7f).max()) - (P13_WINDOW - 1), 1)


def p13_pack_ref(w: torch.Tensor):
    """bf16 [N, K] (N % 16 == 0, K % 128 == 0) -> (uint8 [N * K * 13 / 8] tiles, base7, exoff int32 [N / 16 + 1],
    exlist int32 [exceptions] (the 32-bit words), largest per-group exception count).  The matrix is packable iff
    that count is at most P13_EXCAP; the list of an unpackable matrix is still complete here."""
    N, K = w.shape
    assert w.dtype == torch.bfloat16 and N % 16 == 0 and K % 128 == 0 and K // 128 < 0x3fff
    u = _p14_lanes(p14_bits(w))  # [T, 64, 4, 8]
    base7 = p13_base7(w)
    e7 = (u >> 8) & 0x7f
    exc = (e7 != 0) & (e7 < base7)
    c4 = torch.where((e7 == 0) | exc, torch.zeros_like(e7), e7 - base7 + 1)
    assert int(c4.max()) <= P13_WINDOW
    sg = u >> 15
    T = u.shape[0]
    lo = (u & 0xff).reshape(T, 64, 2, 16).permute(0, 2, 1, 3).reshape(T, 2048)
    nib = (c4[..., :4] | c4[..., 4:] << 4).reshape(T, 1024)
    sgn = torch.zeros(T, 64, dtype=torch.int64, device=u.device)
    for i in range(4):
        for e in range(8):
            sgn |= sg[:, :, i, e] << (8 * (e & 3) + 2 * i + (e >> 2))
    sgn = torch.stack([(sgn >> (8 * k)) & 0xff for k in range(4)], dim=-1).reshape(T, 256)
    tiles = torch.cat([lo, nib, sgn], dim=1).to(torch.uint8).reshape(-1)
    nkb = K // 128
    t, lane, i, e = torch.nonzero(exc, as_tuple=True)
    word = (t % nkb) << 18 | lane << 12 | (8 * i + e) << 7 | e7[t, lane, i, e]
    grp = t // nkb
    order = torch.argsort(grp * 2 ** 32 + word)
    grp, word = grp[order], word[order]
    cnt = torch.bincount(grp, minlength=N // 16)
    exoff = torch.zeros(N // 16 + 1, dtype=torch.int64)
    exoff[1:] = torch.cumsum(cnt, 0)
    exlist = torch.where(word >= 2 ** 31, word - 2 ** 32, word).to(torch.int32)
    return tiles, base7, exoff.to(torch.int32), exlist, int(cnt.max()) if cnt.numel() else 0


def p13_unpack_ref(packed: torch.Tensor, base7: int, exoff: torch.Tensor, exlist: torch.Tensor, N: int,
                   K: int) -> torch.Tensor:
    """Inverse of p13_pack_ref: the original bf16 [N, K], bit for bit, exceptions restored from the list."""
    t = packed.reshape(-1, P13_TILE).to(torch.int64)
    T = t.shape[0]
    lo = t[:, :2048].reshape(T, 2, 64, 2, 8).permute(0, 2, 1, 3, 4).reshape(T, 64, 4, 8)
    nb = t[:, 2048:3072].reshape(T, 64, 4, 4)
    c4 = torch.cat([nb & 15, nb >> 4], dim=-1)
    sb = t[:, 3072:].reshape(T, 64, 4)
    sgn = sum(sb[..., k] << (8 * k) for k in range(4))
    e7 = torch.where(c4 == 0, c4, c4 + base7 - 1)
    nkb = K // 128
    words = exlist.to(torch.int64) & 0xffffffff
    for G in range(N // 16):
        for x in words[int(exoff[G]):int(exoff[G + 1])].tolist():
            e7[G * nkb + (x >> 18), (x >> 12) & 63, (x >> 10) & 3, (x >> 7) & 7] = x & 127
    hi = torch.zeros_like(lo)
    for i in range(4):
        for e in range(8):
            hi[:, :, i, e] = ((sgn >> (8 * (e & 3) + 2 * i + (e >> 2))) & 1) << 7 | e7[:, :, i, e]
    u = (hi << 8 | lo).reshape(N // 16, K // 128, 4, 16, 4, 8).permute(0, 3, 1, 4, 2, 5).reshape(N, K)
    u = torch.where(u >= 0x8000, u - 0x10000, u)
    return u.to(torch.int16).view(torch.bfloat16)


def linear(x: torch.Tensor, w) -> torch.Tensor:
    if isinstance(w, Fp8Weight):
        return (x.float() @ w.dequant().t()).to(x.dtype)
    return torch.nn.functional.linear(x, w)


def linear_parts(x: torch.Tensor, w: torch.Tensor, splits: int = 1) -> torch.Tensor:
    """fp32 split-K partial slabs [S, M, N] of x @ w^T (what skinny_gemm EPI_F32_PARTIAL emits)."""
    K = x.shape[1]
    ks = K // splits
    wf = w.dequant() if isinstance(w, Fp8Weight) else w.float()
    return torch.stack([x[:, i * ks:(i + 1) * ks].float() @ wf[:, i * ks:(i + 1) * ks].t()
                        for i in range(splits)])


def linear_swiglu(x: torch.Tensor, w_gu) -> torch.Tensor:
    return swiglu(linear(x, w_gu))


def add_rmsnorm_parts(parts: torch.Tensor, residual: torch.Tensor, w: torch.Tensor, eps: float,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    residual.copy_((parts.float().sum(0) + residual.float()).to(residual.dtype))
    return rmsnorm(residual, w, eps, out)


def embed(ids: torch.Tensor, table: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    y = table[ids.long().clamp(0, table.shape[0] - 1)]
    if out is not None:
        out.copy_(y)
        return out
    return y


def attn_prefill(qkv: torch.Tensor, cu_seqlens: torch.Tensor, hq: int, hkv: int, d: int, scale: float,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    T = qkv.shape[0]
    if out is None:
        out = torch.empty(T, hq * d, dtype=qkv.dtype, device=qkv.device)
    cu = cu_seqlens.tolist()
    g = hq // hkv
    for i in range(len(cu) - 1):
        s, e = cu[i], cu[i + 1]
        if e <= s:
            continue
        n = e - s
        q = qkv[s:e, : hq * d].view(n, hq, d).float().transpose(0, 1)
        k = qkv[s:e, hq * d: (hq + hkv) * d].view(n, hkv, d).float().transpose(0, 1)
        v = qkv[s:e, (hq + hkv) * d: (hq + 2 * hkv) * d].view(n, hkv, d).float().transpose(0, 1)
        k = k.repeat_interleave(g, dim=0)
        v = v.repeat_interleave(g, dim=0)
        sc = torch.matmul(q, k.transpose(1, 2)) * scale
        mask = torch.ones(n, n, dtype=torch.bool, device=qkv.device).triu(1)
        sc.masked_fill_(mask, float("-inf"))
        p = torch.softmax(sc, dim=-1)
        o = torch.matmul(p, v).transpose(0, 1).reshape(n, hq * d)
        out[s:e] = o.to(out.dtype)
    return out


def attn_prefill_paged(qkv: torch.Tensor, cu_seqlens: torch.Tensor, hq: int, hkv: int, d: int, scale: float,
                       paged, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Chunked prefill: slice rows of every packed sequence attend to the cached positions
    [0, prefix) of that sequence (paged cache, already holding this slice's K/V too) and causally
    within the slice."""
    T = qkv.shape[0]
    if out is None:
        out = torch.empty(T, hq * d, dtype=qkv.dtype, device=qkv.device)
    cu = cu_seqlens.tolist()
    g = hq // hkv
    P = 64 if paged.kcache.dtype == torch.uint8 else paged.kcache.shape[2]
    for i in range(len(cu) - 1):
        s, e = cu[i], cu[i + 1]
        if e <= s:
            continue
        n, pre, slot = e - s, paged.prefix_host[i], paged.slot_host[i]
        tot = pre + n
        pages = paged.block_tables[slot, : -(-tot // P)].long()
        k = cache_pages(paged.kcache, pages, P, d).permute(1, 0, 2, 3).reshape(hkv, -1, d)[:, :tot]
        v = cache_pages(paged.vcache, pages, P, d).permute(1, 0, 2, 3).reshape(hkv, -1, d)[:, :tot]
        q = qkv[s:e, : hq * d].view(n, hq, d).float().transpose(0, 1)
        k = k.repeat_interleave(g, dim=0)
        v = v.repeat_interleave(g, dim=0)
        sc = torch.matmul(q, k.transpose(1, 2)) * scale
        qpos = torch.arange(pre, tot, device=qkv.device)[:, None]
        kpos = torch.arange(tot, device=qkv.device)[None, :]
        sc.masked_fill_(kpos > qpos, float("-inf"))
        p = torch.softmax(sc, dim=-1)
        out[s:e] = torch.matmul(p, v).transpose(0, 1).reshape(n, hq * d).to(out.dtype)
    return out


def attn_decode(q: torch.Tensor, kcache: torch.Tensor, vcache: torch.Tensor, block_tables: torch.Tensor,
                positions: torch.Tensor, hq: int, hkv: int, d: int, page: int, scale: float,
                out: Optional[torch.Tensor] = None, num_splits: int = 1) -> torch.Tensor:
    """q: [B, >= hq*d] (rows of the qkv buffer); context = positions + 1."""
    B = q.shape[0]
    if out is None:
        out = torch.empty(B, hq * d, dtype=q.dtype, device=q.device)
    g = hq // hkv
    for b in range(B):
        ctx = int(positions[b]) + 1
        npg = (ctx + page - 1) // page
        pages = block_tables[b, :npg].long()
        k = cache_pages(kcache, pages, page, d).permute(1, 0, 2, 3).reshape(hkv, npg * page, d)[:, :ctx]
        v = cache_pages(vcache, pages, page, d).permute(1, 0, 2, 3).reshape(hkv, npg * page, d)[:, :ctx]
        qq = q[b, : hq * d].view(hkv, g, d).float()
        sc = torch.matmul(qq, k.transpose(1, 2)) * scale
        p = torch.softmax(sc, dim=-1)
        o = torch.matmul(p, v).reshape(hq * d)
        out[b] = o.to(out.dtype)
    return out


# ----------------------------------------------------------------- sampler
_M1 = 0xbf58476d1ce4e5b9
_M2 = 0x94d049bb133111eb
_GOLD = 0x9E3779B97F4A7C15
_TOKMUL = 0xD1B54A32D192ED03
_U64 = (1 << 64) - 1


def _s64(x: int) -> int:
    x &= _U64
    return x - (1 << 64) if x >= (1 << 63) else x


def _lsr(x: torch.Tensor, n: int) -> torch.Tensor:
    return (x >> n) & ((1 << (64 - n)) - 1)


def _mix64_t(x: torch.Tensor) -> torch.Tensor:
    x = x ^ _lsr(x, 30)
    x = x * _s64(_M1)
    x = x ^ _lsr(x, 27)
    x = x * _s64(_M2)
    x = x ^ _lsr(x, 31)
    return x


def gumbel_noise(seed: int, position: int, vocab: int, device=None) -> torch.Tensor:
    """The sampler kernel's counter-based Gumbel noise for one row (fp32)."""
    k0 = _mix64_t(torch.tensor([_s64(seed * _GOLD + position + 1)], dtype=torch.int64))
    tok = torch.arange(vocab, dtype=torch.int64)
    h = _mix64_t(k0 ^ (tok * _s64(_TOKMUL)))
    u = (_lsr(h, 40).double() + 0.5) / 16777216.0
    return (-torch.log(-torch.log(u))).float().to(device)


def nucleus_levels(row: torch.Tensor, temp: float):
    """The levels of one logits row for the top-k / top-p rule: ``(values, counts, weights)``, float64 /
    int64 / float64, values descending.  A level is one distinct stored value (-0 and +0 are one level);
    its weight is count * exp((value - top value) / temp).  NaNs are no level."""
    r = row.detach().double().cpu().reshape(-1)
    r = r[~torch.isnan(r)] + 0.0  # -0.0 + 0.0 = +0.0
    vals, counts = torch.unique(r, return_counts=True)
    vals, counts = vals.flip(0), counts.flip(0)
    if vals.numel() == 0:
        return vals, counts, vals.clone()
    d = (vals - vals[0]) / temp
    d = torch.where(vals == vals[0], torch.zeros_like(d), d)  # inf - inf
    return vals, counts, counts.double() * torch.exp(d)


def nucleus_cut(row: torch.Tensor, temp: float, top_k: int, top_p: float):
    """``(threshold, margin)`` of one row, in float64: the value of the last kept level (-inf for a row
    without a filter or with temp <= 0) and the relative distance of p * Z from the cumulative mass on
    either side of the top-p cut (inf where top-p decides nothing)."""
    V = row.numel()
    if temp <= 0 or (top_k <= 0 and top_p >= 1.0):
        return float("-inf"), float("inf")
    vals, counts, w = nucleus_levels(row, temp)
    if vals.numel() == 0:
        return float("-inf"), float("inf")
    last = vals.numel() - 1
    jk = last
    if 0 < top_k < V:
        jk = min(last, int(torch.searchsorted(torch.cumsum(counts, 0), top_k)))
    j, margin = jk, float("inf")
    if top_p < 1.0:
        cum = torch.cumsum(w[:jk + 1], 0)
        target = top_p * float(cum[-1])
        j = min(jk, int(torch.searchsorted(cum, torch.tensor(target, dtype=torch.float64))))
        below = float(cum[j - 1]) if j > 0 else 0.0
        margin = min(float(cum[j]) - target, target - below) / target
    return float(vals[j]), margin


def nucleus_threshold(logits: torch.Tensor, temps, top_k, top_p) -> torch.Tensor:
    """Per-row top-k / top-p threshold, fp32 [B]: a token is kept iff its logit >= the threshold.

    The levels of a row are its distinct stored values, descending (v1 > v2 > ..., counts n_i, -0 = +0),
    with weights w_i = n_i exp((v_i - v1) / temp).  top-k keeps the levels up to the first whose
    cumulative count reaches k (all of them for k = 0 or k >= V); top-p, over that set, keeps the levels
    up to the first whose cumulative weight reaches p times the set's total.  Whole levels are kept, so
    ties at the cut all stay.  temp <= 0, or k = 0 with p >= 1: -inf (no filter).  Computed in float64;
    sampler.hip's filter kernels match it."""
    B = logits.shape[0]
    out = torch.empty(B, dtype=torch.float32)
    for b in range(B):
        out[b] = nucleus_cut(logits[b], float(temps[b]), int(top_k[b]), float(top_p[b]))[0]
    return out


def apply_penalties(logits: torch.Tensor, out_tokens, gen_count, rep, freq, pres, done=None,
                    tok_offset: int = 0) -> torch.Tensor:
    """Repetition / frequency / presence penalties, in place on the bf16 rows ``logits`` [B, V] (returned).

    For row b let c(t) be the number of times token t occurs in ``out_tokens[b, :gen_count[b]]`` -- the
    GENERATED tokens only, never the prompt.  Every t with c(t) > 0 whose column t - ``tok_offset`` lies in
    [0, V) is rewritten, each step one individually rounded fp32 operation, in vLLM's order:

        x = float32(logit);  x = x / rep if x > 0 else x * rep  (when rep != 1);
        x = x - fl32(freq * c);  x = x - pres;  logit = bf16(x)  (round to nearest even)

    Every other entry keeps its bits.  A row with rep == 1, freq == 0 and pres == 0, with gen_count == 0 or
    with ``done`` set is untouched.  ``tok_offset`` / V describe a vocabulary shard: penalising the shards
    of a row one by one equals penalising the whole row.  sampler.hip's penalize kernel matches it bit for
    bit."""
    B, V = logits.shape
    for b in range(B):
        r = torch.tensor(float(rep[b]), dtype=torch.float32)
        f = torch.tensor(float(freq[b]), dtype=torch.float32)
        p = torch.tensor(float(pres[b]), dtype=torch.float32)
        g = int(gen_count[b])
        if (float(r) == 1.0 and float(f) == 0.0 and float(p) == 0.0) or g <= 0 or (done is not None and int(done[b])):
            continue
        toks, counts = torch.unique(out_tokens[b, :g].to(torch.int64).cpu(), return_counts=True)
        cols = toks - int(tok_offset)
        keep = (cols >= 0) & (cols < V)
        cols, counts = cols[keep].to(logits.device), counts[keep].to(logits.device)
        x = logits[b, cols].to(torch.float32)
        if float(r) != 1.0:
            x = torch.where(x > 0, x / r, x * r)
        x = x - f * counts.to(torch.float32)
        x = x - p
        logits[b, cols] = x.to(logits.dtype)
    return logits


def apply_constraints(logits: torch.Tensor, bias_tok, bias_val, bias_n, gen_count, min_new, stop_ids, eos,
                      done=None, tok_offset: int = 0) -> torch.Tensor:
    """Logit bias and minimum length, in place on the bf16 rows ``logits`` [B, V] (returned), before the
    penalties and before any filter.

    Bias: for every entry i < ``bias_n[b]`` of row b whose column ``bias_tok[b, i] - tok_offset`` lies in
    [0, V) (the tokens of a row are distinct; the host guarantees it):

        finite bias:  x = float32(logit);  x = x + bias (one rounded fp32 add);  logit = bf16(x)  (RNE)
        bias -inf:    a ban -- the entry is STORED as -inf, not added, so a +inf logit is banned too and no
                      NaN appears.  A NaN logit stays a NaN either way.

    Minimum length: with ``gen_count[b] < min_new[b]`` every armed stop id -- the engine's four ``eos`` slots
    and the row's four ``stop_ids[b]``, -1 = unused slot -- that falls into the shard is stored as -inf;
    this wins over a bias on the same token.  With ``gen_count[b] >= min_new[b]`` nothing is suppressed.

    Every other entry keeps its bits; a row with ``bias_n`` 0 and nothing to suppress, or with ``done`` set,
    is untouched.  ``tok_offset`` / V describe a vocabulary shard: constraining the shards of a row one by
    one equals constraining the whole row.  sampler.hip's constrain kernel matches it bit for bit."""
    B, V = logits.shape
    ninf = torch.tensor(float("-inf"), dtype=logits.dtype, device=logits.device)
    armed = [int(x) for x in eos.tolist() if int(x) >= 0]
    for b in range(B):
        n = min(int(bias_n[b]), bias_tok.shape[1])
        suppress = int(gen_count[b]) < int(min_new[b])
        if (n <= 0 and not suppress) or (done is not None and int(done[b])):
            continue
        if n > 0:
            cols = bias_tok[b, :n].to(torch.int64) - int(tok_offset)
            vals = bias_val[b, :n].to(torch.float32)
            keep = (cols >= 0) & (cols < V)
            cols, vals = cols[keep].to(logits.device), vals[keep].to(logits.device)
            x = logits[b, cols].to(torch.float32)
            ban = torch.isneginf(vals)
            y = (x + torch.where(ban, torch.zeros_like(vals), vals)).to(logits.dtype)
            logits[b, cols] = torch.where(ban & ~torch.isnan(x), ninf, y)
        if suppress:
            for t in armed + [int(x) for x in stop_ids[b].tolist() if int(x) >= 0]:
                if 0 <= t - int(tok_offset) < V:
                    logits[b, t - int(tok_offset)] = ninf
    return logits


def token_logprobs(logits: torch.Tensor, top_n):
    """Token log-probabilities of the rows ``logits`` [B, V] (or one row [V]) and their top lists: THE
    definition of what ``logprobs`` / ``top_logprobs`` report, computed in float64 on the stored (bf16) values.

    For a row x:  m = max(x),  S = sum_i exp(x_i - m),  lp(t) = (x_t - m) - log S.  A -inf logit (a ban, a
    suppressed stop id) adds 0 to S and has lp -inf.  Rows that hold a NaN or +inf, or nothing but -inf,
    are unspecified, as sampling from them is.

    The rows are the ones the sampler sees: after apply_constraints and apply_penalties, before the
    temperature and before the top-k / top-p filter (vLLM's processed logits, at T = 1).

    ``top_n``: one int or one per row; a row's list holds its min(n, V) tokens of the largest value, values
    compared as numbers (-0 equals +0), ties broken by the lower token id, each with its lp.  n <= 0: empty.

    Returns ``(lp, tops)``: lp float64 [B, V] on the CPU, tops a list of B lists of (token, lp)."""
    x = logits.detach().to("cpu", torch.float64)
    if x.dim() == 1:
        x = x[None]
    B, V = x.shape
    ns = [int(top_n)] * B if isinstance(top_n, int) else [int(n) for n in top_n]
    m = x.max(dim=1, keepdim=True).values
    S = torch.exp(x - m).sum(dim=1, keepdim=True)
    lp = (x - m) - torch.log(S)
    tops = []
    for b in range(B):
        n = min(max(ns[b], 0), V)
        if n == 0:
            tops.append([])
            continue
        # a stable descending sort: equal values (and -0 / +0 compare equal) stay in token order
        order = torch.sort(x[b], descending=True, stable=True).indices[:n]
        tops.append([(int(t), float(lp[b, t])) for t in order])
    return lp, tops


def sample_tokens(logits: torch.Tensor, temps: torch.Tensor, seeds: torch.Tensor,
                  positions: torch.Tensor, thresh: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Gumbel-max sampling (argmax when temperature <= 0); ties -> lowest id.  ``thresh`` (fp32 [B],
    nucleus_threshold): tokens of row b with a logit below thresh[b] are left out."""
    B, V = logits.shape
    out = torch.empty(B, dtype=torch.int32)
    for b in range(B):
        row = logits[b].float().cpu()
        t = float(temps[b])
        if t > 0:
            keep = None if thresh is None else row >= float(thresh[b])
            row = row / t + gumbel_noise(int(seeds[b]), int(positions[b]), V)
            if keep is not None:
                row = torch.where(keep, row, torch.full_like(row, float("-inf")))
        out[b] = int(torch.argmax(row))
    return out.to(logits.device)


def sample_finish(tokens: torch.Tensor, st) -> None:
    """Bookkeeping identical to the finish kernel (st = engine DecodeState).  A state whose
    ``constrained`` flag is set also retires a row at one of its own ``stop_ids`` (-1 = unused slot)."""
    B = tokens.shape[0]
    eos = set(int(x) for x in st.eos.tolist() if int(x) >= 0)
    row_stops = getattr(st, "constrained", False)
    for b in range(B):
        if int(st.done[b]):
            continue
        tok = int(tokens[b])
        g = int(st.gen_count[b])
        st.out_tokens[b, g] = tok
        st.gen_count[b] = g + 1
        st.next_ids[b] = tok
        own = row_stops and tok in [int(x) for x in st.stop_ids[b].tolist()]  # tok >= 0 never matches -1
        if g + 1 >= int(st.max_new[b]) or tok in eos or own:
            st.done[b] = 1
        else:
            st.positions[b] += 1


def attention_scale(d: int) -> float:
    return 1.0 / math.sqrt(d)
