"""p13 (lossless 13-bit packed bf16 weights with an exception list): the bit-level reference of the format, on
the CPU."""

import torch

from llm_map_reduce_summarizer_amd.ops import reference as ref


def _from_bits(bits: torch.Tensor) -> torch.Tensor:
    """int64 16-bit patterns -> bf16 of exactly those bits."""
    b = torch.where(bits >= 0x8000, bits - 0x10000, bits)
    return b.to(torch.int16).view(torch.bfloat16)


def _matrix(e7_lo: int, e7_hi: int, special, N=32, K=256, seed=0):
    """A bf16 [N, K] matrix of random bit patterns with e7 in [e7_lo, e7_hi], both signs, with the ``special``
    16-bit patterns scattered over rows, k blocks, MFMA steps and element slots (stride 269, a prime)."""
    g = torch.Generator().manual_seed(seed)
    e7 = torch.randint(e7_lo, e7_hi + 1, (N, K), generator=g)
    lo = torch.randint(0, 256, (N, K), generator=g)
    sg = torch.randint(0, 2, (N, K), generator=g)
    bits = sg << 15 | e7 << 8 | lo
    flat = bits.reshape(-1)
    for j, s in enumerate(special):
        flat[(17 + 269 * j) % flat.numel()] = s
    return _from_bits(bits), bits


def _roundtrip(w, bits, base7, nexc):
    packed, b7, exoff, exlist, worst = ref.p13_pack_ref(w)
    N, K = w.shape
    assert b7 == base7 and exlist.numel() == nexc == int(exoff[-1]) and exoff.numel() == N // 16 + 1
    assert packed.dtype == torch.uint8 and packed.numel() == w.numel() * 13 // 8
    assert worst <= ref.P13_EXCAP
    back = ref.p13_unpack_ref(packed, b7, exoff, exlist, N, K)
    assert torch.equal(ref.p14_bits(back), bits)  # bit for bit (NaN payloads and -0 included)
    return packed, exoff, exlist


def test_roundtrip_ordinary_weights_and_zero_class():
    # largest e7 = 63 -> window [49, 63]; +-0, +- subnormals and the smallest normals (e7 = 0) take the zero code
    # and are no exceptions, however far below the window they lie
    special = [0x3fff, 0xbfff, 0x3f00, 0xbf80, 0x3100, 0x3180, 0xb100, 0xb1ff, 0x0000, 0x8000, 0x0001, 0x8001,
               0x007f, 0x807f, 0x0080, 0x80ff]
    w, bits = _matrix(50, 62, special)
    _roundtrip(w, bits, 49, 0)


def test_roundtrip_e7_127():
    # inf / NaN exponents: code 15 + base7 - 1 = 127 must not carry into the sign
    special = [0x7f80, 0xff80, 0x7fc1, 0xffff, 0x7f7f, 0x7100, 0xf180, 0x0000]
    w, bits = _matrix(114, 126, special, seed=3)
    _roundtrip(w, bits, 113, 0)


def test_roundtrip_window_clamped_to_base_one():
    # largest e7 = 9 < 15: base7 clamps to 1, the codes are the e7 values themselves and nothing can be an exception
    special = [0x09ff, 0x89ff, 0x0100, 0x8180, 0x0000, 0x8000, 0x0001, 0x807f, 0x0080]
    w, bits = _matrix(0, 8, special, seed=2)
    _roundtrip(w, bits, 1, 0)
    special = [0x0fff, 0x8f00, 0x0100, 0x8100, 0x0080]  # largest e7 = 15: base7 = 1 exactly, e7 = 1 is code 1
    w, bits = _matrix(1, 14, special, seed=5)
    _roundtrip(w, bits, 1, 0)


def test_element_at_base_and_just_below_and_negative_exceptions():
    # window [49, 63]: e7 = 49 (0x31..) is code 1; e7 = 48 (0x30..), 20 and 1, of both signs, are exceptions
    special = [0x3f80, 0x3100, 0xb17f, 0x3000, 0xb0ff, 0x1434, 0x9400, 0x0100, 0x81ff]
    w, bits = _matrix(50, 62, special, seed=4)
    packed, exoff, exlist = _roundtrip(w, bits, 49, 6)
    words = (exlist.to(torch.int64) & 0xffffffff).tolist()
    assert sorted(x & 127 for x in words) == [1, 1, 20, 20, 48, 48]
    # the tile keeps sign and lo of an exception, with the zero code: dropping the list decodes them as e7 = 0
    lossy = ref.p13_unpack_ref(packed, 49, torch.zeros_like(exoff), exlist[:0], *w.shape)
    got = ref.p14_bits(lossy)
    diff = got != bits
    assert int(diff.sum()) == 6 and torch.equal(got[diff], bits[diff] & 0x80ff)


def test_list_is_sorted_by_group_then_k_block():
    w, bits = _matrix(50, 62, [0x3f80], N=48, K=512, seed=6)
    b = bits.clone()
    # planted out of order: group 2 first, then group 0 at k block 3 before k block 0, two in one tile
    for (r, k, v) in [(40, 130, 0x2000), (5, 400, 0xa011), (3, 7, 0x2b00), (15, 100, 0x0155), (3, 6, 0x9c00),
                      (47, 511, 0x2fff)]:
        b[r, k] = v
    wb = _from_bits(b)
    packed, b7, exoff, exlist, worst = ref.p13_pack_ref(wb)
    assert b7 == 49 and exoff.tolist() == [0, 4, 4, 6] and worst == 4
    words = (exlist.to(torch.int64) & 0xffffffff).tolist()
    kbs = [x >> 18 for x in words]
    assert kbs == [0, 0, 0, 3, 1, 3]
    for lo_, hi_ in zip(exoff[:-1].tolist(), exoff[1:].tolist()):
        assert words[lo_:hi_] == sorted(words[lo_:hi_])
    # (row 3, k 6) and (row 3, k 7): one lane (g = 0, r = 3), MFMA step 0, elements 6 and 7
    assert [(x >> 12) & 63 for x in words[:2]] == [3, 3] and [(x >> 7) & 31 for x in words[:2]] == [6, 7]
    assert torch.equal(ref.p14_bits(ref.p13_unpack_ref(packed, b7, exoff, exlist, 48, 512)), b)


def test_cap_plus_one_exceptions_in_a_group_is_unpackable():
    w, bits = _matrix(50, 62, [0x3f80], seed=7)
    b = bits.clone()
    for j in range(ref.P13_EXCAP):
        b[16 + j, 3 + 31 * j] = 0x2000 | j  # group 1, spread over both k blocks
    assert ref.p13_pack_ref(_from_bits(b))[4] == ref.P13_EXCAP  # at the cap: packable
    _roundtrip(_from_bits(b), b, 49, ref.P13_EXCAP)
    b[31, 255] = 0x9000
    assert ref.p13_pack_ref(_from_bits(b))[4] == ref.P13_EXCAP + 1  # one more in the same group: not
    b[31, 255] = bits[31, 255]
    b[0, 0] = 0x9000  # ... but one more in another group is fine
    assert ref.p13_pack_ref(_from_bits(b))[4] == ref.P13_EXCAP
