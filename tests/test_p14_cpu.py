"""p14 (lossless 14-bit packed bf16 weights): the bit-level reference of the format, on the CPU."""

import pytest
import torch

from llm_map_reduce_summarizer_amd.engine.model import _randn
from llm_map_reduce_summarizer_amd.ops import reference as ref


def _from_bits(bits: torch.Tensor) -> torch.Tensor:
    """int64 16-bit patterns -> bf16 of exactly those bits."""
    b = torch.where(bits >= 0x8000, bits - 0x10000, bits)
    return b.to(torch.int16).view(torch.bfloat16)


def _matrix(e7_lo: int, e7_hi: int, special, N=32, K=256, seed=0):
    """A bf16 [N, K] matrix of random bit patterns with e7 in [e7_lo, e7_hi], both signs, with the ``special``
    16-bit patterns scattered over rows, k blocks, MFMA steps and element slots."""
    g = torch.Generator().manual_seed(seed)
    e7 = torch.randint(e7_lo, e7_hi + 1, (N, K), generator=g)
    lo = torch.randint(0, 256, (N, K), generator=g)
    sg = torch.randint(0, 2, (N, K), generator=g)
    bits = sg << 15 | e7 << 8 | lo
    flat = bits.reshape(-1)
    for j, s in enumerate(special):  # stride 269 (prime): walks every residue of the tile's index fields
        flat[(17 + 269 * j) % flat.numel()] = s
    return _from_bits(bits), bits


def _roundtrip(w: torch.Tensor, bits: torch.Tensor, base7: int):
    packed, b7, bad = ref.p14_pack_ref(w)
    assert (b7, bad) == (base7, 0)
    assert packed.dtype == torch.uint8 and packed.numel() == w.numel() * 7 // 4
    back = ref.p14_unpack_ref(packed, b7, *w.shape)
    assert torch.equal(ref.p14_bits(back), bits)  # bit for bit (NaN payloads and -0 included)


def test_roundtrip_window_edges():
    # largest e7 = 63 -> window [33, 63]: top and bottom e7 with exponent bit 0 clear / set, both signs, the
    # largest element (0x3fff) and its negative -- and the e7 = 0 class (+-0, +- subnormals, the smallest normals)
    # far below the window, as in a matrix of ordinary weights with a few exact zeros
    special = [0x3fff, 0xbfff, 0x3f00, 0x3f80, 0xbf00, 0xbf80, 0x2100, 0x2180, 0xa100, 0xa180, 0x217f, 0x21ff,
               0x3f7f, 0xa1ff, 0x0000, 0x8000, 0x0001, 0x8001, 0x007f, 0x807f, 0x0080, 0x80ff]
    w, bits = _matrix(34, 62, special)
    _roundtrip(w, bits, 33)


def test_roundtrip_window_reaches_zero():
    # largest e7 = 31 -> base7 = 1: the window [1, 31] joins the e7 = 0 class, every smaller value is packable
    special = [0x1fff, 0x9fff, 0x1f00, 0x1f80, 0x0000, 0x8000, 0x0001, 0x8001, 0x007f, 0x807f, 0x0080, 0x8080,
               0x00ff, 0x80ff, 0x0100, 0x8180]
    w, bits = _matrix(1, 30, special, seed=1)
    _roundtrip(w, bits, 1)


def test_roundtrip_base_clamps():
    # largest e7 = 20 < 31: base7 clamps to 1 and the codes are the e7 values themselves
    special = [0x14ff, 0x94ff, 0x1400, 0x1480, 0x0000, 0x8000, 0x0001, 0x807f, 0x0080]
    w, bits = _matrix(0, 19, special, seed=2)
    _roundtrip(w, bits, 1)


def test_roundtrip_large_values_and_nan():
    # e7 = 127 (inf / NaN exponents): code + base7 - 1 = 127 must not carry into the sign
    special = [0x7f80, 0xff80, 0x7fc1, 0xffff, 0x7f7f, 0x6100, 0xe180, 0x0000]
    w, bits = _matrix(98, 126, special, seed=3)
    _roundtrip(w, bits, 97)


def test_one_step_below_window_is_unpackable():
    w, bits = _matrix(34, 62, [0x3f80], seed=4)
    packed, b7, bad = ref.p14_pack_ref(w)
    assert (b7, bad) == (33, 0)
    flat = bits.reshape(-1).clone()
    flat[12345 % flat.numel()] = 0x2080  # e7 = 32: one step below the window [33, 63]
    packed, b7, bad = ref.p14_pack_ref(_from_bits(flat.reshape(bits.shape)))
    assert (b7, bad) == (33, 1)
    flat[4321] = 0x8100  # e7 = 1: the lowest e7 without a code of its own
    assert ref.p14_pack_ref(_from_bits(flat.reshape(bits.shape)))[2] == 2
    flat[77] = 0x8000  # a zero stays packable
    assert ref.p14_pack_ref(_from_bits(flat.reshape(bits.shape)))[2] == 2


@pytest.mark.parametrize("name", ["l0.wq", "l3.wd", "lm_head"])
def test_model_initialisation_is_packable(name):
    """The project's own initialisation must be packable: a condition of the p14 decode path, not a measurement
    (the nearest non-zero value lies ~30 binades below the largest, against a window of 62; the generator's few
    exact zeros take the e7 = 0 code)."""
    w = _randn((4096, 4096), 0.02, 0, name, torch.device("cpu"), torch.bfloat16)
    packed, b7, bad = ref.p14_pack_ref(w)
    assert bad == 0
    assert torch.equal(ref.p14_bits(ref.p14_unpack_ref(packed, b7, 4096, 4096)), ref.p14_bits(w))
