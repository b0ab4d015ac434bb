"""Shared inputs of the top-k / top-p tests (tests/test_sampling_filters_{cpu,gpu}.py).

``HAND``: hand-written rows of 24 logits (all exactly representable in bf16) with their temperature,
top_k, top_p and the threshold rule 1-5 of ops/reference.py nucleus_threshold gives, worked out by hand.
"""

import torch

NINF = float("-inf")
V_HAND = 24

_A = [3.0, 3.0, 2.0, 1.0] + [0.0] * 20
_C = [5.0, 1.0] + [0.0] * 22
_D = [0.0, -0.0, -1.0, -2.0] + [-3.0] * 20
_E = [2.0, 1.0] + [NINF] * 22
_G = [2.0, 1.0] + [0.0] * 22

# (name, row, temperature, top_k, top_p, expected threshold)
HAND = [
    ("k1_tie_at_max", _A, 1.0, 1, 1.0, 3.0),  # two tokens tied at the max: both kept
    ("k_equals_V", _A, 1.0, 24, 1.0, 0.0),  # k >= V: the lowest level
    ("k_above_V", _A, 1.0, 100, 1.0, 0.0),
    ("no_filter", _A, 1.0, 0, 1.0, NINF),
    # Z = 1 + e^-4 + 22 e^-5 = 1.1666, p Z = 0.0117 <= 1: the top level alone
    ("p_small", _C, 1.0, 0, 0.01, 5.0),
    ("signed_zero_one_level", _D, 1.0, 1, 1.0, 0.0),  # -0 and +0: one level of two tokens
    # Z = 1 + e^-1 = 1.3679, p Z = 1.3542: the level 2.0 holds 1 < p Z, the level 1.0 reaches it
    ("neg_inf_entries_p", _E, 1.0, 0, 0.99, 1.0),
    ("neg_inf_entries_k", _E, 1.0, 3, 1.0, NINF),  # counts 1, 2, 24: the third token sits in the -inf level
    ("greedy_zero", _A, 0.0, 1, 0.5, NINF),
    ("greedy_negative", _A, -1.0, 1, 0.5, NINF),
    # top-k first: the set {2, 1} has Z = 1.3679, p Z = 0.9575 <= 1 -> threshold 2.  (top-p over the whole
    # row first, Z = 1 + e^-1 + 22 e^-2 = 4.345, p Z = 3.04, would keep the zeros and top-k then cut at 1.)
    ("k_then_p", _G, 1.0, 2, 0.7, 2.0),
]


def hand_tensors():
    """(logits bf16 [n, 24], temps, top_k, top_p, expected fp32 [n]) of HAND."""
    logits = torch.tensor([h[1] for h in HAND], dtype=torch.float32).to(torch.bfloat16)
    return (logits, [h[2] for h in HAND], [h[3] for h in HAND], [h[4] for h in HAND],
            torch.tensor([h[5] for h in HAND], dtype=torch.float32))


# the random-row cases: (temperature, top_k, top_p), one per row of a B = 5 launch
CASES = [(1.0, 0, 0.9), (0.3, 0, 0.5), (0.7, 40, 0.5), (1.0, 1000, 0.9), (0.3, 5, 0.9)]
SHAPES = [(50, 56), (1000, 1000), (4099, 4104), (8191, 8192), (128256, 128256)]  # (V, row stride)
SCALES = [1, 2, 3, 4]
MARGIN = 1e-4  # fp32 chunk-then-scan sums of <= 65536 positive terms + fast exp stay below ~1e-5 relative
MAX_TRIES = 16


def random_row(V: int, scale: float, seed: int) -> torch.Tensor:
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(V, generator=g) * scale).to(torch.bfloat16)


def pick_rows(V: int, scale: float, base: int):
    """One row per CASES entry: the first seed from ``base + 1000 * row`` whose float64 top-p decision margin
    (reference.nucleus_cut) is >= MARGIN.  Returns (rows bf16 [5, V], thresholds fp32 [5], tries used)."""
    from llm_map_reduce_summarizer_amd.ops import reference
    rows, th, tries = [], [], []
    for b, (tau, k, p) in enumerate(CASES):
        for t in range(MAX_TRIES):
            row = random_row(V, scale, base + 1000 * b + t)
            cut, margin = reference.nucleus_cut(row, tau, k, p)
            if margin >= MARGIN:
                break
        else:
            raise AssertionError("no seed with a decision margin >= %g within %d tries (V=%d scale=%s case %d)"
                                 % (MARGIN, MAX_TRIES, V, scale, b))
        rows.append(row)
        th.append(cut)
        tries.append(t + 1)
    return torch.stack(rows), torch.tensor(th, dtype=torch.float32), tries
