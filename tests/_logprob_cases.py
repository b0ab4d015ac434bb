"""Shared by the logprobs tests: an independent float64 reference (torch.log_softmax and a stable sort by
(-value, id), not ops/reference.py's code), the tolerance, and a wrapper that captures the logits rows an
engine's sampler saw."""

import math

import torch

from llm_map_reduce_summarizer_amd import ops

NINF = float("-inf")


def tol(lp: float) -> float:
    """|kernel - float64| allowed for a finite lp: x - m is exact in fp32 for bf16 operands, a hardware exp of
    an argument up to about 126 ln 2 carries about 1e-5 relative, the fixed-order sum and the log add a few
    1e-6, the final subtraction 2^-24 |lp|: about 3e-5 + 1.2e-7 |lp|, and the bound is about 3 x that."""
    return 1e-4 + 1e-6 * abs(lp)


def independent(row: torch.Tensor, n: int):
    """(lp float64 [V], [(token, lp)] top list) of one row of logits."""
    x = row.detach().to("cpu", torch.float64)
    lp = torch.log_softmax(x, dim=0)
    vals = x.tolist()
    order = sorted(range(len(vals)), key=lambda t: (-vals[t], t))[:max(n, 0)]  # -0.0 == 0.0 in Python too
    return lp, [(t, float(lp[t])) for t in order]


def close(got: float, want: float) -> bool:
    if math.isinf(want) or math.isinf(got):
        return got == want
    return abs(got - want) <= tol(want)


class SampleTap:
    """Wraps ``ops.sample`` for the length of a ``with``: keeps, per (seed, step) of every live row, a CPU
    copy of the logits row the sampler was handed (the seeds of the requests must differ)."""

    def __init__(self):
        self.rows = {}

    def __enter__(self):
        self._orig = ops.sample

        def tapped(logits, st, filtered=False):
            n = logits.shape[0]
            host = logits.detach().to("cpu")
            seeds, gen, done = st.seeds[:n].tolist(), st.gen_count[:n].tolist(), st.done[:n].tolist()
            for b in range(n):
                if not done[b]:
                    self.rows[(int(seeds[b]), int(gen[b]))] = host[b].clone()
            return self._orig(logits, st, filtered=filtered)

        ops.sample = tapped
        return self

    def __exit__(self, *exc):
        ops.sample = self._orig
        return False


def defined(row: torch.Tensor, n: int):
    """``independent``'s answer from the definition itself (ops/reference.py token_logprobs)."""
    from llm_map_reduce_summarizer_amd.ops import reference
    lp, tops = reference.token_logprobs(row, n)
    return lp[0], tops[0]


def check_records(out, rows, seed: int, top_n: int, exact: bool = False, ref=independent):
    """Every record of GenOutput ``out`` against the independent reference on the tapped rows; returns the
    largest |error| over the finite values.  ``exact``: the records are the reference's own float64 values
    rounded to fp32 (the CPU path, with ``ref=defined``)."""
    worst = 0.0
    assert len(out.logprobs) == len(out.top_logprobs) == len(out.token_ids)
    for g, (tok, got_lp, got_top) in enumerate(zip(out.token_ids, out.logprobs, out.top_logprobs)):
        lp, top = ref(rows[(seed, g)], top_n)
        want = float(lp[tok])
        assert [t for t, _ in got_top] == [t for t, _ in top], (seed, g)
        pairs = [(got_lp, want)] + [(a, b) for (_, a), (_, b) in zip(got_top, top)]
        for a, b in pairs:
            if exact and math.isfinite(b):
                assert a == float(torch.tensor(b, dtype=torch.float64).to(torch.float32)), (seed, g, a, b)
            else:
                assert close(a, b), (seed, g, a, b)
            if math.isfinite(b):
                worst = max(worst, abs(a - b))
        for t, a in got_top:  # the sampled token's value is its top-list entry, bit for bit
            if t == tok:
                assert a == got_lp, (seed, g)
    return worst
