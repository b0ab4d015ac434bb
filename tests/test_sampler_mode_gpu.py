"""All 16 sampler modes (engine.SamplerMode) through the engine on the GPU: an engine that replays decode graphs
and an eager one sample the same tokens and take the same log-probability records in every mode, every mode
but the plain one captures exactly one graph of its own under the literal key, and a second pass captures
none.  (The per-feature tests cover the kernels and the modes each feature added; this covers the table.)"""

import pytest

pytestmark = pytest.mark.gpu

from llm_map_reduce_summarizer_amd.engine.config import get_model_config  # noqa: E402
from llm_map_reduce_summarizer_amd.engine.engine import LLMEngine, SamplingParams  # noqa: E402

T, F = True, False
# (filtered, penalised, constrained, logprobs) -> decode-graph key of a batch of 2 in context class 0
KEYS = {
    (F, F, F, F): (2, 0),
    (T, F, F, F): (2, 0, True),
    (F, T, F, F): (2, 0, False, "pen"),
    (T, T, F, F): (2, 0, True, "pen"),
    (F, F, T, F): (2, 0, False, False, "con"),
    (T, F, T, F): (2, 0, True, False, "con"),
    (F, T, T, F): (2, 0, False, True, "con"),
    (T, T, T, F): (2, 0, True, True, "con"),
    (F, F, F, T): (2, 0, False, False, False, "lp"),
    (T, F, F, T): (2, 0, True, False, False, "lp"),
    (F, T, F, T): (2, 0, False, True, False, "lp"),
    (T, T, F, T): (2, 0, True, True, False, "lp"),
    (F, F, T, T): (2, 0, False, False, True, "lp"),
    (T, F, T, T): (2, 0, True, False, True, "lp"),
    (F, T, T, T): (2, 0, False, True, True, "lp"),
    (T, T, T, T): (2, 0, True, True, True, "lp"),
}
MODES = list(KEYS)
PROMPTS = [[128000] + [(i * 37 + j * 11) % 120000 + 5 for j in range(7)] for i in range(2)]  # 8 tokens each
N = 6
BIASED = 4321


def _params(mode, seed):
    f, p, c, lp = mode
    return SamplingParams(N, 0.8, seed, top_k=5 if f else 0, top_p=0.9 if f else 1.0,
                          repetition_penalty=1.3 if p else 1.0, logit_bias={BIASED: 5.0} if c else None,
                          logprobs=lp, top_logprobs=2 if lp else 0)


def _engine(use_graphs):
    return LLMEngine(get_model_config("tiny", init_std=0.05), device="cuda:0", max_model_len=512, max_num_seqs=4,
                     kv_pages=64, sync_every=4, max_new_cap=16, use_graphs=use_graphs)


def _run(eng, mode):
    outs = eng.generate(PROMPTS, [_params(mode, 40), _params(mode, 41)], ignore_eos=True)
    return [(o.token_ids, o.logprobs, o.top_logprobs) for o in outs]


@pytest.fixture(scope="module")
def runs():
    """mode -> what the graph engine gave on a first and a second pass, the graphs each pass captured and the
    keys the first one added, and what the eager engine gave."""
    graphs, eager = _engine(True), _engine(False)
    assert graphs.use_graphs and not eager.use_graphs
    out = {}
    for mode in MODES:  # the plain mode first: it leaves the one plain graph every other mode finds in place
        keys0, c0 = set(graphs._graphs), graphs.stats["graph_captures"]
        first = _run(graphs, mode)
        out[mode] = dict(first=first, new=set(graphs._graphs) - keys0, captured=graphs.stats["graph_captures"] - c0)
    for mode in MODES:
        c0 = graphs.stats["graph_captures"]
        out[mode].update(second=_run(graphs, mode), recaptured=graphs.stats["graph_captures"] - c0,
                         eager=_run(eager, mode))
    assert eager.stats["graph_captures"] == 0 and not eager._graphs
    assert set(graphs._graphs) == set(KEYS.values())
    return out


@pytest.mark.parametrize("mode", MODES, ids=["".join("fpcl"[i] if x else "-" for i, x in enumerate(m)) for m in MODES])
def test_every_mode_graphs_against_eager(runs, mode):
    r = runs[mode]
    assert all(len(ids) == N for ids, _, _ in r["first"])
    assert r["first"] == r["eager"] == r["second"]  # token ids, and the records of the logprobs modes, bit for bit
    for _, lps, tops in r["first"]:
        if mode[3]:
            assert len(lps) == N and [len(t) for t in tops] == [2] * N
        else:
            assert lps is None and tops is None
    # one graph per mode, under the literal key, captured on first use and replayed afterwards
    assert r["new"] == {KEYS[mode]} and r["captured"] == 1 and r["recaptured"] == 0
    assert [type(x) for x in next(iter(r["new"]))] == [type(x) for x in KEYS[mode]]


def test_the_modes_do_change_what_is_sampled(runs):
    """The 16 runs are not 16 copies of one: a filter, a penalty or a bias moves some token, asking for
    log-probabilities moves none."""
    ids = {m: [t for t, _, _ in runs[m]["first"]] for m in MODES}
    for m in MODES:
        assert ids[m] == ids[m[:3] + (False,)]
    assert len({str(ids[m]) for m in MODES if not m[3]}) > 1
