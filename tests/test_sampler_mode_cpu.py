"""The engine's sampler mode (engine.SamplerMode) and its one decode-slot writer (LLMEngine._setup_slot) without
a GPU.  Every expectation is a literal written down from the engine as it was when the mode still travelled as
four positional booleans and three places wrote a slot's rows: the decode-graph keys, the ops launches of
``_sample`` per mode (whole rows and the vocab-parallel shard path), what a first-token sample does, which
batches gather their logits, and the rows a request leaves in its slot however it is admitted."""

from types import SimpleNamespace

import pytest
import torch

from llm_map_reduce_summarizer_amd.engine import engine as engine_mod
from llm_map_reduce_summarizer_amd.engine.config import get_model_config
from llm_map_reduce_summarizer_amd.engine.engine import (DecodeState, ImportedPrefill, LLMEngine, SamplerMode,
                                                         SamplingParams)

T, F = True, False
NINF = float("-inf")

# (filtered, penalised, constrained, logprobs) -> decode-graph key of bucket 4 in context class 0
KEYS = {
    (F, F, F, F): (4, 0),
    (T, F, F, F): (4, 0, True),
    (F, T, F, F): (4, 0, False, "pen"),
    (T, T, F, F): (4, 0, True, "pen"),
    (F, F, T, F): (4, 0, False, False, "con"),
    (T, F, T, F): (4, 0, True, False, "con"),
    (F, T, T, F): (4, 0, False, True, "con"),
    (T, T, T, F): (4, 0, True, True, "con"),
    (F, F, F, T): (4, 0, False, False, False, "lp"),
    (T, F, F, T): (4, 0, True, False, False, "lp"),
    (F, T, F, T): (4, 0, False, True, False, "lp"),
    (T, T, F, T): (4, 0, True, True, False, "lp"),
    (F, F, T, T): (4, 0, False, False, True, "lp"),
    (T, F, T, T): (4, 0, True, False, True, "lp"),
    (F, T, T, T): (4, 0, False, True, True, "lp"),
    (T, T, T, T): (4, 0, True, True, True, "lp"),
}
# ... and in context class 1
KEYS_CLS1 = {
    (F, F, F, F): (4, 1),
    (T, F, F, F): (4, 1, True),
    (F, T, F, F): (4, 1, False, "pen"),
    (T, T, F, F): (4, 1, True, "pen"),
    (F, F, T, F): (4, 1, False, False, "con"),
    (T, F, T, F): (4, 1, True, False, "con"),
    (F, T, T, F): (4, 1, False, True, "con"),
    (T, T, T, F): (4, 1, True, True, "con"),
    (F, F, F, T): (4, 1, False, False, False, "lp"),
    (T, F, F, T): (4, 1, True, False, False, "lp"),
    (F, T, F, T): (4, 1, False, True, False, "lp"),
    (T, T, F, T): (4, 1, True, True, False, "lp"),
    (F, F, T, T): (4, 1, False, False, True, "lp"),
    (T, F, T, T): (4, 1, True, False, True, "lp"),
    (F, T, T, T): (4, 1, False, True, True, "lp"),
    (T, T, T, T): (4, 1, True, True, True, "lp"),
}
MODES = list(KEYS)

CON, PEN, LP, PICK = ("constrain", 0), ("penalize", 0), ("logprobs", None), ("logprobs_pick", None)
CON7, PEN7, TP7 = ("constrain", 7), ("penalize", 7), ("sample_tp", 7)
PLAIN, FILT = ("sample", False), ("sample", True)
# mode -> the ops launches of one _sample, as (name, tok_offset) or ("sample", filtered): whole rows ...
LAUNCHES = {
    (F, F, F, F): [PLAIN],
    (T, F, F, F): [FILT],
    (F, T, F, F): [PEN, PLAIN],
    (T, T, F, F): [PEN, FILT],
    (F, F, T, F): [CON, PLAIN],
    (T, F, T, F): [CON, FILT],
    (F, T, T, F): [CON, PEN, PLAIN],
    (T, T, T, F): [CON, PEN, FILT],
    (F, F, F, T): [LP, PLAIN, PICK],
    (T, F, F, T): [LP, FILT, PICK],
    (F, T, F, T): [PEN, LP, PLAIN, PICK],
    (T, T, F, T): [PEN, LP, FILT, PICK],
    (F, F, T, T): [CON, LP, PLAIN, PICK],
    (T, F, T, T): [CON, LP, FILT, PICK],
    (F, T, T, T): [CON, PEN, LP, PLAIN, PICK],
    (T, T, T, T): [CON, PEN, LP, FILT, PICK],
}
# ... and on a vocab-parallel engine whose shard starts at token 7: only the modes that need no whole rows stay
# on the shard (offset 7, sample_tp); a filtered or logprobs batch runs exactly as above
LAUNCHES_TP = {
    (F, F, F, F): [TP7],
    (T, F, F, F): [FILT],
    (F, T, F, F): [PEN7, TP7],
    (T, T, F, F): [PEN, FILT],
    (F, F, T, F): [CON7, TP7],
    (T, F, T, F): [CON, FILT],
    (F, T, T, F): [CON7, PEN7, TP7],
    (T, T, T, F): [CON, PEN, FILT],
    (F, F, F, T): [LP, PLAIN, PICK],
    (T, F, F, T): [LP, FILT, PICK],
    (F, T, F, T): [PEN, LP, PLAIN, PICK],
    (T, T, F, T): [PEN, LP, FILT, PICK],
    (F, F, T, T): [CON, LP, PLAIN, PICK],
    (T, F, T, T): [CON, LP, FILT, PICK],
    (F, T, T, T): [CON, PEN, LP, PLAIN, PICK],
    (T, T, T, T): [CON, PEN, LP, FILT, PICK],
}
WHOLE = {m for m in MODES if m[0] or m[3]}  # filtered or logprobs


@pytest.fixture(scope="module")
def eng():
    return LLMEngine(get_model_config("tiny", init_std=0.05), device="cpu", max_model_len=512, max_num_seqs=8,
                     kv_pages=64, sync_every=3)


MAX_U64 = object()


@pytest.fixture
def vocab_parallel(eng, monkeypatch):
    """The engine with a stand-in for the attributes of a vocab-parallel model that the sampler reads."""
    monkeypatch.setattr(eng, "model", SimpleNamespace(tp_sampling=True, vocab_offset=7,
                                                      custom_ar=SimpleNamespace(max_u64_=MAX_U64)))
    return eng


def _params(mode, n=4, seed=0):
    """SamplingParams whose four properties are exactly ``mode``."""
    f, p, c, lp = mode
    sp = SamplingParams(n, 0.8, seed, top_k=5 if f else 0, top_p=0.9 if f else 1.0,
                        repetition_penalty=1.3 if p else 1.0, logit_bias={17: 5.0} if c else None,
                        logprobs=lp, top_logprobs=2 if lp else 0)
    assert (sp.filtered, sp.penalised, sp.constrained, sp.logprobs) == mode
    return sp


def _seqs(mode):
    """A batch of three whose middle sequence alone carries ``mode``."""
    return [SimpleNamespace(params=sp) for sp in (_params(MODES[0]), _params(mode), _params(MODES[0]))]


# ------------------------------------------------------------------ the value
def test_mode_defaults_properties_and_first():
    assert tuple(SamplerMode()) == (False, False, False, False)
    assert SamplerMode._fields == ("filtered", "penalised", "constrained", "logprobs")
    with pytest.raises(AttributeError):
        SamplerMode().filtered = True  # immutable
    for m in MODES:
        mode = SamplerMode(*m)
        assert mode.whole is (m in WHOLE)
        assert tuple(mode.first()) == (m[0], False, m[2], m[3])
        assert tuple(SamplerMode.of(_seqs(m))) == m
        assert all(type(x) is bool for x in SamplerMode.of(_seqs(m)))
    assert tuple(SamplerMode.of([])) == (False, False, False, False)
    # flags of different rows add up
    both = [SimpleNamespace(params=_params((T, F, F, F))), SimpleNamespace(params=_params((F, F, T, F)))]
    assert tuple(SamplerMode.of(both)) == (True, False, True, False)


def test_view_carries_the_mode(eng):
    v = eng.state.view(1, 2)
    assert (v.filtered, v.penalised, v.constrained, v.logprobs) == (False, False, False, False)
    for m in MODES:
        v = eng.state.view(1, 2, SamplerMode(*m))
        assert (v.filtered, v.penalised, v.constrained, v.logprobs) == m and v.max_seqs == 2


# ------------------------------------------------------------------ 1. keys
@pytest.mark.parametrize("cls,keys", [(0, KEYS), (1, KEYS_CLS1)])
def test_graph_keys_are_the_literal_tuples(eng, monkeypatch, cls, keys):
    monkeypatch.setattr(eng, "_ctx_cls", cls)
    for m in MODES:
        k = eng._graph_key(4, SamplerMode(*m))
        assert k == keys[m] and [type(x) for x in k] == [type(x) for x in keys[m]], (m, k)
    assert len(set(keys.values())) == 16


# ------------------------------------------------------------------ 2. launch sequence
@pytest.fixture
def launches(monkeypatch):
    """The six sampler ops, as engine.py sees them, replaced by recorders (any other op is an error)."""
    rec = []

    def sample_tp(logits, st, tok_offset, max_reduce):
        assert max_reduce is MAX_U64
        rec.append(("sample_tp", tok_offset))

    monkeypatch.setattr(engine_mod, "ops", SimpleNamespace(
        constrain=lambda logits, st, tok_offset=0: rec.append(("constrain", tok_offset)),
        penalize=lambda logits, st, tok_offset=0: rec.append(("penalize", tok_offset)),
        logprobs=lambda logits, st: rec.append(("logprobs", None)),
        sample=lambda logits, st, filtered=False: rec.append(("sample", filtered)),
        sample_tp=sample_tp,
        logprobs_pick=lambda logits, st: rec.append(("logprobs_pick", None))))
    return rec


def _recorded(eng, rec, m):
    del rec[:]
    eng._sample(torch.zeros(2, 8, dtype=torch.bfloat16), eng.state.view(0, 2, SamplerMode(*m)))
    return list(rec)


def test_launch_sequence_on_whole_rows(eng, launches):
    assert not eng.model.tp_sampling
    for m in MODES:
        assert _recorded(eng, launches, m) == LAUNCHES[m], m


def test_launch_sequence_on_a_vocab_parallel_engine(vocab_parallel, launches):
    for m in MODES:
        assert _recorded(vocab_parallel, launches, m) == LAUNCHES_TP[m], m


def test_sample_reads_the_mode_from_the_view_attributes(eng, launches):
    """``_sample(logits, view)`` stays a two-argument method: a caller that sets the attributes of a plain view
    itself gets the same launches."""
    for m in MODES:
        v = eng.state.view(0, 2)
        v.filtered, v.penalised, v.constrained, v.logprobs = m
        del launches[:]
        eng._sample(torch.zeros(2, 8, dtype=torch.bfloat16), v)
        assert launches == LAUNCHES[m], m


# ------------------------------------------------------------------ 3. first token
def test_first_token_is_never_penalised(eng, monkeypatch):
    seen = []
    orig = eng._sample
    monkeypatch.setattr(eng, "_sample", lambda logits, v: (
        seen.append((v.filtered, v.penalised, v.constrained, v.logprobs)), orig(logits, v)))
    before = dict(eng.stats)
    out = eng.generate([[1, 2, 3, 4, 5]], [_params((T, T, T, T), n=1)])[0]
    assert len(out.token_ids) == 1 and len(out.logprobs) == 1 and len(out.top_logprobs[0]) == 2
    assert seen == [(True, False, True, True)]
    moved = {k: eng.stats[k] - before[k] for k in ("filtered_steps", "penalised_steps", "constrained_steps",
                                                   "logprob_steps", "decode_steps")}
    assert moved == {"filtered_steps": 1, "penalised_steps": 0, "constrained_steps": 1, "logprob_steps": 1,
                     "decode_steps": 0}


def test_decode_steps_count_every_flag(eng):
    before = dict(eng.stats)
    eng.generate([[1, 2, 3, 4, 5]], [_params((T, T, T, T), n=4)], ignore_eos=True)
    moved = {k: eng.stats[k] - before[k] for k in ("filtered_steps", "penalised_steps", "constrained_steps",
                                                   "logprob_steps", "decode_steps")}
    # the first token at the prefill, then 3 decode steps, which alone are penalised
    assert moved == {"filtered_steps": 4, "penalised_steps": 3, "constrained_steps": 4, "logprob_steps": 4,
                     "decode_steps": 3}
    before = dict(eng.stats)
    eng.generate([[1, 2, 3, 4, 5]], [_params((F, F, F, F), n=4)], ignore_eos=True)
    assert all(eng.stats[k] == before[k] for k in ("filtered_steps", "penalised_steps", "constrained_steps",
                                                   "logprob_steps"))


# ------------------------------------------------------------------ 4. gather
def test_gather_without_vocab_parallel_sampling_is_always_on(eng):
    assert all(eng._gather(_seqs(m)) is True for m in MODES)


def test_gather_on_a_vocab_parallel_engine_follows_whole(vocab_parallel):
    assert {m for m in MODES if vocab_parallel._gather(_seqs(m))} == WHOLE
    assert len(WHOLE) == 12 and vocab_parallel._gather([]) is False


# ------------------------------------------------------------------ 5. slots
PROMPT = [11, 12, 13, 14, 15, 16, 17]
# every parameter away from its default (the floats are exact in fp32)
LOADED = dict(max_new_tokens=4, temperature=0.75, seed=1234567891011, top_k=2 ** 31 + 5, top_p=0.875,
              frequency_penalty=0.5, presence_penalty=-0.75, repetition_penalty=1.25,
              logit_bias={17: 2.5, 23: NINF}, min_tokens=2, stop_token_ids=[301, 302], logprobs=True, top_logprobs=3)
ROWS = dict(max_new=4, gen_count=0, done=0, temps=0.75, seeds=1234567891011, top_k=2 ** 31 - 1, top_p=0.875,
            rep_pen=1.25, freq_pen=0.5, pres_pen=-0.75, bias_n=2, bias_tok=[17, 23], bias_val=[2.5, NINF],
            min_new=2, stop_ids=[301, 302, -1, -1], lp_n=3, result=0)
JUNK = dict(block_tables=3, max_new=77, gen_count=5, done=1, temps=9.0, seeds=99, top_k=3, top_p=0.5, rep_pen=2.0,
            freq_pen=3.0, pres_pen=4.0, bias_n=7, bias_tok=5, bias_val=6.0, min_new=6, stop_ids=5, lp_n=11, result=9)


def _soil(eng, slot):
    """The slot's rows as a previous tenant might have left them: none at the value the request needs."""
    for f, x in JUNK.items():
        getattr(eng.state, f)[slot] = x


@pytest.fixture
def slots(eng, monkeypatch):
    """Spy on ``_setup_slot``: every call, with the slot's parameter rows as they stand right after it."""
    calls = []
    orig = eng._setup_slot

    def spy(s, row):
        orig(s, row)
        st, i = eng.state, s.slot
        rows = {f: getattr(st, f)[i].tolist() for f in ROWS if f not in ("bias_tok", "bias_val")}
        rows["bias_tok"], rows["bias_val"] = st.bias_tok[i, :2].tolist(), st.bias_val[i, :2].tolist()
        calls.append(SimpleNamespace(seed=s.params.seed, slot=i, rows=rows, pages=list(s.pages),
                                     table=st.block_tables[i].tolist()))

    monkeypatch.setattr(eng, "_setup_slot", spy)
    return calls


def _check(call, slot, **other):
    assert call.slot == slot and call.rows == dict(ROWS, **other)
    assert call.pages and call.table == call.pages + [0] * (len(call.table) - len(call.pages))


def _loaded_calls(calls):
    return [c for c in calls if c.seed == LOADED["seed"]]


def test_the_literal_rows_cover_every_parameter_row():
    assert set(ROWS) | {"block_tables"} == set(JUNK)
    # the rows of a slot that no request parameter decides are the sampler's own
    assert set(DecodeState._ROW_FIELDS) - set(JUNK) == {"next_ids", "positions", "out_tokens", "thresh"}


@pytest.mark.parametrize("ignore_eos,other", [(False, {}), (True, {"stop_ids": [-1, -1, -1, -1]})])
def test_slot_rows_of_a_blocking_admission(eng, slots, ignore_eos, other):
    _soil(eng, 0)
    out = eng.generate([PROMPT], [SamplingParams(**LOADED)], ignore_eos=ignore_eos)[0]
    assert len(slots) == 1 and 1 <= len(out.token_ids) <= 4
    _check(slots[0], 0, **other)


def test_slot_rows_of_a_request_that_joins_a_running_batch(eng, slots):
    assert eng.interleave
    _soil(eng, 1)
    fed = []

    def feeder(done):
        if not fed:
            fed.append(1)
            return [(PROMPT, SamplingParams(**LOADED))]
        return []

    n0 = eng.stats.get("interleaved_prefills", 0)
    outs = eng.generate([[1, 2, 3]], [SamplingParams(9, 0.0, 0)], ignore_eos=True, feeder=feeder)
    assert len(outs) == 2 and eng.stats["interleaved_prefills"] == n0 + 1
    assert len(slots) == 2 and len(_loaded_calls(slots)) == 1  # once per admission
    _check(_loaded_calls(slots)[0], 1, stop_ids=[-1, -1, -1, -1])
    # with the row's stop ids armed: the same rows, by the same path
    del slots[:], fed[:]
    _soil(eng, 1)
    outs = eng.generate([[1, 2, 3]], [SamplingParams(9, 0.0, 0)], feeder=feeder)
    assert len(outs) == 2 and eng.stats["interleaved_prefills"] == n0 + 2
    assert len(slots) == 2 and len(_loaded_calls(slots)) == 1
    _check(_loaded_calls(slots)[0], 1)


def _imported():
    return ImportedPrefill(first_token=40, kv=None, first_logprobs=(-0.5, [(40, -0.5), (6, -1.0), (7, -2.0)]))


def test_slot_rows_of_an_imported_prefill(eng, slots):
    _soil(eng, 0)
    n0 = eng.stats.get("imported_prefills", 0)
    out = eng.generate([PROMPT], [SamplingParams(**LOADED)], imported={0: _imported()})[0]
    assert out.token_ids[0] == 40 and out.logprobs[0] == -0.5 and eng.stats["imported_prefills"] == n0 + 1
    assert len(slots) == 1
    _check(slots[0], 0)


def test_slot_rows_of_an_imported_prefill_that_joins_a_running_batch(eng, slots):
    """``_admit_interleaved`` installs an imported prefill at once, in the next decode slot."""
    running = SimpleNamespace(slot=0)
    s = eng._new_seq(0, PROMPT, SamplingParams(**LOADED), _imported())
    waiting, active, prefilling = [s], [running], []
    _soil(eng, 1)
    free = eng.kv.alloc.available()
    try:
        eng._admit_interleaved(waiting, active, prefilling)
        assert (waiting, active, prefilling) == ([], [running, s], [])
        assert len(slots) == 1
        _check(slots[0], 1)
        assert int(eng.state.gen_count[1]) == 1 and int(eng.state.next_ids[1]) == 40  # installed afterwards
    finally:
        eng.kv.alloc.free(s.pages)
        eng.state.park_row(1)
    assert eng.kv.alloc.available() == free


CP_SPY = """
import json, os, sys
sys.path.insert(0, %(root)r)
from llm_map_reduce_summarizer_amd.parallel import dist as pdist
pdist.init_distributed_from_env(backend="gloo", timeout_s=120)
world, rank = int(os.environ["WORLD_SIZE"]), int(os.environ["RANK"])
from llm_map_reduce_summarizer_amd.engine.config import get_model_config
from llm_map_reduce_summarizer_amd.engine.engine import LLMEngine, SamplingParams
eng = LLMEngine(get_model_config("tiny-kv8", init_std=0.05), device="cpu", max_model_len=256, max_num_seqs=2,
                kv_pages=16, sync_every=3)
calls = []
orig = eng._setup_slot
def spy(s, row):
    orig(s, row)
    st = eng.state
    calls.append({"slot": s.slot, "pages": list(s.pages), "table": st.block_tables[0].tolist(),
                  "rows": {f: getattr(st, f)[0].tolist() for f in %(fields)r}})
eng._setup_slot = spy
for f, x in %(junk)r.items():
    getattr(eng.state, f)[0] = x
sp = SamplingParams(**%(loaded)r)
sp.logit_bias = {17: 2.5, 23: float("-inf")}
first, kv = eng.prefill_export_cp(list(range(5, 45)), sp, rank, world, group=pdist.tp_group_for(world))
print("RESULT " + json.dumps({"first": first, "calls": calls, "done": int(eng.state.done[0]),
                              "free": eng.kv.alloc.available(), "pages": eng.kv.num_pages}), flush=True)
pdist.shutdown()
"""


@pytest.mark.slow
def test_context_parallel_prefill_sets_its_slot_up_through_the_one_writer():
    """``prefill_export_cp`` is collective: two CPU ranks over gloo, the smallest world of the context-parallel
    tests.  It borrows slot 0 for a one-token request without logprobs; the other rows are the request's."""
    from test_dist_world8_cpu import ROOT, _launch
    fields = [f for f in ROWS if f not in ("bias_tok", "bias_val")]
    loaded = dict(LOADED, logit_bias=None)  # (-inf has no literal: the script puts the bias back)
    outs = _launch(CP_SPY % {"root": ROOT, "fields": fields, "junk": JUNK, "loaded": loaded}, 2, {})
    want = {f: ROWS[f] for f in fields}
    want.update(max_new=1, min_new=1, lp_n=-1)
    for o in outs:
        assert len(o["calls"]) == 1
        c = o["calls"][0]
        assert c["slot"] == 0 and c["rows"] == want
        assert c["pages"] and c["table"] == c["pages"] + [0] * (len(c["table"]) - len(c["pages"]))
        assert o["done"] == 1 and o["free"] == o["pages"] - 1  # parked again, pages returned
    assert outs[0]["first"] == outs[1]["first"]
