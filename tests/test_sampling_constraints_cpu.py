"""logit_bias / min_tokens / stop_token_ids without a GPU: the rule (ops/reference.py apply_constraints, the
definition sampler.hip's constrain kernel matches bit for bit), the engine on the CPU path, and the public
interface (SamplingParams limits, requests, HTTP bodies, hosted providers, CLI flags and the environment).
The HTTP server itself is tests/test_serve_constraints.py."""

import asyncio
import json
from dataclasses import asdict

import pytest
import torch

from llm_map_reduce_summarizer_amd import ops
from llm_map_reduce_summarizer_amd.cli import build_parser, config_from_args
from llm_map_reduce_summarizer_amd.config import LLMConfig, parse_logit_bias
from llm_map_reduce_summarizer_amd.engine.config import get_model_config
from llm_map_reduce_summarizer_amd.engine.engine import DecodeState, LLMEngine, SamplingParams
from llm_map_reduce_summarizer_amd.engine.provider import sampling_params
from llm_map_reduce_summarizer_amd.ops import reference
from llm_map_reduce_summarizer_amd.pipeline.providers import (GenRequest, logit_bias_pairs, make_provider,
                                                              request_constraints)
from llm_map_reduce_summarizer_amd.serve import BadRequest, anthropic_request, openai_request

NINF, INF = float("-inf"), float("inf")
NONE4 = [-1, -1, -1, -1]


def _row(vals):
    return torch.tensor([vals], dtype=torch.float32).to(torch.bfloat16)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _apply(rows, bias=(), gen=0, min_new=0, stops=NONE4, eos=NONE4, done=None, tok_offset=0, width=6):
    """reference.apply_constraints on one or more rows that all carry the same constraints."""
    n = rows.shape[0]
    bt = torch.zeros(n, width, dtype=torch.int32)
    bv = torch.zeros(n, width, dtype=torch.float32)
    for i, (t, x) in enumerate(bias):
        bt[:, i], bv[:, i] = t, x
    i32 = lambda x: torch.tensor([x] * n, dtype=torch.int32)  # noqa: E731
    return reference.apply_constraints(rows, bt, bv, i32(len(bias)), i32(gen), i32(min_new),
                                       torch.tensor([stops] * n, dtype=torch.int32),
                                       torch.tensor(eos, dtype=torch.int32), done, tok_offset)


# name, row, bias entries, keyword arguments, expected row -- every value a bf16, worked out by hand.  bf16
# keeps 8 significant bits: between 256 and 512 its values are 2 apart.
HAND = [
    ("sum_rounds_to_the_same_bf16", [256.0, 1.0], [(0, 0.5)], {}, [256.0, 1.0]),
    ("sum_rounds_up", [256.0, 1.0], [(0, 1.5)], {}, [258.0, 1.0]),
    ("tie_rounds_to_even", [256.0, 258.0], [(0, 1.0), (1, 1.0)], {}, [256.0, 260.0]),
    ("plus_and_minus_100", [1.0, 1.0, 1.0], [(0, 100.0), (2, -100.0)], {}, [101.0, 1.0, -99.0]),
    ("ban_finite_and_plus_inf", [3.0, INF, 2.0], [(0, NINF), (1, NINF)], {}, [NINF, NINF, 2.0]),
    ("bias_on_minus_inf", [NINF, 1.0], [(0, 5.0)], {}, [NINF, 1.0]),
    ("bias_on_plus_inf", [INF, 1.0], [(0, -100.0)], {}, [INF, 1.0]),
    ("suppression_wins_over_plus_100", [1.0, 2.0, 3.0, 4.0], [(1, 100.0), (2, 100.0)],
     dict(gen=1, min_new=2, stops=[1, -1, -1, -1], eos=[-1, 3, -1, -1]), [1.0, NINF, 103.0, NINF]),
    ("gen_count_equal_min_new_suppresses_nothing", [1.0, 2.0, 3.0, 4.0], [(1, 1.0)],
     dict(gen=2, min_new=2, stops=[1, 0, -1, -1], eos=[3, -1, -1, -1]), [1.0, 3.0, 3.0, 4.0]),
    ("suppression_without_a_bias", [1.0, 2.0, 3.0], [], dict(gen=0, min_new=1, stops=[-1, -1, -1, 2]),
     [1.0, 2.0, NINF]),
    ("stop_ids_outside_the_row_are_skipped", [1.0, 2.0], [(7, 5.0)], dict(gen=0, min_new=1, stops=[9, -1, -1, -1],
                                                                        eos=[2, 1, -1, -1]), [1.0, NINF]),
]


@pytest.mark.parametrize("name,row,bias,kw,expect", HAND, ids=[h[0] for h in HAND])
def test_hand_written_rows(name, row, bias, kw, expect):
    r = _row(row)
    got = _apply(r, bias, **kw)
    assert got.data_ptr() == r.data_ptr() and got.dtype == torch.bfloat16  # in place, returned
    assert got[0].float().tolist() == expect


def test_nan_logit_stays_nan():
    got = _apply(_row([float("nan"), float("nan"), 1.0]), [(0, 3.0), (1, NINF)])
    assert torch.isnan(got[0, 0]) and torch.isnan(got[0, 1]) and float(got[0, 2]) == 1.0


def test_done_and_neutral_rows_keep_every_bit():
    g = torch.Generator().manual_seed(3)
    rows = (torch.randn(2, 33, generator=g) * 4).to(torch.bfloat16)
    rows[0, 5], rows[1, 6] = -0.0, INF
    keep = rows.clone()
    # done: biased, suppressing -- and untouched
    _apply(rows, [(5, 7.0), (6, NINF)], gen=0, min_new=3, stops=[1, 2, 3, 4], done=torch.ones(2, dtype=torch.int32))
    assert torch.equal(_bits(rows), _bits(keep))
    # neutral: no entry, gen_count >= min_new (stop ids armed, but nothing to suppress)
    _apply(rows, [], gen=0, min_new=0, stops=[1, 2, 3, 4], eos=[5, 6, 7, 8])
    assert torch.equal(_bits(rows), _bits(keep))
    _apply(rows, [(5, 7.0)], gen=0, min_new=3, stops=[1, 2, 3, 4])  # (the same calls do act on a live row)
    assert not torch.equal(_bits(rows), _bits(keep))


@pytest.mark.parametrize("cuts", [(0, 37, 101), (0, 1, 64, 101), (0, 100, 101)])
def test_shards_equal_the_whole_row(cuts):
    V = 101
    g = torch.Generator().manual_seed(V)
    rows = (torch.randn(3, V, generator=g) * 6).to(torch.bfloat16)
    # entries on both edges of every cut, at columns 0 and V - 1; stop ids in different shards
    bias = [(0, 1.3), (V - 1, NINF), (36, 0.7), (37, -50.0), (63, 100.0), (64, NINF), (99, 3.1), (100 - 50, -0.01)]
    kw = dict(gen=1, min_new=4, stops=[36, 100, -1, 64], eos=[0, -1, 70, -1], width=len(bias))
    whole = _apply(rows.clone(), bias, **kw)
    assert not torch.equal(_bits(whole), _bits(rows))
    parts = [_apply(rows[:, a:b].clone(), bias, tok_offset=a, **kw) for a, b in zip(cuts, cuts[1:])]
    assert torch.equal(_bits(torch.cat(parts, dim=1)), _bits(whole))


# ------------------------------------------------------------------ SamplingParams
def test_constrained_property_and_neutral_defaults():
    sp = SamplingParams(8, 0.7, 0)
    assert (sp.logit_bias, sp.min_tokens, tuple(sp.stop_token_ids)) == (None, 0, ()) and not sp.constrained
    sp.validate(1000)
    assert not SamplingParams(8, 0.7, 0, logit_bias={}, min_tokens=0, stop_token_ids=[]).constrained
    for kw in (dict(logit_bias={5: 1.0}), dict(logit_bias=[(5, NINF)]), dict(min_tokens=1), dict(stop_token_ids=[7])):
        sp = SamplingParams(8, 0.0, 0, **kw)  # greedy rows are constrained too
        sp.validate(1000)
        assert sp.constrained
    assert SamplingParams(8, 0.7, 0, logit_bias={5: 1, 6: NINF}).bias_items() == [(5, 1), (6, NINF)]
    assert SamplingParams(8, 0.7, 0, logit_bias=((5, -100), (6, 100.0))).bias_items() == [(5, -100), (6, 100.0)]


OK_AT_THE_LIMITS = [dict(logit_bias={i: 0.5 for i in range(300)}), dict(logit_bias={0: 100, 999: -100.0}),
                    dict(stop_token_ids=[0, 999, 5, 5]), dict(min_tokens=8), dict(min_tokens=0)]
REFUSED = [dict(logit_bias={i: 0.5 for i in range(301)}), dict(logit_bias={1000: 1.0}), dict(logit_bias={-1: 1.0}),
           dict(logit_bias={"5": 1.0}), dict(logit_bias={5.0: 1.0}), dict(logit_bias={True: 1.0}),
           dict(logit_bias={5: 100.5}), dict(logit_bias={5: -101}), dict(logit_bias={5: INF}),
           dict(logit_bias={5: float("nan")}), dict(logit_bias={5: "1"}), dict(logit_bias={5: None}),
           dict(logit_bias={5: True}), dict(logit_bias=[(5, 1.0), (5, 2.0)]), dict(logit_bias=[5, 1.0]),
           dict(logit_bias="5:1"), dict(logit_bias=5),
           dict(stop_token_ids=[1, 2, 3, 4, 5]), dict(stop_token_ids=[1000]), dict(stop_token_ids=[-1]),
           dict(stop_token_ids=[1.0]), dict(stop_token_ids="12"), dict(stop_token_ids=7), dict(stop_token_ids=[True]),
           dict(min_tokens=9), dict(min_tokens=-1), dict(min_tokens=1.0), dict(min_tokens=True), dict(min_tokens=None)]


@pytest.mark.parametrize("ok", OK_AT_THE_LIMITS)
def test_validate_accepts_the_limits(ok):
    SamplingParams(8, 0.7, 0, **ok).validate(1000)


@pytest.mark.parametrize("bad", REFUSED)
def test_validate_refuses(bad):
    with pytest.raises(ValueError):
        SamplingParams(8, 0.7, 0, **bad).validate(1000)


def test_validate_without_a_vocabulary_checks_the_rest():
    SamplingParams(8, 0.7, 0, logit_bias={10 ** 6: 1.0}, stop_token_ids=[10 ** 6]).validate()
    with pytest.raises(ValueError):
        SamplingParams(8, 0.7, 0, logit_bias={10 ** 6: 101.0}).validate()


# ------------------------------------------------------------------ engine on the reference ops
@pytest.fixture(scope="module")
def eng():
    return LLMEngine(get_model_config("tiny", init_std=0.05), device="cpu", max_model_len=512, max_num_seqs=8,
                     kv_pages=64, sync_every=3)


PROMPTS = [[1, 2, 3, 4, 5], [9, 8, 7], [5, 5, 5, 5, 5, 5, 5], [11, 12]]
N = 16
TEMP = 1.0


def _ids(outs):
    return [o.token_ids for o in outs]


def test_state_rows_exist_are_listed_and_parked(eng):
    st = eng.state
    assert tuple(st.bias_tok.shape) == (8, 300) and st.bias_tok.dtype == torch.int32
    assert tuple(st.bias_val.shape) == (8, 300) and st.bias_val.dtype == torch.float32
    assert tuple(st.stop_ids.shape) == (8, 4) and st.stop_ids.dtype == torch.int32
    assert st.bias_n.dtype == st.min_new.dtype == torch.int32
    for f in ("bias_tok", "bias_val", "bias_n", "min_new", "stop_ids"):
        assert f in DecodeState._ROW_FIELDS
    st.bias_n[2], st.min_new[2] = 5, 9
    st.stop_ids[2] = torch.tensor([4, 5, 6, 7], dtype=torch.int32)
    st.move_row(2, 3)
    assert int(st.bias_n[3]) == 5 and int(st.min_new[3]) == 9 and st.stop_ids[3].tolist() == [4, 5, 6, 7]
    for i in (2, 3):
        st.park_row(i)
        assert int(st.bias_n[i]) == 0 and int(st.min_new[i]) == 0 and st.stop_ids[i].tolist() == NONE4
    assert st.view(0, 2).constrained is False


def test_ops_constrain_runs_the_reference_on_cpu_rows(eng):
    st = eng.state.view(0, 1)
    st.bias_tok[0, :2] = torch.tensor([1, 3], dtype=torch.int32)
    st.bias_val[0, :2] = torch.tensor([2.0, NINF])
    st.bias_n[0], st.min_new[0], st.gen_count[0], st.done[0] = 2, 1, 0, 0
    st.stop_ids[0] = torch.tensor([2, -1, -1, -1], dtype=torch.int32)
    try:
        got = ops.constrain(_row([1.0, 1.0, 1.0, 1.0, 1.0]), st)
        assert got[0].float().tolist() == [1.0, 3.0, NINF, NINF, 1.0]
        got = ops.constrain(_row([1.0, 1.0, 1.0]), st, tok_offset=2)  # the shard of tokens 2, 3, 4
        assert got[0].float().tolist() == [NINF, NINF, 1.0]
    finally:
        eng.state.park_row(0)


def test_plus_100_greedy_generates_only_that_token(eng):
    t = 4321
    n0 = eng.stats["constrained_steps"]
    out = eng.generate(PROMPTS, [SamplingParams(N, 0.0, 0, logit_bias={t: 100.0})] * 4, ignore_eos=True)
    assert _ids(out) == [[t] * N] * 4
    assert eng.stats["constrained_steps"] >= n0 + N  # every decode step, and the first token at the prefill


def test_banning_every_token_of_a_greedy_run_yields_none_of_them(eng):
    plain = _ids(eng.generate(PROMPTS, [SamplingParams(N, 0.0, 0)] * 4, ignore_eos=True))
    sp = [SamplingParams(N, 0.0, 0, logit_bias={t: NINF for t in set(p)}) for p in plain]
    banned = _ids(eng.generate(PROMPTS, sp, ignore_eos=True))
    for p, b in zip(plain, banned):
        assert len(b) == N and not set(b) & set(p)


def test_unconstrained_row_is_batch_invariant(eng):
    plain = SamplingParams(N, TEMP, 5)
    solo = _ids(eng.generate(PROMPTS[1:2], [plain], ignore_eos=True))[0]
    n0 = eng.stats["constrained_steps"]
    all_plain = _ids(eng.generate(PROMPTS, [SamplingParams(N, TEMP, 4), plain, SamplingParams(N // 2, 0.0, 1),
                                            SamplingParams(N, TEMP, 7)], ignore_eos=True))
    assert eng.stats["constrained_steps"] == n0  # no constrained row: no constrained step
    mixed = _ids(eng.generate(PROMPTS, [SamplingParams(N, TEMP, 4, logit_bias={solo[0]: NINF, solo[3]: -5.0}), plain,
                                        SamplingParams(N // 2, 0.0, 1, min_tokens=4, stop_token_ids=[solo[1]]),
                                        SamplingParams(N, TEMP, 7, stop_token_ids=[solo[2]], logit_bias={77: 100})],
                              ignore_eos=True))
    assert eng.stats["constrained_steps"] > n0
    assert mixed[1] == solo == all_plain[1]
    assert mixed[3] == [77] * N  # (ignore_eos: the row's stop id is disarmed, the bias acts)


def _first_occurrence(tokens, lo=2):
    """(s, token): the first step s >= lo whose token occurs there for the first time."""
    return next((s, t) for s, t in enumerate(tokens) if s >= lo and t not in tokens[:s])


@pytest.fixture(scope="module")
def sampled(eng):
    """An unconstrained sampled run of every prompt, with the engine's EOS ids armed."""
    outs = eng.generate(PROMPTS, [SamplingParams(N, TEMP, 20 + i) for i in range(4)])
    assert all(len(o.token_ids) == N and o.finish_reason == "length" for o in outs)
    return _ids(outs)


def test_stop_token_ids_cut_the_run_at_the_stop_id(eng, sampled):
    cuts = [_first_occurrence(t) for t in sampled]
    sp = [SamplingParams(N, TEMP, 20 + i, stop_token_ids=[99999, cuts[i][1]]) for i in range(4)]
    outs = eng.generate(PROMPTS, sp)
    for o, base, (s, t) in zip(outs, sampled, cuts):
        assert o.token_ids == base[:s + 1] and o.token_ids[-1] == t and o.finish_reason == "stop"


def test_min_tokens_keeps_the_stop_id_out_until_then(eng, sampled):
    cuts = [_first_occurrence(t) for t in sampled]
    outs = []
    for i, (s, t) in enumerate(cuts):  # one by one: every row its own minimum
        m = s + 3
        o = eng.generate(PROMPTS[i:i + 1], [SamplingParams(N, TEMP, 20 + i, stop_token_ids=[t], min_tokens=m)])[0]
        # removing a token that does not win leaves a Gumbel-max where it was: the first s tokens stay
        assert o.token_ids[:s] == sampled[i][:s]
        assert t not in o.token_ids[:m] and len(o.token_ids) >= m
        assert o.finish_reason == ("stop" if o.token_ids[-1] == t else "length")
        outs.append(o)
    assert any(o.token_ids[s] != sampled[i][s] for i, ((s, _), o) in enumerate(zip(cuts, outs)))


def test_min_tokens_suppresses_the_engine_eos_ids(eng):
    """+100 on an EOS id and greedy: the run ends at once without a minimum, and with min_tokens = m the
    EOS id comes exactly at step m."""
    eos = eng.state.eos_ids[0]
    o = eng.generate(PROMPTS[:1], [SamplingParams(N, 0.0, 0, logit_bias={eos: 100.0})])[0]
    assert o.token_ids == [eos] and o.finish_reason == "stop"
    o = eng.generate(PROMPTS[:1], [SamplingParams(N, 0.0, 0, logit_bias={eos: 100.0}, min_tokens=5)])[0]
    assert len(o.token_ids) == 6 and eos not in o.token_ids[:5] and o.token_ids[5] == eos
    assert o.finish_reason == "stop"


def test_ignore_eos_disarms_the_row_stop_ids(eng, sampled):
    s, t = _first_occurrence(sampled[0])
    sp = SamplingParams(N, TEMP, 20, stop_token_ids=[t], min_tokens=N)
    o = eng.generate(PROMPTS[:1], [sp], ignore_eos=True)[0]
    assert o.token_ids == sampled[0] and o.finish_reason == "length"  # nothing stops, nothing is suppressed
    o = eng.generate(PROMPTS[:1], [sp])[0]  # armed again afterwards: the same request now runs past the stop id
    assert t not in o.token_ids and o.token_ids[:s] == sampled[0][:s] and len(o.token_ids) == N


def test_window_counts_armed_row_stops_like_an_armed_eos(eng):
    keep = list(eng.state.eos_ids)
    eng.state.set_eos([])
    try:
        assert eng._window([40, 50], False) == 40
        assert eng._window([40, 50], False, True) == eng.sync_every
    finally:
        eng.state.set_eos(keep)


def test_imported_first_token_that_is_a_row_stop_id_finishes_at_once(eng, sampled):
    from llm_map_reduce_summarizer_amd.engine.engine import ImportedPrefill
    imp = {0: ImportedPrefill(first_token=4242, kv=None)}
    o = eng.generate(PROMPTS[:1], [SamplingParams(N, TEMP, 1, stop_token_ids=[4242])], imported=imp)[0]
    assert o.token_ids == [4242] and o.finish_reason == "stop"


def test_prefill_export_constrains_the_first_token(eng):
    firsts, _ = eng.prefill_export(PROMPTS[:2], [SamplingParams(N, 0.0, 0, logit_bias={555: 100.0}, min_tokens=9),
                                                 SamplingParams(N, 0.0, 0)], groups=1)
    plain, _ = eng.prefill_export(PROMPTS[:2], [SamplingParams(N, 0.0, 0)] * 2, groups=1)
    assert firsts[0] == 555 and firsts[1] == plain[1] != 555


def test_invalid_values_raise_at_generate(eng):
    for bad in (dict(logit_bias={128256: 1.0}), dict(stop_token_ids=[128256]), dict(min_tokens=4)):
        with pytest.raises(ValueError):
            eng.generate(PROMPTS[:1], [SamplingParams(3, 0.7, 0, **bad)])


# ------------------------------------------------------------------ requests, providers, CLI
MSGS = [{"role": "user", "content": "u"}]


def _cons(r):
    return (r.logit_bias, r.min_tokens, r.stop_token_ids)


@pytest.mark.parametrize("make", [openai_request, anthropic_request])
def test_http_requests_carry_the_fields(make):
    r = make({"messages": MSGS, "max_tokens": 50, "logit_bias": {"15": -100, 27: 3.5}, "min_tokens": 20,
              "stop_token_ids": [7, 8]})
    assert _cons(r) == ([[15, -100.0], [27, 3.5]], 20, [7, 8])
    assert _cons(make({"messages": MSGS})) == (None, None, None)
    assert _cons(make({"messages": MSGS, "logit_bias": None, "min_tokens": None, "stop_token_ids": None})) == \
        (None, None, None)
    r = make({"messages": MSGS, "logit_bias": {}, "min_tokens": 0, "stop_token_ids": []})
    assert _cons(r) == ([], 0, [])  # explicit neutral values are the request's own: they win over the config
    r = make({"messages": MSGS, "max_tokens": 7, "min_tokens": 7, "logit_bias": {str(i): 100 for i in range(300)},
              "stop_token_ids": [1, 2, 3, 4]}, 1.0, 128256)
    assert len(r.logit_bias) == 300 and r.min_tokens == 7 and r.stop_token_ids == [1, 2, 3, 4]
    multi = MSGS + [{"role": "assistant", "content": "a"}, {"role": "user", "content": "b"}]
    assert _cons(make({"messages": multi, "min_tokens": 3, "top_p": 0.5})) == (None, 3, None)


BAD_BODIES = [{"logit_bias": {str(i): 1 for i in range(301)}}, {"logit_bias": {"5": 100.5}},
              {"logit_bias": {"5": -101}},
              {"logit_bias": {"5": "1"}}, {"logit_bias": {"5": None}}, {"logit_bias": {"5": True}},
              {"logit_bias": {"5": float("nan")}}, {"logit_bias": {"5": float("-inf")}}, {"logit_bias": {"x": 1}},
              {"logit_bias": {"-5": 1}}, {"logit_bias": {"5.0": 1}}, {"logit_bias": [[5, 1]]}, {"logit_bias": "5:1"},
              {"logit_bias": {"5": 1, " 5": 2}}, {"min_tokens": -1}, {"min_tokens": 11}, {"min_tokens": 1.5},
              {"min_tokens": "3"}, {"min_tokens": True}, {"stop_token_ids": [1, 2, 3, 4, 5]}, {"stop_token_ids": 7},
              {"stop_token_ids": ["7"]}, {"stop_token_ids": [-1]}, {"stop_token_ids": [1.0]},
              {"stop_token_ids": [True]},
              {"stop": ["\n"]}, {"n": 2}]


@pytest.mark.parametrize("make", [openai_request, anthropic_request])
@pytest.mark.parametrize("bad", BAD_BODIES)
def test_http_bad_values_are_refused(make, bad):
    with pytest.raises(BadRequest):
        make(dict({"messages": MSGS, "max_tokens": 10}, **bad))


@pytest.mark.parametrize("make", [openai_request, anthropic_request])
def test_http_token_ids_are_checked_against_the_vocabulary(make):
    make({"messages": MSGS, "logit_bias": {"999": 1}, "stop_token_ids": [999]}, 1.0, 1000)
    for bad in ({"logit_bias": {"1000": 1}}, {"stop_token_ids": [1000]}):
        with pytest.raises(BadRequest):
            make(dict({"messages": MSGS}, **bad), 1.0, 1000)


def test_gen_request_survives_the_json_broadcast():
    r = GenRequest(user="u", max_tokens=9, logit_bias=[[15, -100.0], [27, "ban"], [3, 0.25]], min_tokens=4,
                   stop_token_ids=[7, 8])
    back = GenRequest(**json.loads(json.dumps(asdict(r), allow_nan=False)))
    assert back == r
    sp = sampling_params(back, 0, LLMConfig())
    assert sp.bias_items() == [(15, -100.0), (27, NINF), (3, 0.25)]
    assert (sp.min_tokens, tuple(sp.stop_token_ids)) == (4, (7, 8)) and sp.constrained
    sp.validate(128256)
    # a request built by the server round-trips the same way
    r = openai_request({"messages": MSGS, "logit_bias": {"15": -100}, "min_tokens": 2, "stop_token_ids": [5]})
    assert GenRequest(**json.loads(json.dumps(asdict(r), allow_nan=False))) == r


def test_logit_bias_forms_are_normalised():
    want = [(5, 1.5), (6, NINF)]
    for form in ({5: 1.5, 6: NINF}, {"5": 1.5, "6": "ban"}, [[5, 1.5], [6, None]], ((5, 1.5), (6, "BAN"))):
        assert logit_bias_pairs(form) == want
    assert logit_bias_pairs(None) == logit_bias_pairs({}) == []
    for bad in ("5:1", 5, [[5]], [5, 1.5], {"x": 1.0}, {5: "much"}, {True: 1.0}, {5: True}):
        with pytest.raises(ValueError):
            logit_bias_pairs(bad)


def test_request_constraints_defaults_and_precedence():
    assert request_constraints(GenRequest(user="u"), None) == ([], 0, [])
    cfg = LLMConfig(MIN_NEW_TOKENS=30, LOGIT_BIAS="5:1.5, 6:ban")
    assert request_constraints(GenRequest(user="u"), cfg) == ([(5, 1.5), (6, NINF)], 30, [])
    assert request_constraints(GenRequest(user="u", max_tokens=8), cfg)[1] == 8  # a configured minimum is capped
    own = GenRequest(user="u", logit_bias=[], min_tokens=0, stop_token_ids=[9])
    assert request_constraints(own, cfg) == ([], 0, [9])  # the request's own values win
    assert not sampling_params(GenRequest(user="u", logit_bias=[], min_tokens=0), 0, cfg).constrained


def test_parse_logit_bias():
    assert parse_logit_bias("") == [] and parse_logit_bias(" , ") == []
    assert parse_logit_bias("5:1.5,6:ban, 7 : -100 ,8:BAN") == [(5, 1.5), (6, NINF), (7, -100.0), (8, NINF)]
    for bad in ("5", "5:", "x:1", "5:1:2", "5:101", "5:-100.5", "5:nan", "5:inf", "-1:1", "5:1,5:2", "5=1"):
        with pytest.raises(ValueError):
            parse_logit_bias(bad)
    with pytest.raises(ValueError):
        parse_logit_bias(",".join("%d:1" % i for i in range(301)))


def test_flags_and_env_reach_the_sampling_params(monkeypatch):
    monkeypatch.delenv("MIN_NEW_TOKENS", raising=False)
    monkeypatch.delenv("LOGIT_BIAS", raising=False)
    cfg = LLMConfig()
    assert (cfg.MIN_NEW_TOKENS, cfg.LOGIT_BIAS) == (0, "")
    for stage, temp in (("map", 0.6), ("reduce", 0.2)):
        req = GenRequest(user="u", max_tokens=40, temperature=temp, stage=stage)
        assert not sampling_params(req, 0, LLMConfig()).constrained
        args = build_parser().parse_args(["-i", "t.json", "--min-new-tokens", "12", "--logit-bias", "2:ban,9:-3.5"])
        sp = sampling_params(req, 0, config_from_args(args))
        assert sp.bias_items() == [(2, NINF), (9, -3.5)] and sp.min_tokens == 12 and sp.constrained
        assert sp.temperature == temp and tuple(sp.stop_token_ids) == ()
        sp.validate(128256)
    monkeypatch.setenv("MIN_NEW_TOKENS", "7")
    monkeypatch.setenv("LOGIT_BIAS", "100:ban")
    cfg = config_from_args(build_parser().parse_args(["-i", "t.json"]))
    assert (cfg.MIN_NEW_TOKENS, cfg.LOGIT_BIAS) == (7, "100:ban")
    sp = sampling_params(GenRequest(user="u", max_tokens=40, stage="reduce"), 0, cfg)
    assert sp.bias_items() == [(100, NINF)] and sp.min_tokens == 7
    cfg = config_from_args(build_parser().parse_args(["-i", "t.json", "--min-new-tokens", "0", "--logit-bias", ""]))
    assert (cfg.MIN_NEW_TOKENS, cfg.LOGIT_BIAS) == (0, "")  # the flags win over the environment
    for bad in (["--min-new-tokens", "-1"], ["--logit-bias", "5"], ["--logit-bias", "5:101"], ["--logit-bias", "x:1"]):
        with pytest.raises(SystemExit):
            config_from_args(build_parser().parse_args(["-i", "t.json"] + bad))


def test_env_template_lists_the_keys_and_parses():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = open(os.path.join(root, ".env.template"), encoding="utf-8").read().splitlines()
    vals = {ln.split("=", 1)[0]: ln.split("=", 1)[1].split(" #")[0].strip() for ln in lines
            if "=" in ln and not ln.startswith("#")}
    assert int(vals["MIN_NEW_TOKENS"]) == 0 and parse_logit_bias(vals["LOGIT_BIAS"]) == []


def _hosted_body(name, req, **cfg):
    p = make_provider(name, "m", LLMConfig(OPENAI_API_KEY="k", ANTHROPIC_API_KEY="k", **cfg))
    seen = {}

    async def post(headers, body):
        seen.update(body)
        return {"choices": [{"message": {"content": "x"}}], "content": [{"text": "x"}]}

    p._post = post
    asyncio.run(p.generate(req))
    return seen


@pytest.mark.parametrize("name", ["openai", "anthropic"])
def test_hosted_providers_send_none_of_the_three(name):
    keys = ("logit_bias", "min_tokens", "stop_token_ids", "stop", "stop_sequences")
    req = GenRequest(user="u", logit_bias=[[5, 1.0]], min_tokens=3, stop_token_ids=[7])
    assert not any(k in _hosted_body(name, req) for k in keys)  # the ids are the local tokenizer's
    assert not any(k in _hosted_body(name, GenRequest(user="u"), MIN_NEW_TOKENS=5, LOGIT_BIAS="5:ban") for k in keys)


def test_mock_provider_ignores_the_constraints():
    p = make_provider("mock", None, LLMConfig())
    a = asyncio.run(p.generate(GenRequest(user="u")))
    b = asyncio.run(p.generate(GenRequest(user="u", logit_bias=[[5, "ban"]], min_tokens=3, stop_token_ids=[7])))
    assert a.text == b.text
