"""Frequency / presence / repetition penalties without a GPU: the rule (ops/reference.py apply_penalties,
the definition sampler.hip's penalize kernel matches bit for bit), the engine on the CPU path, and the
public interface (requests, HTTP bodies, hosted providers, CLI flags and $..._PENALTY)."""

import asyncio
import json

import pytest
import torch

from llm_map_reduce_summarizer_amd import ops
from llm_map_reduce_summarizer_amd.cli import build_parser, config_from_args
from llm_map_reduce_summarizer_amd.config import LLMConfig
from llm_map_reduce_summarizer_amd.engine.config import get_model_config
from llm_map_reduce_summarizer_amd.engine.engine import LLMEngine, SamplingParams
from llm_map_reduce_summarizer_amd.engine.provider import sampling_params
from llm_map_reduce_summarizer_amd.ops import reference
from llm_map_reduce_summarizer_amd.pipeline.providers import GenRequest, make_provider, request_penalties
from llm_map_reduce_summarizer_amd.serve import BadRequest, anthropic_request, openai_request

NINF = float("-inf")

# name, row, generated tokens, (rep, freq, pres), expected row -- every value a bf16, worked out by hand
HAND = [
    ("rep_positive_and_negative", [3.0, -3.0, 5.0, -5.0], [0, 1], (2.0, 0.0, 0.0), [1.5, -6.0, 5.0, -5.0]),
    ("rep_below_one", [3.0, -3.0, 5.0, -5.0], [0, 1], (0.5, 0.0, 0.0), [6.0, -1.5, 5.0, -5.0]),
    ("freq_three_times", [2.0, 1.0, 0.0, -1.0], [0, 3, 0, 0], (1.0, 0.5, 0.0), [0.5, 1.0, 0.0, -1.5]),
    ("pres_alone", [1.0, 1.0, 1.0, 1.0], [2, 2, 2, 1], (1.0, 0.0, 0.25), [1.0, 0.75, 0.75, 1.0]),
    ("all_three", [4.0, -1.0, 7.0, 0.0], [0, 1, 0, 1], (2.0, 0.5, 0.25), [0.75, -3.25, 7.0, 0.0]),
    ("negative_freq", [1.0, 1.0, 1.0, 1.0], [3, 3], (1.0, -0.5, 0.0), [1.0, 1.0, 1.0, 2.0]),
    # 1 / 3 = 0.0101010101...b: the fp32 quotient rounds to the bf16 0.333984375 = 171 / 512
    ("bf16_rounding", [1.0, 2.0, 2.0, 2.0], [0], (3.0, 0.0, 0.0), [0.333984375, 2.0, 2.0, 2.0]),
    ("minus_inf_stays", [NINF, 1.0, NINF, 0.0], [0, 2, 2], (1.5, 0.5, 1.0), [NINF, 1.0, NINF, 0.0]),
]


def _row(vals):
    return torch.tensor([vals], dtype=torch.float32).to(torch.bfloat16)


def _apply(row, toks, pen, done=None, g=None, tok_offset=0, width=8):
    ot = torch.zeros(1, width, dtype=torch.int32)
    ot[0, :len(toks)] = torch.tensor(toks, dtype=torch.int32)
    g = len(toks) if g is None else g
    rep, freq, pres = pen
    return reference.apply_penalties(row, ot, torch.tensor([g], dtype=torch.int32), torch.tensor([rep]),
                                     torch.tensor([freq]), torch.tensor([pres]), done, tok_offset)


@pytest.mark.parametrize("name,row,toks,pen,expect", HAND, ids=[h[0] for h in HAND])
def test_hand_written_rows(name, row, toks, pen, expect):
    got = _apply(_row(row), toks, pen)
    assert got.dtype == torch.bfloat16 and got.shape == (1, len(row))
    assert got[0].float().tolist() == expect


def test_rewrites_in_place_and_returns_the_rows():
    r = _row([4.0, 1.0])
    out = _apply(r, [0], (1.0, 0.0, 1.0))
    assert out.data_ptr() == r.data_ptr() and r[0].float().tolist() == [3.0, 1.0]


def test_neutral_done_and_empty_rows_are_untouched():
    base = [4.0, -1.0, 7.0, 0.0]
    assert _apply(_row(base), [0, 1], (1.0, 0.0, 0.0))[0].float().tolist() == base  # neutral
    assert _apply(_row(base), [0, 1], (2.0, 1.0, 1.0), done=torch.tensor([1]))[0].float().tolist() == base
    assert _apply(_row(base), [0, 1], (2.0, 1.0, 1.0), done=torch.tensor([0]))[0].float().tolist() != base
    assert _apply(_row(base), [0, 1], (2.0, 1.0, 1.0), g=0)[0].float().tolist() == base  # nothing generated yet


def test_entries_beyond_gen_count_are_not_read():
    got = _apply(_row([1.0, 1.0, 1.0, 1.0]), [0, 1, 2, 3], (1.0, 0.0, 0.5), g=2)
    assert got[0].float().tolist() == [0.5, 0.5, 1.0, 1.0]


def test_shards_equal_the_whole_row():
    g = torch.Generator().manual_seed(5)
    V = 64
    logits = (torch.randn(2, V, generator=g) * 3).to(torch.bfloat16)
    ot = torch.randint(0, V, (2, 40), generator=g, dtype=torch.int32)
    gc = torch.tensor([40, 17], dtype=torch.int32)
    pens = (torch.tensor([1.3, 0.8]), torch.tensor([0.4, -0.3]), torch.tensor([0.7, 0.1]))
    whole = reference.apply_penalties(logits.clone(), ot, gc, *pens)
    assert not torch.equal(whole, logits)
    halves = logits.clone()
    reference.apply_penalties(halves[:, :V // 2], ot, gc, *pens, tok_offset=0)
    reference.apply_penalties(halves[:, V // 2:], ot, gc, *pens, tok_offset=V // 2)
    assert torch.equal(halves.view(torch.int16), whole.view(torch.int16))


# ------------------------------------------------------------------ parameters
def test_sampling_params_fields_and_penalised():
    sp = SamplingParams(5, 0.3, 7)
    assert (sp.frequency_penalty, sp.presence_penalty, sp.repetition_penalty) == (0.0, 0.0, 1.0)
    assert not sp.penalised
    assert SamplingParams(5, 0.3, 7, frequency_penalty=0.1).penalised
    assert SamplingParams(5, 0.3, 7, presence_penalty=-0.1).penalised
    assert SamplingParams(5, 0.0, 7, repetition_penalty=1.1).penalised  # greedy rows are penalised too
    SamplingParams(5, 0.3, 7, frequency_penalty=1, presence_penalty=-2, repetition_penalty=2).validate()


@pytest.mark.parametrize("bad", [dict(frequency_penalty=float("nan")), dict(presence_penalty=float("inf")),
                                 dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0),
                                 dict(repetition_penalty=float("nan")), dict(frequency_penalty="x"),
                                 dict(presence_penalty=True), dict(repetition_penalty=None)])
def test_validate_refuses(bad):
    with pytest.raises(ValueError):
        SamplingParams(3, 0.7, 0, **bad).validate()


# ------------------------------------------------------------------ engine on the reference ops
@pytest.fixture(scope="module")
def eng():
    return LLMEngine(get_model_config("tiny", init_std=0.05), device="cpu", max_model_len=512, max_num_seqs=8,
                     kv_pages=64, sync_every=3)


PROMPTS = [[1, 2, 3, 4, 5], [9, 8, 7], [5, 5, 5, 5, 5, 5, 5], [11, 12]]
N = 24  # the plain greedy run of every one of these prompts repeats a token within 24 steps


def _ids(outs):
    return [o.token_ids for o in outs]


def test_ops_penalize_runs_the_reference_on_cpu_rows(eng):
    st = eng.state.view(0, 1)
    st.out_tokens[0, :2] = torch.tensor([1, 3], dtype=torch.int32)
    st.gen_count[0], st.done[0] = 2, 0
    st.rep_pen[0], st.freq_pen[0], st.pres_pen[0] = 1.0, 0.0, 1.0
    try:
        got = ops.penalize(_row([2.0, 2.0, 2.0, 2.0]), st)
        assert got[0].float().tolist() == [2.0, 1.0, 2.0, 1.0]
    finally:
        eng.state.park_row(0)
    assert (float(eng.state.rep_pen[0]), float(eng.state.freq_pen[0]), float(eng.state.pres_pen[0])) == (1.0, 0.0, 0.0)


def test_presence_1000_greedy_never_repeats(eng):
    plain = _ids(eng.generate(PROMPTS, [SamplingParams(N, 0.0, 0)] * 4, ignore_eos=True))
    assert all(len(t) == N and len(set(t)) < N for t in plain)  # every plain run repeats: not vacuous
    n0 = eng.stats["penalised_steps"]
    pen = _ids(eng.generate(PROMPTS, [SamplingParams(N, 0.0, 0, presence_penalty=1000.0)] * 4, ignore_eos=True))
    assert all(len(t) == N and len(set(t)) == N for t in pen)
    assert eng.stats["penalised_steps"] == n0 + N - 1  # every decode step; the first token has no history


def test_neutral_penalties_change_nothing(eng):
    sp = [SamplingParams(8, 1.2, 40 + i) for i in range(4)]
    n0 = eng.stats["penalised_steps"]
    base = _ids(eng.generate(PROMPTS, sp))
    neutral = [SamplingParams(8, 1.2, 40 + i, frequency_penalty=0.0, presence_penalty=0.0, repetition_penalty=1.0)
               for i in range(4)]
    assert _ids(eng.generate(PROMPTS, neutral)) == base
    assert eng.stats["penalised_steps"] == n0


def test_penalised_request_is_batch_invariant(eng):
    pen = SamplingParams(N, 0.0, 3, presence_penalty=1.5, frequency_penalty=0.5, repetition_penalty=1.2)
    solo = _ids(eng.generate(PROMPTS[1:2], [pen], ignore_eos=True))[0]
    plain_solo = _ids(eng.generate(PROMPTS[1:2], [SamplingParams(N, 0.0, 3)], ignore_eos=True))[0]
    assert solo != plain_solo  # the penalties act
    others = [SamplingParams(N, 0.7, 9), pen, SamplingParams(N // 2, 0.0, 1), SamplingParams(N, 1.0, 4, top_k=5)]
    plain = _ids(eng.generate(PROMPTS, [others[0], SamplingParams(N, 0.0, 3)] + others[2:], ignore_eos=True))
    mixed = _ids(eng.generate(PROMPTS, others, ignore_eos=True))
    assert mixed[1] == solo
    assert [mixed[i] for i in (0, 2, 3)] == [plain[i] for i in (0, 2, 3)]  # the other rows: exactly as without it


def test_invalid_values_raise_at_generate(eng):
    with pytest.raises(ValueError):
        eng.generate(PROMPTS[:1], [SamplingParams(3, 0.7, 0, repetition_penalty=0.0)])


# ------------------------------------------------------------------ server, providers, CLI
MSGS = [{"role": "user", "content": "u"}]


def _pens(r):
    return (r.frequency_penalty, r.presence_penalty, r.repetition_penalty)


@pytest.mark.parametrize("make", [openai_request, anthropic_request])
def test_http_requests_carry_the_fields(make):
    r = make({"messages": MSGS, "frequency_penalty": 0.5, "presence_penalty": -1.5, "repetition_penalty": 1.2})
    assert _pens(r) == (0.5, -1.5, 1.2)
    r = make({"messages": MSGS, "frequency_penalty": 2, "presence_penalty": -2, "repetition_penalty": 2})
    assert _pens(r) == (2.0, -2.0, 2.0) and all(isinstance(x, float) for x in _pens(r))  # integers are numbers
    assert _pens(make({"messages": MSGS})) == (None, None, None)
    r = make({"messages": MSGS, "frequency_penalty": None, "presence_penalty": None, "repetition_penalty": None})
    assert _pens(r) == (None, None, None)
    multi = MSGS + [{"role": "assistant", "content": "a"}, {"role": "user", "content": "b"}]
    assert _pens(make({"messages": multi, "presence_penalty": 0.25, "top_p": 0.5})) == (None, 0.25, None)


@pytest.mark.parametrize("make", [openai_request, anthropic_request])
@pytest.mark.parametrize("bad", [{"frequency_penalty": 2.5}, {"frequency_penalty": -2.01}, {"presence_penalty": 3},
                                 {"presence_penalty": "x"}, {"frequency_penalty": True},
                                 {"frequency_penalty": float("nan")}, {"presence_penalty": float("nan")},
                                 {"repetition_penalty": 0}, {"repetition_penalty": -1}, {"repetition_penalty": 2.5},
                                 {"repetition_penalty": "1.1"}, {"repetition_penalty": False},
                                 {"repetition_penalty": float("nan")}, {"presence_penalty": [1]}])
def test_http_bad_values_are_refused(make, bad):
    with pytest.raises(BadRequest):
        make(dict({"messages": MSGS}, **bad))


def test_broadcast_record_carries_the_fields():
    from dataclasses import asdict
    r = openai_request({"messages": MSGS, "frequency_penalty": 0.5, "repetition_penalty": 1.1})
    back = GenRequest(**json.loads(json.dumps(asdict(r))))
    assert back == r and _pens(back) == (0.5, None, 1.1)


def test_request_penalties_defaults():
    assert request_penalties(GenRequest(user="u"), None) == (0.0, 0.0, 1.0)
    cfg = LLMConfig(FREQUENCY_PENALTY=0.3, PRESENCE_PENALTY=0.2, REPETITION_PENALTY=1.1)
    assert request_penalties(GenRequest(user="u"), cfg) == (0.3, 0.2, 1.1)
    assert request_penalties(GenRequest(user="u", frequency_penalty=0.0, repetition_penalty=1.0), cfg) == (0.0, 0.2, 1.0)


def test_flags_and_env_reach_the_sampling_params(monkeypatch):
    def sp_pens(sp):
        return (sp.frequency_penalty, sp.presence_penalty, sp.repetition_penalty)

    cfg = LLMConfig()
    assert (cfg.FREQUENCY_PENALTY, cfg.PRESENCE_PENALTY, cfg.REPETITION_PENALTY) == (0.0, 0.0, 1.0)
    for stage, temp in (("map", 0.6), ("reduce", 0.2)):
        req = GenRequest(user="u", max_tokens=4, temperature=temp, stage=stage)
        assert sp_pens(sampling_params(req, 0, LLMConfig())) == (0.0, 0.0, 1.0)
        args = build_parser().parse_args(["-i", "t.json", "--frequency-penalty", "0.4", "--presence-penalty", "0.6",
                                          "--repetition-penalty", "1.15"])
        sp = sampling_params(req, 0, config_from_args(args))
        assert sp_pens(sp) == (0.4, 0.6, 1.15) and sp.penalised and sp.temperature == temp
    monkeypatch.setenv("FREQUENCY_PENALTY", "0.25")
    monkeypatch.setenv("PRESENCE_PENALTY", "-0.5")
    monkeypatch.setenv("REPETITION_PENALTY", "1.3")
    cfg = config_from_args(build_parser().parse_args(["-i", "t.json"]))
    assert (cfg.FREQUENCY_PENALTY, cfg.PRESENCE_PENALTY, cfg.REPETITION_PENALTY) == (0.25, -0.5, 1.3)
    req = GenRequest(user="u", max_tokens=4, stage="reduce")
    assert sp_pens(sampling_params(req, 0, cfg)) == (0.25, -0.5, 1.3)
    # a request's own values win over the configured defaults
    own = GenRequest(user="u", frequency_penalty=0.0, presence_penalty=0.0, repetition_penalty=1.0)
    assert not sampling_params(own, 0, cfg).penalised
    for bad in (["--repetition-penalty", "0"], ["--repetition-penalty", "-1"], ["--frequency-penalty", "nan"],
                ["--presence-penalty", "inf"]):
        with pytest.raises(SystemExit):
            config_from_args(build_parser().parse_args(["-i", "t.json"] + bad))


def _hosted_body(name, req, **cfg):
    p = make_provider(name, "m", LLMConfig(OPENAI_API_KEY="k", ANTHROPIC_API_KEY="k", **cfg))
    seen = {}

    async def post(headers, body):
        seen.update(body)
        return {"choices": [{"message": {"content": "x"}}], "content": [{"text": "x"}]}

    p._post = post
    asyncio.run(p.generate(req))
    return seen


def test_hosted_bodies():
    keys = ("frequency_penalty", "presence_penalty", "repetition_penalty")
    req = GenRequest(user="u", frequency_penalty=0.5, presence_penalty=-0.25, repetition_penalty=1.2)
    b = _hosted_body("openai", req)
    assert (b["frequency_penalty"], b["presence_penalty"]) == (0.5, -0.25)
    assert "repetition_penalty" not in b  # no hosted API has it
    assert not any(k in _hosted_body("anthropic", req) for k in keys)  # the Anthropic API has none of them
    # neutral values, explicit or default, are not sent
    assert not any(k in _hosted_body("openai", GenRequest(user="u")) for k in keys)
    b = _hosted_body("openai", GenRequest(user="u", frequency_penalty=0.0, presence_penalty=0.5))
    assert "frequency_penalty" not in b and b["presence_penalty"] == 0.5
    b = _hosted_body("openai", GenRequest(user="u"), FREQUENCY_PENALTY=0.3)  # the configured default
    assert b["frequency_penalty"] == 0.3 and "presence_penalty" not in b
    assert not any(k in _hosted_body("anthropic", GenRequest(user="u"), FREQUENCY_PENALTY=0.3) for k in keys)


def test_mock_provider_ignores_the_penalties():
    p = make_provider("mock", None, LLMConfig())
    a = asyncio.run(p.generate(GenRequest(user="u")))
    b = asyncio.run(p.generate(GenRequest(user="u", frequency_penalty=1.0, presence_penalty=1.0,
                                          repetition_penalty=1.5)))
    assert a.text == b.text
