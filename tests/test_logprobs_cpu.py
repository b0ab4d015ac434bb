"""Token log-probabilities without a GPU: the definition (ops/reference.py token_logprobs) against an independent
float64 log_softmax and a stable sort, SamplingParams limits, the engine on the CPU path (records, compaction,
a request finished at prefill), the request / result plumbing, and a gloo TP=2 engine against TP=1."""

import asyncio
import json
import math
import os
import socket
import subprocess
import sys
import textwrap
from dataclasses import asdict

import pytest
import torch

from llm_map_reduce_summarizer_amd import ops
from llm_map_reduce_summarizer_amd.config import LLMConfig
from llm_map_reduce_summarizer_amd.engine.config import get_model_config
from llm_map_reduce_summarizer_amd.engine.engine import DecodeState, ImportedPrefill, LLMEngine, SamplingParams
from llm_map_reduce_summarizer_amd.engine.provider import LocalEngineProvider, _result, logprobs_record, sampling_params
from llm_map_reduce_summarizer_amd.ops import reference
from llm_map_reduce_summarizer_amd.pipeline.providers import GenRequest, make_provider

from _logprob_cases import NINF, SampleTap, check_records, defined, independent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _row(vals):
    return torch.tensor([vals], dtype=torch.float32).to(torch.bfloat16)


def _against_independent(rows, ns):
    lp, tops = reference.token_logprobs(rows, ns)
    assert lp.dtype == torch.float64 and tuple(lp.shape) == tuple(rows.shape)
    for b in range(rows.shape[0]):
        n = ns if isinstance(ns, int) else ns[b]
        want_lp, want_top = independent(rows[b], n)
        fin = torch.isfinite(want_lp)
        assert torch.equal(torch.isneginf(lp[b]), torch.isneginf(want_lp))
        assert float((lp[b][fin] - want_lp[fin]).abs().max()) <= 1e-12 * (1.0 + float(want_lp[fin].abs().max()))
        assert [t for t, _ in tops[b]] == [t for t, _ in want_top], b
        for (t, x), (_, y) in zip(tops[b], want_top):
            assert x == float(lp[b, t]) and (x == y or abs(x - y) <= 1e-12 * (1.0 + abs(y)))
    return lp, tops


# ------------------------------------------------------------------ the definition
@pytest.mark.parametrize("V", [8, 1007])
@pytest.mark.parametrize("scale", [1.0, 30.0])
def test_token_logprobs_against_an_independent_reference(V, scale):
    g = torch.Generator().manual_seed(V)
    rows = (torch.randn(5, V, generator=g) * scale).to(torch.bfloat16)
    rows[:, 3], rows[:, 4], rows[:, 6] = NINF, -0.0, 0.0
    rows[:, 1] = rows[:, 7]
    lp, _ = _against_independent(rows, [20, 0, 1, 5, 20])
    assert torch.allclose(torch.exp(lp).sum(dim=1), torch.ones(5, dtype=torch.float64), atol=1e-12)


def test_ties_go_to_the_lower_id_and_minus_zero_equals_plus_zero():
    _, tops = _against_independent(_row([0.0, 2.0, -0.0, 2.0, -1.0, 0.0, 2.0]), 7)
    assert [t for t, _ in tops[0]] == [1, 3, 6, 0, 2, 5, 4]
    vals = dict(tops[0])
    assert vals[0] == vals[2] == vals[5] and vals[1] == vals[3] == vals[6]


def test_minus_inf_entries_add_nothing_and_report_minus_inf():
    lp, tops = _against_independent(_row([1.0, NINF, 1.0, NINF]), 4)
    assert lp[0].tolist() == [-math.log(2), NINF, -math.log(2), NINF]
    assert tops[0] == [(0, -math.log(2)), (2, -math.log(2)), (1, NINF), (3, NINF)]  # banned tokens last, by id


def test_fewer_tokens_than_n():
    _, tops = _against_independent(_row([0.5, 3.0, -2.0]), 20)
    assert [t for t, _ in tops[0]] == [1, 0, 2]
    assert reference.token_logprobs(_row([0.5, 3.0, -2.0]), 0)[1] == [[]]


@pytest.mark.parametrize("V,n", [(8, 20), (1007, 20), (1007, 5)])
def test_all_equal_row(V, n):
    lp, tops = _against_independent(torch.full((1, V), -3.5, dtype=torch.bfloat16), n)
    assert [t for t, _ in tops[0]] == list(range(min(n, V)))
    assert float((lp + math.log(V)).abs().max()) <= 1e-12


def test_one_row_and_per_row_lengths():
    rows = (torch.randn(3, 33, generator=torch.Generator().manual_seed(1)) * 3).to(torch.bfloat16)
    lp, tops = reference.token_logprobs(rows, [2, 0, 33])
    assert [len(t) for t in tops] == [2, 0, 33]
    lp1, tops1 = reference.token_logprobs(rows[2], 33)
    assert torch.equal(lp1[0], lp[2]) and tops1[0] == tops[2]


# ------------------------------------------------------------------ SamplingParams
def test_sampling_params_defaults_and_limits():
    sp = SamplingParams(8, 0.7, 0)
    assert sp.logprobs is False and sp.top_logprobs == 0
    for kw in (dict(logprobs=True), dict(logprobs=True, top_logprobs=20), dict(logprobs=False, top_logprobs=0)):
        SamplingParams(8, 0.7, 0, **kw).validate(1000)


@pytest.mark.parametrize("bad", [dict(logprobs=True, top_logprobs=21), dict(logprobs=True, top_logprobs=-1),
                                 dict(logprobs=True, top_logprobs=2.0), dict(logprobs=True, top_logprobs=True),
                                 dict(logprobs=True, top_logprobs=None), dict(top_logprobs=1),
                                 dict(logprobs=False, top_logprobs=3), dict(logprobs=1), dict(logprobs="yes"),
                                 dict(logprobs=None)])
def test_validate_refuses(bad):
    with pytest.raises(ValueError):
        SamplingParams(8, 0.7, 0, **bad).validate(1000)


# ------------------------------------------------------------------ engine on the reference ops
@pytest.fixture(scope="module")
def eng():
    return LLMEngine(get_model_config("tiny", init_std=0.05), device="cpu", max_model_len=512, max_num_seqs=8,
                     kv_pages=64, sync_every=3, max_new_cap=32)


PROMPTS = [[1, 2, 3, 4, 5], [9, 8, 7], [5, 5, 5, 5, 5, 5, 5], [11, 12]]
N = 10


def _ids(outs):
    return [o.token_ids for o in outs]


def test_state_row_is_listed_set_and_parked(eng):
    st = eng.state
    assert "lp_n" in DecodeState._ROW_FIELDS and st.lp_n.dtype == torch.int32 and st.lp_n.tolist() == [-1] * 8
    assert isinstance(st.lp, ops.LogprobStore) and st.lp.cap == 32
    st.lp_n[2] = 7
    st.move_row(2, 3)
    assert int(st.lp_n[3]) == 7
    for i in (2, 3):
        st.park_row(i)
        assert int(st.lp_n[i]) == -1
    assert st.view(0, 2).logprobs is False and st.view(1, 2).lp.rows == 2


def test_records_follow_the_definition_and_change_no_token(eng):
    plain = [SamplingParams(N, 1.0, 20 + i) for i in range(4)]
    base = eng.generate(PROMPTS, plain, ignore_eos=True)
    assert all(o.logprobs is None and o.top_logprobs is None for o in base)
    n0 = eng.stats["logprob_steps"]
    asking = [SamplingParams(N, 1.0, 20 + i, logprobs=True, top_logprobs=(5, 0, 20, 1)[i]) for i in range(4)]
    with SampleTap() as tap:
        outs = eng.generate(PROMPTS, asking, ignore_eos=True)
    assert _ids(outs) == _ids(base)
    assert eng.stats["logprob_steps"] >= n0 + N  # every decode window, and the first tokens at the prefill
    for o, sp in zip(outs, asking):
        assert [len(t) for t in o.top_logprobs] == [sp.top_logprobs] * N
        check_records(o, tap.rows, sp.seed, sp.top_logprobs, exact=True, ref=defined)
    n1 = eng.stats["logprob_steps"]
    assert _ids(eng.generate(PROMPTS, plain, ignore_eos=True)) == _ids(base)
    assert eng.stats["logprob_steps"] == n1  # nobody asks: no logprob step


def test_greedy_token_is_the_top_entry(eng):
    outs = eng.generate(PROMPTS[:2], [SamplingParams(N, 0.0, 1, logprobs=True, top_logprobs=3)] * 2, ignore_eos=True)
    for o in outs:
        for tok, lp, top in zip(o.token_ids, o.logprobs, o.top_logprobs):
            assert top[0] == (tok, lp)


def test_records_see_the_processed_logits(eng):
    """A ban and a +100 bias, greedy: the biased token is sampled with lp ~ 0, the banned one reports -inf."""
    sp = SamplingParams(4, 0.0, 3, logit_bias={4321: 100.0, 77: NINF}, logprobs=True, top_logprobs=2)
    with SampleTap() as tap:
        o = eng.generate(PROMPTS[:1], [sp], ignore_eos=True)[0]
    assert o.token_ids == [4321] * 4 and all(top[0][0] == 4321 and abs(lp) < 1e-6 for lp, top in
                                             zip(o.logprobs, o.top_logprobs))
    check_records(o, tap.rows, 3, 2, exact=True, ref=defined)
    assert all(float(reference.token_logprobs(tap.rows[(3, g)], 0)[0][0, 77]) == NINF for g in range(4))


def test_compaction_keeps_every_rows_records(eng):
    """Short and long budgets, asking and non-asking rows: the short rows retire at the first syncs, the others
    move down to the freed slots in the middle of their generation -- with their records."""
    budgets = [3, 16, 2, 14, 16, 4]
    prompts = PROMPTS + [[21, 22, 23], [31]]
    sp = [SamplingParams(b, 1.0, 40 + i, logprobs=i != 3, top_logprobs=(3, 20, 0, 0, 1, 2)[i] if i != 3 else 0)
          for i, b in enumerate(budgets)]
    with SampleTap() as tap:
        outs = eng.generate(prompts, sp, ignore_eos=True)
    assert [len(o.token_ids) for o in outs] == budgets
    plain = eng.generate(prompts, [SamplingParams(b, 1.0, 40 + i) for i, b in enumerate(budgets)], ignore_eos=True)
    assert _ids(plain) == _ids(outs)
    for o, p in zip(outs, sp):
        if not p.logprobs:
            assert o.logprobs is None and o.top_logprobs is None
            continue
        assert len(o.logprobs) == p.max_new_tokens
        check_records(o, tap.rows, p.seed, p.top_logprobs, exact=True, ref=defined)


def test_request_finished_at_prefill_has_one_record(eng):
    with SampleTap() as tap:
        o = eng.generate(PROMPTS[:1], [SamplingParams(1, 1.0, 5, logprobs=True, top_logprobs=4)])[0]
    assert len(o.token_ids) == len(o.logprobs) == len(o.top_logprobs) == 1 and len(o.top_logprobs[0]) == 4
    check_records(o, tap.rows, 5, 4, exact=True, ref=defined)


def test_imported_prefill_carries_its_first_record(eng):
    sp = SamplingParams(1, 1.0, 5, logprobs=True, top_logprobs=2)
    with pytest.raises(ValueError):
        eng.generate(PROMPTS[:1], [sp], imported={0: ImportedPrefill(first_token=42, kv=None)})
    imp = ImportedPrefill(first_token=42, kv=None, first_logprobs=(-1.5, [(7, -0.5), (42, -1.5), (9, -2.0)]))
    o = eng.generate(PROMPTS[:1], [sp], imported={0: imp})[0]
    assert o.token_ids == [42] and o.logprobs == [-1.5] and o.top_logprobs == [[(7, -0.5), (42, -1.5)]]


def test_prefill_export_takes_no_records(eng):
    firsts, _ = eng.prefill_export(PROMPTS[:2], [SamplingParams(N, 0.0, 0, logprobs=True, top_logprobs=5)] * 2,
                                   groups=1)
    plain, _ = eng.prefill_export(PROMPTS[:2], [SamplingParams(N, 0.0, 0)] * 2, groups=1)
    assert firsts == plain


def test_invalid_values_raise_at_generate(eng):
    for bad in (dict(logprobs=True, top_logprobs=21), dict(top_logprobs=2)):
        with pytest.raises(ValueError):
            eng.generate(PROMPTS[:1], [SamplingParams(3, 0.7, 0, **bad)])


def test_ops_logprobs_early_exits_on_cpu_rows():
    """Off, done and out-of-width rows get lp_slot -1 and no record."""
    from types import SimpleNamespace
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)  # noqa: E731
    st = SimpleNamespace(lp_n=i32([2, -1, 2, 2]), done=i32([0, 0, 1, 0]), gen_count=i32([1, 1, 1, 3]),
                         out_tokens=torch.zeros(4, 3, dtype=torch.int32), lp=ops.LogprobStore(4, 3, "cpu"))
    st.lp.ensure()
    st.lp.out_logprobs.fill_(777.0)
    st.lp.out_top_tok.fill_(-7)
    rows = (torch.randn(4, 50, generator=torch.Generator().manual_seed(2)) * 2).to(torch.bfloat16)
    keep = rows.clone()
    ops.logprobs(rows, st)
    assert st.lp.lp_slot.tolist() == [1, -1, -1, -1]
    st.out_tokens[0, 1] = 17
    ops.logprobs_pick(rows, st)
    assert torch.equal(rows.view(torch.int16), keep.view(torch.int16))
    lp, tops = reference.token_logprobs(rows[0], 2)
    assert st.lp.out_top_tok[0, 1].tolist()[:2] == [t for t, _ in tops[0]] and st.lp.out_top_tok[0, 1, 2:].tolist() == [-7] * 18
    assert float(st.lp.out_logprobs[0, 1]) == float(lp[0, 17].to(torch.float32))
    assert (st.lp.out_logprobs[1:] == 777.0).all() and (st.lp.out_top_tok[1:] == -7).all()
    assert (st.lp.out_logprobs[0, [0, 2]] == 777.0).all()


# ------------------------------------------------------------------ requests, providers
def test_gen_request_fields_reach_the_sampling_params():
    assert (GenRequest(user="u").logprobs, GenRequest(user="u").top_logprobs) == (None, None)
    sp = sampling_params(GenRequest(user="u"), 0, LLMConfig())
    assert sp.logprobs is False and sp.top_logprobs == 0
    r = GenRequest(user="u", logprobs=True, top_logprobs=7)
    back = GenRequest(**json.loads(json.dumps(asdict(r), allow_nan=False)))  # the serve broadcast
    assert back == r
    sp = sampling_params(back, 0, LLMConfig())
    assert sp.logprobs is True and sp.top_logprobs == 7
    sp.validate(128256)


def test_result_record_round_trips_minus_inf_through_the_all_gather_json():
    from llm_map_reduce_summarizer_amd.engine.engine import GenOutput
    o = GenOutput([5, 6], 3, "length", logprobs=[-0.25, NINF], top_logprobs=[[(5, -0.25), (9, NINF)], []])
    rec = dict({"i": 0, "text": "x", "pt": 3, "ct": 2, "fr": "length"}, **logprobs_record(o))
    back = json.loads(json.dumps([rec]))[0]  # parallel.dist.all_gather_json's serialisation
    res = _result(back)
    assert res.extra["logprobs"] == {"token_ids": [5, 6], "token_logprobs": [-0.25, NINF],
                                     "top": [[[5, -0.25], [9, NINF]], []]}
    assert logprobs_record(GenOutput([5], 3, "stop")) == {}
    assert "logprobs" not in _result({"i": 0, "text": "x", "pt": 3, "ct": 1, "fr": "stop"}).extra


def test_local_provider_reports_the_engines_records():
    prov = LocalEngineProvider("tiny", LLMConfig(), device="cpu", use_graphs=False, max_model_len=512,
                               engine_options={"kv_pages": 64, "max_num_seqs": 4, "max_new_cap": 16})
    reqs = [GenRequest(user="hello there", max_tokens=4, temperature=0.0, logprobs=True, top_logprobs=3),
            GenRequest(user="hello there", max_tokens=4, temperature=0.0)]
    a, b = asyncio.run(prov.generate_batch(reqs))
    assert a.text == b.text and "logprobs" not in b.extra
    rec = a.extra["logprobs"]
    assert len(rec["token_ids"]) == len(rec["token_logprobs"]) == len(rec["top"]) == 4
    assert prov.tokenizer.decode(rec["token_ids"]) == a.text
    assert all(len(t) == 3 and t[0] == [tok, lp] for t, tok, lp in zip(rec["top"], rec["token_ids"],
                                                                       rec["token_logprobs"]))
    ids = prov.encode_request(reqs[0])
    o = prov.engine.generate([ids], [sampling_params(reqs[0], prov.seed, prov.config)])[0]
    assert rec["token_logprobs"] == o.logprobs and rec["top"] == [[list(p) for p in t] for t in o.top_logprobs]
    assert prov._handoff_pays([ids, ids], reqs) is False  # (and never with a request that asks)
    prov.handoff = True
    assert prov._handoff_pays([ids, ids], reqs[1:] * 2) is True and prov._handoff_pays([ids, ids], reqs) is False


def test_mock_and_hosted_providers_ignore_the_fields():
    p = make_provider("mock", None, LLMConfig())
    a = asyncio.run(p.generate(GenRequest(user="u")))
    b = asyncio.run(p.generate(GenRequest(user="u", logprobs=True, top_logprobs=5)))
    assert a.text == b.text and "logprobs" not in (b.extra or {})
    for name in ("openai", "anthropic"):
        hp = make_provider(name, "m", LLMConfig(OPENAI_API_KEY="k", ANTHROPIC_API_KEY="k"))
        seen = {}

        async def post(headers, body):
            seen.update(body)
            return {"choices": [{"message": {"content": "x"}}], "content": [{"text": "x"}]}

        hp._post = post
        asyncio.run(hp.generate(GenRequest(user="u", logprobs=True, top_logprobs=5)))
        assert "logprobs" not in seen and "top_logprobs" not in seen


# ------------------------------------------------------------------ gloo TP=2
TP_SCRIPT = textwrap.dedent("""
    import json, os, sys
    sys.path.insert(0, %(root)r)
    sys.path.insert(0, os.path.join(%(root)r, "tests"))
    import torch
    from llm_map_reduce_summarizer_amd.parallel import dist as pdist
    pdist.init_distributed_from_env(backend="gloo")
    par = pdist.setup_parallel(int(os.environ.get("TP", "1")))
    from llm_map_reduce_summarizer_amd.engine.config import get_model_config
    from llm_map_reduce_summarizer_amd.engine.engine import LLMEngine, SamplingParams
    from _logprob_cases import SampleTap, check_records, defined
    cfg = get_model_config("tiny-gqa4", init_std=0.05)
    eng = LLMEngine(cfg, device="cpu", max_model_len=512, max_num_seqs=4, kv_pages=64, sync_every=3, max_new_cap=16,
                    tp_rank=par.tp_rank, tp_size=par.tp, tp_group=par.tp_group)
    prompts = [[128000] + [(i * 7 + j * 3) %% 9000 + 5 for j in range(20 + 9 * i)] for i in range(3)]
    sp = [SamplingParams(5, 0.0, i, logprobs=i != 1, top_logprobs=(4, 0, 20)[i]) for i in range(3)]
    with SampleTap() as tap:
        outs = eng.generate(prompts, sp)
    for o, p in zip(outs, sp):
        if p.logprobs:
            check_records(o, tap.rows, p.seed, p.top_logprobs, exact=True, ref=defined)
    print("RESULT " + json.dumps([[o.token_ids, o.logprobs, o.top_logprobs] for o in outs]), flush=True)
    pdist.shutdown()
""")


def _run_tp(world: int, tp: int):
    code = TP_SCRIPT % {"root": ROOT}
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world),
               OMP_NUM_THREADS="2", TP=str(tp))
    procs = [subprocess.Popen([sys.executable, "-c", code], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(world)]
    outs = []
    for p in procs:
        o, err = p.communicate(timeout=600)
        assert p.returncode == 0, err[-3000:]
        outs.append(json.loads([ln for ln in o.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    return outs


@pytest.mark.slow
def test_tp2_gives_the_records_of_tp1():
    """Every rank of a gloo TP=2 engine gathers the logits and runs the single-GPU ops on whole rows: the ranks
    agree exactly, each rank's records are the definition on the logits its sampler saw (checked in the
    worker), and against TP=1 they differ only by what the sharded projections' bf16 rounding does to the
    logits: a few bf16 ulps of logits below 4 (2^-6 each), |d lp| <= 2 max |d logit|, so 0.1 at the most --
    compared where the greedy tokens agree (a bf16 near-tie may flip a sequence, as in test_dist_cpu)."""
    ref = _run_tp(1, 1)[0]
    tp = _run_tp(2, 2)
    assert tp[0] == tp[1]
    assert ref[1][1] is None and tp[0][1][1] is None  # the row that did not ask
    same = 0
    for (ta, la, pa), (tb, lb, pb) in zip(tp[0], ref):
        if ta != tb or la is None:
            continue
        same += 1
        assert all(abs(x - y) <= 0.1 for x, y in zip(la, lb))
        assert [len(t) for t in pa] == [len(t) for t in pb]
    assert same >= 1
