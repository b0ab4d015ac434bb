"""Top-k / top-p sampling without a GPU: the threshold rule (ops/reference.py nucleus_threshold, the
definition the filter kernels of sampler.hip match), the engine on the CPU path, and the public interface
(requests, HTTP bodies, hosted providers, CLI flags and $TOP_P / $TOP_K)."""

import asyncio
import json
import os
import socket
import subprocess
import sys
import textwrap

import pytest
import torch

from llm_map_reduce_summarizer_amd.cli import build_parser, config_from_args
from llm_map_reduce_summarizer_amd.config import LLMConfig
from llm_map_reduce_summarizer_amd.engine.config import get_model_config
from llm_map_reduce_summarizer_amd.engine.engine import LLMEngine, SamplingParams
from llm_map_reduce_summarizer_amd.engine.provider import LocalEngineProvider, sampling_params
from llm_map_reduce_summarizer_amd.ops import reference
from llm_map_reduce_summarizer_amd.pipeline.providers import GenRequest, make_provider
from llm_map_reduce_summarizer_amd.serve import BadRequest, anthropic_request, openai_request

import _filter_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = float("-inf")


# ------------------------------------------------------------------ threshold semantics
@pytest.mark.parametrize("name,row,tau,k,p,expect", FC.HAND, ids=[h[0] for h in FC.HAND])
def test_hand_written_thresholds(name, row, tau, k, p, expect):
    logits = torch.tensor([row], dtype=torch.float32).to(torch.bfloat16)
    got = reference.nucleus_threshold(logits, [tau], [k], [p])
    assert got.dtype == torch.float32 and got.shape == (1,)
    assert float(got[0]) == expect


def test_ties_at_the_cut_are_all_kept():
    row = torch.tensor([[1.0, 3.0, 3.0, 2.0]]).to(torch.bfloat16)
    th = reference.nucleus_threshold(row, [1.0], [1], [1.0])
    assert (row[0].float() >= th[0]).tolist() == [False, True, True, False]


def test_signed_zeros_are_one_level():
    row = torch.tensor([0.0, -0.0, -1.0, 0.0]).to(torch.bfloat16)
    vals, counts, w = reference.nucleus_levels(row, 1.0)
    assert vals.tolist() == [0.0, -1.0] and counts.tolist() == [3, 1]
    assert w.tolist() == pytest.approx([3.0, 0.36787944117144233])


def test_top_k_then_top_p_order():
    """top-p is taken over the top-k set (HF / vLLM order); the other order gives another answer here."""
    name, row, tau, k, p, expect = next(h for h in FC.HAND if h[0] == "k_then_p")
    logits = torch.tensor([row]).to(torch.bfloat16)
    assert float(reference.nucleus_threshold(logits, [tau], [k], [p])[0]) == expect == 2.0
    p_first = float(reference.nucleus_threshold(logits, [tau], [0], [p])[0])
    k_alone = float(reference.nucleus_threshold(logits, [tau], [k], [1.0])[0])
    assert (p_first, k_alone) == (0.0, 1.0)  # p over the whole row keeps the zeros; then top-2 would cut at 1


def test_sample_tokens_takes_thresholds():
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(3, 500, generator=g) * 2).to(torch.bfloat16)
    temps, seeds, pos = torch.tensor([1.5, 1.5, 0.0]), torch.tensor([1, 2, 3]), torch.tensor([4, 5, 6])
    plain = reference.sample_tokens(logits, temps, seeds, pos)
    none = reference.sample_tokens(logits, temps, seeds, pos, torch.full((3,), NINF))
    assert torch.equal(plain, none)
    th = reference.nucleus_threshold(logits, temps, [1, 3, 1], [1.0, 1.0, 1.0])
    toks = reference.sample_tokens(logits, temps, seeds, pos, th)
    assert float(logits[0, int(toks[0])]) == float(logits[0].float().max())  # k = 1: a token at the row max
    assert float(logits[1, int(toks[1])]) >= float(th[1])
    assert int(toks[2]) == int(plain[2]) and float(th[2]) == NINF  # greedy rows are never filtered


# ------------------------------------------------------------------ engine and parameters
def test_sampling_params_positional_and_validation():
    sp = SamplingParams(5, 0.3, 7)
    assert (sp.max_new_tokens, sp.temperature, sp.seed, sp.top_k, sp.top_p) == (5, 0.3, 7, 0, 1.0)
    assert not sp.filtered
    assert SamplingParams(5, 0.3, 7, 40).top_k == 40 and SamplingParams(5, 0.3, 7, 0, 0.9).top_p == 0.9
    assert SamplingParams(5, 0.3, 7, top_k=2).filtered and SamplingParams(5, 0.3, 7, top_p=0.5).filtered
    assert not SamplingParams(5, 0.0, 7, top_k=2).filtered  # greedy


@pytest.fixture(scope="module")
def eng():
    return LLMEngine(get_model_config("tiny", init_std=0.05), device="cpu", max_model_len=512, max_num_seqs=8,
                     kv_pages=64, sync_every=3)


PROMPTS = [[1, 2, 3, 4, 5], [9, 8, 7], [5, 5, 5, 5, 5, 5, 5], [11, 12]]


@pytest.mark.parametrize("bad", [dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=-0.1),
                                 dict(top_k=1.5), dict(top_p="x")])
def test_invalid_values_raise_at_generate(eng, bad):
    with pytest.raises(ValueError):
        eng.generate(PROMPTS[:1], [SamplingParams(3, 0.7, 0, **bad)])


def _ids(outs):
    return [o.token_ids for o in outs]


def test_filtered_generation_deterministic_and_order_invariant(eng):
    kinds = [dict(top_k=2), dict(top_p=0.5), dict(top_k=40, top_p=0.9), dict(top_k=1)]
    sp = [SamplingParams(6, 1.5, 20 + i, **kinds[i]) for i in range(4)]
    a = _ids(eng.generate(PROMPTS, sp))
    assert _ids(eng.generate(PROMPTS, sp)) == a
    assert _ids(eng.generate(PROMPTS[::-1], sp[::-1]))[::-1] == a
    assert [_ids(eng.generate([p], [s]))[0] for p, s in zip(PROMPTS, sp)] == a


def test_mixed_batch_and_counter(eng):
    plain = [SamplingParams(6, 1.5, 30 + i) for i in range(4)]
    n0 = eng.stats["filtered_steps"]
    base = _ids(eng.generate(PROMPTS, plain))
    assert eng.stats["filtered_steps"] == n0  # an unfiltered run takes no filtered step
    mixed = list(plain)
    mixed[1] = SamplingParams(6, 1.5, 31, top_k=2)
    got = _ids(eng.generate(PROMPTS, mixed))
    assert eng.stats["filtered_steps"] > n0
    assert [got[i] for i in (0, 2, 3)] == [base[i] for i in (0, 2, 3)]  # unfiltered rows: exactly as before
    assert got[1] != base[1]  # top_k = 2 against none at temperature 1.5, same seed


def test_fresh_engine_counter_is_zero_without_filters():
    e = LLMEngine(get_model_config("tiny", init_std=0.05), device="cpu", max_model_len=128, max_num_seqs=4,
                  kv_pages=16)
    e.generate(PROMPTS[:2], [SamplingParams(3, 0.8, 1), SamplingParams(3, 0.0, 2, top_k=5)])  # greedy: no filter
    assert e.stats["filtered_steps"] == 0
    e.generate(PROMPTS[:2], [SamplingParams(3, 0.8, 1, top_p=0.9), SamplingParams(3, 0.8, 2)])
    assert e.stats["filtered_steps"] == 3  # the first token (prefill row) + 2 decode steps


def test_first_token_is_filtered(eng):
    """top_k = 1 at a high temperature: every token, the first included, is the greedy one."""
    greedy = _ids(eng.generate(PROMPTS[:2], [SamplingParams(4, 0.0, 0)] * 2))
    k1 = _ids(eng.generate(PROMPTS[:2], [SamplingParams(4, 2.0, 5, top_k=1), SamplingParams(4, 2.0, 6, top_k=1)]))
    assert k1 == greedy


# ------------------------------------------------------------------ server, providers, CLI
def test_http_requests_carry_the_fields():
    msgs = [{"role": "user", "content": "u"}]
    r = openai_request({"messages": msgs, "top_p": 0.9, "top_k": 40})
    assert (r.top_p, r.top_k) == (0.9, 40)
    r = openai_request({"messages": msgs})
    assert (r.top_p, r.top_k) == (None, None)
    r = openai_request({"messages": msgs, "top_p": 1, "top_k": None})
    assert (r.top_p, r.top_k) == (1.0, None)
    r = anthropic_request({"messages": msgs, "top_p": 0.5, "top_k": 3, "system": "s"})
    assert (r.top_p, r.top_k, r.system) == (0.5, 3, "s")
    multi = msgs + [{"role": "assistant", "content": "a"}, {"role": "user", "content": "b"}]
    assert anthropic_request({"messages": multi, "top_k": 7}).top_k == 7
    assert openai_request({"messages": multi, "top_p": 0.25}).top_p == 0.25


def test_broadcast_record_carries_the_fields():
    """The multi-rank server broadcasts ``asdict(request)`` and the peers rebuild ``GenRequest(**record)``."""
    from dataclasses import asdict
    r = openai_request({"messages": [{"role": "user", "content": "u"}], "top_p": 0.9, "top_k": 40})
    back = GenRequest(**json.loads(json.dumps(asdict(r))))
    assert back == r and (back.top_p, back.top_k) == (0.9, 40)


@pytest.mark.parametrize("make", [openai_request, anthropic_request])
@pytest.mark.parametrize("bad", [{"top_p": 0}, {"top_p": 1.5}, {"top_p": "x"}, {"top_k": -1}, {"top_k": "many"},
                                 {"top_k": 2.5}, {"top_p": True}])
def test_http_bad_values_are_refused(make, bad):
    with pytest.raises(BadRequest):
        make(dict({"messages": [{"role": "user", "content": "u"}]}, **bad))


def _hosted_body(name, req, **cfg):
    p = make_provider(name, "m", LLMConfig(OPENAI_API_KEY="k", ANTHROPIC_API_KEY="k", **cfg))
    seen = {}

    async def post(headers, body):
        seen.update(body)
        return {"choices": [{"message": {"content": "x"}}], "content": [{"text": "x"}]}

    p._post = post
    asyncio.run(p.generate(req))
    return seen


def test_hosted_bodies_carry_the_keys_only_when_set():
    plain = GenRequest(user="u", temperature=0.3, max_tokens=5)
    assert _hosted_body("openai", plain) == {"model": "m", "messages": [{"role": "user", "content": "u"}],
                                             "temperature": 0.3, "max_tokens": 5}
    assert _hosted_body("anthropic", plain) == {"model": "m", "messages": [{"role": "user", "content": "u"}],
                                                "temperature": 0.3, "max_tokens": 5}
    # explicit defaults are not sent either
    assert "top_p" not in _hosted_body("openai", GenRequest(user="u", top_p=1.0, top_k=0))
    b = _hosted_body("openai", GenRequest(user="u", top_p=0.9, top_k=40))
    assert b["top_p"] == 0.9 and "top_k" not in b  # the OpenAI API has no top_k
    b = _hosted_body("anthropic", GenRequest(user="u", top_p=0.9, top_k=40))
    assert (b["top_p"], b["top_k"]) == (0.9, 40)
    b = _hosted_body("anthropic", plain, TOP_P=0.8, TOP_K=5)  # the configured defaults
    assert (b["top_p"], b["top_k"]) == (0.8, 5)


def test_mock_provider_ignores_the_filters():
    p = make_provider("mock", None, LLMConfig())
    a = asyncio.run(p.generate(GenRequest(user="u")))
    b = asyncio.run(p.generate(GenRequest(user="u", top_p=0.5, top_k=3)))
    assert a.text == b.text


def test_flags_and_env_reach_the_sampling_params(monkeypatch):
    req = GenRequest(user="u", max_tokens=4, temperature=0.6)
    sp = sampling_params(req, 0, LLMConfig())
    assert (sp.max_new_tokens, sp.temperature, sp.top_k, sp.top_p) == (4, 0.6, 0, 1.0)
    args = build_parser().parse_args(["-i", "t.json", "--top-p", "0.8", "--top-k", "12"])
    sp = sampling_params(req, 0, config_from_args(args))
    assert (sp.top_k, sp.top_p) == (12, 0.8)
    monkeypatch.setenv("TOP_P", "0.7")
    monkeypatch.setenv("TOP_K", "9")
    cfg = config_from_args(build_parser().parse_args(["-i", "t.json"]))
    assert (cfg.TOP_K, cfg.TOP_P) == (9, 0.7)
    sp = sampling_params(req, 0, cfg)
    assert (sp.top_k, sp.top_p) == (9, 0.7)
    # a request's own values win over the configured defaults
    sp = sampling_params(GenRequest(user="u", top_k=0, top_p=1.0), 0, cfg)
    assert (sp.top_k, sp.top_p) == (0, 1.0)
    with pytest.raises(SystemExit):
        config_from_args(build_parser().parse_args(["-i", "t.json", "--top-p", "0"]))


def test_local_provider_applies_configured_filters():
    cfg = LLMConfig(MAX_TOKENS=4, TOP_K=2)
    prov = LocalEngineProvider("tiny", cfg, device="cpu", max_model_len=256,
                               engine_options={"kv_pages": 32, "max_num_seqs": 4})
    reqs = [GenRequest(user="hello there", max_tokens=4, temperature=1.5),
            GenRequest(user="second", max_tokens=4, temperature=1.5, top_k=0)]
    asyncio.run(prov.generate_batch(reqs))
    assert prov.stats()["filtered_steps"] > 0
    prov.close()


# ------------------------------------------------------------------ gloo TP=2 (CPU)
TP_SCRIPT = textwrap.dedent("""
    import json, os, sys
    sys.path.insert(0, %(root)r)
    import torch
    from llm_map_reduce_summarizer_amd.parallel import dist as pdist
    pdist.init_distributed_from_env(backend="gloo")
    par = pdist.setup_parallel(int(os.environ.get("TP", "1")))
    from llm_map_reduce_summarizer_amd.engine.config import get_model_config
    from llm_map_reduce_summarizer_amd.engine.engine import LLMEngine, SamplingParams
    cfg = get_model_config("tiny-gqa4", init_std=0.05)
    eng = LLMEngine(cfg, device="cpu", dtype=torch.float32, max_model_len=512, max_num_seqs=4, kv_pages=64,
                    sync_every=3, tp_rank=par.tp_rank, tp_size=par.tp, tp_group=par.tp_group)
    prompts = [[128000] + [(i * 7 + j * 3) %% 9000 + 5 for j in range(20 + 9 * i)] for i in range(3)]
    sp = [SamplingParams(5, 1.5, 1, top_k=3), SamplingParams(5, 1.5, 2, top_p=0.6), SamplingParams(5, 1.5, 3)]
    outs = eng.generate(prompts, sp)
    assert eng.stats["filtered_steps"] > 0
    print("RESULT " + json.dumps([o.token_ids for o in outs]), flush=True)
    pdist.shutdown()
""")


def _run_tp(world: int, tp: int):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world),
               OMP_NUM_THREADS="2", TP=str(tp))
    procs = [subprocess.Popen([sys.executable, "-c", TP_SCRIPT % {"root": ROOT}],
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for r in range(world)]
    outs = []
    for p in procs:
        o, err = p.communicate(timeout=600)
        assert p.returncode == 0, err[-3000:]
        outs.append(json.loads([ln for ln in o.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    return outs


@pytest.mark.slow
def test_tp2_filtered_matches_tp1():
    ref = _run_tp(1, 1)[0]
    tp = _run_tp(2, 2)
    assert tp[0] == tp[1]  # both TP ranks sample identically
    assert tp[0] == ref
