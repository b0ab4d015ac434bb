"""``n`` on the chat endpoint and the prefix cache through the HTTP server (CPU engine; two servers of its own, as
tests/test_serve.py starts one: cache off and cache on): n choices against n single requests with seeds
seed + i, the refusals, ``usage.prompt_tokens_details.cached_tokens`` and the /metrics counters."""

import asyncio
import json
import os
import socket
import sys
import threading
import time
import urllib.error
import urllib.request

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
uvicorn = pytest.importorskip("uvicorn")
pytest.importorskip("fastapi")

from llm_map_reduce_summarizer_amd.config import LLMConfig  # noqa: E402
from llm_map_reduce_summarizer_amd.engine.provider import LocalEngineProvider, sampling_params  # noqa: E402
from llm_map_reduce_summarizer_amd.pipeline.providers import GenRequest  # noqa: E402
from llm_map_reduce_summarizer_amd.serve import (BadRequest, ContinuousBatcher, _n, build_app,  # noqa: E402
                                                 make_batcher)

KEY = "sk-local-test"
CHAT, MESSAGES = "/v1/chat/completions", "/v1/messages"
LONG = "Summarize the minutes. " + " ".join("item %d was moved to week %d;" % (i, i % 7) for i in range(60))
MSGS = [{"role": "user", "content": LONG}]


def _serve(prefix_cache):
    provider = LocalEngineProvider("tiny-gqa4", LLMConfig(), device="cpu", use_graphs=False, max_model_len=2048,
                                   engine_options={"max_new_cap": 64, "dtype": torch.float32},
                                   prefix_cache=prefix_cache)
    batcher = make_batcher(provider, max_batch=16, window_s=0.05)
    assert isinstance(batcher, ContinuousBatcher)
    batcher.start()
    app = build_app(batcher, "mrsum-tiny", api_key=KEY, max_n=16)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    srv = uvicorn.Server(uvicorn.Config(app, host="127.0.0.1", port=port, log_level="warning"))
    th = threading.Thread(target=srv.run, daemon=True)
    th.start()
    t0 = time.time()
    while not srv.started and time.time() - t0 < 30:
        time.sleep(0.05)
    assert srv.started
    return provider, batcher, "http://127.0.0.1:%d" % port, srv, th


def _stop(srv, th, batcher):
    srv.should_exit = True
    th.join(10)
    batcher.shutdown(10)


@pytest.fixture(scope="module")
def server():
    provider, batcher, base, srv, th = _serve(False)
    yield provider, batcher, base
    _stop(srv, th, batcher)


@pytest.fixture(scope="module")
def cached_server():
    provider, batcher, base, srv, th = _serve(True)
    yield provider, batcher, base
    _stop(srv, th, batcher)


def _post(url, body, anthropic=False):
    headers = {"Content-Type": "application/json"}
    headers.update({"x-api-key": KEY} if anthropic else {"Authorization": "Bearer " + KEY})
    req = urllib.request.Request(url, data=json.dumps(body).encode(), headers=headers, method="POST")
    try:
        with urllib.request.urlopen(req, timeout=120) as r:
            return r.status, json.loads(r.read())
    except urllib.error.HTTPError as e:
        return e.code, json.loads(e.read())


def _singles(provider, n, max_tokens, temperature, **kw):
    """The n single requests choice i stands for: the same request with the seed seed + i."""
    reqs = [GenRequest(LONG, None, max_tokens, temperature, stage="serve", seed_offset=i, **kw) for i in range(n)]
    base = sampling_params(reqs[0], provider.seed, provider.config).seed
    assert [sampling_params(r, provider.seed, provider.config).seed for r in reqs] == [base + i for i in range(n)]
    return [asyncio.run(provider.generate_batch([r]))[0] for r in reqs]


@pytest.mark.parametrize("which", ["server", "cached_server"])
def test_n_choices_equal_single_requests(which, request):
    provider, _, base = request.getfixturevalue(which)
    body = {"messages": MSGS, "max_tokens": 6, "temperature": 0.9, "n": 3, "logprobs": True, "top_logprobs": 2}
    st, out = _post(base + CHAT, body)
    assert st == 200, out
    singles = _singles(provider, 3, 6, 0.9, logprobs=True, top_logprobs=2)
    assert [c["index"] for c in out["choices"]] == [0, 1, 2]
    assert [c["message"]["content"] for c in out["choices"]] == [r.text for r in singles]
    assert len({r.text for r in singles}) > 1  # the seeds differ, and so do the samples
    for c, r in zip(out["choices"], singles):
        assert c["finish_reason"] == "length"
        want = r.extra["logprobs"]["token_logprobs"]
        assert [e["logprob"] for e in c["logprobs"]["content"]] == pytest.approx(want, abs=1e-6)
        assert all(len(e["top_logprobs"]) == 2 for e in c["logprobs"]["content"])
    assert out["usage"]["prompt_tokens"] == singles[0].prompt_tokens  # counted once
    assert out["usage"]["completion_tokens"] == 18 and out["usage"]["total_tokens"] == singles[0].prompt_tokens + 18
    if which == "cached_server":
        assert provider.prefix_stats()["prefix_hit_requests"] >= 2  # the siblings shared the prompt's pages
    st, one = _post(base + CHAT, dict(body, n=1))
    assert st == 200 and len(one["choices"]) == 1 and one["choices"][0]["message"]["content"] == singles[0].text


@pytest.mark.parametrize("bad", [0, 17, -1, 2.0, "2", True, [2]])
def test_n_out_of_range_is_400(server, bad):
    _, batcher, base = server
    before = batcher.stats["requests"]
    st, out = _post(base + CHAT, {"messages": MSGS, "max_tokens": 2, "n": bad})
    assert st == 400 and out["error"]["type"] == "invalid_request_error", out
    assert batcher.stats["requests"] == before


def test_n_with_stream_and_on_messages_is_400(server):
    _, batcher, base = server
    before = batcher.stats["requests"]
    st, out = _post(base + CHAT, {"messages": MSGS, "max_tokens": 2, "n": 2, "stream": True})
    assert st == 400 and out["error"]["type"] == "invalid_request_error"
    st, out = _post(base + MESSAGES, {"messages": MSGS, "max_tokens": 2, "n": 2}, anthropic=True)
    assert st == 400 and out["error"]["type"] == "invalid_request_error"
    assert batcher.stats["requests"] == before


def test_max_n_bounds_n():
    """``build_app(max_n=...)``: its default of 1 keeps refusing n > 1; the server's --max-n default is 16."""
    assert _n({}) == 1 and _n({"n": None}, 1) == 1 and _n({"n": 1}, 1) == 1 and _n({"n": 16}) == 16
    with pytest.raises(BadRequest, match="not supported"):
        _n({"n": 2}, 1)
    with pytest.raises(BadRequest, match="at most 4"):
        _n({"n": 5}, 4)
    with pytest.raises(ValueError):
        build_app(None, "x", max_n=17)


def test_second_identical_request_reports_cached_tokens(cached_server):
    provider, _, base = cached_server
    body = {"messages": [{"role": "user", "content": "Again: " + LONG}], "max_tokens": 4, "temperature": 0}
    st, first = _post(base + CHAT, body)
    st2, second = _post(base + CHAT, body)
    assert st == 200 and st2 == 200
    n = first["usage"]["prompt_tokens"]
    assert n > 128
    assert first["usage"]["prompt_tokens_details"] == {"cached_tokens": 0}  # (new from its first page on)
    assert second["usage"]["prompt_tokens_details"] == {"cached_tokens": 64 * ((n - 1) // 64)}
    assert second["choices"][0]["message"]["content"] == first["choices"][0]["message"]["content"]
    assert second["usage"]["prompt_tokens"] == n
    # the next turn of the chat re-sends the first: its full pages are found again
    turn = body["messages"] + [{"role": "assistant", "content": first["choices"][0]["message"]["content"]},
                               {"role": "user", "content": "And the week after?"}]
    st, third = _post(base + CHAT, dict(body, messages=turn))
    assert st == 200 and third["usage"]["prompt_tokens_details"]["cached_tokens"] >= 64 * ((n - 8) // 64)
    # the messages endpoint has no such field
    st, msg = _post(base + MESSAGES, dict(body), anthropic=True)
    assert st == 200 and set(msg["usage"]) == {"input_tokens", "output_tokens"}


def test_metrics_show_the_counters(cached_server, server):
    provider, _, base = cached_server
    _post(base + CHAT, {"messages": MSGS, "max_tokens": 2, "temperature": 0})
    _post(base + CHAT, {"messages": MSGS, "max_tokens": 2, "temperature": 0})
    text = urllib.request.urlopen(base + "/metrics", timeout=30).read().decode()
    vals = {ln.split()[0]: float(ln.split()[1]) for ln in text.splitlines() if ln and not ln.startswith("#")}
    assert vals["mrsum_prefix_hit_requests"] >= 1 and vals["mrsum_prefix_hit_tokens"] >= 64
    assert "mrsum_prefix_evictions" in vals
    assert vals["mrsum_prefix_hit_tokens"] == provider.engine.engine_stats()["prefix_hit_tokens"]
    off = urllib.request.urlopen(server[2] + "/metrics", timeout=30).read().decode()
    assert "prefix" not in off and "mrsum_requests" in off


def test_without_the_flag_usage_has_no_details(server):
    provider, _, base = server
    body = {"messages": MSGS, "max_tokens": 3, "temperature": 0}
    _post(base + CHAT, body)
    st, out = _post(base + CHAT, body)
    assert st == 200 and "prompt_tokens_details" not in out["usage"]
    assert set(out["usage"]) == {"prompt_tokens", "completion_tokens", "total_tokens"}
    assert provider.prefix_cache is False and provider.engine.prefix_cache is False
