"""logprobs / top_logprobs through the HTTP server (its own server, as tests/test_serve.py starts one): the
chat endpoint's ``choices[0].logprobs.content`` against the in-process engine's records, the refusals, and a
request without the fields."""

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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
uvicorn = pytest.importorskip("uvicorn")
pytest.importorskip("fastapi")

from llm_map_reduce_summarizer_amd.config import LLMConfig  # noqa: E402
from llm_map_reduce_summarizer_amd.engine.provider import LocalEngineProvider  # noqa: E402
from llm_map_reduce_summarizer_amd.pipeline.providers import GenRequest, GenResult  # noqa: E402
from llm_map_reduce_summarizer_amd.serve import (BadRequest, ContinuousBatcher, anthropic_request, build_app,  # noqa: E402
                                                 make_batcher, openai_request, openai_response)

KEY = "sk-local-test"
CHAT, MESSAGES = "/v1/chat/completions", "/v1/messages"
MSGS = [{"role": "user", "content": "Summarize: the meeting moved to Tuesday."}]
BAN = 4321  # banned by the server's configuration ($LOGIT_BIAS): no request body can carry a -inf


@pytest.fixture(scope="module")
def server():
    provider = LocalEngineProvider("tiny-gqa4", LLMConfig(LOGIT_BIAS="%d:ban" % BAN), device="cpu", use_graphs=False,
                                   max_model_len=2048, engine_options={"max_new_cap": 64})
    batcher = make_batcher(provider, max_batch=16, window_s=0.05)
    assert isinstance(batcher, ContinuousBatcher)
    batcher.start()
    app = build_app(batcher, "mrsum-tiny", api_key=KEY)
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
    yield provider, batcher, "http://127.0.0.1:%d" % port
    srv.should_exit = True
    th.join(10)
    batcher.shutdown(10)


def _post(url, body, anthropic=False):
    headers = {"Content-Type": "application/json"}
    headers.update({"x-api-key": KEY} if anthropic else {"Authorization": "Bearer " + KEY})
    req = urllib.request.Request(url, data=json.dumps(body).encode(), headers=headers, method="POST")
    try:
        with urllib.request.urlopen(req, timeout=120) as r:
            return r.status, json.loads(r.read())
    except urllib.error.HTTPError as e:
        return e.code, json.loads(e.read())


def _direct(provider, **kw):
    req = GenRequest(MSGS[0]["content"], None, kw.pop("max_tokens", 5), 0.0, stage="serve", **kw)
    return asyncio.run(provider.generate_batch([req]))[0]


def _entry(tok, tokenizer):
    raw = tokenizer.decode_bytes([tok], skip_special=False)
    return raw.decode("utf-8", errors="replace"), list(raw)


@pytest.mark.parametrize("n", [0, 3, 20])
def test_content_matches_the_engines_records(server, n):
    provider, _, base = server
    want = _direct(provider, logprobs=True, top_logprobs=n)
    rec = want.extra["logprobs"]
    body = {"messages": MSGS, "max_tokens": 5, "temperature": 0, "logprobs": True}
    if n:
        body["top_logprobs"] = n
    st, out = _post(base + CHAT, body)
    assert st == 200 and out["choices"][0]["message"]["content"] == want.text
    content = out["choices"][0]["logprobs"]["content"]
    assert len(content) == out["usage"]["completion_tokens"] == len(rec["token_ids"]) == 5
    tk = provider.tokenizer
    for c, tok, lp, top in zip(content, rec["token_ids"], rec["token_logprobs"], rec["top"]):
        assert (c["token"], c["bytes"]) == _entry(tok, tk) and c["logprob"] == lp
        assert len(c["top_logprobs"]) == n == len(top)
        for e, (t, x) in zip(c["top_logprobs"], top):
            assert (e["token"], e["bytes"]) == _entry(t, tk) and e["logprob"] == x and set(e) == {"token", "logprob",
                                                                                                  "bytes"}
        if n:
            assert c["top_logprobs"][0]["logprob"] == c["logprob"]  # greedy: the sampled token leads its list
    assert "".join(c["token"] for c in content) == tk.decode(rec["token_ids"], skip_special=False)


def test_a_banned_token_is_sent_as_minus_9999(server):
    """The served configuration bans one token ($LOGIT_BIAS, on top of which the request adds a bias of its
    own): the engine's records hold its -inf, and wherever such a value reaches a response it is -9999.0.  In a
    vocabulary of 128256 tokens a banned token never makes a top-20 list, so the wire form is checked on the
    response built from a record that holds one, after the JSON round trip of the result all-gather."""
    provider, _, base = server
    st, out = _post(base + CHAT, {"messages": MSGS, "max_tokens": 3, "temperature": 0, "logprobs": True,
                                  "top_logprobs": 20, "logit_bias": {"77": 100}})
    assert st == 200  # (the request's own logit_bias replaces the configured ban: token 77 wins every step)
    content = out["choices"][0]["logprobs"]["content"]
    assert all(c["bytes"] == _entry(77, provider.tokenizer)[1] and abs(c["logprob"]) < 1e-6 for c in content)
    st, out = _post(base + CHAT, {"messages": MSGS, "max_tokens": 3, "temperature": 0, "logprobs": True,
                                  "top_logprobs": 20})
    assert st == 200  # the configured ban acts: the banned token is in no list, every value is finite
    for c in out["choices"][0]["logprobs"]["content"]:
        assert all(e["bytes"] != _entry(BAN, provider.tokenizer)[1] and e["logprob"] > -9999.0
                   for e in c["top_logprobs"])
    rec = {"token_ids": [5, BAN], "token_logprobs": [-0.5, float("-inf")],
           "top": [[[5, -0.5], [BAN, float("-inf")]], [[BAN, float("-inf")]]]}
    rec = json.loads(json.dumps(rec))
    res = GenResult("x", 3, 2, extra={"finish_reason": "length", "logprobs": rec})
    content = openai_response(res, "m", provider.tokenizer)["choices"][0]["logprobs"]["content"]
    assert [c["logprob"] for c in content] == [-0.5, -9999.0]
    assert [e["logprob"] for e in content[0]["top_logprobs"]] == [-0.5, -9999.0]
    assert content[1]["top_logprobs"][0] == {"token": _entry(BAN, provider.tokenizer)[0], "logprob": -9999.0,
                                             "bytes": _entry(BAN, provider.tokenizer)[1]}
    json.dumps(content, allow_nan=False)  # nothing non-finite is left for the wire


def test_a_request_without_the_fields_is_as_before(server):
    provider, _, base = server
    want = _direct(provider)
    assert "logprobs" not in want.extra
    for extra in ({}, {"logprobs": False}, {"logprobs": None, "top_logprobs": None}, {"logprobs": False,
                                                                                      "top_logprobs": 0}):
        st, out = _post(base + CHAT, dict({"messages": MSGS, "max_tokens": 5, "temperature": 0}, **extra))
        assert st == 200 and out["choices"][0]["message"]["content"] == want.text
        assert "logprobs" not in out["choices"][0]
    st, out = _post(base + CHAT, {"messages": MSGS, "max_tokens": 5, "temperature": 0, "logprobs": True})
    assert out["choices"][0]["message"]["content"] == want.text  # asking changes no token


BAD = [{"logprobs": 1}, {"logprobs": "true"}, {"logprobs": [True]}, {"logprobs": True, "top_logprobs": 21},
       {"logprobs": True, "top_logprobs": -1}, {"logprobs": True, "top_logprobs": 2.5},
       {"logprobs": True, "top_logprobs": "3"}, {"logprobs": True, "top_logprobs": True}, {"top_logprobs": 3},
       {"logprobs": False, "top_logprobs": 3}, {"logprobs": True, "stream": True},
       {"logprobs": True, "top_logprobs": 2, "stream": True}]


@pytest.mark.parametrize("bad", BAD)
def test_bad_values_are_400(server, bad):
    _, batcher, base = server
    before = batcher.stats["requests"]
    st, out = _post(base + CHAT, dict({"messages": MSGS, "max_tokens": 8}, **bad))
    assert st == 400 and out["error"]["type"] == "invalid_request_error", out
    assert batcher.stats["requests"] == before  # refused at the door: nothing reached the engine
    with pytest.raises(BadRequest):
        openai_request(dict({"messages": MSGS, "max_tokens": 8}, **bad))


@pytest.mark.parametrize("extra", [{"logprobs": True}, {"logprobs": False}, {"top_logprobs": 0},
                                   {"logprobs": True, "top_logprobs": 5}])
def test_the_messages_api_refuses_the_fields(server, extra):
    _, batcher, base = server
    before = batcher.stats["requests"]
    st, out = _post(base + MESSAGES, dict({"messages": MSGS, "max_tokens": 8}, **extra), anthropic=True)
    assert st == 400 and out["error"]["type"] == "invalid_request_error" and "logprobs" in out["error"]["message"]
    assert batcher.stats["requests"] == before
    with pytest.raises(BadRequest):
        anthropic_request(dict({"messages": MSGS, "max_tokens": 8}, **extra))


def test_the_stream_refusal_says_why(server):
    _, _, base = server
    st, out = _post(base + CHAT, {"messages": MSGS, "max_tokens": 8, "logprobs": True, "stream": True})
    assert st == 400 and "stream" in out["error"]["message"]
    r = openai_request({"messages": MSGS, "logprobs": True, "top_logprobs": 20})
    assert (r.logprobs, r.top_logprobs) == (True, 20)
    r = openai_request({"messages": MSGS, "stream": True})  # streaming without logprobs stays what it was
    assert (r.logprobs, r.top_logprobs) == (None, None)
