"""logit_bias / min_tokens / stop_token_ids through the HTTP server (its own server, as tests/test_serve.py
starts one): both endpoints map the three fields onto the engine, and a value out of range is a 400."""

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
from llm_map_reduce_summarizer_amd.pipeline.providers import GenRequest  # noqa: E402
from llm_map_reduce_summarizer_amd.serve import ContinuousBatcher, build_app, make_batcher  # noqa: E402

KEY = "sk-local-test"
CHAT, MESSAGES = "/v1/chat/completions", "/v1/messages"
MSGS = [{"role": "user", "content": "Summarize: the meeting moved to Tuesday."}]


@pytest.fixture(scope="module")
def server():
    provider = LocalEngineProvider("tiny-gqa4", LLMConfig(), device="cpu", use_graphs=False, max_model_len=2048)
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
    req = GenRequest(MSGS[0]["content"], None, kw.pop("max_tokens", 6), 0.0, stage="serve", **kw)
    return asyncio.run(provider.generate_batch([req]))[0]


def test_logit_bias_reaches_the_engine_on_both_endpoints(server):
    provider, _, base = server
    tok = 4321
    want = _direct(provider, logit_bias=[[tok, 100.0]])
    assert want.text == provider.tokenizer.decode([tok] * 6) != _direct(provider).text
    st, out = _post(base + CHAT, {"messages": MSGS, "max_tokens": 6, "temperature": 0, "logit_bias": {str(tok): 100}})
    assert st == 200 and out["choices"][0]["message"]["content"] == want.text
    assert out["usage"]["completion_tokens"] == 6 and out["choices"][0]["finish_reason"] == "length"
    st, out = _post(base + MESSAGES, {"messages": MSGS, "max_tokens": 6, "temperature": 0, "logit_bias": {tok: 100}},
                    anthropic=True)
    assert st == 200 and out["content"][0]["text"] == want.text


def test_stop_token_ids_and_min_tokens_reach_the_engine(server):
    provider, _, base = server
    tok = 4321
    body = {"messages": MSGS, "max_tokens": 9, "temperature": 0, "logit_bias": {str(tok): 100}, "stop_token_ids": [tok]}
    st, out = _post(base + CHAT, body)
    assert st == 200 and out["usage"]["completion_tokens"] == 1 and out["choices"][0]["finish_reason"] == "stop"
    st, out = _post(base + CHAT, dict(body, min_tokens=4))  # the stop id is kept out of the first four tokens
    assert st == 200 and out["usage"]["completion_tokens"] == 5 and out["choices"][0]["finish_reason"] == "stop"
    st, out = _post(base + MESSAGES, dict(body, min_tokens=4), anthropic=True)
    assert st == 200 and out["usage"]["output_tokens"] == 5 and out["stop_reason"] == "end_turn"


@pytest.mark.parametrize("path,anthropic", [(CHAT, False), (MESSAGES, True)])
@pytest.mark.parametrize("bad", [{"logit_bias": {"5": 101}}, {"logit_bias": {"5": "1"}}, {"logit_bias": [[5, 1]]},
                                 {"logit_bias": {str(i): 1 for i in range(301)}}, {"logit_bias": {"128256": 1}},
                                 {"logit_bias": {"five": 1}}, {"min_tokens": 9}, {"min_tokens": -1},
                                 {"min_tokens": 2.5}, {"stop_token_ids": [1, 2, 3, 4, 5]},
                                 {"stop_token_ids": [128256]}, {"stop_token_ids": "7"}, {"stop": ["\n"]}, {"n": 2}])
def test_bad_values_are_400(server, path, anthropic, bad):
    _, batcher, base = server
    before = batcher.stats["requests"]
    st, out = _post(base + path, dict({"messages": MSGS, "max_tokens": 8}, **bad), anthropic=anthropic)
    assert st == 400 and out["error"]["type"] == "invalid_request_error", out
    assert batcher.stats["requests"] == before  # refused at the door: nothing reached the engine
