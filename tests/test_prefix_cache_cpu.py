"""KV prefix caching on the CPU: the page allocator's reference counts and content index (native library
and Python fallback, same ids for the same calls), and the engine on the reference ops (tiny-gqa4, greedy,
fp32): cache-on cold, cache-on warm and cache-off generate the same tokens, and the token counts are exact."""

import pytest
import torch

from llm_map_reduce_summarizer_amd.engine.config import get_model_config
from llm_map_reduce_summarizer_amd.engine.engine import LLMEngine, SamplingParams
from llm_map_reduce_summarizer_amd.engine.kv_cache import PageAllocator

P = 64


# ------------------------------------------------------------------ allocator
def _alloc(native, n=16):
    a = PageAllocator(n, native=native)
    assert a.native == native
    return a


def _toks(n, salt=0):
    return [(salt * 7919 + j * 13) % 9000 + 5 for j in range(n)]


def _seq(a, prompt, extra=1):
    """Admit ``prompt`` the way the engine does: match, allocate the rest, publish the full pages."""
    hit = a.match(prompt)
    pages = hit + a.alloc(-(-(len(prompt) + extra) // P) - len(hit))
    a.publish(prompt, pages, len(prompt) // P)
    return pages, len(hit)


BOTH = pytest.mark.parametrize("native", [True, False])


@BOTH
def test_match_publish_release_round_trip(native):
    a = _alloc(native)
    prompt = _toks(200)
    assert a.match(prompt) == [] and a.cached() == 0
    pages = a.alloc(4)
    assert a.publish(prompt, pages, 3) == 3 and a.cached() == 3
    assert a.available() == 15 - 4
    hit = a.match(prompt)
    assert hit == pages[:3]  # found by content, a second holder
    a.release(pages)
    assert a.available() == 15 - 4 + 1  # the private tail page is free again, the shared ones are held
    a.release(hit)
    assert a.available() == 15 and a.cached() == 3  # evictable: content kept, still findable
    assert a.match(prompt) == pages[:3]
    a.release(pages[:3])
    a.reset()
    assert a.cached() == 0 and a.match(prompt) == [] and a.available() == 15


@BOTH
@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 129])
def test_match_cap(native, n):
    """At most (len - 1) // 64 pages: one prompt token at least is always computed and sampled from."""
    a = _alloc(native)
    long = _toks(4 * P)
    pages = a.alloc(4)
    a.publish(long, pages, 4)
    hit = a.match(long[:n])
    assert hit == pages[:(n - 1) // P]
    a.release(hit)
    a.release(pages)
    assert a.available() == 15


@BOTH
def test_publish_onto_existing_node_keeps_it(native):
    a = _alloc(native)
    prompt = _toks(130)
    first, second = a.alloc(3), a.alloc(3)
    assert a.publish(prompt, first, 2) == 2
    assert a.publish(prompt, second, 2) == 0  # the nodes exist: the second caller's pages stay private
    assert a.match(prompt) == first[:2]
    a.release(second)
    assert a.available() == 15 - 3  # private pages go straight back to the free list
    a.release(first)
    a.release(first[:2])
    assert a.available() == 15
    with pytest.raises(ValueError):
        a.publish(prompt, first, 3)  # the third page is not full of prompt tokens
    x = a.alloc(1)
    a.release(x)
    with pytest.raises(ValueError):
        a.publish(prompt, x + x, 2)  # pages the caller does not hold


@BOTH
def test_chains_that_differ_in_page_two_share_one_page(native):
    a = _alloc(native)
    one = _toks(200)
    two = list(one)
    two[P + 17] += 1  # one token id of page 2
    p1, h1 = _seq(a, one)
    p2, h2 = _seq(a, two)
    assert (h1, h2) == (0, 1) and p2[0] == p1[0] and not set(p2[1:]) & set(p1)
    assert a.cached() == 5  # page 1 shared, pages 2 and 3 of each chain
    three = list(one)
    three[3] += 1  # page 1 differs: nothing shared, although pages 2 and 3 hold the same ids
    p3, h3 = _seq(a, three)
    assert h3 == 0 and not set(p3) & (set(p1) | set(p2))
    for p in (p1, p2, p3):
        a.release(p)
    assert a.available() == 15


@BOTH
def test_eviction_order_and_no_orphans(native):
    """alloc takes free pages first, then the least recently used evictable page; a chain is eaten from its
    tail (its head is its most recent page), and a node below an evicted one is gone with it."""
    a = _alloc(native, 8)  # 7 usable pages
    old, new = _toks(3 * P + 1, 1), _toks(2 * P + 1, 2)
    po, _ = _seq(a, old, extra=0)   # 4 pages, 3 of them nodes
    pn, _ = _seq(a, new, extra=0)   # 3 pages, 2 of them nodes
    a.release(po)
    a.release(pn)
    assert a.available() == 7 and a.cached() == 5 and a.evictions() == 0
    assert a.alloc(2) == [pn[2], po[3]]  # the free ones first, LIFO
    assert a.cached() == 5
    assert a.alloc(1) == [po[2]] and a.evictions() == 1  # the older chain's tail
    hit = a.match(old)
    assert hit == po[:2]  # the rest of the chain is still reachable, now the most recent and held
    assert a.alloc(2) == [pn[1], pn[0]] and a.evictions() == 3
    assert a.match(new) == []
    with pytest.raises(MemoryError):
        a.alloc(1)  # everything left is held
    a.release(hit)
    # the head goes last; taking it while its child is cached would orphan the child: they go together
    child_holder = a.match(old[:2 * P + 1])
    assert child_holder == po[:2]
    a.release(child_holder[:1])  # (a holder of the child only: not something the engine does)
    before = a.evictions()
    got = a.alloc(1)
    assert got == [po[0]] and a.evictions() == before + 2 and a.cached() == 0
    assert a.match(old) == []  # po[1] is held but no longer findable
    a.release(child_holder[1:])
    assert a.available() == 1


@BOTH
def test_available_when_idle_and_double_release(native):
    a = _alloc(native)
    assert a.available() == a.num_pages - 1
    pages, _ = _seq(a, _toks(300))
    a.release(pages)
    assert a.available() == a.num_pages - 1
    with pytest.raises(ValueError):
        a.release(pages)  # cached pages nobody holds
    with pytest.raises(ValueError):
        a.release([0])
    with pytest.raises(ValueError):
        a.release([a.num_pages + 3])
    x = a.alloc(2)
    with pytest.raises(ValueError):
        a.release([x[0], x[0]])
    a.release(x)
    with pytest.raises(ValueError):
        a.free(x)
    assert a.available() == a.num_pages - 1


def _script(a):
    """A fixed call sequence over every entry point; returns everything it saw."""
    seen = []
    held = []
    for k in range(40):
        prompt = _toks(40 + 37 * (k % 9), salt=k % 5)
        while held and (len(prompt) + 8) // P + 1 > a.available():
            a.release(held.pop(0))
        pages, hit = _seq(a, prompt, extra=8)
        seen.append((tuple(pages), hit, a.available(), a.cached(), a.evictions()))
        held.append(pages)
        if k % 3 == 2:
            a.release(held.pop(0))
        if k == 25:
            a.reset()
    for p in held:
        a.release(p)
    seen.append(a.available())
    return seen


def test_native_and_fallback_agree():
    assert _script(_alloc(True, 24)) == _script(_alloc(False, 24))


@BOTH
def test_index_unused_is_the_plain_allocator(native):
    """With the index never used, alloc / free return the ids of the plain LIFO free list."""
    a = _alloc(native, 12)
    free = list(range(11, 0, -1))  # the plain allocator: a stack, page 1 on top
    held = []
    for n in (3, 2, -1, 4, -1, -1, 5, 6):
        if n < 0:
            pages = held.pop(0)
            a.free(pages)
            free.extend(reversed(pages))
        else:
            want = [free.pop() for _ in range(n)]
            assert a.alloc(n) == want
            held.append(want)
        assert a.available() == len(free)
    assert a.cached() == 0 and a.evictions() == 0


# ------------------------------------------------------------------ engine
CFG = get_model_config("tiny-gqa4", init_std=0.05)


def _engine(cache, **kw):
    args = dict(device="cpu", dtype=torch.float32, max_model_len=1024, max_num_seqs=8, kv_pages=96, sync_every=3)
    args.update(kw)
    return LLMEngine(CFG, prefix_cache=cache, **args)


def _prompt(n, salt):
    return [128000] + [(salt * 31 + j * 7) % 9000 + 5 for j in range(n - 1)]


def _greedy(n, k=6):
    return [SamplingParams(k, 0.0, i) for i in range(n)]


def _ids(outs):
    return [o.token_ids for o in outs]


LENS = (450, 130, 61, 300, 64, 65)


def test_cold_warm_and_off_agree_with_exact_counts():
    prompts = [_prompt(n, i) for i, n in enumerate(LENS)]
    off = _engine(False)
    ref = off.generate(prompts, _greedy(len(prompts)))
    assert all(o.cached_tokens == 0 for o in ref) and "prefix_hit_tokens" not in off.stats
    on = _engine(True)
    cold = on.generate(prompts, _greedy(len(prompts)))
    assert _ids(cold) == _ids(ref) and all(o.cached_tokens == 0 for o in cold)
    assert on.stats["prefill_tokens"] == sum(LENS)
    assert on.kv.alloc.available() == on.kv.num_pages - 1
    assert on.kv.alloc.cached() == sum(n // P for n in LENS)
    warm = on.generate(prompts, _greedy(len(prompts)))
    assert _ids(warm) == _ids(ref)
    want = [P * ((n - 1) // P) for n in LENS]
    assert [o.cached_tokens for o in warm] == want
    assert on.stats["prefill_tokens"] == 2 * sum(LENS) - sum(want)
    st = on.engine_stats()
    assert st["prefix_hit_tokens"] == sum(want) and st["prefix_hit_requests"] == sum(1 for w in want if w)
    assert st["prefix_evictions"] == 0
    assert on.kv.alloc.available() == on.kv.num_pages - 1


def test_common_head_with_distinct_tails():
    head = _prompt(200, 77)
    totals = (63, 64, 65, 128, 129, 300)
    prompts = [(head + [(i * 131 + j * 11) % 9000 + 5 for j in range(300)])[:n] for i, n in enumerate(totals)]
    ref = _engine(False).generate(prompts, _greedy(len(prompts)))
    on = _engine(True)
    on.generate([head], _greedy(1))  # the head's 3 full pages
    got = on.generate(prompts, _greedy(len(prompts)))
    assert _ids(got) == _ids(ref)
    assert [o.cached_tokens for o in got] == [P * min(3, (n - 1) // P) for n in totals]
    assert on.kv.alloc.available() == on.kv.num_pages - 1


def test_chunked_prefill_and_a_follow_up_turn():
    prompt = _prompt(2600, 5)
    kw = dict(max_model_len=4096, kv_pages=128, prefill_chunk=512)
    off, on = _engine(False, **kw), _engine(True, **kw)
    first_ref = off.generate([prompt], _greedy(1, 8))[0]
    first = on.generate([prompt], _greedy(1, 8))[0]
    assert first.token_ids == first_ref.token_ids and first.cached_tokens == 0
    slices = on.stats["prefill_slices"]
    assert slices == 6  # 2600 tokens, end-aligned slices of 512
    turn = prompt + first.token_ids + _prompt(50, 9)[1:] + [17]
    ref = off.generate([turn], _greedy(1, 8))[0]
    got = on.generate([turn], _greedy(1, 8))[0]
    assert got.token_ids == ref.token_ids
    assert got.cached_tokens == P * (2600 // P) == 2560  # every full page of the first prompt
    assert on.stats["prefill_tokens"] == 2600 + len(turn) - 2560
    assert on.stats.get("prefill_slices", 0) == slices  # the remainder fits one pass
    # a remainder longer than the chunk is cut by the end-aligned rule applied to the remainder
    assert on._slices(2600, 1024) == [(1024, 1064), (1064, 1576), (1576, 2088), (2088, 2600)]
    assert on._slices(2600, 0) == off._slices(2600)
    longer = turn + _prompt(700, 3)[1:]
    ref = off.generate([longer], _greedy(1, 4))[0]
    got = on.generate([longer], _greedy(1, 4))[0]
    assert got.token_ids == ref.token_ids and got.cached_tokens == P * (len(turn) // P)
    assert on.stats["prefill_slices"] == slices + 2  # 700-odd new tokens: two slices


def test_feeder_joiner_hits_the_cache():
    running = [_prompt(40 + 9 * i, i) for i in range(3)]
    joiner = _prompt(600, 42)

    def run(eng):
        fed = []

        def feeder(done):
            if not fed:
                fed.append(1)
                return [(joiner, SamplingParams(12, 0.0, 99))]
            return []
        return eng.generate(running, _greedy(3, 30), feeder=feeder)

    kw = dict(prefill_chunk=64, sync_every=2)
    ref = run(_engine(False, **kw))
    on = _engine(True, **kw)
    on.generate([joiner[:400]], _greedy(1, 2))
    before = on.stats["prefill_tokens"]
    got = run(on)
    assert _ids(got) == _ids(ref)
    assert on.stats["interleaved_prefills"] == 1
    assert got[3].cached_tokens == P * (400 // P) == 384
    assert on.stats["prefill_tokens"] - before == sum(len(p) for p in running) + 600 - 384
    # a second joiner of the same prompt finds what the first one published when its last slice ran
    again = run(on)
    assert _ids(again) == _ids(ref) and again[3].cached_tokens == P * (599 // P)
    assert on.kv.alloc.available() == on.kv.num_pages - 1


def test_identical_prompts_in_one_call_flush_the_batch():
    prompt = _prompt(300, 8)
    other = _prompt(90, 2)
    ref = _engine(False).generate([prompt, prompt, other], _greedy(3))
    on = _engine(True)
    got = on.generate([prompt, prompt, other], _greedy(3))
    assert _ids(got) == _ids(ref)
    assert [o.cached_tokens for o in got] == [0, P * (299 // P), 0]
    assert on.stats["prefill_tokens"] == 300 + (300 - 256) + 90
    # prompts that share only what the index already serves do not flush again
    trio = [prompt[:256] + _prompt(80, 20 + i)[1:] for i in range(3)]
    before = on.stats["prefill_tokens"]
    got = on.generate(trio, _greedy(3))
    assert [o.cached_tokens for o in got] == [256] * 3
    assert on.stats["prefill_tokens"] - before == 3 * 79


def test_eviction_under_pressure():
    kw = dict(kv_pages=64, max_model_len=1024)
    prompts = [_prompt(500, 100 + i) for i in range(12)]  # 8 pages each: 96 > 63
    off, on = _engine(False, **kw), _engine(True, **kw)
    ref = off.generate(prompts, _greedy(12, 4))
    got = on.generate(prompts, _greedy(12, 4))  # finishes: no MemoryError
    assert _ids(got) == _ids(ref)
    st = on.engine_stats()
    assert st["prefix_evictions"] > 0 and on.kv.alloc.available() == 63
    # whichever prompt ran first is long gone: it repeats as a cold one, with its cold tokens
    # (equal lengths: admission keeps the request order, so request 0 was published first and evicted first)
    again = on.generate([prompts[0]], _greedy(1, 4))[0]
    assert again.cached_tokens == 0 and again.token_ids == ref[0].token_ids
    assert on.kv.alloc.available() == 63


def test_exception_in_a_prefill_pass_empties_the_index(monkeypatch):
    on = _engine(True)
    prompts = [_prompt(n, i) for i, n in enumerate((300, 200))]
    ref = on.generate(prompts, _greedy(2))
    assert on.kv.alloc.cached() > 0
    real = on.model.prefill

    def boom(*a, **kw):
        raise RuntimeError("injected")

    monkeypatch.setattr(on.model, "prefill", boom)
    with pytest.raises(RuntimeError, match="injected"):
        on.generate([_prompt(300, 0)[:280] + [9, 9, 9], _prompt(150, 50)], _greedy(2))
    assert on.kv.alloc.cached() == 0 and on.kv.alloc.available() == on.kv.num_pages - 1
    monkeypatch.setattr(on.model, "prefill", real)
    got = on.generate(prompts, _greedy(2))
    assert _ids(got) == _ids(ref) and all(o.cached_tokens == 0 for o in got)


def test_flag_off_keeps_the_page_ids(monkeypatch):
    """Off by default, and then the allocator is the plain LIFO list: the ids of an admission are the top of
    the free list in order, nothing is cached, and everything is free again afterwards."""
    monkeypatch.delenv("MRSUM_PREFIX_CACHE", raising=False)
    off = LLMEngine(CFG, device="cpu", dtype=torch.float32, max_model_len=1024, max_num_seqs=8, kv_pages=96,
                    sync_every=3)
    assert off.prefix_cache is False
    prompts = [_prompt(n, i) for i, n in enumerate((300, 130))]
    seen = []
    off.generate(prompts, _greedy(2), on_prefill=lambda seqs: seen.extend(list(s.pages) for s in seqs))
    assert seen == [[1, 2, 3, 4, 5], [6, 7, 8]]
    assert off.kv.alloc.cached() == 0 and off.kv.alloc.available() == off.kv.num_pages - 1
    off.generate(prompts[:1], _greedy(1), on_prefill=lambda seqs: seen.extend(list(s.pages) for s in seqs))
    assert seen[-1] == [6, 7, 8, 1, 2]  # LIFO reuse, as the plain list


def test_exports_skip_the_cache():
    on = _engine(True)
    prompt = _prompt(200, 4)
    on.prefill_export([prompt], _greedy(1), groups=1)
    assert on.kv.alloc.cached() == 0
    on.generate([prompt], _greedy(1))
    assert on.kv.alloc.cached() == 3
    hits = on.stats["prefix_hit_requests"]
    on.prefill_export([prompt], _greedy(1), groups=1)
    assert on.stats["prefix_hit_requests"] == hits and on.kv.alloc.available() == on.kv.num_pages - 1


# ------------------------------------------------------------------ public surface
def test_cached_tokens_travel_as_a_plain_int():
    """GenResult.extra["cached_tokens"]: present only when non-zero, and a plain int through the JSON of the DP
    all-gather and of the serve broadcast."""
    import json

    from llm_map_reduce_summarizer_amd.engine.engine import GenOutput
    from llm_map_reduce_summarizer_amd.engine.provider import _result, result_record
    hit, cold = GenOutput([5, 6], 200, "length", cached_tokens=128), GenOutput([5, 6], 200, "length")
    assert result_record(cold) == {} and result_record(hit) == {"cached": 128}
    rec = json.loads(json.dumps({"i": 0, "text": "x", "pt": 200, "ct": 2, "fr": "length", **result_record(hit)}))
    extra = _result(rec).extra
    assert extra == {"finish_reason": "length", "cached_tokens": 128} and type(extra["cached_tokens"]) is int
    rec = json.loads(json.dumps({"i": 0, "text": "x", "pt": 200, "ct": 2, "fr": "length", **result_record(cold)}))
    assert _result(rec).extra == {"finish_reason": "length"}


def test_flag_reaches_the_engine_from_cli_environment_and_provider(monkeypatch):
    from llm_map_reduce_summarizer_amd.cli import build_parser
    from llm_map_reduce_summarizer_amd.config import LLMConfig
    from llm_map_reduce_summarizer_amd.engine.provider import LocalEngineProvider
    args = build_parser().parse_args(["--input", "x.json", "--prefix-cache"])
    assert args.prefix_cache is True
    assert build_parser().parse_args(["--input", "x.json"]).prefix_cache is None
    monkeypatch.delenv("ENGINE_PREFIX_CACHE", raising=False)
    assert LLMConfig().ENGINE_PREFIX_CACHE == 0
    assert LocalEngineProvider("tiny-gqa4", LLMConfig(), device="cpu").prefix_cache is False
    assert LocalEngineProvider("tiny-gqa4", LLMConfig(ENGINE_PREFIX_CACHE=1), device="cpu").prefix_cache is True
    monkeypatch.setenv("ENGINE_PREFIX_CACHE", "1")
    assert LocalEngineProvider("tiny-gqa4", LLMConfig(), device="cpu").prefix_cache is True
    monkeypatch.delenv("ENGINE_PREFIX_CACHE")
    prov = LocalEngineProvider("tiny-gqa4", LLMConfig(), device="cpu", prefix_cache=True, max_model_len=512,
                               engine_options={"kv_pages": 32, "max_num_seqs": 4})
    assert prov.engine.prefix_cache is True and prov.prefix_stats() == {
        "prefix_hit_tokens": 0, "prefix_hit_requests": 0, "prefix_evictions": 0}
    monkeypatch.setenv("MRSUM_PREFIX_CACHE", "1")  # a bare engine
    assert LLMEngine(CFG, device="cpu", max_model_len=256, max_num_seqs=2, kv_pages=8).prefix_cache is True
    with pytest.raises(ValueError, match="64-token pages"):
        LLMEngine(CFG, device="cpu", max_model_len=256, max_num_seqs=2, kv_pages=8, page_size=32)
