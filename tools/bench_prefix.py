#!/usr/bin/env python3
"""What the KV prefix cache saves, and what its flush rule costs: the same engine with the cache off and on,
in one process, on four workloads (Llama-3-8B dims, random weights, one GPU; generate(max_new = 1) = prefill +
one sampled token, except where noted):

* ``map``: the map prompts of the bench's 10 h transcript (they share the chat header, the system prompt and
  the instruction sentence) -- cache on: one small first batch (the flush rule), then every prompt shares
  the head's full pages;
* ``repeat``: one 8k-token prompt sent twice (a regenerate, a retried chunk);
* ``turn``: an 8k-token prompt, then the same prompt + 200 new tokens (the next turn of a chat);
* ``n4``: four requests with one 4k-token prompt in one call (``n = 4``).

Per run: ``prefill_s`` (the engine's own clock), computed and cached prompt tokens, prefill passes (forward
launches) and the wall time.  One JSON line per run on stdout and appended to ``--out``.

    python tools/bench_prefix.py [--model llama3-8b] [--hours 10] [--out profiles/prefix_cache.jsonl]
"""
import argparse
import asyncio
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def map_prompts(model: str, hours: float, chunk_tokens):
    """Token ids of the map-stage prompts of the bench's synthetic transcript: the pipeline runs against a
    provider that only records its requests, and the local provider's own rendering encodes them."""
    from llm_map_reduce_summarizer_amd.config import LLMConfig
    from llm_map_reduce_summarizer_amd.engine.provider import LocalEngineProvider
    from llm_map_reduce_summarizer_amd.pipeline.executor import LLMExecutor
    from llm_map_reduce_summarizer_amd.pipeline.orchestrator import TranscriptSummarizer
    from llm_map_reduce_summarizer_amd.pipeline.providers import GenResult, Provider
    from llm_map_reduce_summarizer_amd.utils.synth import synthetic_transcript

    seen = []

    class Recorder(Provider):
        name, batched = "recorder", True

        async def generate_batch(self, reqs):
            seen.extend(reqs)
            return [GenResult("summary", 1, 1) for _ in reqs]

        async def generate(self, req):
            return (await self.generate_batch([req]))[0]

    cfg = LLMConfig(MAX_TOKENS=1000, TEMPERATURE=0.3, REDUCE_TEMPERATURE=0.2)
    kw = {"max_tokens_per_chunk": chunk_tokens} if chunk_tokens else {}
    summarizer = TranscriptSummarizer(executor=LLMExecutor(config=cfg, provider_obj=Recorder(model, cfg)), **kw)
    asyncio.run(summarizer.summarize(synthetic_transcript(hours, seed=0)))
    local = LocalEngineProvider(model, cfg, device="cpu")  # (rendering + tokenizer only: no engine is built)
    return [local.encode_request(r) for r in seen if r.stage == "map"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--hours", type=float, default=10.0)
    ap.add_argument("--chunk-tokens", type=int, default=None, help="map chunk size (default: the pipeline's)")
    ap.add_argument("--long", type=int, default=8192, help="tokens of the repeat / turn prompt")
    ap.add_argument("--short", type=int, default=4096, help="tokens of the n = 4 prompt")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--kv-fraction", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join("profiles", "prefix_cache.jsonl"))
    a = ap.parse_args()
    import torch
    from llm_map_reduce_summarizer_amd.engine.config import get_model_config
    from llm_map_reduce_summarizer_amd.engine.engine import LLMEngine, SamplingParams

    maps = map_prompts(a.model, a.hours, a.chunk_tokens)
    cfg = get_model_config(a.model)
    cuda = a.device.startswith("cuda")
    eng = LLMEngine(cfg, device=a.device, max_model_len=16384, max_num_seqs=64, kv_fraction=a.kv_fraction,
                    prefix_cache=True, **({} if cuda else {"kv_pages": 2048}))
    V = cfg.vocab_size
    rnd = lambda n, salt: [128000] + [(salt * 7919 + j * 31) % (V - 300) + 10 for j in range(n - 1)]  # noqa: E731
    p8k, p4k = rnd(a.long, 1), rnd(a.short, 2)
    one = lambda k: [SamplingParams(1, 0.0, i) for i in range(k)]  # noqa: E731
    cases = [("map", [(maps, one(len(maps))), (maps, one(len(maps)))]),
             ("repeat", [([p8k], one(1)), ([p8k], one(1))]),
             ("turn", [([p8k], one(1)), ([p8k + rnd(201, 3)[1:]], one(1))]),
             ("n4", [([p4k] * 4, [SamplingParams(1, 0.8, 100 + i) for i in range(4)])])]

    passes = [0]
    real = eng.model.prefill

    def counted(*args, **kw):
        passes[0] += 1
        return real(*args, **kw)
    eng.model.prefill = counted

    def run(prompts, sp):
        s0, p0 = dict(eng.stats), passes[0]
        if cuda:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = eng.generate(prompts, sp, ignore_eos=True)
        if cuda:
            torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        return {"requests": len(prompts), "prompt_tokens": sum(len(p) for p in prompts),
                "computed_tokens": eng.stats["prefill_tokens"] - s0["prefill_tokens"],
                "cached_tokens": sum(o.cached_tokens for o in outs),
                "prefill_passes": passes[0] - p0, "prefill_s": round(eng.stats["prefill_s"] - s0["prefill_s"], 4),
                "wall_s": round(wall, 4), "first_tokens": [o.token_ids[0] for o in outs][:8]}

    eng.prefix_cache = False
    run(maps, one(len(maps)))  # warm-up: kernel libraries, allocator pools
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for name, calls in cases:
            for cache in (False, True):
                eng.prefix_cache = cache
                eng.kv.alloc.reset()  # every case starts with an empty index
                for k, (prompts, sp) in enumerate(calls):
                    rec = {"case": name, "call": k, "prefix_cache": cache, "model": a.model, "hours": a.hours}
                    rec.update(run(prompts, sp))
                    line = json.dumps(rec)
                    print(line, flush=True)
                    f.write(line + "\n")
    print(json.dumps({"prefix_evictions": eng.kv.alloc.evictions(), "kv_pages": eng.kv.num_pages}), flush=True)


if __name__ == "__main__":
    main()
