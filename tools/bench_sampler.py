#!/usr/bin/env python3
"""Cost of the sampler launch (ops.hip.sample) without and with the top-k / top-p filter, at decode batch
sizes over the real vocabulary.

Every timed launch is preceded by a rewrite of the logits (a device copy from one of several source
buffers), as the LM head rewrites them before every decode step: the histogram kernel then does not read
rows that an earlier iteration of this loop left in cache.  Device events time N x (rewrite + sample) and
N x (rewrite) back to back; the difference / N is the sampler's cost.  Modes: ``plain`` (the unfiltered
launch), ``all`` (every row top_k=40 top_p=0.9), ``one`` (row 0 filtered, the others not: they exit the
filter kernels at once), ``thresh`` (the two filter kernels alone, every row filtered).

    python tools/bench_sampler.py --bs 1,10,39 > profiles/sampler_filter.jsonl

``--penalties``: the cost of the penalize launch (ops.hip.penalize, which a penalised decode step runs
before the sampler) instead, timed the same way, for every row penalised with ``gen_count`` generated
tokens (half as many distinct ids), in both forms of the kernel's token reduction -- ``table`` (the LDS
open-addressing table the engine runs) and ``scan`` (the ownership scan).

    python tools/bench_sampler.py --penalties --bs 1,10,39 > profiles/sampler_penalties.jsonl

``--constraints``: the cost of the constrain launch (ops.hip.constrain, which a constrained decode step runs
before the penalties and the sampler), timed the same way, for every row carrying ``entries`` logit-bias
entries (a quarter of them bans) and a minimum length that suppresses its armed stop ids; ``neutral`` is the
same launch over rows with nothing to do (every workgroup exits at once).

    python tools/bench_sampler.py --constraints --bs 1,10,39 > profiles/sampler_constraints.jsonl

``--logprobs``: the cost of the two launches a logprob decode step adds -- ops.hip.logprobs (segments + merge)
before the sampler and ops.hip.logprobs_pick after it -- for every row asking with a top list of ``n`` entries,
next to the plain sampler launch timed in the same run: ``logprobs_us`` = (rewrite + logprobs) - rewrite,
``plain_us`` = (rewrite + sample) - rewrite, ``pick_us`` = (rewrite + sample + pick) - (rewrite + sample),
``off_us`` = the logprobs launch over rows that do not ask (every workgroup exits at once).

    python tools/bench_sampler.py --logprobs --bs 1,10,39 > profiles/sampler_logprobs.jsonl
"""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--bs", default="1,10,39")
ap.add_argument("--vocab", type=int, default=128256)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--temperature", type=float, default=0.3)
ap.add_argument("--scale", type=float, default=3.0, help="std of the random logits")
ap.add_argument("--penalties", action="store_true", help="time the penalize launch instead of the filter")
ap.add_argument("--gen-counts", default="1,256,2048", help="--penalties: generated tokens per row")
ap.add_argument("--constraints", action="store_true", help="time the constrain launch instead of the filter")
ap.add_argument("--entries", default="1,300", help="--constraints: logit-bias entries per row")
ap.add_argument("--logprobs", action="store_true", help="time the logprobs launches instead of the filter")
ap.add_argument("--top-ns", default="0,5,20", help="--logprobs: top-list entries per row")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import torch  # noqa: E402

from llm_map_reduce_summarizer_amd.ops import hip  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("bench_sampler needs a GPU")
dev = "cuda:0"
NSRC = 4


class State:
    def __init__(self, B, cap, top_k, top_p):
        i32 = dict(dtype=torch.int32, device=dev)
        self.next_ids = torch.zeros(B, **i32)
        self.positions = torch.zeros(B, **i32)
        self.gen_count = torch.zeros(B, **i32)
        self.max_new = torch.full((B,), cap, **i32)
        self.out_tokens = torch.zeros(B, cap, **i32)
        self.done = torch.zeros(B, **i32)
        self.result = torch.zeros(B, dtype=torch.int64, device=dev)
        self.temps = torch.full((B,), args.temperature, dtype=torch.float32, device=dev)
        self.seeds = torch.arange(B, dtype=torch.int64, device=dev)
        self.eos = torch.full((4,), -1, **i32)
        self.top_k = torch.tensor(top_k, **i32)
        self.top_p = torch.tensor(top_p, dtype=torch.float32, device=dev)
        self.thresh = torch.zeros(B, dtype=torch.float32, device=dev)


def timed(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(n):
        fn(i)
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / n  # us per iteration


for B in (int(b) for b in args.bs.split(",")):
    g = torch.Generator(device="cpu").manual_seed(B)
    srcs = [(torch.randn(B, args.vocab, generator=g) * args.scale).to(torch.bfloat16).to(dev) for _ in range(NSRC)]
    logits = torch.empty_like(srcs[0])
    cap = (args.repeats + 1) * args.iters + 8
    modes = {
        "plain": ([0] * B, [1.0] * B),
        "all": ([40] * B, [0.9] * B),
        "one": ([40] + [0] * (B - 1), [0.9] + [1.0] * (B - 1)),
        "thresh": ([40] * B, [0.9] * B),
    }

    def rewrite(i):
        logits.copy_(srcs[i % NSRC])

    if args.penalties:
        for gc in (int(x) for x in args.gen_counts.split(",")):
            st = State(B, max(gc, 2048), [0] * B, [1.0] * B)
            pool = torch.randint(0, args.vocab, (B, max(1, gc // 2)), generator=g)
            st.out_tokens[:, :gc] = torch.gather(pool, 1, torch.randint(0, pool.shape[1], (B, gc), generator=g)).to(dev)
            st.gen_count.fill_(gc)
            st.rep_pen = torch.full((B,), 1.2, dtype=torch.float32, device=dev)
            st.freq_pen = torch.full((B,), 0.5, dtype=torch.float32, device=dev)
            st.pres_pen = torch.full((B,), 0.5, dtype=torch.float32, device=dev)
            rec = {"B": B, "V": args.vocab, "gen_count": gc, "iters": args.iters, "repeats": args.repeats}
            for form in ("table", "scan"):
                def step(i, st=st, form=form):
                    rewrite(i)
                    hip.penalize(logits, st, form=form)

                timed(step, args.iters)
                d = [timed(step, args.iters) - timed(rewrite, args.iters) for _ in range(args.repeats)]
                rec["penalize_%s_us" % form] = round(statistics.median(d), 2)
                rec["penalize_%s_us_min_max" % form] = [round(min(d), 2), round(max(d), 2)]
            print(json.dumps(rec), flush=True)
        continue

    if args.constraints:
        for n in (int(x) for x in args.entries.split(",")):
            st = State(B, 8, [0] * B, [1.0] * B)
            st.eos = torch.tensor([128001, 128009, -1, -1], dtype=torch.int32, device=dev) % args.vocab
            st.bias_tok = torch.stack([torch.randperm(args.vocab, generator=g)[:300] for _ in range(B)]).to(
                torch.int32).to(dev)
            vals = torch.rand(B, 300, generator=g) * 200.0 - 100.0
            vals[torch.rand(B, 300, generator=g) < 0.25] = float("-inf")
            st.bias_val = vals.to(dev)
            st.stop_ids = torch.randint(0, args.vocab, (B, 4), generator=g).to(torch.int32).to(dev)
            rec = {"B": B, "V": args.vocab, "entries": n, "iters": args.iters, "repeats": args.repeats}
            for mode, (bn, mn) in (("constrain", (n, 1)), ("neutral", (0, 0))):
                st.bias_n = torch.full((B,), bn, dtype=torch.int32, device=dev)
                st.min_new = torch.full((B,), mn, dtype=torch.int32, device=dev)  # gen_count is 0

                def step(i, st=st):
                    rewrite(i)
                    hip.constrain(logits, st)

                timed(step, args.iters)
                d = [timed(step, args.iters) - timed(rewrite, args.iters) for _ in range(args.repeats)]
                rec["%s_us" % mode] = round(statistics.median(d), 2)
                rec["%s_us_min_max" % mode] = [round(min(d), 2), round(max(d), 2)]
            print(json.dumps(rec), flush=True)
        continue

    if args.logprobs:
        from llm_map_reduce_summarizer_amd import ops
        for n in (int(x) for x in args.top_ns.split(",")):
            st = State(B, args.iters + 8, [0] * B, [1.0] * B)
            st.lp = ops.LogprobStore(B, args.iters + 8, dev)
            rec = {"B": B, "V": args.vocab, "top_n": n, "iters": args.iters, "repeats": args.repeats}

            def lp_only(i, st=st):
                rewrite(i)
                hip.logprobs(logits, st)

            def sample_only(i, st=st):
                rewrite(i)
                hip.sample(logits, st)

            def sample_pick(i, st=st):
                rewrite(i)
                hip.sample(logits, st)
                hip.logprobs_pick(logits, st)

            def loop(fn, st=st):
                st.gen_count.zero_()  # the sampler advances it: every timed loop starts at record 0
                st.done.zero_()
                return timed(fn, args.iters)

            for mode, lp_n in (("logprobs", n), ("off", -1)):
                st.lp_n = torch.full((B,), lp_n, dtype=torch.int32, device=dev)
                loop(lp_only)
                d = [loop(lp_only) - timed(rewrite, args.iters) for _ in range(args.repeats)]
                rec["%s_us" % mode] = round(statistics.median(d), 2)
                rec["%s_us_min_max" % mode] = [round(min(d), 2), round(max(d), 2)]
            st.lp_n = torch.full((B,), n, dtype=torch.int32, device=dev)
            loop(lp_only)  # a slot for the pick (lp_slot 0: the sampler's first record of every loop)
            loop(sample_pick)
            plain, pick = [], []
            for _ in range(args.repeats):
                a, b, c = loop(sample_pick), loop(sample_only), timed(rewrite, args.iters)
                plain.append(b - c)
                pick.append(a - b)
            for name, d in (("plain", plain), ("pick", pick)):
                rec["%s_us" % name] = round(statistics.median(d), 2)
                rec["%s_us_min_max" % name] = [round(min(d), 2), round(max(d), 2)]
            print(json.dumps(rec), flush=True)
        continue

    res = {}
    for mode, (ks, ps) in modes.items():
        st = State(B, cap, ks, ps)

        def step(i, st=st, mode=mode):
            rewrite(i)
            if mode == "thresh":
                hip.sample_thresholds(logits, st)
            else:
                hip.sample(logits, st, filtered=mode != "plain")

        timed(step, args.iters)  # warm-up (code objects, the filter workspace)
        # alternate the two loops so a clock or neighbour change hits both
        d = []
        for _ in range(args.repeats):
            d.append(timed(step, args.iters) - timed(rewrite, args.iters))
        res[mode] = d
        if mode != "thresh":
            assert int(st.gen_count.min()) == (args.repeats + 1) * args.iters
    rec = {"B": B, "V": args.vocab, "temperature": args.temperature, "iters": args.iters, "repeats": args.repeats}
    for mode, d in res.items():
        rec[mode + "_us"] = round(statistics.median(d), 2)
        rec[mode + "_us_min_max"] = [round(min(d), 2), round(max(d), 2)]
    rec["filter_extra_us"] = round(rec["all_us"] - rec["plain_us"], 2)
    print(json.dumps(rec), flush=True)
