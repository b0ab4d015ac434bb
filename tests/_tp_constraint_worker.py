"""Worker for tests/test_sampling_constraints_gpu.py::test_tp2_constrained_generate_one_gpu: a TP=2 engine with
vocab-parallel sampling whose two ranks share ONE GPU (as tests/_tp_penalty_worker.py).  A constrained,
unfiltered generate stays vocab-parallel: every rank constrains its own logits shard (both hold the same
bias rows and stop ids) inside its own decode graphs and runs the same finish after the key max-reduce; the
plain graphs are not touched by it and replay afterwards."""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llm_map_reduce_summarizer_amd.engine.config import get_model_config  # noqa: E402
from llm_map_reduce_summarizer_amd.engine.engine import LLMEngine, SamplingParams  # noqa: E402

NINF = float("-inf")


def main():
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    torch.cuda.set_device(0)
    cfg = get_model_config("tiny-gqa4", init_std=0.05)
    kw = dict(device="cuda:0", max_model_len=512, max_num_seqs=8, kv_pages=64, seed=7)
    prompts = [[128000] + [t] * n for t, n in ((77, 12), (9000, 20), (31, 9))]
    n = 24
    half = cfg.vocab_size // 2
    lo, hi, lo2 = 1234, half + 4321, 77  # tokens of rank 0's shard, of rank 1's, of rank 0's
    plain = [SamplingParams(n, 0.0, 100 + i) for i in range(3)]
    tp = LLMEngine(cfg, tp_rank=rank, tp_size=2, tp_group=None, use_graphs=True, **kw)
    assert tp.model.custom_ar is not None and tp.model.tp_sampling
    p0 = [o.token_ids for o in tp.generate(prompts, plain, ignore_eos=True)]
    captures = tp.stats["graph_captures"]
    assert captures > 0 and tp.stats["constrained_steps"] == 0

    def run(bias, **more):
        sp = [SamplingParams(n, 0.0, 100 + i, logit_bias=bias, **more) for i in range(3)]
        return [o.token_ids for o in tp.generate(prompts, sp, ignore_eos=not more)]

    # greedy: +100 wins, in either shard; a ban in either shard hands the win to the runner-up in the other
    a = run({lo: 100.0, hi: 60.0, lo2: 20.0})
    assert a == [[lo] * n] * 3, "the bias in rank 0's shard wins"
    assert tp.stats["constrained_steps"] > 0 and tp.stats["filtered_steps"] == 0
    con_captures = tp.stats["graph_captures"] - captures
    assert con_captures > 0, "a constrained vocab-parallel step runs through its own graphs"
    assert all(len(k) == 5 for k in tp._graphs if k[-1] == "con") and any(k[-1] == "con" for k in tp._graphs)
    b = run({lo: NINF, hi: 60.0, lo2: 20.0})
    assert b == [[hi] * n] * 3, "the ban in rank 0's shard is honoured, rank 1's token wins"
    c = run({lo: NINF, hi: NINF, lo2: 20.0})
    assert c == [[lo2] * n] * 3, "the ban in rank 1's shard is honoured too"
    banned = {t for seq in p0 for t in seq}
    d = run({t: NINF for t in banned})
    assert all(len(seq) == n and not set(seq) & banned for seq in d), "the plain run's tokens are all banned"
    assert tp.stats["graph_captures"] == captures + con_captures, "the constrained graphs are re-used"
    assert tp.model.custom_ar.error() == 0
    # the row's own stop id in rank 1's shard, held back by min_tokens: the same finish on every rank
    e = run({hi: 100.0}, stop_token_ids=[hi], min_tokens=5)
    assert all(len(seq) == 6 and hi not in seq[:5] and seq[5] == hi for seq in e), e
    assert tp.stats["filtered_steps"] == 0 and tp.model.custom_ar.error() == 0
    captures2 = tp.stats["graph_captures"]
    p1 = [o.token_ids for o in tp.generate(prompts, plain, ignore_eos=True)]
    assert tp.stats["graph_captures"] == captures2, "the plain graphs are replayed, not re-captured"
    assert p1 == p0
    assert tp.model.custom_ar.error() == 0
    allg = [None, None]
    dist.all_gather_object(allg, (p0, a, b, c, d, e, p1))
    assert allg[0] == allg[1], "ranks disagree"
    dist.barrier()
    print("rank %d tp constraint worker ok" % rank, flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
