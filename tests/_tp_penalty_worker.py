"""Worker for tests/test_sampling_penalties_gpu.py::test_tp2_penalised_generate_one_gpu: a TP=2 engine with
vocab-parallel sampling whose two ranks share ONE GPU (as tests/_tp_worker.py).  A penalised, unfiltered
generate stays vocab-parallel: every rank penalises its own logits shard (both hold the same out_tokens)
inside its own decode graphs; the plain graphs are not touched by it and replay afterwards."""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llm_map_reduce_summarizer_amd.engine.config import get_model_config  # noqa: E402
from llm_map_reduce_summarizer_amd.engine.engine import LLMEngine, SamplingParams  # noqa: E402


def main():
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    torch.cuda.set_device(0)
    cfg = get_model_config("tiny-gqa4", init_std=0.05)
    kw = dict(device="cuda:0", max_model_len=512, max_num_seqs=8, kv_pages=64, seed=7)
    prompts = [[128000] + [t] * n for t, n in ((77, 12), (9000, 20), (31, 9))]
    n = 32
    plain = [SamplingParams(n, 0.0, 100 + i) for i in range(3)]
    pen = [SamplingParams(n, 0.0, 100, presence_penalty=1000.0),
           SamplingParams(n, 0.0, 101, presence_penalty=1000.0),
           SamplingParams(n, 0.7, 102, frequency_penalty=0.5, presence_penalty=1.5, repetition_penalty=1.2)]
    tp = LLMEngine(cfg, tp_rank=rank, tp_size=2, tp_group=None, use_graphs=True, **kw)
    assert tp.model.custom_ar is not None and tp.model.tp_sampling
    p0 = [o.token_ids for o in tp.generate(prompts, plain, ignore_eos=True)]
    captures = tp.stats["graph_captures"]
    assert captures > 0 and tp.stats["penalised_steps"] == 0
    f = [o.token_ids for o in tp.generate(prompts, pen, ignore_eos=True)]
    assert tp.stats["penalised_steps"] > 0 and tp.stats["filtered_steps"] == 0
    pen_captures = tp.stats["graph_captures"] - captures
    assert pen_captures > 0, "a penalised vocab-parallel step runs through its own graphs"
    assert all(len(k) == 4 for k in tp._graphs if k[-1] == "pen")
    for t in f[:2]:
        assert len(t) == n and len(set(t)) == n, "presence 1000, greedy: no token twice"
    assert tp.model.custom_ar.error() == 0
    f2 = [o.token_ids for o in tp.generate(prompts, pen, ignore_eos=True)]
    assert f2 == f and tp.stats["graph_captures"] == captures + pen_captures, "the penalised graphs are re-used"
    p1 = [o.token_ids for o in tp.generate(prompts, plain, ignore_eos=True)]
    assert tp.stats["graph_captures"] == captures + pen_captures, "the plain graphs are replayed, not re-captured"
    assert p1 == p0
    assert tp.model.custom_ar.error() == 0
    allg = [None, None]
    dist.all_gather_object(allg, (p0, f, p1))
    assert allg[0] == allg[1], "ranks disagree"
    dist.barrier()
    print("rank %d tp penalty worker ok" % rank, flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
