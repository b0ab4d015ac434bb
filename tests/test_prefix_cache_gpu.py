"""KV prefix caching on the GPU.  No new kernel: the feature is the paged prefill kernel with a non-zero prefix
on a sequence's FIRST slice and block-table rows that name the same physical page.  Checked here: the kernel
on the counting probes through aliased rows (exact), the engine's warm call against a cache-off engine with
exact token counts, that a shared page is never written again (bit-equal snapshots across a warm call that
decodes over a page boundary), chunked prompts and feeder joiners, and decode graphs against eager steps."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import _probes as pr  # noqa: E402
from llm_map_reduce_summarizer_amd.engine.config import get_model_config  # noqa: E402
from llm_map_reduce_summarizer_amd.engine.engine import LLMEngine, SamplingParams  # noqa: E402
from llm_map_reduce_summarizer_amd.ops import hip  # noqa: E402

DEV = "cuda:0"
P = 64
SC = 1.0 / math.sqrt(pr.D)
CFG = get_model_config("tiny-gqa4", init_std=0.05)


# ------------------------------------------------------------------ kernel, exact
def aliased_prefill_probe(spans, shared, hq, hkv, fmt, seed=0):
    """``_probes.paged_prefill_probe`` with aliased block-table rows: sequence 0 (the owner) keeps its pages,
    and the first ``shared[i]`` entries of sequence i's row name the owner's pages of the same positions.  The
    pages sequence i had there are no valid keys any more: they take the scratch page's poison.  The expected
    counts do not change -- the owner's pages hold the keys of the same positions."""
    g = torch.Generator().manual_seed(seed)
    pre = torch.tensor([b for b, _ in spans]).long()
    end = torch.tensor([e for _, e in spans]).long()
    n = end - pre
    nseq = len(spans)
    slots = torch.randperm(nseq, generator=g)
    lens = torch.zeros(nseq, dtype=torch.long)
    lens[slots] = end  # block-table row slots[i] holds sequence i
    kc, vc, bt = pr.paged_cache(lens, hkv, fmt, nseq, g)
    owner = int(slots[0])
    for i in range(1, nseq):
        k, row = shared[i], int(slots[i])
        assert k * P <= min(int(end[0]), int(end[i])) and k * P <= int(pre[i])  # full pages both hold, before the slice
        orphans = bt[row, :k].long()
        kc[orphans], vc[orphans] = kc[0].clone(), vc[0].clone()
        bt[row, :k] = bt[owner, :k]
    T = int(n.sum())
    cu = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(n, 0)])
    absolute = torch.arange(T) - torch.repeat_interleave(cu[:-1], n) + torch.repeat_interleave(pre, n)
    qkv = torch.zeros(T, (hq + 2 * hkv) * pr.D)
    qkv[:, : hq * pr.D] = pr.rand_q((T, hq * pr.D), g)
    qkv[:, (hq + hkv) * pr.D:] = pr.onehot_v(absolute)[:, None, :].expand(T, hkv, pr.D).reshape(T, hkv * pr.D)
    return pr.Probe(qkv=qkv.to(torch.bfloat16), cu_seqlens=cu.to(torch.int32), seqlens=[int(x) for x in n],
                    kcache=kc, vcache=vc, block_tables=bt, seq_slot=slots.to(torch.int32),
                    prefix=pre.to(torch.int32), slot_host=[int(x) for x in slots],
                    prefix_host=[int(x) for x in pre], absolute=absolute, expect=pr.expect_prefix(absolute + 1),
                    T=T, hq=hq, hkv=hkv, fmt=fmt)


@pytest.mark.parametrize("hq,hkv", [(8, 2), (6, 2)])
@pytest.mark.parametrize("fmt", ["bf16", "fp8v"])
def test_paged_prefill_reads_through_aliased_rows(hq, hkv, fmt):
    """An owner covers (0, 200); (192, 300) reads its first three pages, (128, 129) its first two, through the
    owner's physical pages."""
    spans, shared = [(0, 200), (192, 300), (128, 129)], [0, 3, 2]
    p = aliased_prefill_probe(spans, shared, hq, hkv, fmt)
    bt = p.block_tables
    rows = p.slot_host
    assert torch.equal(bt[rows[1], :3], bt[rows[0], :3]) and torch.equal(bt[rows[2], :2], bt[rows[0], :2])
    assert bt[rows[1], 3] != bt[rows[0], 3]
    p = p.to(DEV)
    out = hip.attn_prefill(p.qkv, p.cu_seqlens, hq, hkv, pr.D, SC, paged=pr.paged_args(p))
    pr.check_counts(out, p.expect)


# ------------------------------------------------------------------ engine
def _engine(cache, **kw):
    args = dict(device=DEV, max_model_len=2048, max_num_seqs=16, kv_pages=256, sync_every=8)
    args.update(kw)
    return LLMEngine(CFG, prefix_cache=cache, **args)


def _prompt(n, salt):
    return [128000] + [(salt * 53 + j * 7) % 120000 + 5 for j in range(n - 1)]


def _greedy(n, k=8):
    return [SamplingParams(k, 0.0, 0)] * n


def _ids(outs):
    return [o.token_ids for o in outs]


def _same(a, b):
    return sum(x == y for x, y in zip(_ids(a), _ids(b)))


LENS = (1500, 300, 129, 128, 65, 64, 40)


def test_warm_call_equals_cache_off():
    prompts = [_prompt(n, i) for i, n in enumerate(LENS)]
    ref = _engine(False).generate(prompts, _greedy(len(prompts)))
    on = _engine(True)
    cold = on.generate(prompts, _greedy(len(prompts)))
    assert [o.cached_tokens for o in cold] == [0] * len(LENS) and on.stats["prefill_tokens"] == sum(LENS)
    warm = on.generate(prompts, _greedy(len(prompts)))
    want = [P * ((n - 1) // P) for n in LENS]
    assert [o.cached_tokens for o in warm] == want
    assert on.stats["prefill_tokens"] == 2 * sum(LENS) - sum(want)
    assert on.stats["prefix_hit_tokens"] == sum(want)
    assert on.kv.alloc.available() == on.kv.num_pages - 1
    assert _same(cold, ref) >= len(prompts) - 1  # a bf16 near-tie may flip one sequence
    assert _same(warm, ref) >= len(prompts) - 1, (_ids(warm), _ids(ref))


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8v"])
def test_shared_pages_are_never_written(kv_dtype):
    on = _engine(True, kv_dtype=kv_dtype)
    lens = (130, 300, 700)
    prompts = [_prompt(n, 10 + i) for i, n in enumerate(lens)]
    owners = {}
    on.generate(prompts, _greedy(3, 4), on_prefill=lambda seqs: owners.update({s.rid: list(s.pages) for s in seqs}))
    cached = sorted(pg for rid, n in enumerate(lens) for pg in owners[rid][:n // P])
    assert len(cached) == sum(n // P for n in lens) == on.kv.alloc.cached()
    idx = torch.tensor(cached, device=DEV)
    snap_k, snap_v = on.kv.k[:, idx].clone(), on.kv.v[:, idx].clone()  # every layer
    rows = {}
    # 70 decoded tokens: every sequence writes past a page boundary ((130, 300, 700) + 70 cross 192, 320, 768)
    warm = on.generate(prompts, _greedy(3, 70), on_prefill=lambda seqs: rows.update({s.rid: list(s.pages) for s in seqs}))
    assert [len(o.token_ids) for o in warm] == [70] * 3
    for rid, n in enumerate(lens):
        k = (n - 1) // P
        assert warm[rid].cached_tokens == P * k and rows[rid][:k] == owners[rid][:k]  # the owners' page ids
        assert not set(rows[rid][k:]) & set(cached)
    assert torch.equal(on.kv.k[:, idx], snap_k) and torch.equal(on.kv.v[:, idx], snap_v)  # bit-equal
    # and they still serve: a third call decodes what the second did
    again = on.generate(prompts, _greedy(3, 70))
    assert _same(again, warm) >= 2
    assert torch.equal(on.kv.k[:, idx], snap_k) and torch.equal(on.kv.v[:, idx], snap_v)


def test_chunked_prompts_and_follow_up_turns():
    lens = (2600, 1500, 700, 90)
    prompts = [_prompt(n, 20 + i) for i, n in enumerate(lens)]
    kw = dict(max_model_len=4096, max_num_seqs=8, prefill_chunk=512)
    off, on = _engine(False, **kw), _engine(True, **kw)
    first_ref = off.generate(prompts, _greedy(4))
    first = on.generate(prompts, _greedy(4))
    assert _same(first, first_ref) >= 3
    assert on.stats["prefill_slices"] == sum(-(-n // 512) for n in lens)
    turns = [p + o.token_ids + _prompt(50, 40 + i)[1:] for i, (p, o) in enumerate(zip(prompts, first_ref))]
    ref = off.generate(turns, _greedy(4))
    got = on.generate(turns, _greedy(4))
    assert [o.cached_tokens for o in got] == [P * (n // P) for n in lens]  # every full page of the first prompts
    assert on.stats["prefill_tokens"] == sum(lens) + sum(len(t) - o.cached_tokens for t, o in zip(turns, got))
    assert _same(got, ref) >= 3, (_ids(got), _ids(ref))


def test_feeder_joiners_hit_the_cache():
    running = [_prompt(40 + 9 * i, i) for i in range(3)]
    heads = [_prompt(n, 60 + i) for i, n in enumerate((400, 900))]
    joiners = [heads[0] + _prompt(200, 70)[1:], heads[1] + _prompt(300, 71)[1:], _prompt(500, 72)]

    def run(eng):
        fed = []

        def feeder(done):
            if not fed:
                fed.append(1)
                return [(j, SamplingParams(8, 0.0, 0)) for j in joiners]
            return []
        return eng.generate(running, _greedy(3, 40), feeder=feeder)

    kw = dict(prefill_chunk=256)
    ref = run(_engine(False, **kw))
    on = _engine(True, **kw)
    on.generate(heads, _greedy(2, 2))
    before = on.stats["prefill_tokens"]
    got = run(on)
    assert on.stats["interleaved_prefills"] == 3
    assert [o.cached_tokens for o in got[3:]] == [P * (400 // P), P * (900 // P), 0]
    new = sum(len(p) for p in running) + sum(len(j) for j in joiners) - P * (400 // P) - P * (900 // P)
    assert on.stats["prefill_tokens"] - before == new
    assert _same(got, ref) >= len(got) - 1, (_ids(got), _ids(ref))
    assert on.kv.alloc.available() == on.kv.num_pages - 1


def test_warm_tokens_with_graphs_equal_eager():
    prompts = [_prompt(n, 80 + i) for i, n in enumerate((40, 300, 7, 129))]
    sp = [SamplingParams(10, 0.3, 5 + i) for i in range(len(prompts))]
    on = _engine(True)
    assert on.use_graphs
    on.generate(prompts, sp)
    a = on.generate(prompts, sp)
    on.use_graphs = False
    b = on.generate(prompts, sp)
    assert [o.cached_tokens for o in a] == [o.cached_tokens for o in b] == [0, 256, 0, 128]
    assert _ids(a) == _ids(b)
