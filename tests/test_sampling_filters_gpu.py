"""Top-k / top-p sampling on the GPU: the filter kernels of sampler.hip against ops/reference.py
(nucleus_threshold is the definition), the filtered sampler, and the engine's filtered decode graphs."""

import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from llm_map_reduce_summarizer_amd.engine.config import get_model_config  # noqa: E402
from llm_map_reduce_summarizer_amd.engine.engine import LLMEngine, SamplingParams  # noqa: E402
from llm_map_reduce_summarizer_amd.ops import hip, reference  # noqa: E402

import _filter_cases as FC  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _FSt:
    """A decode state with the filter rows (the _St of test_kernels_gpu.py + top_k / top_p / thresh)."""

    def __init__(self, B, temps, seeds, positions, top_k, top_p, max_new=100):
        i32 = dict(dtype=torch.int32, device=DEV)
        self.next_ids = torch.zeros(B, **i32)
        self.positions = torch.tensor(positions, **i32)
        self.gen_count = torch.zeros(B, **i32)
        self.max_new = torch.full((B,), max_new, **i32)
        self.out_tokens = torch.full((B, 8), -1, **i32)
        self.done = torch.zeros(B, **i32)
        self.result = torch.zeros(B, dtype=torch.int64, device=DEV)
        self.temps = torch.tensor(temps, dtype=torch.float32, device=DEV)
        self.seeds = torch.tensor(seeds, dtype=torch.int64, device=DEV)
        self.eos = torch.tensor([-1, -1, -1, -1], **i32)
        self.top_k = torch.tensor(top_k, **i32)
        self.top_p = torch.tensor(top_p, dtype=torch.float32, device=DEV)
        self.thresh = torch.full((B,), 12345.0, dtype=torch.float32, device=DEV)  # poison: every row is written


def _device_rows(rows: torch.Tensor, ld: int) -> torch.Tensor:
    """``rows`` [B, V] on the GPU with row stride ``ld``; the padding holds +100 (larger than any logit:
    a kernel reading past V would move the threshold)."""
    B, V = rows.shape
    buf = torch.full((B, ld), 100.0, dtype=torch.bfloat16, device=DEV)
    buf[:, :V] = rows.to(DEV)
    return buf[:, :V]


def _check_sampled(rows, st, temps, seeds, pos, thresh_ref):
    """Every sampled token is kept (exact) and is the reference's argmax over the kept set, or a near-tie
    within the 1e-3 test_sampler_greedy_and_gumbel allows for the fast log."""
    B, V = rows.shape
    got = st.out_tokens[:, 0].cpu()
    ref = reference.sample_tokens(rows, torch.tensor(temps), torch.tensor(seeds), torch.tensor(pos), thresh_ref)
    for b in range(B):
        row = rows[b].float()
        tok = int(got[b])
        assert 0 <= tok < V
        assert float(row[tok]) >= float(thresh_ref[b]), (b, tok, float(row[tok]), float(thresh_ref[b]))
        noisy = row.clone()
        if temps[b] > 0:
            noisy = row / temps[b] + reference.gumbel_noise(seeds[b], pos[b], V)
            noisy[row < float(thresh_ref[b])] = float("-inf")
        assert tok == int(ref[b]) or noisy[tok] >= noisy.max() - 1e-3, (b, tok, int(ref[b]))


@pytest.mark.parametrize("scale", FC.SCALES)
@pytest.mark.parametrize("V,ld", FC.SHAPES)
def test_threshold_and_sample_match_reference(V, ld, scale):
    rows, thresh_ref, tries = FC.pick_rows(V, scale, base=7000 + V)
    print("seed tries per row:", tries)
    temps = [c[0] for c in FC.CASES]
    ks, ps = [c[1] for c in FC.CASES], [c[2] for c in FC.CASES]
    seeds, pos = [11, 12, 13, 14, 15], [0, 5, 17, 300, 4000]
    logits = _device_rows(rows, ld)
    st = _FSt(5, temps, seeds, pos, ks, ps)
    hip.sample(logits, st, filtered=True)
    got = st.thresh.cpu()
    print("thresh kernel", got.tolist(), "reference", thresh_ref.tolist())
    assert torch.equal(got, thresh_ref)
    _check_sampled(rows, st, temps, seeds, pos, thresh_ref)
    assert st.gen_count.cpu().tolist() == [1] * 5
    assert st.positions.cpu().tolist() == [p + 1 for p in pos]
    assert st.result.abs().sum().item() == 0
    # a second launch on the same workspace: the same thresholds and tokens
    st2 = _FSt(5, temps, seeds, pos, ks, ps)
    hip.sample(logits, st2, filtered=True)
    assert torch.equal(st2.thresh.cpu(), got)
    assert torch.equal(st2.out_tokens.cpu(), st.out_tokens.cpu())
    # the thresholds alone
    st3 = _FSt(5, temps, seeds, pos, ks, ps)
    assert torch.equal(hip.sample_thresholds(logits, st3).cpu(), thresh_ref)


def test_hand_written_rows():
    rows, temps, ks, ps, expect = FC.hand_tensors()
    n = rows.shape[0]
    seeds, pos = list(range(40, 40 + n)), list(range(3, 3 + n))
    logits = _device_rows(rows, FC.V_HAND)
    st = _FSt(n, temps, seeds, pos, ks, ps)
    hip.sample(logits, st, filtered=True)
    got = st.thresh.cpu()
    print("thresh kernel", got.tolist(), "expected", expect.tolist())
    assert torch.equal(got, expect)
    assert torch.equal(reference.nucleus_threshold(rows, temps, ks, ps), expect)
    _check_sampled(rows, st, temps, seeds, pos, expect)
    toks = st.out_tokens[:, 0].cpu().tolist()
    names = [h[0] for h in FC.HAND]
    i = names.index("k1_tie_at_max")
    assert float(rows[i, toks[i]]) == float(rows[i].float().max())  # k = 1: a token at the row max
    # rows without a filter inside a filtered launch: bit-identical to the unfiltered sampler
    plain = _FSt(n, temps, seeds, pos, ks, ps)
    hip.sample(logits, plain)
    for name in ("no_filter", "greedy_zero", "greedy_negative"):
        i = names.index(name)
        assert torch.equal(st.out_tokens[i].cpu(), plain.out_tokens[i].cpu()), name


def test_unfiltered_rows_and_done_rows_in_a_filtered_launch():
    V, ld, B = 4099, 4104, 4
    rows = torch.stack([FC.random_row(V, 2.0, 900 + b) for b in range(B)])
    temps, seeds, pos = [0.8, 0.8, 0.0, 0.8], [1, 2, 3, 4], [9, 10, 11, 12]
    ks, ps = [3, 0, 3, 0], [1.0, 1.0, 0.5, 0.3]
    logits = _device_rows(rows, ld)
    st = _FSt(B, temps, seeds, pos, ks, ps)
    st.done[3] = 1
    hip.sample(logits, st, filtered=True)
    plain = _FSt(B, temps, seeds, pos, ks, ps)
    plain.done[3] = 1
    hip.sample(logits, plain)
    for b in (1, 2):  # no filter / greedy
        assert torch.equal(st.out_tokens[b].cpu(), plain.out_tokens[b].cpu())
        assert float(st.thresh[b]) == float("-inf")
    assert float(rows[0, int(st.out_tokens[0, 0])]) >= float(torch.topk(rows[0].float(), 3).values[-1])
    # the done row is untouched
    assert st.out_tokens[3].cpu().tolist() == [-1] * 8
    assert st.gen_count.cpu().tolist() == [1, 1, 1, 0] and st.positions.cpu().tolist() == [10, 11, 12, 12]
    assert st.result.abs().sum().item() == 0


def test_state_without_filter_fields_is_the_plain_sampler():
    """A state object without top_k / top_p / thresh (test_kernels_gpu._St) samples as ever; asking for the
    filtered path with it is an error, not a silent fall-back."""
    class Bare:
        pass
    full = _FSt(2, [0.5, 0.5], [1, 2], [3, 4], [0, 0], [1.0, 1.0])
    bare = Bare()
    for f in ("next_ids", "positions", "gen_count", "max_new", "out_tokens", "done", "result", "temps", "seeds", "eos"):
        setattr(bare, f, getattr(full, f))
    logits = _device_rows(torch.stack([FC.random_row(1000, 1.0, 5), FC.random_row(1000, 1.0, 6)]), 1000)
    hip.sample(logits, bare)
    assert bare.gen_count.cpu().tolist() == [1, 1]
    with pytest.raises(ValueError):
        hip.sample(logits, bare, filtered=True)


# ------------------------------------------------------------------ engine
@pytest.fixture(scope="module")
def eng():
    return LLMEngine(get_model_config("tiny-gqa4", init_std=0.05), device="cuda:0", max_model_len=2048,
                     max_num_seqs=16, kv_pages=256, sync_every=8)


def _prompts():
    return [[128000] + [(i * 37 + j * 11) % 120000 + 5 for j in range(n)] for i, n in enumerate((40, 300, 7, 129))]


def _filtered_params(n, new=10):
    kinds = [dict(top_k=2), dict(top_p=0.5), dict(top_k=40, top_p=0.9), dict(top_k=1)]
    return [SamplingParams(new, 1.5, 50 + i, **kinds[i % 4]) for i in range(n)]


def test_engine_filtered_graph_equals_eager(eng):
    prompts = _prompts()
    sp = _filtered_params(len(prompts))
    before = eng.stats["filtered_steps"]
    a = eng.generate(prompts, sp)
    assert eng.stats["filtered_steps"] > before
    eng.use_graphs = False
    try:
        b = eng.generate(prompts, sp)
    finally:
        eng.use_graphs = True
    assert [o.token_ids for o in a] == [o.token_ids for o in b]
    # the filter changes what is sampled at this temperature
    plain = eng.generate(prompts, [SamplingParams(10, 1.5, 50 + i) for i in range(len(prompts))])
    assert [o.token_ids for o in plain] != [o.token_ids for o in a]


def test_engine_mixed_batch_leaves_unfiltered_rows_alone(eng):
    prompts = _prompts()
    plain = [SamplingParams(10, 0.7, 200 + i) for i in range(len(prompts))]
    base = eng.generate(prompts, plain)
    mixed = list(plain)
    mixed[1] = SamplingParams(10, 0.7, 201, top_k=3)
    mixed[3] = SamplingParams(10, 0.7, 203, top_p=0.4)
    got = eng.generate(prompts, mixed)
    for i in (0, 2):
        assert got[i].token_ids == base[i].token_ids


def test_engine_filtered_order_invariance(eng):
    prompts = _prompts()
    sp = _filtered_params(len(prompts))
    a = eng.generate(prompts, sp)
    b = eng.generate(prompts[::-1], sp[::-1])[::-1]
    same = sum(x.token_ids == y.token_ids for x, y in zip(a, b))
    assert same >= len(prompts) - 1  # the allowance of test_engine_gpu.test_order_invariance


def test_engine_filtered_graphs_captured_once_per_bucket():
    e = LLMEngine(get_model_config("tiny-gqa4", init_std=0.05), device="cuda:0", max_model_len=1024,
                  max_num_seqs=8, kv_pages=128, sync_every=8)
    prompts = _prompts()
    plain = [SamplingParams(6, 0.7, i) for i in range(4)]
    e.generate(prompts, plain)  # bucket 4, unfiltered
    c0 = e.stats["graph_captures"]
    assert e.stats["filtered_steps"] == 0
    e.generate(prompts, _filtered_params(4, 6))  # bucket 4, filtered: one more graph
    assert e.stats["graph_captures"] == c0 + 1
    e.generate(prompts, _filtered_params(4, 6))
    e.generate(prompts, plain)
    assert e.stats["graph_captures"] == c0 + 1  # both re-used
    e.generate(prompts[:2], _filtered_params(2, 6))  # bucket 2, filtered
    assert e.stats["graph_captures"] == c0 + 2
    with pytest.raises(ValueError):
        e.generate(prompts[:1], [SamplingParams(4, 0.7, 0, top_p=0.0)])


# ------------------------------------------------------------------ TP=2 on one GPU
def test_tp2_filtered_generate_one_gpu():
    """Two processes, one vocab-parallel TP=2 engine (tests/_tp_filter_worker.py, launched like
    test_custom_ar_gpu.test_tp2_engine_one_gpu): a filtered generate gathers the logits and samples eagerly,
    the same tokens on both ranks; the unfiltered graphs are untouched by it and still replay."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "_tp_filter_worker.py")]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("tp filter worker ok") == 2, r.stdout[-2000:]
