"""Frequency / presence / repetition penalties on the GPU: sampler.hip's penalize kernel against
ops/reference.py (apply_penalties is the definition) bit for bit, its composition with the top-k / top-p
filter, and the engine's penalised decode graphs."""

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

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTH = 2048  # out_tokens width: the engine's default max_new_cap
POISON = 100.0  # padding columns between V and the row stride

# one row per case: (rep, freq, pres, done, empty, temperature); values that are no bf16 / no short fp32
ROWS = [
    (1.0, 0.0, 0.0, 0, False, 0.8),     # neutral
    (1.3, 0.5, 0.5, 1, False, 0.8),     # done
    (1.3, 0.5, 0.5, 0, True, 0.8),      # gen_count 0
    (1.0, 0.7, 0.0, 0, False, 0.8),     # freq only
    (1.0, 0.0, 0.6, 0, False, 0.8),     # pres only
    (1.3, 0.0, 0.0, 0, False, 0.8),     # rep only (0.8 on another launch)
    (1.2, -0.3, 0.4, 0, False, 0.8),    # all three, negative freq
    (1.1, 0.45, 0.25, 0, False, 0.0),   # all three on a greedy row
]
B = len(ROWS)
HISTORIES = ["distinct", "one_token", "cycle7", "ends", "congruent", "tail"]
GEN_COUNTS = [1, 7, 64, 65, 2047, 2048]


class _PSt:
    """A decode state with the filter rows (the _FSt of the filter test) and the penalty rows."""

    def __init__(self, out_tokens, gen_count, rep=None, freq=None, pres=None, done=None, temps=None, seeds=None,
                 positions=None, top_k=None, top_p=None):
        n = out_tokens.shape[0]
        i32 = dict(dtype=torch.int32, device=DEV)
        f32 = dict(dtype=torch.float32, device=DEV)
        self.out_tokens = out_tokens.to(DEV)
        self.gen_count = torch.tensor(gen_count, **i32)
        self.rep_pen = torch.tensor(rep if rep is not None else [r[0] for r in ROWS], **f32)
        self.freq_pen = torch.tensor(freq if freq is not None else [r[1] for r in ROWS], **f32)
        self.pres_pen = torch.tensor(pres if pres is not None else [r[2] for r in ROWS], **f32)
        self.done = torch.tensor(done if done is not None else [r[3] for r in ROWS], **i32)
        self.temps = torch.tensor(temps if temps is not None else [r[5] for r in ROWS], **f32)
        self.next_ids = torch.zeros(n, **i32)
        self.positions = torch.tensor(positions if positions is not None else [0] * n, **i32)
        self.max_new = torch.full((n,), WIDTH, **i32)
        self.result = torch.zeros(n, dtype=torch.int64, device=DEV)
        self.seeds = torch.tensor(seeds if seeds is not None else [0] * n, dtype=torch.int64, device=DEV)
        self.eos = torch.tensor([-1, -1, -1, -1], **i32)
        self.top_k = torch.tensor(top_k if top_k is not None else [0] * n, **i32)
        self.top_p = torch.tensor(top_p if top_p is not None else [1.0] * n, **f32)
        self.thresh = torch.full((n,), 12345.0, **f32)

    def reference(self, logits, tok_offset=0):
        """reference.apply_penalties of CPU rows ``logits`` (rewritten and returned) with this state."""
        return reference.apply_penalties(logits, self.out_tokens.cpu(), self.gen_count.cpu(), self.rep_pen.cpu(),
                                         self.freq_pen.cpu(), self.pres_pen.cpu(), self.done.cpu(), tok_offset)


def _history(kind: str, V: int, g: int, seed: int) -> torch.Tensor:
    """One out_tokens row [WIDTH]: ``g`` generated tokens of the given kind, then OTHER valid token ids (of
    a range the history does not use where V allows), which no kernel may read."""
    gen = torch.Generator().manual_seed(seed)
    lo = V // 2  # histories draw from [0, lo) (+ V - 1 for "ends"), the unread tail from [lo, V - 1)
    if kind == "distinct":  # all distinct (as far as the range allows: V = 1000 has fewer ids than steps)
        perm = torch.randperm(lo, generator=gen)
        h = perm[torch.arange(g) % lo]
    elif kind == "one_token":
        h = torch.full((g,), int(torch.randint(0, lo, (1,), generator=gen)))
    elif kind == "cycle7":
        h = torch.randperm(lo, generator=gen)[:7][torch.arange(g) % 7]
    elif kind == "ends":  # tokens 0 and V - 1 present
        h = torch.randint(0, lo, (g,), generator=gen)
        h[0] = 0
        h[1:g:2] = V - 1
    elif kind == "congruent":  # pairwise congruent modulo 1024, 4096 and 8192 where the range holds two such ids
        stride = next(s for s in (8192, 4096, 1024, 128) if lo >= 2 * s)
        r = int(torch.randint(0, stride, (1,), generator=gen))
        n = (lo - 1 - r) // stride + 1
        h = r + stride * (torch.randperm(n, generator=gen)[torch.arange(g) % n])
    elif kind == "tail":  # a few ids, many repeats
        h = torch.randperm(lo, generator=gen)[:50][torch.randint(0, 50, (g,), generator=gen)]
    else:
        raise AssertionError(kind)
    row = torch.randint(lo, V - 1, (WIDTH,), generator=gen)
    row[:g] = h
    return row.to(torch.int32)


def _rows(V: int, scale: float, seed: int, n: int = B) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, V, generator=g) * scale).to(torch.bfloat16)


def _buffer(rows: torch.Tensor, ld: int) -> torch.Tensor:
    """The whole [n, ld] device buffer: ``rows`` in the first V columns, POISON in the padding."""
    n, V = rows.shape
    buf = torch.full((n, ld), POISON, dtype=torch.bfloat16, device=DEV)
    buf[:, :V] = rows.to(DEV)
    return buf


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16).cpu()


@pytest.mark.parametrize("scale", [0.5, 8.0])
@pytest.mark.parametrize("V,ld", [(1000, 1000), (4099, 4104), (128256, 128256)])
def test_kernel_matches_reference_bit_for_bit(V, ld, scale):
    rows = _rows(V, scale, 31 * V + int(scale * 2))
    pristine = _buffer(rows, ld)
    want_pad = torch.full((B, ld - V), POISON, dtype=torch.bfloat16)
    for hi, kind in enumerate(HISTORIES):
        for g in GEN_COUNTS:
            ot = torch.stack([_history(kind, V, g, 1000 * hi + 10 * g + b) for b in range(B)])
            st = _PSt(ot, [0 if r[4] else g for r in ROWS])
            want = torch.cat([st.reference(rows.clone()), want_pad], dim=1)
            buf = pristine.clone()
            hip.penalize(buf[:, :V], st)
            assert torch.equal(_bits(buf), _bits(want)), (kind, g)
            for b in (0, 1, 2):  # neutral, done, empty: untouched
                assert torch.equal(_bits(buf[b]), _bits(pristine[b])), (kind, g, b)
            for b in range(3, B):
                assert not torch.equal(_bits(buf[b]), _bits(pristine[b])), (kind, g, b)
            # a second launch on freshly restored logits: the same bits (no state between launches)
            buf2 = pristine.clone()
            hip.penalize(buf2[:, :V], st)
            assert torch.equal(_bits(buf2), _bits(buf)), (kind, g)
    # rep < 1 on another launch
    ot = torch.stack([_history("tail", V, 65, 77 + b) for b in range(B)])
    st = _PSt(ot, [0 if r[4] else 65 for r in ROWS], rep=[0.8 if r[0] != 1.0 else 1.0 for r in ROWS])
    want = torch.cat([st.reference(rows.clone()), want_pad], dim=1)
    buf = pristine.clone()
    hip.penalize(buf[:, :V], st)
    assert torch.equal(_bits(buf), _bits(want))


def test_scan_form_equals_table_form():
    V = 4099
    rows = _rows(V, 3.0, 5)
    for g in (1, 65, 2048):
        ot = torch.stack([_history("tail", V, g, 300 + g + b) for b in range(B)])
        st = _PSt(ot, [0 if r[4] else g for r in ROWS])
        a, b = _buffer(rows, 4104), _buffer(rows, 4104)
        hip.penalize(a[:, :V], st)
        hip.penalize(b[:, :V], st, form="scan")
        assert torch.equal(_bits(a), _bits(b)), g
        assert torch.equal(_bits(a[:, :V]), _bits(st.reference(rows.clone()))), g


@pytest.mark.parametrize("V", [4096, 128256])
def test_shards_equal_the_whole_row(V):
    rows = _rows(V, 4.0, V + 1)
    for kind, g in (("ends", 64), ("congruent", 2048), ("tail", 2047)):
        ot = torch.stack([_history(kind, V, g, 50 + g + b) for b in range(B)])
        st = _PSt(ot, [0 if r[4] else g for r in ROWS])
        want = st.reference(rows.clone())
        whole = _buffer(rows, V)
        hip.penalize(whole, st)
        halves = _buffer(rows, V)
        hip.penalize(halves[:, :V // 2], st, 0)
        hip.penalize(halves[:, V // 2:], st, V // 2)
        assert torch.equal(_bits(whole), _bits(want)), (kind, g)
        assert torch.equal(_bits(halves), _bits(whole)), (kind, g)
        # each half alone equals the reference on that shard
        lo = rows[:, :V // 2].clone()
        assert torch.equal(_bits(halves[:, :V // 2]), _bits(st.reference(lo, 0))), (kind, g)


# ------------------------------------------------------------------ composition with top-k / top-p
MARGIN = 1e-4  # the top-p decision margin the filter test asks of its rows (fp32 sums + fast exp: ~1e-5)


def _check_sampled(rows, toks, temps, seeds, pos, thresh_ref):
    """Every sampled token is kept (exact) and is the reference's argmax over the kept set, or a near-tie
    within the 1e-3 test_sampler_greedy_and_gumbel allows for the fast log."""
    n, V = rows.shape
    ref = reference.sample_tokens(rows, torch.tensor(temps), torch.tensor(seeds), torch.tensor(pos), thresh_ref)
    for b in range(n):
        row = rows[b].float()
        tok = int(toks[b])
        assert 0 <= tok < V
        assert float(row[tok]) >= float(thresh_ref[b]), (b, tok, float(row[tok]), float(thresh_ref[b]))
        noisy = row.clone()
        if temps[b] > 0:
            noisy = row / temps[b] + reference.gumbel_noise(seeds[b], pos[b], V)
            noisy[row < float(thresh_ref[b])] = float("-inf")
        assert tok == int(ref[b]) or noisy[tok] >= noisy.max() - 1e-3, (b, tok, int(ref[b]))


@pytest.mark.parametrize("V,ld", [(4099, 4104), (128256, 128256)])
def test_penalize_then_filtered_sample(V, ld):
    g = 40
    temps = [0.8, 0.8, 0.8, 1.0, 0.3, 0.7, 1.0, 0.0]
    ks, ps = [0, 40, 0, 40, 5, 0, 1000, 3], [0.9, 1.0, 0.5, 0.5, 0.9, 0.5, 0.9, 0.5]
    seeds, pos = list(range(11, 11 + B)), [0, 5, 17, 300, 4000, 41, 42, 43]
    ot = torch.stack([_history("tail", V, g, 900 + b) for b in range(B)])
    for t in range(16):  # rows whose float64 top-p decision is not within MARGIN of a tie, as FC.pick_rows
        rows = _rows(V, 2.0, 4000 + V + t)
        st = _PSt(ot, [0 if r[4] else g for r in ROWS], temps=temps, seeds=seeds, positions=pos, top_k=ks, top_p=ps)
        pen = st.reference(rows.clone())
        cuts = [reference.nucleus_cut(pen[b], temps[b], ks[b], ps[b]) for b in range(B)]
        if min(m for _, m in cuts) >= MARGIN:
            break
    else:
        raise AssertionError("no seed with a decision margin >= %g" % MARGIN)
    thresh_ref = reference.nucleus_threshold(pen, temps, ks, ps)
    buf = _buffer(rows, ld)
    logits = buf[:, :V]
    hip.penalize(logits, st)
    assert torch.equal(_bits(logits), _bits(pen))
    gc0 = st.gen_count.cpu().tolist()
    hip.sample(logits, st, filtered=True)
    got = st.thresh.cpu()
    print("thresh kernel", got.tolist(), "reference", thresh_ref.tolist())
    want = thresh_ref.clone()
    want[1] = float("-inf")  # the done row is not filtered
    assert torch.equal(got, want)
    live = [b for b in range(B) if not ROWS[b][3]]
    toks = [int(st.out_tokens[b, gc0[b]]) for b in live]
    _check_sampled(pen[live], toks, [temps[b] for b in live], [seeds[b] for b in live], [pos[b] for b in live],
                   thresh_ref[live])
    assert st.gen_count.cpu().tolist() == [c + (0 if ROWS[b][3] else 1) for b, c in enumerate(gc0)]
    assert torch.equal(st.out_tokens[1].cpu(), ot[1])  # done: untouched


# ------------------------------------------------------------------ launcher refusals
def _small_state(n=B):
    ot = torch.stack([_history("tail", 1000, 7, b) for b in range(n)])
    return _PSt(ot, [7] * n, rep=[1.1] * n, freq=[0.1] * n, pres=[0.1] * n, done=[0] * n)


def test_launcher_refusals():
    logits = _buffer(_rows(1000, 1.0, 1), 1000)
    hip.penalize(logits, _small_state())  # the good call
    with pytest.raises(ValueError):
        hip.penalize(logits.float(), _small_state())  # wrong logits dtype
    st = _small_state()
    st.freq_pen = st.freq_pen.double()  # wrong penalty dtype
    with pytest.raises(ValueError):
        hip.penalize(logits, st)
    st = _small_state()
    st.pres_pen = torch.zeros(2 * B, dtype=torch.float32, device=DEV)[::2]  # a non-contiguous penalty row
    with pytest.raises(ValueError):
        hip.penalize(logits, st)
    with pytest.raises(ValueError):
        hip.penalize(logits, _small_state(B - 1))  # a state smaller than the batch
    st = _small_state()
    st.out_tokens = torch.zeros(B, hip.PENALTY_MAX_TOKENS + 1, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):  # more generated tokens per row than the LDS table holds: never truncated
        hip.penalize(logits, st)
    st = _small_state()
    del st.rep_pen
    with pytest.raises(ValueError):
        hip.penalize(logits, st)


# ------------------------------------------------------------------ engine
@pytest.fixture(scope="module")
def eng():
    return LLMEngine(get_model_config("tiny-gqa4", init_std=0.05), device="cuda:0", max_model_len=2048,
                     max_num_seqs=16, kv_pages=256, sync_every=8)


def _prompts():
    return [[128000] + [(i * 37 + j * 11) % 120000 + 5 for j in range(n)] for i, n in enumerate((40, 300, 7, 129))]


# prompts whose plain greedy continuation falls into a loop within a few tokens (36, 12, 27 and 31 distinct
# tokens of 48 on the CPU reference path)
LOOPING = [[128000] + [t] * n for t, n in ((77, 12), (9000, 20), (31, 9), (4242, 15))]
PEN = dict(frequency_penalty=0.5, presence_penalty=1.5, repetition_penalty=1.2)


def _ids(outs):
    return [o.token_ids for o in outs]


def test_engine_penalised_graph_equals_eager(eng):
    sp = [SamplingParams(24, 0.0 if i % 2 else 0.7, 60 + i, **PEN) for i in range(4)]
    before = eng.stats["penalised_steps"]
    a = _ids(eng.generate(LOOPING, sp, ignore_eos=True))
    assert eng.stats["penalised_steps"] > before
    eng.use_graphs = False
    try:
        b = _ids(eng.generate(LOOPING, sp, ignore_eos=True))
    finally:
        eng.use_graphs = True
    assert a == b
    plain = _ids(eng.generate(LOOPING, [SamplingParams(24, 0.0 if i % 2 else 0.7, 60 + i) for i in range(4)],
                              ignore_eos=True))
    assert plain != a  # the penalties change what is sampled


def test_engine_presence_1000_greedy_never_repeats(eng):
    n = 48
    plain = _ids(eng.generate(LOOPING, [SamplingParams(n, 0.0, 0)] * 4, ignore_eos=True))
    assert all(len(t) == n and len(set(t)) < n for t in plain)  # every plain run repeats: not vacuous
    pen = _ids(eng.generate(LOOPING, [SamplingParams(n, 0.0, 0, presence_penalty=1000.0)] * 4, ignore_eos=True))
    assert all(len(t) == n and len(set(t)) == n for t in pen)


def test_engine_mixed_batch_leaves_plain_rows_alone(eng):
    prompts = _prompts()
    plain = [SamplingParams(12, 0.7, 200 + i) for i in range(4)]
    n0 = eng.stats["penalised_steps"]
    base = _ids(eng.generate(prompts, plain))
    assert eng.stats["penalised_steps"] == n0  # an unpenalised run takes no penalised step
    mixed = list(plain)
    mixed[1] = SamplingParams(12, 0.7, 201, **PEN)
    mixed[3] = SamplingParams(12, 0.0, 203, presence_penalty=1000.0)
    got = _ids(eng.generate(prompts, mixed))
    assert eng.stats["penalised_steps"] > n0
    for i in (0, 2):
        assert got[i] == base[i]


def test_engine_rows_retire_and_compact(eng):
    """Different budgets: rows retire one after the other and move_row compacts the batch, the penalty rows
    and the token history with it.  Every sequence matches its solo run (n - 1 of n: the allowance of
    test_engine_gpu.test_order_invariance)."""
    prompts = LOOPING + _prompts()[:2]
    news = [3, 16, 8, 12, 10, 5]
    sp = [SamplingParams(news[i], 0.0 if i % 2 else 0.9, 80 + i, **PEN) for i in range(len(prompts))]
    sp[4] = SamplingParams(news[4], 0.9, 84)  # one plain row in between
    batch = _ids(eng.generate(prompts, sp, ignore_eos=True))
    assert [len(t) for t in batch] == news
    solo = [_ids(eng.generate([p], [s], ignore_eos=True))[0] for p, s in zip(prompts, sp)]
    same = sum(x == y for x, y in zip(batch, solo))
    assert same >= len(prompts) - 1


def test_engine_penalised_graphs_captured_once_per_bucket():
    e = LLMEngine(get_model_config("tiny-gqa4", init_std=0.05), device="cuda:0", max_model_len=1024,
                  max_num_seqs=8, kv_pages=128, sync_every=8)
    prompts = _prompts()
    plain = [SamplingParams(6, 0.7, i) for i in range(4)]
    filt = [SamplingParams(6, 1.5, i, top_k=3) for i in range(4)]
    pen = [SamplingParams(6, 0.7, i, **PEN) for i in range(4)]
    both = [SamplingParams(6, 1.5, i, top_k=3, **PEN) for i in range(4)]
    e.generate(prompts, plain)  # bucket 4, plain
    e.generate(prompts, filt)  # bucket 4, filtered
    c0 = e.stats["graph_captures"]
    keys0 = set(e._graphs)
    assert e.stats["penalised_steps"] == 0
    e.generate(prompts, pen)  # bucket 4, penalised: one more graph
    assert e.stats["graph_captures"] == c0 + 1
    e.generate(prompts, pen)
    e.generate(prompts, plain)
    e.generate(prompts, filt)
    assert e.stats["graph_captures"] == c0 + 1  # all three re-used
    e.generate(prompts, both)  # bucket 4, penalised and filtered
    assert e.stats["graph_captures"] == c0 + 2
    e.generate(prompts[:2], pen[:2])  # bucket 2, penalised
    assert e.stats["graph_captures"] == c0 + 3
    assert keys0 <= set(e._graphs) and all(len(k) in (2, 3) for k in keys0)  # the two older key shapes stay
    assert all(len(k) == 4 for k in set(e._graphs) - keys0)
    keys1 = set(e._graphs)
    e.capture_graphs(2)  # captures the plain graphs only
    assert all(len(k) == 2 for k in set(e._graphs) - keys1)


def test_engine_penalties_with_filters_graph_equals_eager(eng):
    prompts = _prompts()
    kinds = [dict(top_k=2), dict(top_p=0.5), dict(top_k=40, top_p=0.9), dict()]
    sp = [SamplingParams(12, 1.5, 50 + i, **PEN, **kinds[i]) for i in range(4)]
    f0, p0 = eng.stats["filtered_steps"], eng.stats["penalised_steps"]
    a = _ids(eng.generate(prompts, sp))
    assert eng.stats["filtered_steps"] > f0 and eng.stats["penalised_steps"] > p0
    eng.use_graphs = False
    try:
        b = _ids(eng.generate(prompts, sp))
    finally:
        eng.use_graphs = True
    assert a == b


# ------------------------------------------------------------------ TP=2 on one GPU
def test_tp2_penalised_generate_one_gpu():
    """Two processes, one vocab-parallel TP=2 engine (tests/_tp_penalty_worker.py, launched like
    test_sampling_filters_gpu.test_tp2_filtered_generate_one_gpu): a penalised, unfiltered generate runs
    through its own graphs, each rank penalising its own logits shard; the same tokens on both ranks."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "_tp_penalty_worker.py")]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("tp penalty worker ok") == 2, r.stdout[-2000:]
