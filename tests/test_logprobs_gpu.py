"""Token log-probabilities on the GPU: sampler.hip's logprobs kernels (segments, merge, pick) against
ops/reference.py token_logprobs -- the top lists exactly, the values within a derived tolerance, -inf exactly,
batch invariance bit for bit -- and the engine's logprob decode graphs."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from llm_map_reduce_summarizer_amd import ops  # noqa: E402
from llm_map_reduce_summarizer_amd.engine.config import get_model_config  # noqa: E402
from llm_map_reduce_summarizer_amd.engine.engine import LLMEngine, SamplingParams  # noqa: E402
from llm_map_reduce_summarizer_amd.ops import hip, reference  # noqa: E402

from _logprob_cases import NINF, SampleTap, check_records, close  # noqa: E402

DEV = "cuda:0"
POISON = 100.0  # padding columns between V and the row stride
P_LP, P_TOK = 777.0, -7  # what an untouched record holds
CAP = 6  # record width of the kernel tests
LP_N = [20, -1, 0, 1, 5]  # per row, cycling
GEN = [0, CAP // 2, CAP - 1, CAP]  # per row, cycling: first, middle and last record, and one past the width
EQUAL_ROW = 0  # an all-equal row (B >= 3): lp_n 20, step 0


def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous().reshape(-1) if t.dim() == 0 else t.contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


def _rows(B, V, scale, seed):
    g = torch.Generator().manual_seed(seed)
    rows = (torch.randn(B, V, generator=g) * scale).to(torch.bfloat16)
    rows[:, 3], rows[:, 4], rows[:, 6] = NINF, -0.0, 0.0  # a ban; -0 before +0: equal values, the lower id first
    top = rows.float().max(dim=1).values + 1.0
    rows[:, V - 1], rows[:, 5] = top.to(torch.bfloat16), top.to(torch.bfloat16)  # a tie at the top, last column
    rows[:, 1] = rows[:, 7]  # ... and one further down
    if B >= 3:
        rows[EQUAL_ROW] = 1.5
    return rows


def _buffer(rows, ld):
    n, V = rows.shape
    buf = torch.full((n, ld), POISON, dtype=torch.bfloat16, device=DEV)
    buf[:, :V] = rows.to(DEV)
    return buf


class _LSt:
    """The rows of a decode state the logprobs ops read, and a poison-filled record store."""

    def __init__(self, B, lp_n=None, gen=None, done=None, cap=CAP):
        i32 = dict(dtype=torch.int32, device=DEV)
        self.lp_n = torch.tensor(lp_n if lp_n is not None else [LP_N[b % 5] for b in range(B)], **i32)
        self.gen_count = torch.tensor(gen if gen is not None else [GEN[b % 4] for b in range(B)], **i32)
        self.done = torch.tensor(done if done is not None else [int(b % 7 == 3) for b in range(B)], **i32)
        self.out_tokens = torch.full((B, cap), -3, **i32)
        self.lp = ops.LogprobStore(B, cap, DEV).ensure()
        self.lp.out_logprobs.fill_(P_LP)
        self.lp.out_top_lp.fill_(P_LP)
        self.lp.out_top_tok.fill_(P_TOK)
        self.lp.lp_slot.fill_(55)

    def live(self, b):
        return int(self.lp_n[b]) >= 0 and not int(self.done[b]) and int(self.gen_count[b]) < self.lp.cap


def _run(buf, V, st, picks):
    """logprobs, the token ``picks[b]`` appended at the row's step as the finish would, logprobs_pick."""
    logits = buf[:, :V]
    hip.logprobs(logits, st)
    slot = st.lp.lp_slot.cpu().tolist()
    for b, g in enumerate(slot):
        if g >= 0:
            st.out_tokens[b, g] = picks[b]
    hip.logprobs_pick(logits, st)
    torch.cuda.synchronize()
    return slot


WORST = {}


@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("V,ld", [(8, 8), (1007, 1016), (128256, 128264)])
def test_kernels_match_the_reference(V, ld, B, scale):
    rows = _rows(B, V, scale, 17 * V + B)
    buf = _buffer(rows, ld)
    pristine = buf.clone()
    st = _LSt(B)
    ns = [max(int(n), 0) for n in st.lp_n.tolist()]
    ref_lp, ref_top = reference.token_logprobs(rows, ns)
    # the appended token: the most likely one, the banned column, the -0 column, a tied one, any other
    picks = [[int(rows[b].float().argmax()), 3, 4, 7, (31 * b + 2) % V][(b + b // 5) % 5] for b in range(B)]
    slot = _run(buf, V, st, picks)
    assert torch.equal(_bits(buf), _bits(pristine))  # the logits are only read, padding included
    out_lp, top_tok, top_lp = st.lp.out_logprobs.cpu(), st.lp.out_top_tok.cpu(), st.lp.out_top_lp.cpu()
    worst, seen_live = 0.0, 0
    for b in range(B):
        g, n = int(st.gen_count[b]), ns[b]
        if not st.live(b):
            assert slot[b] == -1, b
            assert (out_lp[b] == P_LP).all() and (top_tok[b] == P_TOK).all() and (top_lp[b] == P_LP).all(), b
            continue
        seen_live += 1
        assert slot[b] == g, b
        keep = torch.ones(CAP, dtype=torch.bool)
        keep[g] = False  # the other steps' records, and the entries past the row's list, keep the poison
        assert (out_lp[b][keep] == P_LP).all() and (top_tok[b][keep] == P_TOK).all() and (top_lp[b][keep] == P_LP).all()
        assert (top_tok[b, g, n:] == P_TOK).all() and (top_lp[b, g, n:] == P_LP).all(), b
        want = ref_top[b]
        assert len(want) == min(n, V)
        assert top_tok[b, g, :n].tolist() == [t for t, _ in want] + [-1] * (n - len(want)), (b, n)
        assert all(x == NINF for x in top_lp[b, g, len(want):n].tolist())
        got = [(float(a), x) for a, (_, x) in zip(top_lp[b, g, :n].tolist(), want)]
        got.append((float(out_lp[b, g]), float(ref_lp[b, picks[b]])))
        for a, x in got:
            assert close(a, x), (b, a, x)
            if math.isfinite(x):
                worst = max(worst, abs(a - x))
        for i, (t, _) in enumerate(want):  # the picked value IS the list's entry of the same token
            if t == picks[b]:
                assert torch.equal(_bits(out_lp[b, g]), _bits(top_lp[b, g, i])), (b, t)
        if b == EQUAL_ROW and B >= 3:
            assert [t for t, _ in want] == list(range(min(n, V)))
            assert abs(float(out_lp[b, g]) + math.log(V)) <= 1e-4 + 1e-6 * math.log(V)
    assert seen_live >= 1
    if B == 65:  # (not vacuous: some live row picked the banned column, and reports -inf exactly)
        assert any(st.live(b) and picks[b] == 3 and float(out_lp[b, int(st.gen_count[b])]) == NINF for b in range(B))
    WORST[(V, B, scale)] = worst
    print("logprobs max |error| V=%d B=%d scale=%g: %.3e" % (V, B, scale, worst))


def test_row_wider_than_the_register_cache():
    """V > 131072: a segment no longer fits the keys a thread keeps in registers, and the columns past them are
    read again in every pass -- the kernel's other path, with an odd tail."""
    test_kernels_match_the_reference(140003, 140008, 3, 4.0)
    test_kernels_match_the_reference(262144 + 8, 262144 + 8, 1, 30.0)  # ... and twice the cache


def test_all_equal_row_alone():
    V = 1007
    rows = torch.full((1, V), -2.25, dtype=torch.bfloat16)
    buf = _buffer(rows, 1016)
    st = _LSt(1, lp_n=[20], gen=[0], done=[0])
    _run(buf, V, st, [V - 1])
    assert st.lp.out_top_tok[0, 0].tolist() == list(range(20))
    want = -math.log(V)
    for x in st.lp.out_top_lp[0, 0].tolist() + [float(st.lp.out_logprobs[0, 0])]:
        assert abs(x - want) <= 1e-4 + 1e-6 * abs(want)
    assert torch.equal(_bits(st.lp.out_logprobs[0, 0]), _bits(st.lp.out_top_lp[0, 0, 0]))


def test_minus_zero_and_bans_in_a_short_row():
    """V = 8, n = 20: every token is listed -- -0 (column 4) before +0 (column 6) by id, their values equal
    bit for bit, the banned column last with -inf, the entries past the vocabulary -1 / -inf."""
    rows = _rows(1, 8, 1.0, 5)
    st = _LSt(1, lp_n=[20], gen=[1], done=[0])
    _run(_buffer(rows, 8), 8, st, [4])
    toks, lps = st.lp.out_top_tok[0, 1].tolist(), st.lp.out_top_lp[0, 1].cpu()
    assert sorted(toks[:8]) == list(range(8)) and toks[8:] == [-1] * 12
    assert toks[7] == 3 and float(lps[7]) == NINF and all(x == NINF for x in lps[8:].tolist())
    i4, i6 = toks.index(4), toks.index(6)
    assert i6 == i4 + 1 and torch.equal(_bits(lps[i4]), _bits(lps[i6]))
    assert torch.equal(_bits(st.lp.out_logprobs[0, 1]), _bits(lps[i4]))  # the pick of -0 equals the entry


@pytest.mark.parametrize("V,ld", [(1007, 1016), (128256, 128264)])
def test_batch_invariance_is_exact(V, ld):
    row = _rows(1, V, 4.0, 99)
    tok = int(row[0].float().argmax())

    def records(B, at, gen):
        rows = _rows(B, V, 4.0, 1000 + B)
        for i in at:
            rows[i] = row[0]
        st = _LSt(B, lp_n=[20] * B, gen=[gen] * B, done=[0] * B)
        _run(_buffer(rows, ld), V, st, [tok] * B)
        return [(_bits(st.lp.out_top_tok[i, gen]), _bits(st.lp.out_top_lp[i, gen]), _bits(st.lp.out_logprobs[i, gen]))
                for i in at]

    solo = records(1, [0], 0)[0]
    for other in records(65, [7, 40], 3):
        for a, b in zip(solo, other):
            assert torch.equal(a, b)


def test_launcher_refusals():
    V, B = 1007, 3
    logits = _buffer(_rows(B, V, 1.0, 1), 1016)[:, :V]
    st = _LSt(B)
    hip.logprobs(logits, st)
    with pytest.raises(ValueError):
        hip.logprobs(logits.float(), st)
    with pytest.raises(ValueError):
        hip.logprobs(logits[:, 1:], st)  # rows off the 16-byte grid
    bad = _LSt(B)
    bad.lp_n = bad.lp_n.long()
    with pytest.raises(ValueError):
        hip.logprobs(logits, bad)
    with pytest.raises(ValueError):
        hip.logprobs(logits, _LSt(B - 1))  # a store smaller than the batch
    bad = _LSt(B)
    del bad.lp
    with pytest.raises(ValueError):
        hip.logprobs(logits, bad)
    bad = _LSt(B)
    bad.out_tokens = bad.out_tokens[:, :CAP - 1]  # narrower than the record store
    with pytest.raises(ValueError):
        hip.logprobs_pick(logits, bad)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ engine
@pytest.fixture(scope="module")
def eng():
    return LLMEngine(get_model_config("tiny-gqa4", init_std=0.05), device="cuda:0", max_model_len=2048,
                     max_num_seqs=16, kv_pages=256, sync_every=8, max_new_cap=64)


PROMPTS = [[128000] + [(i * 37 + j * 11) % 120000 + 5 for j in range(n)] for i, n in enumerate((40, 300, 7, 129))]
N = 12


def _ids(outs):
    return [o.token_ids for o in outs]


def test_engine_logprob_graphs(eng):
    plain = [SamplingParams(N, 1.0, 20 + i) for i in range(4)]
    base = eng.generate(PROMPTS, plain, ignore_eos=True)
    assert all(o.logprobs is None and o.top_logprobs is None for o in base)
    keys0, c0 = set(eng._graphs), eng.stats["graph_captures"]
    assert keys0 and all(len(k) == 2 for k in keys0) and eng.stats["logprob_steps"] == 0
    assert not eng.state.lp.allocated  # nobody asked: no store
    asking = [SamplingParams(N, 1.0, 20 + i, logprobs=True, top_logprobs=(5, 0, 20, 1)[i]) for i in range(4)]
    a = eng.generate(PROMPTS, asking, ignore_eos=True)
    assert _ids(a) == _ids(base)  # asking changes no token
    assert eng.stats["logprob_steps"] >= N
    new = set(eng._graphs) - keys0
    assert new and eng.stats["graph_captures"] > c0 and all(k[-1] == "lp" and k[:2] in keys0 for k in new)
    for o, sp in zip(a, asking):
        assert len(o.logprobs) == N and [len(t) for t in o.top_logprobs] == [sp.top_logprobs] * N
        assert all(x <= 0.0 for x in o.logprobs)
    eng.use_graphs = False
    try:
        b = eng.generate(PROMPTS, asking, ignore_eos=True)
    finally:
        eng.use_graphs = True
    assert _ids(b) == _ids(a)
    for x, y in zip(a, b):  # graphs against eager: bit-equal records
        assert x.logprobs == y.logprobs and x.top_logprobs == y.top_logprobs
    c1 = eng.stats["graph_captures"]
    again = eng.generate(PROMPTS, plain, ignore_eos=True)  # a plain generate afterwards: the plain graphs, as before
    assert _ids(again) == _ids(base) and eng.stats["graph_captures"] == c1
    assert all(o.logprobs is None for o in again)


def test_engine_greedy_token_is_the_top_entry(eng):
    outs = eng.generate(PROMPTS[:2], [SamplingParams(N, 0.0, 1, logprobs=True, top_logprobs=3)] * 2, ignore_eos=True)
    for o in outs:
        for tok, lp, top in zip(o.token_ids, o.logprobs, o.top_logprobs):
            assert top[0] == (tok, lp)


def test_engine_mixed_batch_against_the_reference(eng):
    """Asking and non-asking rows, filtered + penalised + constrained rows with logprobs, graphs against eager,
    and every record against the definition on the logits the GPU sampler saw (read back in the eager run)."""
    ban = {t: NINF for t in range(0, 400, 2)}
    ban[11] = 4.0
    sp = [SamplingParams(N, 1.0, 31, logprobs=True, top_logprobs=20, top_k=50, top_p=0.9, frequency_penalty=0.7,
                         repetition_penalty=1.3, logit_bias=ban, min_tokens=3),
          SamplingParams(N, 0.8, 32, top_k=7),
          SamplingParams(N, 0.0, 33, logprobs=True, top_logprobs=2, presence_penalty=1.5),
          SamplingParams(N, 1.2, 34, logprobs=True)]
    a = eng.generate(PROMPTS, sp)
    eng.use_graphs = False
    try:
        with SampleTap() as tap:
            b = eng.generate(PROMPTS, sp)
    finally:
        eng.use_graphs = True
    assert _ids(a) == _ids(b)
    worst = 0.0
    for x, y, p in zip(a, b, sp):
        assert (x.logprobs, x.top_logprobs) == (y.logprobs, y.top_logprobs)
        if not p.logprobs:
            assert y.logprobs is None and y.top_logprobs is None
            continue
        worst = max(worst, check_records(y, tap.rows, p.seed, p.top_logprobs))
    print("engine logprobs max |error|: %.3e" % worst)
    plain = eng.generate(PROMPTS, [SamplingParams(**{**vars(p), "logprobs": False, "top_logprobs": 0}) for p in sp])
    assert _ids(plain) == _ids(a)
