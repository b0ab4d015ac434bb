"""The counting probes (tests/_probes.py) bite: on their inputs the references give the exact counts, and
every one-key / one-page mutant misses them in every row it applies to -- long contexts included, where
random-data tests cannot see such a mistake.  Runs without a GPU.

The mutants are applied to the probe's inputs or to a local copy of the reference's attention loop (a query
attending to an explicit list of key positions gathered through the block table), never to the package."""

import math

import pytest
import torch

import _probes as pr
from llm_map_reduce_summarizer_amd.ops import reference

SC = 1.0 / math.sqrt(pr.D)
CTXS = [1, 2, 63, 64, 65, 127, 128, 129, 700, 1000, 2048]
FMTS = ["bf16", "fp8", "fp8v"]
HQ, HKV = 4, 2


def test_closed_form_matches_a_brute_force_count():
    n = torch.tensor([1, 2, 63, 64, 65, 129, 700, 2048, 4096, 4097, 9000])
    for i, ni in enumerate(n.tolist()):
        brute = pr.onehot_v(torch.arange(ni)).double().sum(0) / ni
        assert torch.equal(brute, pr.expect_prefix(n)[i])


def test_probe_values_are_exact_in_every_cache_format():
    p16 = pr.decode_probe([1, 65, 700], HKV, "bf16", n_idle=1)
    p8 = pr.decode_probe([1, 65, 700], HKV, "fp8", n_idle=1)
    pv = pr.decode_probe([1, 65, 700], HKV, "fp8v", n_idle=1)
    allp = torch.arange(p16.kcache.shape[0])
    for a, b in ((p16.kcache, p8.kcache), (p16.vcache, p8.vcache), (p16.vcache, pv.vcache)):
        assert b.dtype == torch.uint8
        assert torch.equal(reference.cache_pages(reference.kv8_from_bf16(a), allp, pr.PAGE, pr.D), a.float())
        assert torch.equal(reference.cache_pages(b, allp, pr.PAGE, pr.D), a.float())
    assert pv.kcache.dtype == torch.bfloat16 and torch.equal(pv.kcache, p16.kcache)
    # the scratch page, the spare pages and every slot past a context hold the poison
    assert bool((p16.kcache[0] == pr.POISON_K).all()) and bool((p16.vcache[0] == pr.POISON_V).all())
    assert bool((p16.block_tables[3] == 0).all()) and int(p16.positions[3]) == 0
    last = int(p16.block_tables[1, 1])
    assert bool((p16.kcache[last, :, 0] == 0).all()) and bool((p16.kcache[last, :, 1:] == pr.POISON_K).all())
    assert bool((p16.vcache[last, :, 1:] == pr.POISON_V).all())


def test_check_counts_bounds():
    e = pr.expect_prefix(torch.tensor([700]))
    pr.check_counts(e.repeat(1, 3), e)
    pr.check_counts(e.repeat(1, 3) * (1 + 0.9 * pr.BOUND), e)
    for bad in (e * (1 + 1.1 * pr.BOUND), e + 2e-6, torch.full_like(e, float("nan"))):
        with pytest.raises(AssertionError):
            pr.check_counts(torch.cat([e, bad, e], 1), e)
        assert pr.count_errors(torch.cat([e, bad, e], 1), e).tolist() == [[False, True, False]]


# ------------------------------------------------------------------ the references give the exact counts
@pytest.mark.parametrize("fmt", FMTS)
def test_reference_decode(fmt):
    p = pr.decode_probe(CTXS, HKV, fmt, n_idle=2, hq=HQ)
    out = reference.attn_decode(p.q, p.kcache, p.vcache, p.block_tables, p.positions, HQ, HKV, pr.D, pr.PAGE, SC)
    pr.check_counts(out[:p.live], p.expect)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("sp", [1, 4])
def test_reference_rope_then_decode(fmt, sp):
    p = pr.decode_rope_probe(CTXS, HQ, HKV, fmt, n_idle=2, sp=sp)
    cs = reference.rope_cos_sin(pr.MAX_CTX, pr.D, 500000.0)
    k0, v0 = p.kcache.clone(), p.vcache.clone()
    sidx = torch.arange(p.B, dtype=torch.int32)
    qkv = reference.rope_kv_parts(p.parts, p.positions, sidx, p.block_tables, p.kcache, p.vcache, cs, HQ, HKV,
                                  pr.D, pr.PAGE)
    out = reference.attn_decode(qkv, p.kcache, p.vcache, p.block_tables, p.positions, HQ, HKV, pr.D, pr.PAGE, SC)
    pr.check_counts(out[:p.live], p.expect)
    pr.check_new_rows(p, k0, v0, p.kcache, p.vcache)
    # without the new token's row the slot still holds the poison: the probe would notice
    stale = reference.attn_decode(qkv, k0, v0, p.block_tables, p.positions, HQ, HKV, pr.D, pr.PAGE, SC)
    assert bool(pr.count_errors(stale[:p.live], p.expect).all())


@pytest.mark.parametrize("hq,hkv", [(2, 2), (4, 1), (6, 2)])
def test_reference_prefill(hq, hkv):
    p = pr.prefill_probe([1, 63, 64, 65, 257, 700], hq, hkv)
    out = reference.attn_prefill(p.qkv, p.cu_seqlens, hq, hkv, pr.D, SC)
    pr.check_counts(out[:p.T], p.expect)


SPANS = [[(0, 200)], [(130, 300), (0, 77), (1000, 1129)], [(64, 128), (2047, 2048)]]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("spans", SPANS)
def test_reference_prefill_paged(fmt, spans):
    p = pr.paged_prefill_probe(spans, HQ, HKV, fmt)
    out = reference.attn_prefill_paged(p.qkv, p.cu_seqlens, HQ, HKV, pr.D, SC, pr.paged_args(p))
    pr.check_counts(out, p.expect)


# ------------------------------------------------------------------ mutants
def _attend(q, k, v, hq, hkv):
    """fp32 attention of one query row q [hq * d] over keys k / v [hkv, n, d] -> bf16 [hq * d] (the
    reference's arithmetic: fp32 scores, softmax, bf16 output)."""
    qq = q[: hq * pr.D].view(hkv, hq // hkv, pr.D).float()
    w = torch.softmax(torch.matmul(qq, k.transpose(1, 2)) * SC, dim=-1)
    return torch.matmul(w, v).reshape(hq * pr.D).to(torch.bfloat16)


def _cached(cache, bt_row, keys):
    """fp32 [hkv, len(keys), d]: the cache rows at positions ``keys`` of the sequence with block-table row
    ``bt_row`` (positions may repeat or lie past the context)."""
    keys = keys.long()
    npg = int(keys.max()) // pr.PAGE + 1
    pages = reference.cache_pages(cache, bt_row[:npg].long(), pr.PAGE, pr.D)
    return pages.permute(1, 0, 2, 3).reshape(cache.shape[1], npg * pr.PAGE, pr.D)[:, keys]


def _decode_with(p, keys_of, bt=None):
    """Decode attention of the live rows of probe ``p`` where row b attends to the positions keys_of(ctx_b)."""
    bt = p.block_tables if bt is None else bt
    return torch.stack([_attend(p.q[b], _cached(p.kcache, bt[b], keys_of(c)), _cached(p.vcache, bt[b], keys_of(c)),
                                p.hq, p.hkv) for b, c in enumerate(p.ctxs)])


def _rows(p, cond):
    return torch.tensor([i for i, c in enumerate(p.ctxs) if cond(c)])


def _all_fail(out, expect, rows):
    assert len(rows) > 0
    bad = pr.count_errors(out, expect)
    assert bool(bad[rows].all()), "undetected in rows %s" % rows[~bad[rows].all(-1)].tolist()


@pytest.fixture(scope="module", params=FMTS)
def dprobe(request):
    return pr.decode_probe(CTXS, HKV, request.param, n_idle=2, hq=HQ)


def test_local_decode_loop_is_faithful(dprobe):
    pr.check_counts(_decode_with(dprobe, lambda c: torch.arange(c)), dprobe.expect)


def test_mutant_newest_key_forgotten(dprobe):
    p = dprobe
    rows = _rows(p, lambda c: c >= 2)
    _all_fail(_decode_with(p, lambda c: torch.arange(max(c - 1, 1))), p.expect, rows)
    # the same through the package's reference, by its inputs
    pos = (p.positions - 1).clamp_min(0)
    out = reference.attn_decode(p.q, p.kcache, p.vcache, p.block_tables, pos, HQ, HKV, pr.D, pr.PAGE, SC)
    _all_fail(out[:p.live], p.expect, rows)


def test_mutant_one_slot_past_the_context(dprobe):
    p = dprobe
    _all_fail(_decode_with(p, lambda c: torch.arange(c + 1)), p.expect, _rows(p, lambda c: True))
    out = reference.attn_decode(p.q, p.kcache, p.vcache, p.block_tables, p.positions + 1, HQ, HKV, pr.D, pr.PAGE, SC)
    _all_fail(out[:p.live], p.expect, _rows(p, lambda c: True))


def test_mutant_first_page_lost(dprobe):
    p = dprobe
    _all_fail(_decode_with(p, lambda c: torch.arange(64, c) if c > 64 else torch.arange(c)), p.expect,
              _rows(p, lambda c: c > 64))


def test_mutant_one_page_read_twice(dprobe):
    p = dprobe
    twice = lambda c: torch.cat([torch.arange(c), torch.arange(64)]) if c > 64 else torch.arange(c)  # noqa: E731
    _all_fail(_decode_with(p, twice), p.expect, _rows(p, lambda c: c > 64))


def test_mutant_block_table_entries_swapped(dprobe):
    """The first and the last page of a context swapped.  Attention does not depend on the order of its keys,
    so the swap shows exactly where the last page is partial: positions [0, 64) then read its stale slots."""
    p = dprobe
    bt = p.block_tables.clone()
    last = torch.tensor([(c - 1) // pr.PAGE for c in p.ctxs])
    live = torch.arange(p.live)
    bt[live, 0], bt[live, last] = p.block_tables[live, last], p.block_tables[live, 0]
    rows = _rows(p, lambda c: c > 64 and c % 64 != 0)
    _all_fail(_decode_with(p, lambda c: torch.arange(c), bt), p.expect, rows)
    out = reference.attn_decode(p.q, p.kcache, p.vcache, bt, p.positions, HQ, HKV, pr.D, pr.PAGE, SC)
    _all_fail(out[:p.live], p.expect, rows)


def _prefill_with(p, keys_of):
    """Packed prefill where packed row t attends to the packed rows keys_of(t, start of its sequence)."""
    hq, hkv = p.hq, p.hkv
    k = p.qkv[:, hq * pr.D: (hq + hkv) * pr.D].view(-1, hkv, pr.D).float().transpose(0, 1)
    v = p.qkv[:, (hq + hkv) * pr.D:].view(-1, hkv, pr.D).float().transpose(0, 1)
    starts = (torch.arange(p.T) - p.local).tolist()
    return torch.stack([_attend(p.qkv[t], k[:, keys_of(t, s)], v[:, keys_of(t, s)], hq, hkv)
                        for t, s in enumerate(starts)])


@pytest.fixture(scope="module")
def pprobe():
    return pr.prefill_probe([1, 63, 64, 65, 257, 700], 2, 1)


def test_local_prefill_loop_is_faithful(pprobe):
    pr.check_counts(_prefill_with(pprobe, lambda t, s: torch.arange(s, t + 1)), pprobe.expect)


def test_mutant_causal_mask_sees_one_key_ahead(pprobe):
    """Only the last row of every 32-row block sees key i + 1 (a mask wrong at a tile edge)."""
    p = pprobe
    n_of = torch.repeat_interleave(torch.tensor(p.seqlens), torch.tensor(p.seqlens))
    hit = (p.local % 32 == 31) & (p.local + 1 < n_of)
    out = _prefill_with(p, lambda t, s: torch.arange(s, t + 2) if bool(hit[t]) else torch.arange(s, t + 1))
    _all_fail(out, p.expect, hit.nonzero()[:, 0])
    assert not bool(pr.count_errors(out, p.expect)[~hit].any())


def test_mutant_previous_sequence_leaks(pprobe):
    p = pprobe
    out = _prefill_with(p, lambda t, s: torch.arange(max(s - 1, 0), t + 1))
    # every row of every sequence but the first -- except packed row 1: it is position 0 of its sequence and the
    # leaked key is position 0 of the one-token sequence before it, so its output is the same by construction
    rows = ((torch.arange(p.T) - p.local > 0) & (torch.arange(p.T) != 1)).nonzero()[:, 0]
    assert p.seqlens[0] == 1 and len(rows) == p.T - 2
    _all_fail(out, p.expect, rows)


def test_mutant_padding_row_leaks(pprobe):
    """The last sequence's last query also sees the poison row that follows the packed batch."""
    p = pprobe
    out = _prefill_with(p, lambda t, s: torch.arange(s, t + 2) if t == p.T - 1 else torch.arange(s, t + 1))
    _all_fail(out, p.expect, torch.tensor([p.T - 1]))


@pytest.mark.parametrize("fmt", FMTS)
def test_mutant_paged_slice_ignores_its_prefix(fmt):
    p = pr.paged_prefill_probe(SPANS[1], HQ, HKV, fmt)
    rel = p.absolute - torch.repeat_interleave(p.prefix.long(), torch.tensor(p.seqlens))
    seq = torch.repeat_interleave(torch.arange(len(p.seqlens)), torch.tensor(p.seqlens))

    def run(keys_of):
        return torch.stack([_attend(p.qkv[t], _cached(p.kcache, p.block_tables[p.slot_host[int(seq[t])]], keys_of(t)),
                                    _cached(p.vcache, p.block_tables[p.slot_host[int(seq[t])]], keys_of(t)), HQ, HKV)
                            for t in range(p.T)])
    pr.check_counts(run(lambda t: torch.arange(int(p.absolute[t]) + 1)), p.expect)
    out = run(lambda t: torch.arange(int(rel[t]) + 1))
    _all_fail(out, p.expect, (p.absolute != rel).nonzero()[:, 0])
