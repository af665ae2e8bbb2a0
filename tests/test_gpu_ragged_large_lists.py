"""Ragged batches up to order 1024 with the reference's exact `_path` lists (fwx_solve_ragged_large_lists_f64 / _f32,
fwx_dev_solve_ragged_large with a trace + fwx_dev_exact_paths_ragged_large): every matrix of a batch of DIFFERENT
orders bit for bit what the oracle's loop leaves of it, and every list asked for, list for list, what the rope oracle
(oracle.list_ropes.solve) gives for that matrix alone.

One batch holds the large orders 257, 272, 273 and 289 (the first large order, a matrix that goes inactive at a block
edge, a last block of one pivot, a strip edge) between the small ones 1, 17, 65, 129 and 256, so that the wave tier,
the 128-wide tier, the mid tier and the large tier write the trace in one call.  The oracle side of every matrix is
tests/test_gpu_batch_mid_lists.py's _Ref (ropes, dense solution, the direct definition of the three trace arrays),
computed once and shared with that file; every precondition is asserted from the oracle before any GPU call.  A
matrix of order 1024 rides in a batch of its own with two small ones: a seeded sample of its lists against a traced
single-matrix handle on the same input (test_gpu_batch_large_lists.py's _limit_case).

Which lists: all pairs at the orders up to 65; above, the pairs whose src or dst lies in the edge set {0, 16, 48, 256,
n - 17, n - 16, n - 1} (block, strip and tile-column edges, the last block) plus a seeded sample.  The host form runs
once per capacity class of the ORACLE's lengths, so that one long list does not set the capacity of every item."""
import ctypes
import functools

import numpy as np
import pytest

from floydwarshall_amd import _lib, engine, hip
from floydwarshall_amd._lib import FWX_ERR_CAPACITY, FWX_ERR_INVALID

from helpers import assert_bits_equal, dev, host
from test_gpu_batch_large_lists import _limit_case
from test_gpu_batch_mid_lists import CALL_INTS, CAP_CLASSES, INT_SENTINEL, MAX_LIST, NAN_SENTINEL, _synth_refs

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
ORDERS = (257, 1, 272, 17, 273, 65, 129, 289, 256)
LARGE = (0, 2, 4, 7)                 # where the large orders stand
SAMPLE = 512
SETTINGS = ("FWX_BATCH_WAVE_MAX_N", "FWX_BATCH_MID_MIN_N", "FWX_BATCH_LARGE_MIN_N", "FWX_BATCH_LISTS_CHUNK")


def _name(dtype):
    return np.dtype(dtype).name


def _defaults(monkeypatch):
    for name in SETTINGS:
        monkeypatch.delenv(name, raising=False)


@functools.lru_cache(maxsize=None)
def _refs(dtype_name):
    return tuple(_synth_refs(n, 1, dtype_name)[0] for n in ORDERS)


def _edge_set(n):
    return sorted({v for v in (0, 16, 48, 256, n - 17, n - 16, n - 1) if 0 <= v < n})


def _pairs(ref, sample_seed=0):
    n = ref.n
    if n <= 65:
        return [(i, j) for i in range(n) for j in range(n)]
    edge = set(_edge_set(n))
    pairs = [(i, j) for i in range(n) for j in range(n) if i in edge or j in edge]
    rnd = np.random.default_rng(3100 + n + sample_seed)
    return pairs + [(int(i), int(j)) for i, j in zip(rnd.integers(0, n, SAMPLE), rnd.integers(0, n, SAMPLE))]


def _preconditions(refs):
    for b, ref in enumerate(refs):
        assert ref.longest <= MAX_LIST, "matrix %d: a list of %d entries" % (b, ref.longest)
        if ref.n >= 4:
            assert ref.ropes.updates > 0, "the oracle relaxes nothing in matrix %d" % b
    assert [refs[b].n for b in LARGE] == [257, 272, 273, 289]


def _pack(refs, f):
    return np.concatenate([np.ascontiguousarray(getattr(r, f)).reshape(-1) for r in refs])


def _raw(refs, items, cap, with_hops=True):
    """One call of the host form as the C caller sees it: (status, rate, next, hops, [U_b], lens, paths), packed."""
    rate, nxt = _pack(refs, "rate"), _pack(refs, "next")
    hops = _pack(refs, "hops") if with_hops else None
    n_each = np.array([r.n for r in refs], dtype=np.int32)
    mat, src, dst = (np.ascontiguousarray([it[f] for it in items], dtype=np.int32) for f in range(3))
    lens = np.full(len(items), -99, dtype=np.int32)
    paths = np.full((max(len(items), 1), cap), -7, dtype=np.int32)
    us = np.full(len(refs), 99, dtype=np.uint64)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    fn = getattr(_lib.lib(), "fwx_solve_ragged_large_lists_" + ("f64" if rate.dtype == np.float64 else "f32"))
    st = fn(len(refs), p(n_each), p(rate), p(nxt), p(hops), p(us), len(items), p(mat), p(src), p(dst), p(lens),
            p(paths), cap, None)
    return st, rate, nxt, hops, [int(u) for u in us], lens, paths


def _check_solution(refs, got, what):
    _, rate, nxt, hops, us, _, _ = got
    for f, (field, arr) in enumerate((("rate", rate), ("next", nxt), ("hops", hops))):
        if arr is not None:
            want = np.concatenate([r.solved[f].reshape(-1) for r in refs])
            assert_bits_equal(arr, want, "%s packed %s" % (what, field))
    assert us == [int(r.solved[3]) for r in refs], what


def _check_lists(refs, items, lens, paths, what):
    bad = []
    for q, (b, i, j) in enumerate(items):
        want = refs[b].path(i, j)
        if int(lens[q]) != len(want) or tuple(paths[q, :len(want)].tolist()) != want:
            bad.append((b, i, j, int(lens[q]), len(want)))
    assert not bad, "%s: %d lists differ, first (matrix, src, dst, length or status, oracle's length) %r" % (
        what, len(bad), bad[0])


def _ask(refs, items, what, with_hops=True):
    """The lists of `items` through the host form, one call (or more, CALL_INTS of list capacity each) per capacity
    class; the solution of every call is checked against the dense oracle, every list against the ropes."""
    want_len = np.array([int(refs[b].lengths[i, j]) for b, i, j in items], dtype=np.int64)
    lo = -1
    for hi in CAP_CLASSES:
        sel = np.nonzero((want_len > lo) & (want_len <= hi))[0]
        lo = hi
        step = max(CALL_INTS // (hi + 2), 1)
        for c0 in range(0, len(sel), step):
            part = [items[q] for q in sel[c0:c0 + step]]
            got = _raw(refs, part, hi + 2, with_hops)
            assert got[0] == 0, got[0]
            _check_solution(refs, got, what)
            _check_lists(refs, part, got[5], got[6], "%s cap %d" % (what, hi + 2))


def _cap(refs, items):
    return max(int(refs[b].lengths[i, j]) for b, i, j in items) + 2


# ---- 1. the mixed batch through the host form -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("with_hops", [True, False])
def test_mixed_batch_lists(with_hops, dtype, monkeypatch):
    _defaults(monkeypatch)
    refs = _refs(_name(dtype))
    _preconditions(refs)
    tiers = [int(t) for t in engine.ragged_large_plan([r.n for r in refs])[2]]
    assert tiers == [1, 1, 1, 2, 4]                   # wave: 1; 64-wide: 17; 128-wide: 65; mid: 129, 256; large: four
    items = [(b, i, j) for b, ref in enumerate(refs) for i, j in _pairs(ref)]
    _ask(refs, items, "mixed batch %s hops=%s" % (_name(dtype), with_hops), with_hops)


# ---- 2. the device pair: traced solve plus walk -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_device_forms_trace_cells_and_unpacked_offsets(dtype, monkeypatch):
    """fwx_dev_solve_ragged_large with a trace and fwx_dev_exact_paths_ragged_large on a caller's stream, the matrices
    in reverse memory order with sentinel gaps, scratch for the largest order alone: the three trace arrays equal the
    direct definition cell for cell, the gaps survive in all six arrays, and the walk addresses by the same offsets."""
    _defaults(monkeypatch)
    refs = _refs(_name(dtype))
    _preconditions(refs)
    count = len(refs)
    rnd = np.random.default_rng(99)
    offset, at = np.zeros(count, dtype=np.int64), 0
    for b in reversed(range(count)):
        at += int(rnd.integers(1, 8))
        offset[b] = at
        at += refs[b].n ** 2
    total = at + 3
    bits = np.uint64 if dtype == np.float64 else np.uint32
    flat = [np.full(total, NAN_SENTINEL[dtype], dtype=bits).view(dtype)] + [
        np.full(total, INT_SENTINEL, dtype=np.int32) for _ in range(5)]
    expect = [a.copy() for a in flat]
    for b, ref in enumerate(refs):
        sl = slice(int(offset[b]), int(offset[b]) + ref.n ** 2)
        for f, field in enumerate(("rate", "next", "hops")):
            flat[f][sl] = getattr(ref, field).reshape(-1)
            expect[f][sl] = ref.solved[f].reshape(-1)
        for f in range(3):
            expect[3 + f][sl] = ref.trace[f].reshape(-1)
    n_each = np.array([r.n for r in refs], dtype=np.int32)
    _, order, tiers, work = engine.ragged_large_plan(n_each)
    d = [dev(a) for a in flat]
    next0 = dev(flat[1])
    upd = dev(np.full(count, 5, dtype=np.uint64))
    d_n, d_off, d_order, d_work = dev(n_each), dev(offset), dev(order), dev(work)
    scratch = dev(np.zeros(_lib.batch_large_scratch_bytes(289), dtype=np.uint8))
    trace = engine.Trace(0, 0, _views=(d[3], d[4], d[5]))
    s = hip.Stream()
    engine.dev_solve_ragged_large(d[0], d_n, d_off, d_order, tiers, work, d_work, next_t=d[1], hops_t=d[2],
                                  trace=trace, updates_t=upd, scratch_t=scratch, stream=s)
    items = [(b, i, j) for b, ref in enumerate(refs) for i, j in _pairs(ref, sample_seed=2)[-SAMPLE:]]
    items += [(0, 257, 0), (count, 0, 0), (-1, 0, 0)]
    cap = _cap(refs, items[:-3])
    mat, src, dst = (dev(np.ascontiguousarray([it[f] for it in items], dtype=np.int32)) for f in range(3))
    len_t, path_t = engine.dev_exact_paths_ragged_large(next0, d_n, d_off, 289, trace, mat, src, dst, cap, stream=s)
    s.synchronize()
    for f, field in enumerate(("rate", "next", "hops", "last", "at_col", "at_row")):
        assert_bits_equal(host(d[f]), expect[f], "device forms %s %s" % (_name(dtype), field))
    assert [int(u) for u in host(upd)] == [5 + int(r.solved[3]) for r in refs]
    lens, paths = host(len_t), host(path_t)
    assert [int(v) for v in lens[-3:]] == [FWX_ERR_INVALID] * 3
    _check_lists(refs, items[:-3], lens[:-3], paths[:-3], "device walk %s" % _name(dtype))
    s.close()


# ---- 3. items, capacity, chunks ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_items_are_judged_by_their_own_order_and_the_capacity_rule(dtype, monkeypatch):
    """An item's src and dst are judged by the order of ITS matrix, not by the largest; cap = L returns the longest
    list of the order-289 matrix, cap = L - 1 is FWX_ERR_CAPACITY for that item alone; an empty list fits cap = 1."""
    _defaults(monkeypatch)
    refs = _refs(_name(dtype))
    good = [(7, 288, 0), (0, 256, 1), (2, 271, 271), (4, 272, 5), (8, 255, 0), (3, 16, 1)]
    bad = [(0, 257, 0), (2, 0, 272), (4, 273, 273), (1, 1, 0), (3, 17, 0), (8, 256, 0), (len(refs), 0, 0), (7, 289, 0),
           (7, 0, -1)]
    items = [x for pair in zip(good + good[:3], bad) for x in pair]
    got = _raw(refs, items, _cap(refs, good))
    assert got[0] == 0
    _check_solution(refs, got, "bad items %s" % _name(dtype))
    for q, (b, i, j) in enumerate(items):
        if (b, i, j) in bad:
            assert int(got[5][q]) == FWX_ERR_INVALID, (q, b, i, j, int(got[5][q]))
        else:
            w = refs[b].path(i, j)
            assert int(got[5][q]) == len(w) and tuple(got[6][q, :len(w)].tolist()) == w, (q, b, i, j)
    ref = refs[7]
    i, j = (int(v) for v in np.unravel_index(int(np.argmax(ref.lengths)), (289, 289)))
    L = ref.longest
    assert L >= 2 and int(ref.lengths[i, j]) == L and ref.path(0, 0) == ()
    items = [(7, i, j), (7, 0, 0), (3, 1, 0)]
    want = [refs[m].path(s, d) for m, s, d in items]
    for cap in (L, L - 1):
        st, _, _, _, _, lens, paths = _raw(refs, items, cap)
        assert st == 0
        for q, w in enumerate(want):
            have = (int(lens[q]), tuple(paths[q, :max(int(lens[q]), 0)].tolist()))
            expect = (len(w), w) if cap >= len(w) else (FWX_ERR_CAPACITY, ())
            assert have == expect, "cap %d item %d %r: %r, expected %r" % (cap, q, items[q], have[0], expect[0])
    st, _, _, _, _, lens, _ = _raw(refs, [(7, 0, 0)], 1)
    assert st == 0 and int(lens[0]) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_chunked_walk_gives_the_same_answer(dtype, monkeypatch):
    """FWX_BATCH_LISTS_CHUNK=1000 walks 2500 items in three launches: the same lengths and lists."""
    _defaults(monkeypatch)
    refs = _refs(_name(dtype))
    rnd = np.random.default_rng(3131)
    mats = rnd.integers(0, len(refs), 2500)
    items = [(int(b), int(rnd.integers(0, refs[b].n)), int(rnd.integers(0, refs[b].n))) for b in mats]
    cap = _cap(refs, items)
    assert _lib.lib().fwx_test_batch_lists_chunk(289, cap) >= 2500
    whole = _raw(refs, items, cap)
    monkeypatch.setenv("FWX_BATCH_LISTS_CHUNK", "1000")
    assert _lib.lib().fwx_test_batch_lists_chunk(289, cap) == 1000
    chunked = _raw(refs, items, cap)
    assert whole[0] == 0 and chunked[0] == 0
    _check_solution(refs, chunked, "chunked")
    assert np.array_equal(whole[5], chunked[5])
    _check_lists(refs, items, whole[5], whole[6], "whole")           # what lies past a list's length is nobody's
    _check_lists(refs, items, chunked[5], chunked[6], "chunked")


# ---- 4. order 1024 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_a_1024_in_the_batch_against_a_traced_handle(dtype, monkeypatch):
    """One matrix of order 1024 between two small ones: its bits are the dense oracle's, and a seeded sample of its
    lists (rows 0 and 1023 whole, 4096 seeded pairs) those of a traced single-matrix handle on the same input."""
    _defaults(monkeypatch)
    (rate, nxt, hops), (er, en, eh, eu), (src, dst, want_len, want_paths) = _limit_case(1024, _name(dtype))
    small = (_synth_refs(17, 1, _name(dtype))[0], _synth_refs(129, 1, _name(dtype))[0])
    mats = [[small[0].rate.copy(), rate.copy(), small[1].rate.copy()], [small[0].next.copy(), nxt.copy(),
            small[1].next.copy()], [small[0].hops.copy(), hops.copy(), small[1].hops.copy()]]
    assert list(engine.ragged_large_plan([17, 1024, 129])[2]) == [0, 1, 0, 1, 1]
    cap = int(want_len.max()) + 2
    items = (np.ones(len(src), dtype=np.int32), src, dst)
    lists, us = engine.solve_ragged_large_lists(mats[0], mats[1], mats[2], items=items, cap=cap, count_updates=True)
    what = "n=1024 in a batch %s" % _name(dtype)
    for f, (field, want) in enumerate((("rate", er), ("next", en), ("hops", eh))):
        assert_bits_equal(mats[f][1], want, "%s %s" % (what, field))
        for b, ref in ((0, small[0]), (2, small[1])):
            assert_bits_equal(mats[f][b], ref.solved[f], "%s matrix %d %s" % (what, b, field))
    assert [int(u) for u in us] == [int(small[0].solved[3]), eu, int(small[1].solved[3])]
    bad = [q for q in range(len(src)) if lists[q] != tuple(want_paths[q, :want_len[q]].tolist())]
    assert not bad, "%s: %d lists differ from the handle's, first (%d, %d)" % (what, len(bad), src[bad[0]], dst[bad[0]])
