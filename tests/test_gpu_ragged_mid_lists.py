"""Ragged batches up to order 256 with the reference's exact `_path` lists (fwx_solve_ragged_mid_lists_f64 / _f32,
fwx_dev_solve_ragged_mid with a trace + fwx_dev_exact_paths_ragged_mid): every matrix of a batch of DIFFERENT orders
bit for bit what the oracle's loop leaves of it, and every list asked for, list for list, what the rope oracle
(oracle.list_ropes.solve) gives for that matrix alone.

One batch mixes the market construction (hostile_inputs.market_rates: exact ties, lists that are not the walk of the
final next-hops) at the mid orders 129, 145, 192 and 256 with synthetic matrices of the orders 3, 16, 17 and 64 and
with hostile draws at 5 and 130, so that the wave tier, the 64-wide tier and the mid tier write the trace in one call
(FWX_BATCH_MID_MIN_N=1 then puts every matrix through the mid kernel).  The oracle side of every matrix
(tests/test_gpu_batch_mid_lists.py's _Ref: ropes, dense solution, the direct definition of the three trace arrays) is
computed once and shared with that file.  Every precondition is asserted from the oracle before any GPU call.

Which lists: all n^2 pairs at the orders up to 145; at 192 and 256 the pairs whose src or dst lies in the edge set of
that file ({0, 1, B-1, B, B+1, n-B-1 ... n-1}) plus a seeded sample."""
import ctypes
import functools

import numpy as np
import pytest

import oracle
from floydwarshall_amd import _lib, engine, hip
from floydwarshall_amd._lib import FWX_ERR_CAPACITY, FWX_ERR_INVALID

from helpers import assert_bits_equal, dev, host
from test_gpu_batch_mid_lists import (ALL_PAIRS_MAX_N, INT_SENTINEL, NAN_SENTINEL, _edge_set, _hostile_refs,
                                      _market_ref, _synth_refs)

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
MARKET_ORDERS = (129, 145, 192, 256)
SAMPLE = 1024
LONGEST = 62                         # the file's capacity limit: every call runs with cap = 64


def _name(dtype):
    return np.dtype(dtype).name


@functools.lru_cache(maxsize=None)
def _market_with_a_tie(n, dtype_name):
    """The first market draw of order n with a list that is not the walk of its final next-hops: the oracle alone
    decides."""
    for seed_offset in range(4):
        ref = _market_ref(n, dtype_name, seed_offset)
        if _has_tie(ref):
            return ref
    raise AssertionError("no market draw of order %d has a tie" % n)


def _pairs(ref, sample_seed=0):
    n = ref.n
    if n <= ALL_PAIRS_MAX_N:
        return [(i, j) for i in range(n) for j in range(n)]
    edge = set(_edge_set(n))
    pairs = [(i, j) for i in range(n) for j in range(n) if i in edge or j in edge]
    rnd = np.random.default_rng(2200 + n + sample_seed)
    return pairs + [(int(i), int(j)) for i, j in zip(rnd.integers(0, n, SAMPLE), rnd.integers(0, n, SAMPLE))]


def _has_tie(ref):
    """Some asked list of the matrix is not the walk of its final next-hops -- from the oracle alone."""
    for i, j in _pairs(ref):
        walk = oracle.follow_path(ref.ropes.next, i, j)
        if walk is None or tuple(walk) != ref.path(i, j):
            return True
    return False


@functools.lru_cache(maxsize=None)
def _mixed_refs(dtype_name):
    """Index: 0 synth 3, 1 market 256, 2 synth 16, 3 market 129, 4 hostile 5, 5 synth 17, 6 market 192, 7 synth 64,
    8 hostile 130, 9 market 145.  (The second synthetic draw of each order: the first one of order 64 has a list of
    3782 entries, which would set the capacity of every item of a call.)"""
    s = lambda n: _synth_refs(n, 2, dtype_name)[1]  # noqa: E731
    m = lambda n: _market_with_a_tie(n, dtype_name)  # noqa: E731
    return (s(3), m(256), s(16), m(129), _hostile_refs(5, dtype_name)[0], s(17), m(192), s(64),
            _hostile_refs(130, dtype_name)[0], m(145))


def _preconditions(refs):
    for b, ref in enumerate(refs):
        assert ref.longest <= LONGEST, "matrix %d: a list of %d entries" % (b, ref.longest)
        if ref.n >= 4:
            assert ref.ropes.updates > 0, "the oracle relaxes nothing in matrix %d" % b
    for b in (1, 3, 6, 9):
        assert refs[b].n in MARKET_ORDERS and _has_tie(refs[b]), b


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
    fn = getattr(_lib.lib(), "fwx_solve_ragged_mid_lists_" + ("f64" if rate.dtype == np.float64 else "f32"))
    st = fn(len(refs), p(n_each), p(rate), p(nxt), p(hops), p(us), len(items), p(mat), p(src), p(dst), p(lens),
            p(paths), cap, None)
    return st, rate, nxt, hops, [int(u) for u in us], lens, paths


def _check_solution(refs, got, what, with_hops=True):
    _, rate, nxt, hops, us, _, _ = got
    for f, (field, arr) in enumerate((("rate", rate), ("next", nxt), ("hops", hops))):
        if arr is not None:
            want = np.concatenate([r.solved[f].reshape(-1) for r in refs])
            assert_bits_equal(arr, want, "%s packed %s" % (what, field))
    assert us == [int(r.solved[3]) for r in refs], what


def _check_lists(refs, items, got, what):
    lens, paths = got[5], got[6]
    bad = []
    for q, (b, i, j) in enumerate(items):
        want = refs[b].path(i, j)
        if int(lens[q]) != len(want) or tuple(paths[q, :len(want)].tolist()) != want:
            bad.append((b, i, j, int(lens[q]), len(want)))
    assert not bad, "%s: %d lists differ, first (matrix, src, dst, length or status, oracle's length) %r" % (
        what, len(bad), bad[0])


# ---- 1. the mixed batch -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("with_hops", [True, False])
def test_mixed_batch_lists(with_hops, dtype, monkeypatch):
    """Market matrices of the orders 129, 145, 192, 256 between small and hostile ones in one call: all four tiers, the
    lists of every matrix."""
    monkeypatch.delenv("FWX_BATCH_WAVE_MAX_N", raising=False)
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    refs = _mixed_refs(_name(dtype))
    _preconditions(refs)
    tiers = [int(t) for t in engine.ragged_mid_plan([r.n for r in refs])[2]]
    assert tiers == [3, 2, 0, 5]                      # wave: 3, 16, 5; 64-wide: 17, 64; mid: the markets and 130
    items = [(b, i, j) for b, ref in enumerate(refs) for i, j in _pairs(ref)]
    cap = LONGEST + 2
    got = _raw(refs, items, cap, with_hops)
    assert got[0] == 0
    what = "mixed batch %s hops=%s" % (_name(dtype), with_hops)
    _check_solution(refs, got, what, with_hops)
    _check_lists(refs, items, got, what)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_mid_min_n_changes_no_list(dtype, monkeypatch):
    """FWX_BATCH_MID_MIN_N=1: every matrix of the mixed batch through the traced mid kernel; the same lists."""
    monkeypatch.setenv("FWX_BATCH_MID_MIN_N", "1")
    refs = _mixed_refs(_name(dtype))
    assert list(engine.ragged_mid_plan([r.n for r in refs])[2]) == [0, 0, 0, len(refs)]
    items = [(b, i, j) for b, ref in enumerate(refs) for i, j in _pairs(ref, sample_seed=1) if ref.n <= 145 or b == 1]
    got = _raw(refs, items, LONGEST + 2)
    assert got[0] == 0
    _check_solution(refs, got, "mid>=1 %s" % _name(dtype))
    _check_lists(refs, items, got, "mid>=1 %s" % _name(dtype))


# ---- 2. the device forms: trace arrays cell for cell, offsets that are not packed ---------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_device_forms_trace_cells_and_unpacked_offsets(dtype, monkeypatch):
    """fwx_dev_solve_ragged_mid with a trace and fwx_dev_exact_paths_ragged_mid on a caller's stream, the matrices in
    reverse memory order with sentinel gaps: the three trace arrays equal the direct definition cell for cell, the
    gaps survive in all six arrays, and the walk addresses by the same offsets."""
    monkeypatch.delenv("FWX_BATCH_WAVE_MAX_N", raising=False)
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    refs = _mixed_refs(_name(dtype))
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
    _, order, tiers = engine.ragged_mid_plan(n_each)
    d = [dev(a) for a in flat]
    next0 = dev(flat[1])
    upd = dev(np.full(count, 5, dtype=np.uint64))
    d_n, d_off, d_order = dev(n_each), dev(offset), dev(order)
    trace = engine.Trace(0, 0, _views=(d[3], d[4], d[5]))
    s = hip.Stream()
    engine.dev_solve_ragged_mid(d[0], d_n, d_off, d_order, tiers, next_t=d[1], hops_t=d[2], trace=trace, updates_t=upd,
                                stream=s)
    items = [(b, i, j) for b, ref in enumerate(refs) for i, j in _pairs(ref, sample_seed=2)[-SAMPLE:]]
    items += [(1, 300, 0), (count, 0, 0), (-1, 0, 0)]
    cap = LONGEST + 2
    mat, src, dst = (dev(np.ascontiguousarray([it[f] for it in items], dtype=np.int32)) for f in range(3))
    len_t, path_t = engine.dev_exact_paths_ragged_mid(next0, d_n, d_off, 256, trace, mat, src, dst, cap, stream=s)
    s.synchronize()
    for f, field in enumerate(("rate", "next", "hops", "last", "at_col", "at_row")):
        assert_bits_equal(host(d[f]), expect[f], "device forms %s %s" % (_name(dtype), field))
    assert [int(u) for u in host(upd)] == [5 + int(r.solved[3]) for r in refs]
    lens, paths = host(len_t), host(path_t)
    assert [int(v) for v in lens[-3:]] == [FWX_ERR_INVALID] * 3
    got = (0, None, None, None, None, lens[:-3], paths[:-3])
    _check_lists(refs, items[:-3], got, "device walk %s" % _name(dtype))
    s.close()


# ---- 3. items, capacity, chunks -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_items_valid_for_n_max_but_not_for_their_matrix_are_refused_alone(dtype, monkeypatch):
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    refs = _mixed_refs(_name(dtype))
    good = [(1, 255, 0), (3, 128, 1), (0, 2, 0), (6, 191, 5), (9, 144, 144), (7, 63, 1)]
    bad = [(3, 129, 0), (0, 3, 0), (6, 0, 192), (9, 255, 255), (7, 64, 0), (2, 16, 16), (len(refs), 0, 0), (1, 256, 0),
           (1, 0, -1)]
    items = [x for pair in zip(good + good[:3], bad) for x in pair]
    got = _raw(refs, items, LONGEST + 2)
    assert got[0] == 0
    _check_solution(refs, got, "bad items %s" % _name(dtype))
    for q, (b, i, j) in enumerate(items):
        if (b, i, j) in bad:
            assert int(got[5][q]) == FWX_ERR_INVALID, (q, b, i, j, int(got[5][q]))
        else:
            w = refs[b].path(i, j)
            assert int(got[5][q]) == len(w) and tuple(got[6][q, :len(w)].tolist()) == w, (q, b, i, j)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_capacity_rule_at_the_longest_list_of_the_256_matrix(dtype, monkeypatch):
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    refs = _mixed_refs(_name(dtype))
    ref = refs[1]
    assert ref.n == 256
    i, j = (int(v) for v in np.unravel_index(int(np.argmax(ref.lengths)), (256, 256)))
    L = ref.longest
    assert L >= 2 and int(ref.lengths[i, j]) == L
    assert ref.path(0, 0) == ()
    items = [(1, i, j), (1, 0, 0), (7, 1, 0)]
    want = [refs[m].path(s, d) for m, s, d in items]
    for cap in (L, L - 1):
        st, _, _, _, _, lens, paths = _raw(refs, items, cap)
        assert st == 0
        for q, w in enumerate(want):
            got = (int(lens[q]), tuple(paths[q, :max(int(lens[q]), 0)].tolist()))
            expect = (len(w), w) if cap >= len(w) else (FWX_ERR_CAPACITY, ())
            assert got == expect, "cap %d item %d %r: %r, expected %r" % (cap, q, items[q], got[0], expect[0])
    st, _, _, _, _, lens, _ = _raw(refs, [(1, 0, 0)], 1)
    assert st == 0 and int(lens[0]) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_chunked_walk_gives_the_same_answer(dtype, monkeypatch):
    """FWX_BATCH_LISTS_CHUNK=7 walks 100 items in fifteen launches: the same lengths and lists."""
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    refs = _mixed_refs(_name(dtype))
    rnd = np.random.default_rng(8822)
    mats = rnd.integers(0, len(refs), 100)
    items = [(int(b), int(rnd.integers(0, refs[b].n)), int(rnd.integers(0, refs[b].n))) for b in mats]
    cap = LONGEST + 2
    monkeypatch.delenv("FWX_BATCH_LISTS_CHUNK", raising=False)
    assert _lib.lib().fwx_test_batch_lists_chunk(256, cap) >= 100
    whole = _raw(refs, items, cap)
    monkeypatch.setenv("FWX_BATCH_LISTS_CHUNK", "7")
    assert _lib.lib().fwx_test_batch_lists_chunk(256, cap) == 7
    chunked = _raw(refs, items, cap)
    assert whole[0] == 0 and chunked[0] == 0
    _check_solution(refs, chunked, "chunked")
    assert np.array_equal(whole[5], chunked[5])
    _check_lists(refs, items, whole, "whole")
    _check_lists(refs, items, chunked, "chunked")


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_python_binding(dtype, monkeypatch):
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    refs = _mixed_refs(_name(dtype))
    mats = [[getattr(r, f).copy() for r in refs] for f in ("rate", "next", "hops")]
    some = ([1, 3, 0, 9], [255, 0, 2, 5], [0, 128, 1, 5])
    lists, us = engine.solve_ragged_mid_lists(mats[0], mats[1], mats[2], items=some, count_updates=True)
    assert lists == [refs[m].path(s, d) for m, s, d in zip(*some)]
    assert [int(u) for u in us] == [int(r.solved[3]) for r in refs]
    for b, ref in enumerate(refs):
        for f, field in enumerate(("rate", "next", "hops")):
            assert_bits_equal(mats[f][b], ref.solved[f], "binding matrix %d %s" % (b, field))
    with pytest.raises(engine.FwxError) as e:
        engine.solve_ragged_lists([r.rate.copy() for r in refs], [r.next.copy() for r in refs], items=some)
    assert e.value.status == _lib.FWX_ERR_UNSUPPORTED
