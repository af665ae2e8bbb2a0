"""Ragged batched small solves with the reference's exact `_path` lists (fwx_solve_ragged_lists_f64 / _f32,
fwx_dev_solve_ragged with a trace + fwx_dev_exact_paths_ragged): matrices of different orders in one call, every one
bit for bit what the oracle's loop leaves of it and every list, list for list, what the rope oracle
(oracle.list_ropes.solve) gives for that matrix alone.

Inputs (the one-matrix reference objects and the market / hostile generators are those of
tests/test_gpu_batch_lists.py).  The main batch holds, at each of the orders 4, 5, 16, 17, 64, 65 and 128, a market
matrix (exact ties: lists that are not the walk of the final next-hops), a synthetic one -- kinds cycling d1, t2, t1,
d2, t3, the first seed whose matrix has work in it and whose longest list stays within MAX_LIST, by the oracle alone
-- and a hostile draw, in a seeded shuffle.  All n^2 pairs are asked at orders <= 17, 2048 seeded pairs per matrix
above, grouped into capacity classes by the ORACLE's length as the uniform test does.  Every case asserts its
preconditions from the oracle before any GPU call; the oracle side of an input is computed once and shared."""
import ctypes
import functools

import numpy as np
import pytest

import oracle
from floydwarshall_amd import _lib, engine, synth
from floydwarshall_amd._lib import FWX_ERR_CAPACITY, FWX_ERR_INVALID

from helpers import assert_bits_equal, dev, host
from test_gpu_batch_lists import CAP_CLASSES, KINDS, MAX_LIST, _hostile_refs, _market_ref, _Ref

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
ORDERS = [4, 5, 16, 17, 64, 65, 128]
PAIRS_ABOVE_17 = 2048


def _name(dtype):
    return np.dtype(dtype).name


def _synth_ref(kind, n, dtype, seed):
    """The first seed at or after `seed` whose matrix the oracle relaxes and whose longest list is <= MAX_LIST."""
    for s in range(seed, seed + 64):
        ref = _Ref(*synth.make(kind, n, dtype, seed=s))
        if ref.longest <= MAX_LIST and ref.ropes.updates > 0:
            return ref
    raise AssertionError("no usable seed for kind %s order %d" % (kind, n))


def _offsets(refs):
    return np.concatenate([[0], np.cumsum([r.n * r.n for r in refs])]).astype(np.int64)


def _packed(refs, field, solved=False):
    pick = (lambda r: r.solved[("rate", "next", "hops").index(field)]) if solved else (lambda r: getattr(r, field))
    return np.concatenate([pick(r).reshape(-1) for r in refs])


class _Empty:
    """An order-0 matrix of a batch: no cells, no lists."""
    n, longest = 0, 0

    def __init__(self, dtype):
        self.rate = np.zeros((0, 0), dtype=dtype)
        self.next = self.hops = np.zeros((0, 0), dtype=np.int32)
        self.solved = (self.rate, self.next, self.hops, 0)


@functools.lru_cache(maxsize=None)
def _main_batch(dtype_name):
    """(refs, items): three matrices per order -- market, synthetic, hostile -- shuffled."""
    dtype = np.dtype(dtype_name).type
    refs = []
    for i, n in enumerate(ORDERS):
        refs.append(_market_ref(n, dtype_name))
        refs.append(_synth_ref(KINDS[i % len(KINDS)], n, dtype, synth.BASE_SEED + 8000 + 100 * i))
        refs.append(_hostile_refs(n, dtype_name)[i % 16])
    assert "t3" in [KINDS[i % len(KINDS)] for i in range(len(ORDERS))]
    refs = [refs[int(b)] for b in np.random.default_rng(41).permutation(len(refs))]
    assert max(r.longest for r in refs) <= MAX_LIST
    rnd = np.random.default_rng(4100)
    items = []
    for b, r in enumerate(refs):
        if r.n <= 17:
            items += [(b, i, j) for i in range(r.n) for j in range(r.n)]
        else:
            items += [(b, int(i), int(j)) for i, j in zip(rnd.integers(0, r.n, PAIRS_ABOVE_17),
                                                          rnd.integers(0, r.n, PAIRS_ABOVE_17))]
    return tuple(refs), tuple(items)


def _a_list_that_is_not_the_walk(ref):
    """The first (src, dst) whose list differs from the walk of the final next-hops, or None; the oracle alone."""
    en = ref.ropes.next
    for s in range(ref.n):
        for d in range(ref.n):
            walk = oracle.follow_path(en, s, d)
            if walk is None or tuple(walk) != ref.path(s, d):
                return s, d
    return None


def _raw(refs, items, cap, with_hops=True, each=True):
    """One call of the host form as the C caller sees it, on packed arrays: (status, rate, next, hops, [U_b], lens,
    paths)."""
    rate, nxt, hops = (_packed(refs, f) for f in ("rate", "next", "hops"))
    hops = hops if with_hops else None
    n_each = np.array([r.n for r in refs], dtype=np.int32)
    mat, src, dst = (np.ascontiguousarray([it[f] for it in items], dtype=np.int32) for f in range(3))
    lens = np.full(len(items), -99, dtype=np.int32)
    paths = np.full((max(len(items), 1), cap), -7, dtype=np.int32)
    us = np.full(len(refs), 99, dtype=np.uint64) if each else None
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    fn = _lib.lib().fwx_solve_ragged_lists_f64 if rate.dtype == np.float64 else _lib.lib().fwx_solve_ragged_lists_f32
    st = fn(len(refs), p(n_each), p(rate), p(nxt), p(hops), p(us), len(items), p(mat), p(src), p(dst), p(lens),
            p(paths), cap, None)
    return st, rate, nxt, hops, None if us is None else [int(u) for u in us], lens, paths


def _check_solution(refs, got, what, with_hops=True):
    """The packed arrays, compared whole, and U per matrix."""
    _, rate, nxt, hops, us, _, _ = got
    assert_bits_equal(rate, _packed(refs, "rate", True), "%s packed rate" % what)
    assert_bits_equal(nxt, _packed(refs, "next", True), "%s packed next" % what)
    if with_hops:
        assert_bits_equal(hops, _packed(refs, "hops", True), "%s packed hops" % what)
    assert us == [r.solved[3] for r in refs], "%s: U per matrix" % what


def _classes(refs, items):
    """The items grouped by capacity class of the oracle's length: [(cap, [index into items])]."""
    want_len = np.array([int(refs[b].lengths[i, j]) for b, i, j in items], dtype=np.int64)
    assert int(want_len.max(initial=0)) <= MAX_LIST
    out, lo = [], -1
    for hi in CAP_CLASSES:
        sel = np.nonzero((want_len > lo) & (want_len <= hi))[0]
        lo = hi
        if len(sel):
            out.append((hi + 2, sel))
    assert sum(len(sel) for _, sel in out) == len(items)
    return out


def _differing(refs, part, lens, paths):
    bad = []
    for q, (b, i, j) in enumerate(part):
        want = refs[b].path(i, j)
        if int(lens[q]) != len(want) or tuple(paths[q, :len(want)].tolist()) != want:
            bad.append((b, i, j, int(lens[q]), len(want)))
    return bad


def _ask_host(refs, items, what, with_hops=True):
    bad, first = [], True
    for cap, sel in _classes(refs, items):
        part = [items[q] for q in sel]
        got = _raw(refs, part, cap, with_hops)
        assert got[0] == 0, got[0]
        if first:
            _check_solution(refs, got, what, with_hops)
            first = False
        bad += _differing(refs, part, got[5], got[6])
    assert not bad, "%s: %d lists differ, first (matrix, src, dst, length or status, oracle's length) %r" % (
        what, len(bad), bad[0])


def _ask_device(refs, items, what):
    """fwx_dev_solve_ragged with a trace, once, then fwx_dev_exact_paths_ragged per capacity class."""
    n_each = np.array([r.n for r in refs], dtype=np.int32)
    offset, order, tiers = engine.ragged_plan(n_each)
    cells = int(offset[-1])
    d = [dev(_packed(refs, f)) for f in ("rate", "next", "hops")]
    next0 = dev(_packed(refs, "next"))
    tr = [dev(np.full(cells, 0x5A5A5A5A, dtype=np.int32)) for _ in range(3)]
    trace = engine.Trace(0, 0, _views=tuple(tr))
    upd = dev(np.zeros(len(refs), dtype=np.uint64))
    d_n, d_off, d_order = dev(n_each), dev(offset[:-1]), dev(order)
    engine.dev_solve_ragged(d[0], d_n, d_off, d_order, tiers, next_t=d[1], hops_t=d[2], trace=trace, updates_t=upd)
    got = (0, host(d[0]), host(d[1]), host(d[2]), [int(u) for u in host(upd)], None, None)
    _check_solution(refs, got, what)
    bad = []
    for cap, sel in _classes(refs, items):
        part = [items[q] for q in sel]
        mat, src, dst = (dev(np.ascontiguousarray([it[f] for it in part], dtype=np.int32)) for f in range(3))
        len_t, path_t = engine.dev_exact_paths_ragged(next0, d_n, d_off, int(n_each.max()), trace, mat, src, dst, cap)
        bad += _differing(refs, part, host(len_t), host(path_t))
    assert not bad, "%s: %d lists differ, first %r" % (what, len(bad), bad[0])


# ---- 1. lists against the rope oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("wave", ["16", "0"])
@pytest.mark.parametrize("form", ["host", "device"])
def test_lists_of_a_mixed_batch(form, wave, dtype, monkeypatch):
    monkeypatch.setenv("FWX_BATCH_WAVE_MAX_N", wave)
    refs, items = _main_batch(_name(dtype))
    assert sorted(r.n for r in refs) == sorted(ORDERS * 3)
    for b, r in enumerate(refs):
        assert r.ropes.updates > 0, "the oracle relaxes nothing in matrix %d" % b
    # at least one list per tier that is not the walk of the final next-hops (the market matrices have them)
    for tier_orders in ([4, 5, 16], [17, 64], [65, 128]):
        assert any(_a_list_that_is_not_the_walk(_market_ref(n, _name(dtype))) is not None for n in tier_orders)
    what = "mixed batch %s wave<=%s %s" % (form, wave, _name(dtype))
    if form == "host":
        _ask_host(refs, list(items), what)
    else:
        _ask_device(refs, list(items), what)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_python_binding_all_pairs_and_growing_cap(dtype, monkeypatch):
    """engine.solve_ragged_lists: items=None is every pair of every matrix in (b, i, j) order; cap=None grows until
    every list fits (started at 1 here so that it has to); the matrices come back solved in place."""
    monkeypatch.delenv("FWX_BATCH_WAVE_MAX_N", raising=False)
    monkeypatch.setattr(engine, "BATCH_LISTS_FIRST_CAP", 1)
    name = _name(dtype)
    refs = [_market_ref(5, name), _Empty(dtype), _market_ref(17, name), _market_ref(4, name), _market_ref(16, name)]
    assert max(r.longest for r in refs) >= 2                       # the first cap is too small
    rates, nexts, hops = ([getattr(r, f).copy() for r in refs] for f in ("rate", "next", "hops"))
    lists, us = engine.solve_ragged_lists(rates, nexts, hops, count_updates=True)
    assert [int(u) for u in us] == [r.solved[3] for r in refs]
    for b, r in enumerate(refs):
        for got, f in zip((rates[b], nexts[b], hops[b]), range(3)):
            assert_bits_equal(got, r.solved[f], "binding matrix %d field %d" % (b, f))
    assert lists == [r.path(i, j) for r in refs for i in range(r.n) for j in range(r.n)]
    longest = max(r.longest for r in refs)
    with pytest.raises(engine.FwxError) as e:                      # an explicit cap is not grown
        engine.solve_ragged_lists([r.rate.copy() for r in refs], [r.next.copy() for r in refs], cap=longest - 1)
    assert e.value.status == FWX_ERR_CAPACITY
    some = ([4, 0, 2], [1, 0, 16], [0, 4, 1])
    got = engine.solve_ragged_lists([r.rate.copy() for r in refs], [r.next.copy() for r in refs], items=some,
                                    cap=longest)
    assert got == [refs[b].path(i, j) for b, i, j in zip(*some)]


# ---- 2. per-item errors ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small_batch(dtype_name):
    dtype = np.dtype(dtype_name).type
    return (_market_ref(4, dtype_name), _Empty(dtype), _market_ref(17, dtype_name), _market_ref(65, dtype_name),
            _hostile_refs(5, dtype_name)[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("wave", ["16", "0"])
def test_bad_items_are_refused_alone(wave, dtype, monkeypatch):
    """src / dst are checked against the order of the item's OWN matrix: an index that a larger matrix of the batch
    has is refused; so are mat outside the batch and any item of an order-0 matrix.  The others are answered."""
    monkeypatch.setenv("FWX_BATCH_WAVE_MAX_N", wave)
    refs = _small_batch(_name(dtype))
    count = len(refs)
    assert [r.n for r in refs] == [4, 0, 17, 65, 5]
    good = [(0, 1, 2), (3, 64, 0), (2, 16, 1), (4, 0, 4), (3, 5, 64), (0, 3, 0), (2, 0, 16), (4, 4, 1)]
    bad = [(0, 4, 1), (0, 1, 16), (2, 17, 0), (2, 3, 64), (4, 5, 0), (4, 0, 64),      # valid for a larger matrix only
           (3, 65, 0), (3, 0, -1), (-1, 0, 1), (count, 0, 1), (1, 0, 0), (1, -1, 0)]  # ..., mat outside, order 0
    items = [x for pair in zip((good + good)[:len(bad)], bad) for x in pair]         # good, bad, good, bad, ...
    cap = max(r.longest for r in refs) + 2
    got = _raw(refs, items, cap)
    assert got[0] == 0
    _check_solution(refs, got, "bad items")
    for q, (b, i, j) in enumerate(items):
        if (b, i, j) in bad:
            assert int(got[5][q]) == FWX_ERR_INVALID, (q, b, i, j, int(got[5][q]))
        else:
            w = refs[b].path(i, j)
            assert int(got[5][q]) == len(w) and tuple(got[6][q, :len(w)].tolist()) == w, (q, b, i, j)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_capacity_rule_item_by_item(dtype, monkeypatch):
    """cap >= L returns the list, L > cap is FWX_ERR_CAPACITY for that item alone, an empty list fits cap 1: a list of
    two or more entries from each non-empty matrix and an empty list, all in one call."""
    monkeypatch.delenv("FWX_BATCH_WAVE_MAX_N", raising=False)
    refs = _small_batch(_name(dtype))
    items = []
    for b, r in enumerate(refs):
        pick = [(b, i, j) for i in range(r.n) for j in range(r.n) if i != j and int(r.lengths[i, j]) >= 2][:1]
        assert pick or r.n == 0, b
        items += pick
    empty = [(b, i, j) for b, r in enumerate(refs) for i in range(r.n) for j in range(r.n)
             if i != j and int(r.lengths[i, j]) == 0][:1]
    assert len(items) == 4 and len(empty) == 1
    items += empty
    want = [refs[b].path(i, j) for b, i, j in items]
    caps = sorted({len(w) + d for w in want[:-1] for d in (-1, 0, 1)} | {1})
    for cap in caps:
        st, _, _, _, _, lens, paths = _raw(refs, items, cap)
        assert st == 0
        for q, w in enumerate(want):
            got = (int(lens[q]), tuple(paths[q, :max(int(lens[q]), 0)].tolist()))
            expect = (len(w), w) if cap >= len(w) else (FWX_ERR_CAPACITY, ())
            assert got == expect, "cap %d item %d %r: %r, expected %r" % (cap, q, items[q], got, expect)


# ---- 3. chunking -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_chunked_walk_gives_the_same_answer(dtype, monkeypatch):
    """FWX_BATCH_LISTS_CHUNK = 1 and = 3 walk 40 items in forty and fourteen launches: the same lengths and lists."""
    monkeypatch.delenv("FWX_BATCH_WAVE_MAX_N", raising=False)
    refs = _small_batch(_name(dtype))
    rnd = np.random.default_rng(8900)
    items = []
    while len(items) < 40:
        b = int(rnd.integers(0, len(refs)))
        if refs[b].n:
            items.append((b, int(rnd.integers(0, refs[b].n)), int(rnd.integers(0, refs[b].n))))
    cap = max(r.longest for r in refs) + 2
    n_max = max(r.n for r in refs)
    monkeypatch.delenv("FWX_BATCH_LISTS_CHUNK", raising=False)
    assert _lib.lib().fwx_test_batch_lists_chunk(n_max, cap) >= 40
    whole = _raw(refs, items, cap)
    assert whole[0] == 0
    _check_solution(refs, whole, "one chunk")
    assert not _differing(refs, items, whole[5], whole[6])
    for chunk in ("1", "3"):
        monkeypatch.setenv("FWX_BATCH_LISTS_CHUNK", chunk)
        assert _lib.lib().fwx_test_batch_lists_chunk(n_max, cap) == int(chunk)
        got = _raw(refs, items, cap)
        assert got[0] == 0
        _check_solution(refs, got, "chunk " + chunk)
        assert np.array_equal(whole[5], got[5])
        assert not _differing(refs, items, got[5], got[6])
