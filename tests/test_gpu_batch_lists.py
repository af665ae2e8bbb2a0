"""Batched small solves with the reference's exact `_path` lists (fwx_solve_batch_lists_f64 / _f32,
fwx_dev_solve_batch_traced + fwx_dev_exact_paths_batch): every matrix of a batch bit for bit what the oracle's loop
(oracle.relax) leaves of it -- rates, next, hops, U -- and every list, list for list, what the rope oracle
(oracle.list_ropes.solve, pinned to the list-faithful restatement by tests/test_oracle_ropes.py) gives for that
matrix alone.

Two tiers keep the trace: one wave per matrix (n <= FWX_BATCH_WAVE_MAX_N <= 16, the trace in four registers per lane)
and small_solve's body with one workgroup per matrix.  FWX_BATCH_WAVE_MAX_N = 16 / 0 puts the same input through both.

Inputs.  Synthetic batches cycle the kinds d1, t2, t1, d2, t3 so that neighbours differ; matrix b takes the first
seed, ascending from one counter, whose matrix has work in it (the ORACLE's U > 0 at n >= 4) and whose longest list
stays within MAX_LIST (t3 has arbitrage: its lists can double per pivot) -- decided by the oracle alone.  Market
matrices are built as tests/test_gpu_exact_lists_edges.py builds them (exact ties: lists that are not the walk of
the final next-hops).  Hostile batches are sixteen draws of hostile_matrix_mix from default_rng(HOSTILE_SEED[n]).
Every case asserts its preconditions from the oracle before any GPU call; the oracle side of an input is computed
once and shared.

How the lists are asked for.  cap is one number per call, so a call over all n^2 pairs of sixteen matrices with one
4096-entry list among them would move gigabytes of mostly empty capacity.  _ask therefore groups the items by the
ORACLE's length into a few capacity classes and makes one call of the host form per class (each call solves the
batch again from the input, which is what the entry point does); the first call's arrays and counters are the ones
compared.  Every item still gets cap >= its length; the capacity rule itself has its own case."""
import ctypes
import functools

import numpy as np
import pytest

import oracle
from floydwarshall_amd import _lib, engine, synth
from floydwarshall_amd._lib import FWX_ERR_CAPACITY, FWX_ERR_INVALID
from oracle import list_faithful as lf
from oracle import list_ropes

from helpers import assert_bits_equal, dev, host
from hostile_inputs import hostile_matrix_mix, market_rates

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
KINDS = ("d1", "t2", "t1", "d2", "t3")
MAX_LIST = 4096
CAP_CLASSES = (8, 64, 512, MAX_LIST)
CALL_INTS = 1 << 23                  # list capacity moved per call of the host form, in int32
WAVE_ORDERS = [1, 2, 3, 4, 5, 15, 16]
WORKGROUP_ORDERS = [17, 63, 64, 65, 127, 128]
ORDER_TIERS = [(n, w) for n in WAVE_ORDERS for w in ("16", "0")] + [(n, "16") for n in WORKGROUP_ORDERS]
# default_rng seed of the sixteen hostile draws of order n: 7100 + n, or the next seed whose batch shows all three
# facts of _facts (decided by the oracle alone, see test_hostile_batches; none had to move)
HOSTILE_SEED = {4: 7104, 5: 7105, 15: 7115, 16: 7116, 17: 7117, 64: 7164, 65: 7165, 128: 7228}


def _name(dtype):
    return np.dtype(dtype).name


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


class _Ref:
    """One matrix: the input, the dense oracle's solution and U, the ropes; lists on demand, each computed once."""

    def __init__(self, rate, nxt, hops):
        self.rate, self.next, self.hops = _frozen(*(np.ascontiguousarray(a) for a in (rate, nxt, hops)))
        self.n = rate.shape[0]
        self.ropes = list_ropes.solve(self.rate, self.next)
        self.lengths = self.ropes.lengths
        self.longest = int(self.lengths.max(initial=0))
        self._solved = None
        self._lists = {}

    @property
    def solved(self):
        """(rate, next, hops, U) of oracle.relax, checked against the ropes."""
        if self._solved is None:
            er, en, eh = self.rate.copy(), self.next.copy(), self.hops.copy()
            eu = oracle.relax(er, en, eh)
            assert_bits_equal(self.ropes.rate, er, "ropes vs dense loop: rate")
            assert_bits_equal(self.ropes.next, en, "ropes vs dense loop: next")
            assert self.ropes.updates == eu
            self._solved = _frozen(er, en, eh) + (eu,)
        return self._solved

    def path(self, s, d):
        key = (int(s), int(d))
        if key not in self._lists:
            self._lists[key] = self.ropes.path(*key)
        return self._lists[key]


def _facts(ref):
    """(lists that are not the walk of the final next-hops, updates with an empty ikPath, off-diagonal entries with a
    positive rate and an empty list) -- from the oracle alone, as tests/test_gpu_exact_lists_edges.py counts them."""
    n, en = ref.n, ref.ropes.next
    differ = 0
    for s in range(n):
        for d in range(n):
            walk = oracle.follow_path(en, s, d)
            differ += walk is None or tuple(walk) != ref.path(s, d)
    off = ~np.eye(n, dtype=bool)
    with np.errstate(invalid="ignore"):
        positive_empty = int(((ref.ropes.rate > 0) & (ref.lengths == 0) & off).sum())
    return differ, ref.ropes.updates_empty_left, positive_empty


@functools.lru_cache(maxsize=None)
def _synth_refs(n, count, dtype_name):
    """Matrix b: kind KINDS[b % 5], the first seed at or after the previous matrix's + 1 that has U > 0 (n >= 4) and
    no list longer than MAX_LIST."""
    dtype = np.dtype(dtype_name).type
    refs, seed = [], synth.BASE_SEED + 3000 + n
    while len(refs) < count:
        assert seed < synth.BASE_SEED + 3000 + n + 8 * count + 64, "no usable seed for matrix %d" % len(refs)
        ref = _Ref(*synth.make(KINDS[len(refs) % len(KINDS)], n, dtype, seed=seed))
        seed += 1
        if ref.longest <= MAX_LIST and (n < 4 or ref.ropes.updates > 0):
            refs.append(ref)
    return tuple(refs)


@functools.lru_cache(maxsize=None)
def _market_ref(n, dtype_name):
    """The leading n vertices of a market of 8 currencies: _input("market", ...) of the edge test."""
    dtype = np.dtype(dtype_name).type
    n_ccy = 8
    n_exch = -(-n // n_ccy) + 1
    m0 = lf.build_matrix(market_rates(n_exch, n_ccy, seed=23 + n), dtype)
    assert len(m0) >= n
    _, rate, nxt, hops = lf.to_dense(m0, dtype)
    return _Ref(*(np.ascontiguousarray(a[:n, :n]) for a in (rate, nxt, hops)))


@functools.lru_cache(maxsize=None)
def _hostile_refs(n, dtype_name, draws=16):
    dtype = np.dtype(dtype_name).type
    rnd = np.random.default_rng(HOSTILE_SEED[n])
    return tuple(_Ref(*hostile_matrix_mix(rnd, n, dtype)[:3]) for _ in range(draws))


def _stack(refs):
    return tuple(np.ascontiguousarray(np.stack([getattr(r, f) for r in refs])) for f in ("rate", "next", "hops"))


def _all_items(refs, which=None):
    n = refs[0].n
    return [(b, i, j) for b in (range(len(refs)) if which is None else which) for i in range(n) for j in range(n)]


def _raw(refs, items, cap, with_hops=True, each=True):
    """One call of the host form as the C caller sees it: (status, rate, next, hops, [U_b], lens, paths)."""
    rate, nxt, hops = _stack(refs)
    hops = hops if with_hops else None
    count, n = rate.shape[0], rate.shape[1]
    mat, src, dst = (np.ascontiguousarray([it[f] for it in items], dtype=np.int32) for f in range(3))
    lens = np.full(len(items), -99, dtype=np.int32)
    paths = np.full((max(len(items), 1), cap), -7, dtype=np.int32)
    us = np.full(count, 99, dtype=np.uint64) if each else None
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    fn = _lib.lib().fwx_solve_batch_lists_f64 if rate.dtype == np.float64 else _lib.lib().fwx_solve_batch_lists_f32
    st = fn(count, n, p(rate), p(nxt), p(hops), p(us), len(items), p(mat), p(src), p(dst), p(lens), p(paths), cap, None)
    return st, rate, nxt, hops, None if us is None else [int(u) for u in us], lens, paths


def _check_solution(refs, got, what, with_hops=True):
    _, rate, nxt, hops, us, _, _ = got
    for b, ref in enumerate(refs):
        er, en, eh, eu = ref.solved
        assert_bits_equal(rate[b], er, "%s matrix %d rate" % (what, b))
        assert_bits_equal(nxt[b], en, "%s matrix %d next" % (what, b))
        if with_hops:
            assert_bits_equal(hops[b], eh, "%s matrix %d hops" % (what, b))
        assert us[b] == eu, "%s matrix %d: U %d, the oracle's %d" % (what, b, us[b], eu)


def _ask(refs, items, what, with_hops=True):
    """The lists of `items` through the host form, grouped by capacity class (module docstring); the solution of the
    first call is checked against the dense oracle.  Every list is compared with the ropes'."""
    want_len = np.array([int(refs[b].lengths[i, j]) for b, i, j in items], dtype=np.int64)
    assert int(want_len.max(initial=0)) <= MAX_LIST
    bad, first, lo = [], True, -1
    for hi in CAP_CLASSES:
        sel = np.nonzero((want_len > lo) & (want_len <= hi))[0]
        lo = hi
        cap = hi + 2
        step = max(CALL_INTS // cap, 1)
        for c0 in range(0, len(sel), step):
            part = [items[q] for q in sel[c0:c0 + step]]
            got = _raw(refs, part, cap, with_hops)
            assert got[0] == 0, got[0]
            if first:
                _check_solution(refs, got, what, with_hops)
                first = False
            lens, paths = got[5], got[6]
            for q, (b, i, j) in enumerate(part):
                want = refs[b].path(i, j)
                if int(lens[q]) != len(want) or tuple(paths[q, :len(want)].tolist()) != want:
                    bad.append((b, i, j, int(lens[q]), len(want)))
    assert not first or not items
    assert not bad, "%s: %d lists differ, first (matrix, src, dst, length or status, oracle's length) %r" % (
        what, len(bad), bad[0])


def _not_vacuous(refs):
    if refs[0].n >= 4:
        for b, ref in enumerate(refs):
            assert ref.ropes.updates > 0, "the oracle relaxes nothing in matrix %d" % b


# ---- 1. orders, tiers, fields ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n,wave", ORDER_TIERS)
def test_orders_tiers_and_fields(n, wave, dtype, monkeypatch):
    """Every order at which a tile, a row group or a tier changes, with and without hops: all n^2 lists of every
    matrix."""
    monkeypatch.setenv("FWX_BATCH_WAVE_MAX_N", wave)
    refs = _synth_refs(n, 2 if n >= 127 else 5, _name(dtype))
    _not_vacuous(refs)
    items = _all_items(refs)
    for with_hops in (True, False):
        _ask(refs, items, "n=%d wave<=%s %s hops=%s" % (n, wave, _name(dtype), with_hops), with_hops)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n,wave", [(5, "16"), (16, "16"), (16, "0"), (17, "16")])
def test_python_binding_all_pairs_and_growing_cap(n, wave, dtype, monkeypatch):
    """engine.solve_batch_lists: items=None is every pair of every matrix in (b, i, j) order; cap=None grows until
    every list fits (started at 1 here so that it has to); the arrays come back solved in place."""
    monkeypatch.setenv("FWX_BATCH_WAVE_MAX_N", wave)
    monkeypatch.setattr(engine, "BATCH_LISTS_FIRST_CAP", 1)
    refs = _synth_refs(n, 5, _name(dtype))
    _not_vacuous(refs)
    assert max(r.longest for r in refs) >= 2                       # the first cap is too small
    rate, nxt, hops = _stack(refs)
    lists, us = engine.solve_batch_lists(rate, nxt, hops, count_updates=True)
    _check_solution(refs, (0, rate, nxt, hops, [int(u) for u in us], None, None), "binding n=%d" % n)
    assert lists == [refs[b].path(i, j) for b, i, j in _all_items(refs)]
    longest = max(r.longest for r in refs)
    with pytest.raises(engine.FwxError) as e:                      # an explicit cap is not grown
        engine.solve_batch_lists(*_stack(refs), cap=longest - 1)
    assert e.value.status == FWX_ERR_CAPACITY
    some = ([4, 0, 2], [1, 0, n - 1], [0, n - 1, 1])
    got = engine.solve_batch_lists(*_stack(refs), items=some, cap=longest)
    assert got == [refs[b].path(i, j) for b, i, j in zip(*some)]


# ---- 2. ties ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n,wave", [(16, "16"), (16, "0"), (64, "16"), (128, "16")])
def test_market_ties_inside_a_batch(n, wave, dtype, monkeypatch):
    """The reference's own kind of graph between two other kinds: its lists are not the next-hop walk."""
    monkeypatch.setenv("FWX_BATCH_WAVE_MAX_N", wave)
    market = _market_ref(n, _name(dtype))
    others = _synth_refs(n, 2, _name(dtype))
    differ = _facts(market)[0]
    print("market n=%d %s: %d of %d lists differ from the next-hop walk" % (n, _name(dtype), differ, n * n))
    assert differ >= 1
    refs = (others[0], market, others[1])
    _not_vacuous(refs)
    _ask(refs, _all_items(refs), "market n=%d wave<=%s %s" % (n, wave, _name(dtype)))


# ---- 3. outside the domain ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n,wave", [(n, w) for n in (4, 5, 15, 16) for w in ("16", "0")]
                         + [(17, "16"), (64, "16"), (65, "16"), (128, "16")])
def test_hostile_batches(n, wave, dtype, monkeypatch):
    """Sixteen draws outside the domain as one batch (the first four at n = 128): no domain check, no routing, every
    list the reference's -- updates with an empty ikPath, positive rates with an empty list, leaves without an edge."""
    monkeypatch.setenv("FWX_BATCH_WAVE_MAX_N", wave)
    refs = _hostile_refs(n, _name(dtype))
    assert len(refs) == 16 and max(r.longest for r in refs) <= MAX_LIST            # none is left out
    if n == 128:
        refs = refs[:4]
    facts = [_facts(r) for r in refs]
    print("hostile n=%d %s: (differ, empty ikPath, positive and empty) per draw %r" % (n, _name(dtype), facts))
    if n <= 33:
        assert any(all(f) for f in facts), facts                   # one draw shows all three
    for which in range(3):
        assert any(f[which] for f in facts), (which, facts)        # each occurs somewhere in the batch
    _not_vacuous(refs)
    _ask(refs, _all_items(refs), "hostile n=%d wave<=%s %s" % (n, wave, _name(dtype)))


# ---- 4. counts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n,count", [(n, c) for n in (4, 16) for c in (1, 3, 5, 257)] + [(64, 257)])
def test_counts(n, count, dtype, monkeypatch):
    """A last wave-tier workgroup with 1 or 3 of its 4 waves in use; more workgroups than the chip has CUs."""
    monkeypatch.setenv("FWX_BATCH_WAVE_MAX_N", "16")
    refs = _synth_refs(n, count, _name(dtype))
    _not_vacuous(refs)
    if count == 257:
        rnd = np.random.default_rng(4400 + n)
        items = _all_items(refs, (0, count - 1)) + [
            (int(b), int(i), int(j)) for b, i, j in zip(rnd.integers(0, count, 2000), rnd.integers(0, n, 2000),
                                                       rnd.integers(0, n, 2000))]
    else:
        items = _all_items(refs)
    _ask(refs, items, "n=%d count=%d %s" % (n, count, _name(dtype)))


# ---- 5. stride and gaps, through the device forms ----------------------------------------------------------------
NAN_SENTINEL = {np.float64: np.uint64(0x7FF80000DEADBEEF), np.float32: np.uint32(0x7FC0BEEF)}
INT_SENTINEL = 0x5A5A5A5A            # no pivot, -1 included, equals it


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n,wave", [(4, "16"), (4, "0"), (16, "16"), (16, "0"), (17, "16"), (65, "16")])
def test_device_forms_with_a_stride(n, wave, dtype, monkeypatch):
    """fwx_dev_solve_batch_traced and fwx_dev_exact_paths_batch on caller-owned device memory, matrices n*n + 5
    elements apart: all six arrays are pre-filled with sentinels, the gaps come back untouched, every trace cell
    inside a matrix has been written, the counters are INCREMENTED, and the walk addresses by the same stride."""
    monkeypatch.setenv("FWX_BATCH_WAVE_MAX_N", wave)
    count, stride = 5, n * n + 5
    refs = _synth_refs(n, count, _name(dtype))
    _not_vacuous(refs)
    batch = _stack(refs)
    bits = np.uint64 if dtype == np.float64 else np.uint32
    flat = [np.full(count * stride, NAN_SENTINEL[dtype], dtype=bits).view(dtype)] + [
        np.full(count * stride, INT_SENTINEL, dtype=np.int32) for _ in range(5)]
    inside = np.zeros(count * stride, dtype=bool)
    for b in range(count):
        inside[b * stride:b * stride + n * n] = True
        for f in range(3):
            flat[f][b * stride:b * stride + n * n] = batch[f][b].reshape(-1)
    expect = [a.copy() for a in flat[:3]]
    for b, ref in enumerate(refs):
        for f in range(3):
            expect[f][b * stride:b * stride + n * n] = ref.solved[f].reshape(-1)
    d = [dev(a) for a in flat]
    next0 = dev(flat[1])
    upd = dev(np.full(count, 3, dtype=np.uint64))

    trace = engine.Trace(0, 0, _views=(d[3], d[4], d[5]))
    engine.dev_solve_batch_traced(d[0], count, n, trace, next_t=d[1], hops_t=d[2], stride=stride, updates_t=upd)
    items = _all_items(refs)
    cap = max(r.longest for r in refs) + 2
    mat, src, dst = (dev(np.ascontiguousarray([it[f] for it in items], dtype=np.int32)) for f in range(3))
    len_t, path_t = engine.dev_exact_paths_batch(next0, count, n, trace, mat, src, dst, cap, stride=stride)
    what = "n=%d wave<=%s %s" % (n, wave, _name(dtype))
    for f, field in enumerate(("rate", "next", "hops")):
        assert_bits_equal(host(d[f]), expect[f], "%s %s with gaps" % (what, field))
    assert [int(u) for u in host(upd)] == [3 + r.solved[3] for r in refs]
    for f, field in ((3, "last"), (4, "at_col"), (5, "at_row")):
        t = host(d[f])
        assert (t[~inside] == INT_SENTINEL).all(), "%s: the gap of %s was written" % (what, field)
        assert (t[inside] != INT_SENTINEL).all(), "%s: a cell of %s inside a matrix was not written" % (what, field)
        assert ((t[inside] >= -1) & (t[inside] < n)).all()
    lens, paths = host(len_t), host(path_t)
    bad = [(it, int(lens[q])) for q, it in enumerate(items)
           if int(lens[q]) != len(refs[it[0]].path(it[1], it[2]))
           or tuple(paths[q, :max(int(lens[q]), 0)].tolist()) != refs[it[0]].path(it[1], it[2])]
    assert not bad, "%s: %d lists differ, first %r" % (what, len(bad), bad[0])


# ---- 6. the capacity rule, item by item --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_capacity_rule_item_by_item(dtype):
    """cap >= L returns the list, L > cap is FWX_ERR_CAPACITY for that item alone: a list of two or more entries, a
    list of ONE entry that an update made (one half of its tree contributes nothing: a stack sized by cap would run
    out before the list does) and an empty list, all in one call."""
    n = 65
    refs = _hostile_refs(n, _name(dtype))
    found = {}
    for b, ref in enumerate(refs):
        updated = ref.ropes.node > n
        for i in range(n):
            for j in range(n):
                L = int(ref.lengths[i, j])
                if i != j and L >= 2 and "long" not in found:
                    found["long"] = (b, i, j)
                if i != j and L == 1 and updated[i, j] and "one" not in found:
                    found["one"] = (b, i, j)
                if i != j and L == 0 and "empty" not in found:
                    found["empty"] = (b, i, j)
    assert set(found) == {"long", "one", "empty"}, found
    items = [found["long"], found["one"], found["empty"]]
    want = [refs[b].path(i, j) for b, i, j in items]
    L = len(want[0])
    assert L >= 2 and len(want[1]) == 1 and want[2] == ()
    for cap in sorted({L + 1, L, L - 1, 1}):
        st, _, _, _, _, lens, paths = _raw(refs, items, cap)
        assert st == 0
        for q, w in enumerate(want):
            got = (int(lens[q]), tuple(paths[q, :max(int(lens[q]), 0)].tolist()))
            expect = (len(w), w) if cap >= len(w) else (FWX_ERR_CAPACITY, ())
            assert got == expect, "cap %d item %d %r: %r, expected %r" % (cap, q, items[q], got, expect)


# ---- 7. bad items -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n,wave", [(16, "16"), (65, "16")])
def test_bad_items_are_refused_alone(n, wave, dtype, monkeypatch):
    monkeypatch.setenv("FWX_BATCH_WAVE_MAX_N", wave)
    count = 3
    refs = _synth_refs(n, count, _name(dtype))
    good = [(0, 1, 2), (2, n - 1, 0), (1, 3, 1), (2, 0, n - 1)]
    bad = [(count, 0, 1), (0, n, 1), (0, 1, -1), (-1, 0, 1), (1, -1, 0), (1, 0, n)]
    items = [x for pair in zip(good + good[:2], bad) for x in pair]      # good, bad, good, bad, ...
    cap = max(r.longest for r in refs) + 2
    got = _raw(refs, items, cap)
    assert got[0] == 0
    _check_solution(refs, got, "bad items n=%d" % n)
    for q, (b, i, j) in enumerate(items):
        if (b, i, j) in bad:
            assert int(got[5][q]) == FWX_ERR_INVALID, (q, b, i, j, int(got[5][q]))
        else:
            w = refs[b].path(i, j)
            assert int(got[5][q]) == len(w) and tuple(got[6][q, :len(w)].tolist()) == w, (q, b, i, j)


# ---- 8. chunking --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_chunked_walk_gives_the_same_answer(dtype, monkeypatch):
    """FWX_BATCH_LISTS_CHUNK=7 walks 100 items in fifteen launches: the same lengths and lists, the oracle's."""
    n, count = 17, 5
    refs = _synth_refs(n, count, _name(dtype))
    rnd = np.random.default_rng(8800)
    items = [(int(b), int(i), int(j)) for b, i, j in zip(rnd.integers(0, count, 100), rnd.integers(0, n, 100),
                                                         rnd.integers(0, n, 100))]
    cap = max(r.longest for r in refs) + 2
    monkeypatch.delenv("FWX_BATCH_LISTS_CHUNK", raising=False)
    assert _lib.lib().fwx_test_batch_lists_chunk(n, cap) >= 100
    whole = _raw(refs, items, cap)
    monkeypatch.setenv("FWX_BATCH_LISTS_CHUNK", "7")
    assert _lib.lib().fwx_test_batch_lists_chunk(n, cap) == 7
    chunked = _raw(refs, items, cap)
    assert whole[0] == 0 and chunked[0] == 0
    _check_solution(refs, chunked, "chunked")
    assert np.array_equal(whole[5], chunked[5])
    for q, (b, i, j) in enumerate(items):
        w = refs[b].path(i, j)
        for got in (whole, chunked):
            assert int(got[5][q]) == len(w) and tuple(got[6][q, :len(w)].tolist()) == w, (q, b, i, j)
