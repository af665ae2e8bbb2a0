"""Batched mid-size solves with the reference's exact `_path` lists (fwx_solve_batch_mid_lists_f64 / _f32,
fwx_dev_solve_batch_mid_traced + fwx_dev_exact_paths_batch_mid): every matrix of a batch of order n <= 256 bit for bit
what the oracle's loop (oracle.relax) leaves of it -- rates, next, hops, U -- and every list asked for, list for list,
what the rope oracle (oracle.list_ropes.solve) gives for that matrix alone.

Orders from FWX_BATCH_MID_MIN_N (default 129) up run the mid tier (floydwarshall_amd/csrc/fwx_mid.hip with the trace:
B pivots per pass, B = fwx_test_batch_mid_block()); FWX_BATCH_MID_MIN_N=1 puts small orders through the same kernel,
where the traced tiers of fwx_dev_solve_batch_traced give a second answer for the three trace arrays, cell for cell.
At the mid orders the trace arrays are compared with the direct definition (the k-i-j loop that records `last` on
every win and copies column k / row k of it at the start of step k), cell for cell too.

Inputs as in tests/test_gpu_batch_lists.py: synthetic kinds cycling d1, t2, t1, d2, t3 (the cycle starts at n % 5 so
that every kind meets some order), matrix b the first seed, ascending from one counter, whose ORACLE U is > 0 and whose
longest list stays within MAX_LIST; the market construction of that file (exact ties: lists that are not the walk of the
final next-hops); sixteen hostile draws of hostile_matrix_mix.  Every case asserts its preconditions from the oracle
before any GPU call; the oracle side of an input is computed once and shared.

Which lists.  All n^2 pairs of a matrix only at n <= 145; above, every pair whose src or dst lies in
{0, 1, B-1, B, B+1, n-B-1 ... n-1} plus a seeded sample of 4096 others.  The items of a call are grouped by the
ORACLE's length into capacity classes, one call of the host form per class, as that file does."""
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
ALL_PAIRS_MAX_N = 145
SAMPLE = 4096
B = _lib.lib().fwx_test_batch_mid_block()
MID_ORDERS = [129, 130, 143, 144, 145, 191, 192, 193, 255, 256]
SMALL_ORDERS = sorted({1, 2, 3, B - 1, B, B + 1, 2 * B + 1, 63, 64, 65, 127, 128} - {0})
NAN_SENTINEL = {np.float64: np.uint64(0x7FF80000DEADBEEF), np.float32: np.uint32(0x7FC0BEEF)}
INT_SENTINEL = 0x5A5A5A5A            # no pivot, -1 included, equals it


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
        self._trace = None
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

    @property
    def trace(self):
        """(last, at_col, at_row) by the direct definition; its solution is checked against the dense oracle's."""
        if self._trace is None:
            n = self.n
            rate, nxt = self.rate.copy(), self.next.copy()
            last = np.full((n, n), -1, dtype=np.int32)
            at_col, at_row = last.copy(), last.copy()
            idx = np.arange(n)
            off = idx[:, None] != idx[None, :]
            with np.errstate(all="ignore"):
                for k in range(n):
                    at_col[:, k] = last[:, k]
                    at_row[k, :] = last[k, :]
                    col, row, cn, rn = rate[:, k].copy(), rate[k, :].copy(), nxt[:, k].copy(), nxt[k, :].copy()
                    cand = col[:, None] * row[None, :]
                    win = (rate < cand) & off & (idx[:, None] != k) & (idx[None, :] != k)
                    rate[win] = cand[win]
                    nxt[win] = np.where(cn[:, None] >= 0, cn[:, None], rn[None, :])[win]
                    last[win] = k
            assert_bits_equal(rate, self.solved[0], "direct definition vs dense loop: rate")
            assert_bits_equal(nxt, self.solved[1], "direct definition vs dense loop: next")
            self._trace = _frozen(last, at_col, at_row)
        return self._trace

    def path(self, s, d):
        key = (int(s), int(d))
        if key not in self._lists:
            self._lists[key] = self.ropes.path(*key)
        return self._lists[key]


@functools.lru_cache(maxsize=None)
def _synth_refs(n, count, dtype_name):
    """Matrix b: kind KINDS[(n + b) % 5], the first seed at or after the previous matrix's + 1 that has U > 0 (n >= 4)
    and no list longer than MAX_LIST -- the oracle alone decides."""
    dtype = np.dtype(dtype_name).type
    refs, seed = [], synth.BASE_SEED + 5000 + n
    while len(refs) < count:
        assert seed < synth.BASE_SEED + 5000 + n + 8 * count + 64, "no usable seed for matrix %d" % len(refs)
        ref = _Ref(*synth.make(KINDS[(n + len(refs)) % len(KINDS)], n, dtype, seed=seed))
        seed += 1
        if ref.longest <= MAX_LIST and (n < 4 or ref.ropes.updates > 0):
            refs.append(ref)
    return tuple(refs)


@functools.lru_cache(maxsize=None)
def _market_ref(n, dtype_name, seed_offset=0):
    """The leading n vertices of a market of 8 currencies, as tests/test_gpu_batch_lists.py builds it (seed 23 + n;
    seed_offset: test_market_ties_inside_a_batch moves on when the oracle finds no tie in that draw)."""
    dtype = np.dtype(dtype_name).type
    n_ccy = 8
    n_exch = -(-n // n_ccy) + 1
    m0 = lf.build_matrix(market_rates(n_exch, n_ccy, seed=23 + n + seed_offset), dtype)
    assert len(m0) >= n
    _, rate, nxt, hops = lf.to_dense(m0, dtype)
    return _Ref(*(np.ascontiguousarray(a[:n, :n]) for a in (rate, nxt, hops)))


@functools.lru_cache(maxsize=None)
def _hostile_refs(n, dtype_name, draws=16):
    dtype = np.dtype(dtype_name).type
    rnd = np.random.default_rng(7100 + n)
    return tuple(_Ref(*hostile_matrix_mix(rnd, n, dtype)[:3]) for _ in range(draws))


def _stack(refs):
    return tuple(np.ascontiguousarray(np.stack([getattr(r, f) for r in refs])) for f in ("rate", "next", "hops"))


def _edge_set(n):
    return sorted({v for v in [0, 1, B - 1, B, B + 1] + list(range(n - B - 1, n)) if 0 <= v < n})


def _items(refs, which=None, sample_seed=0):
    """Module docstring, "Which lists": per matrix of `which` (default: all) all pairs at n <= 145, else the pairs
    that touch the edge set; plus SAMPLE seeded items over the whole batch at n > 145."""
    n, count = refs[0].n, len(refs)
    which = range(count) if which is None else which
    if n <= ALL_PAIRS_MAX_N:
        return [(b, i, j) for b in which for i in range(n) for j in range(n)]
    edge = set(_edge_set(n))
    items = [(b, i, j) for b in which for i in range(n) for j in range(n) if i in edge or j in edge]
    rnd = np.random.default_rng(6600 + n + sample_seed)
    items += [(int(b), int(i), int(j)) for b, i, j in zip(rnd.integers(0, count, SAMPLE), rnd.integers(0, n, SAMPLE),
                                                         rnd.integers(0, n, SAMPLE))]
    return items


def _host_fn(dtype):
    return _lib.lib().fwx_solve_batch_mid_lists_f64 if dtype == np.float64 else _lib.lib().fwx_solve_batch_mid_lists_f32


def _raw(refs, items, cap, with_hops=True, each=True, batch=None):
    """One call of the host form as the C caller sees it: (status, rate, next, hops, [U_b], lens, paths)."""
    rate, nxt, hops = _stack(refs) if batch is None else tuple(a.copy() for a in batch)
    hops = hops if with_hops else None
    count, n = rate.shape[0], rate.shape[1]
    mat, src, dst = (np.ascontiguousarray([it[f] for it in items], dtype=np.int32) for f in range(3))
    lens = np.full(len(items), -99, dtype=np.int32)
    paths = np.full((max(len(items), 1), cap), -7, dtype=np.int32)
    us = np.full(count, 99, dtype=np.uint64) if each else None
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    st = _host_fn(rate.dtype)(count, n, p(rate), p(nxt), p(hops), p(us), len(items), p(mat), p(src), p(dst), p(lens),
                              p(paths), cap, None)
    return st, rate, nxt, hops, None if us is None else [int(u) for u in us], lens, paths


def _check_solution(refs, got, what, with_hops=True):
    _, rate, nxt, hops, us, _, _ = got
    for b in range(rate.shape[0]):
        er, en, eh, eu = refs[b % len(refs)].solved
        assert_bits_equal(rate[b], er, "%s matrix %d rate" % (what, b))
        assert_bits_equal(nxt[b], en, "%s matrix %d next" % (what, b))
        if with_hops:
            assert_bits_equal(hops[b], eh, "%s matrix %d hops" % (what, b))
        assert us[b] == eu, "%s matrix %d: U %d, the oracle's %d" % (what, b, us[b], eu)


def _ask(refs, items, what, with_hops=True, batch=None):
    """The lists of `items` through the host form, grouped by capacity class; the solution of the first call is
    checked against the dense oracle.  Every list is compared with the ropes'.  batch: the arrays to solve when they
    are not _stack(refs) (a tiled batch: matrix b is refs[b % len(refs)])."""
    want_len = np.array([int(refs[b % len(refs)].lengths[i, j]) for b, i, j in items], dtype=np.int64)
    assert int(want_len.max(initial=0)) <= MAX_LIST
    bad, first, lo = [], True, -1
    for hi in CAP_CLASSES:
        sel = np.nonzero((want_len > lo) & (want_len <= hi))[0]
        lo = hi
        cap = hi + 2
        step = max(CALL_INTS // cap, 1)
        for c0 in range(0, len(sel), step):
            part = [items[q] for q in sel[c0:c0 + step]]
            got = _raw(refs, part, cap, with_hops, batch=batch)
            assert got[0] == 0, got[0]
            if first:
                _check_solution(refs, got, what, with_hops)
                first = False
            lens, paths = got[5], got[6]
            for q, (b, i, j) in enumerate(part):
                want = refs[b % len(refs)].path(i, j)
                if int(lens[q]) != len(want) or tuple(paths[q, :len(want)].tolist()) != want:
                    bad.append((b, i, j, int(lens[q]), len(want)))
    assert not first or not items
    assert not bad, "%s: %d lists differ, first (matrix, src, dst, length or status, oracle's length) %r" % (
        what, len(bad), bad[0])


def _not_vacuous(refs):
    if refs[0].n >= 4:
        for b, ref in enumerate(refs):
            assert ref.ropes.updates > 0, "the oracle relaxes nothing in matrix %d" % b


def _differ(refs, items):
    """Of the items, the lists that are not the walk of the final next-hops -- from the oracle alone."""
    out = 0
    for b, i, j in items:
        walk = oracle.follow_path(refs[b].ropes.next, i, j)
        out += walk is None or tuple(walk) != refs[b].path(i, j)
    return out


def _panel_phase_matters(ref):
    """Cells of at_row / at_col that differ from `last` as it stood at the start of their block of B pivots: the
    bookkeeping of the panel phase is exercised (a block of one pivot has none)."""
    n = ref.n
    last, at_col, at_row = ref.trace
    moved = 0
    for k0 in range(0, n, B):
        for k in range(k0 + 1, min(k0 + B, n)):
            moved += int((at_row[k, :] >= k0).sum() + (at_col[:, k] >= k0).sum())
    return moved


# ---- 1. orders and fields ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n", MID_ORDERS)
def test_mid_orders_and_fields(n, dtype, monkeypatch):
    """129 (cw 192, one idle wave, a last block of ONE pivot), 130, around 144, 191 / 192 / 193 (cw 192 -> 256), 255,
    256; with and without hops."""
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    refs = _synth_refs(n, 2, _name(dtype))
    _not_vacuous(refs)
    assert all(_panel_phase_matters(r) > 0 for r in refs)
    items = _items(refs, which=(0,))
    for with_hops in (True, False):
        _ask(refs, items, "n=%d %s hops=%s" % (n, _name(dtype), with_hops), with_hops)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n", SMALL_ORDERS)
def test_small_orders_through_the_mid_kernel(n, dtype, monkeypatch):
    """FWX_BATCH_MID_MIN_N=1: the traced mid kernel at 1, 2, 3, around B and 2B, 63 .. 65, 127, 128: all n^2 lists."""
    monkeypatch.setenv("FWX_BATCH_MID_MIN_N", "1")
    refs = _synth_refs(n, 2 if n >= 63 else 5, _name(dtype))
    _not_vacuous(refs)
    items = _items(refs, which=(0,) if n >= 63 else None)
    for with_hops in (True, False):
        _ask(refs, items, "n=%d through the mid kernel %s hops=%s" % (n, _name(dtype), with_hops), with_hops)


# ---- 2. ties -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n", [129, 145, 240, 256])
def test_market_ties_inside_a_batch(n, dtype, monkeypatch):
    """The reference's own kind of graph (20 exchanges x 12 currencies is order 240) between two other matrices: its
    lists are not the next-hop walk."""
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    others = _synth_refs(n, 2, _name(dtype))
    for seed_offset in range(4):         # the first draw with a tie among the asked lists: the oracle alone decides
        market = _market_ref(n, _name(dtype), seed_offset)             # (only f32 at 145 has to move on, by one)
        refs = (others[0], market, others[1])
        items = _items(refs, which=(1,))
        differ = _differ(refs, [it for it in items if it[0] == 1])
        if differ > 0:
            break
    print("market n=%d %s: %d of %d asked lists differ from the next-hop walk" % (n, _name(dtype), differ, len(items)))
    assert differ > 0
    assert _panel_phase_matters(market) > 0
    _not_vacuous(refs)
    _ask(refs, items, "market n=%d %s" % (n, _name(dtype)))


# ---- 3. outside the domain ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n", [129, 256])
def test_hostile_batches(n, dtype, monkeypatch):
    """Sixteen draws outside the domain as one batch: updates with an empty ikPath and positive rates with an empty
    list occur, and every list asked for is the reference's."""
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    refs = _hostile_refs(n, _name(dtype))
    assert len(refs) == 16 and max(r.longest for r in refs) <= MAX_LIST            # none is left out
    off = ~np.eye(n, dtype=bool)
    with np.errstate(invalid="ignore"):
        positive_empty = sum(int(((r.ropes.rate > 0) & (r.lengths == 0) & off).sum()) for r in refs)
    empty_left = sum(r.ropes.updates_empty_left for r in refs)
    print("hostile n=%d %s: %d updates with an empty ikPath, %d positive rates with an empty list" % (
        n, _name(dtype), empty_left, positive_empty))
    assert empty_left > 0 and positive_empty > 0
    _not_vacuous(refs)
    edge = set(_edge_set(n))
    items = [(0, i, j) for i in range(n) for j in range(n) if i in edge or j in edge]
    rnd = np.random.default_rng(6700 + n)
    items += [(int(b), int(i), int(j)) for b, i, j in zip(rnd.integers(0, 16, SAMPLE), rnd.integers(0, n, SAMPLE),
                                                         rnd.integers(0, n, SAMPLE))]
    _ask(refs, items, "hostile n=%d %s" % (n, _name(dtype)))


# ---- 4. the trace arrays themselves, through the device forms ------------------------------------------------------
def _device_case(refs, dtype, stride, with_hops, traced_fn, stream=None):
    """The traced device solve on sentinel-filled arrays `stride` apart.  Returns the six host arrays after the
    solve, the counters, `inside` (the mask of cells inside a matrix) and the device handles for a walk."""
    count, n = len(refs), refs[0].n
    batch = _stack(refs)
    bits = np.uint64 if dtype == np.float64 else np.uint32
    flat = [np.full(count * stride, NAN_SENTINEL[dtype], dtype=bits).view(dtype)] + [
        np.full(count * stride, INT_SENTINEL, dtype=np.int32) for _ in range(5)]
    inside = np.zeros(count * stride, dtype=bool)
    for b in range(count):
        inside[b * stride:b * stride + n * n] = True
        for f in range(3):
            flat[f][b * stride:b * stride + n * n] = batch[f][b].reshape(-1)
    d = [dev(a) for a in flat]
    next0 = dev(flat[1])
    upd = dev(np.arange(3, 3 + count, dtype=np.uint64))
    trace = engine.Trace(0, 0, _views=(d[3], d[4], d[5]))
    traced_fn(d[0], count, n, trace, next_t=d[1], hops_t=d[2] if with_hops else None, stride=stride, updates_t=upd,
              stream=stream)
    if stream is not None:
        stream.synchronize()
    return [host(a) for a in d], [int(u) for u in host(upd)], inside, (next0, trace)


def _check_device_case(refs, dtype, stride, with_hops, got, us, inside, what):
    count, n = len(refs), refs[0].n
    for f, field in enumerate(("rate", "next", "hops")):
        expect = got[f].copy()
        if f == 0:
            expect.view(np.uint64 if dtype == np.float64 else np.uint32)[~inside] = NAN_SENTINEL[dtype]
        else:
            expect[~inside] = INT_SENTINEL
        if f == 2 and not with_hops:
            for b, ref in enumerate(refs):
                expect[b * stride:b * stride + n * n] = ref.hops.reshape(-1)            # hops absent: untouched
        else:
            for b, ref in enumerate(refs):
                expect[b * stride:b * stride + n * n] = ref.solved[f].reshape(-1)
        assert_bits_equal(got[f], expect, "%s %s with gaps" % (what, field))
    assert us == [3 + b + r.solved[3] for b, r in enumerate(refs)], "%s: the counters are incremented" % what
    for f, field in ((3, "last"), (4, "at_col"), (5, "at_row")):
        t = got[f]
        assert (t[~inside] == INT_SENTINEL).all(), "%s: the gap of %s was written" % (what, field)
        assert (t[inside] != INT_SENTINEL).all(), "%s: a cell of %s inside a matrix was not written" % (what, field)
        for b, ref in enumerate(refs):
            assert np.array_equal(t[b * stride:b * stride + n * n].reshape(n, n), ref.trace[f - 3]), (
                "%s: %s of matrix %d is not the definition's" % (what, field, b))


@pytest.mark.parametrize("dtype,n,with_hops", [(np.float64, 129, True), (np.float64, 255, True),
                                               (np.float32, 193, True), (np.float64, 145, False),
                                               (np.float32, 130, False), (np.float64, 256, True),
                                               (np.float32, 256, True)])
def test_device_forms_with_a_stride_counters_and_a_stream(dtype, n, with_hops, monkeypatch):
    """fwx_dev_solve_batch_mid_traced and fwx_dev_exact_paths_batch_mid on caller-owned device memory and a caller's
    non-default stream, matrices n*n + 37 elements apart (odd n: rows and matrices off 16-byte alignment): all six
    arrays pre-filled with sentinels, the gaps come back untouched, every trace cell inside a matrix equals the direct
    definition's (diagonals -1), the counters are INCREMENTED, and the walk addresses by the same stride."""
    from floydwarshall_amd import hip
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    count, stride = 3, n * n + 37
    refs = _synth_refs(n, 2, _name(dtype)) + (_market_ref(n, _name(dtype)),)
    _not_vacuous(refs)
    assert all(_panel_phase_matters(r) > 0 for r in refs)
    what = "n=%d %s hops=%s" % (n, _name(dtype), with_hops)
    s = hip.Stream()
    got, us, inside, (next0, trace) = _device_case(refs, dtype, stride, with_hops, engine.dev_solve_batch_mid_traced, s)
    _check_device_case(refs, dtype, stride, with_hops, got, us, inside, what)
    rnd = np.random.default_rng(6800 + n)
    items = [(int(b), int(i), int(j)) for b, i, j in zip(rnd.integers(0, count, 2000), rnd.integers(0, n, 2000),
                                                         rnd.integers(0, n, 2000))]
    cap = max(r.longest for r in refs) + 2
    mat, src, dst = (dev(np.ascontiguousarray([it[f] for it in items], dtype=np.int32)) for f in range(3))
    len_t, path_t = engine.dev_exact_paths_batch_mid(next0, count, n, trace, mat, src, dst, cap, stride=stride, stream=s)
    s.synchronize()
    lens, paths = host(len_t), host(path_t)
    bad = [(it, int(lens[q])) for q, it in enumerate(items)
           if int(lens[q]) != len(refs[it[0]].path(it[1], it[2]))
           or tuple(paths[q, :max(int(lens[q]), 0)].tolist()) != refs[it[0]].path(it[1], it[2])]
    assert not bad, "%s: %d lists differ, first %r" % (what, len(bad), bad[0])
    s.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n", SMALL_ORDERS)
def test_the_trace_equals_the_small_tiers(n, dtype, monkeypatch):
    """FWX_BATCH_MID_MIN_N=1: the three trace arrays of the mid kernel against those of fwx_dev_solve_batch_traced
    (wave tier or workgroup tier) on the same input, cell for cell with the diagonals, sentinels in the gaps of all
    six arrays; both against the direct definition."""
    count, stride = 3, n * n + 5
    refs = _synth_refs(n, count, _name(dtype))
    _not_vacuous(refs)
    what = "n=%d %s" % (n, _name(dtype))
    monkeypatch.setenv("FWX_BATCH_MID_MIN_N", "1")
    mid = _device_case(refs, dtype, stride, True, engine.dev_solve_batch_mid_traced)
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N")
    small = _device_case(refs, dtype, stride, True, engine.dev_solve_batch_traced)
    _check_device_case(refs, dtype, stride, True, mid[0], mid[1], mid[2], what + " mid")
    _check_device_case(refs, dtype, stride, True, small[0], small[1], small[2], what + " small")
    for f, field in enumerate(("rate", "next", "hops", "last", "at_col", "at_row")):
        assert_bits_equal(mid[0][f], small[0][f], "%s %s: mid kernel against the small tiers" % (what, field))


# ---- 5. counts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_more_workgroups_than_cus(dtype, monkeypatch):
    """4 distinct matrices of order 129 tiled to 600 workgroups: every copy equals its oracle, lists from the first,
    the last and sampled copies."""
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    n, count = 129, 600
    refs = _synth_refs(n, 2, _name(dtype)) + (_market_ref(n, _name(dtype)), _hostile_refs(n, _name(dtype))[0])
    _not_vacuous(refs)
    tiled = tuple(np.ascontiguousarray(np.tile(a, (count // 4, 1, 1))) for a in _stack(refs))
    rnd = np.random.default_rng(6900)
    items = [(b, i, j) for b in (0, count - 1) for i in (0, 1, B, n - 1) for j in range(n)]
    items += [(int(b), int(i), int(j)) for b, i, j in zip(rnd.integers(0, count, 3000), rnd.integers(0, n, 3000),
                                                         rnd.integers(0, n, 3000))]
    _ask(refs, items, "600 x n=129 %s" % _name(dtype), batch=tiled)


# ---- 6. the capacity rule and bad items -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_capacity_rule_at_the_longest_list(dtype, monkeypatch):
    """The longest list of a matrix of order 256: cap = L returns it, cap = L - 1 is FWX_ERR_CAPACITY for that item
    alone; an empty list fits cap = 1."""
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    n = 256
    refs = _synth_refs(n, 2, _name(dtype))
    b = int(np.argmax([r.longest for r in refs]))
    i, j = (int(v) for v in np.unravel_index(int(np.argmax(refs[b].lengths)), (n, n)))
    L = refs[b].longest
    assert L >= 2 and int(refs[b].lengths[i, j]) == L
    short = (b, 0, 0)                                                    # the diagonal's list is empty
    assert refs[b].path(0, 0) == ()
    items = [(b, i, j), short, (1 - b, 1, 0)]
    want = [refs[m].path(s, d) for m, s, d in items]
    for cap in (L, L - 1):
        st, _, _, _, _, lens, paths = _raw(refs, items, cap)
        assert st == 0
        for q, w in enumerate(want):
            got = (int(lens[q]), tuple(paths[q, :max(int(lens[q]), 0)].tolist()))
            expect = (len(w), w) if cap >= len(w) else (FWX_ERR_CAPACITY, ())
            assert got == expect, "cap %d item %d %r: %r, expected %r" % (cap, q, items[q], got[0], expect[0])
    st, _, _, _, _, lens, _ = _raw(refs, [short], 1)
    assert st == 0 and int(lens[0]) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_bad_items_are_refused_alone(dtype, monkeypatch):
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    n, count = 130, 2
    refs = _synth_refs(n, count, _name(dtype))
    good = [(0, 1, 2), (1, n - 1, 0), (1, 3, 1), (0, 0, n - 1)]
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


# ---- 7. the binding, chunks, and the untraced call --------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_python_binding_and_growing_cap(dtype, monkeypatch):
    """engine.solve_batch_mid_lists: cap=None grows until every list fits (started at 1 so that it has to); an
    explicit cap is not grown; the arrays come back solved in place; engine.solve_batch_lists still refuses."""
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    monkeypatch.setattr(engine, "BATCH_LISTS_FIRST_CAP", 1)
    n = 130
    refs = _synth_refs(n, 2, _name(dtype))
    longest = max(r.longest for r in refs)
    assert longest >= 2
    b = int(np.argmax([r.longest for r in refs]))
    i, j = (int(v) for v in np.unravel_index(int(np.argmax(refs[b].lengths)), (n, n)))
    some = ([b, 0, 1, 1], [i, 0, n - 1, 5], [j, n - 1, 1, 5])
    rate, nxt, hops = _stack(refs)
    lists, us = engine.solve_batch_mid_lists(rate, nxt, hops, items=some, count_updates=True)
    _check_solution(refs, (0, rate, nxt, hops, [int(u) for u in us], None, None), "binding n=%d" % n)
    assert lists == [refs[m].path(s, d) for m, s, d in zip(*some)]
    with pytest.raises(engine.FwxError) as e:
        engine.solve_batch_mid_lists(*_stack(refs), items=some, cap=longest - 1)
    assert e.value.status == FWX_ERR_CAPACITY
    with pytest.raises(engine.FwxError) as e:
        engine.solve_batch_lists(*_stack(refs), items=some, cap=longest)
    assert e.value.status == _lib.FWX_ERR_UNSUPPORTED


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_chunked_walk_gives_the_same_answer(dtype, monkeypatch):
    """FWX_BATCH_LISTS_CHUNK=7 walks 100 items of order 256 in fifteen launches: the same lengths and lists."""
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    n, count = 256, 2
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


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n", [129, 192, 256])
def test_the_untraced_call_is_unchanged(n, dtype, monkeypatch):
    """fwx_solve_batch_mid_* on the same inputs still equals the oracle: rates only, + next, + hops (the kernel body is
    shared with the traced forms)."""
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    refs = _synth_refs(n, 2, _name(dtype)) + (_market_ref(n, _name(dtype)),)
    batch = _stack(refs)
    for fields in (0, 1, 2):
        got = [batch[f].copy() if f <= fields else None for f in range(3)]
        us = engine.solve_batch_mid(got[0], got[1], got[2], count_updates=True)
        for b, ref in enumerate(refs):
            for f, field in enumerate(("rate", "next", "hops")[:fields + 1]):
                assert_bits_equal(got[f][b], ref.solved[f], "untraced n=%d fields=%d matrix %d %s" % (n, fields, b, field))
            assert int(us[b]) == ref.solved[3]
