"""Batched large solves with the reference's exact `_path` lists (fwx_solve_batch_large_lists_f64 / _f32,
fwx_dev_solve_batch_large_traced + fwx_dev_exact_paths_batch_large): every matrix of a batch of order n <= 1024 bit for
bit what the oracle's loop (oracle.relax) leaves of it -- rates, next, hops, U -- and every list asked for, list for
list, what the rope oracle (oracle.list_ropes.solve) gives for that matrix alone.

Orders from FWX_BATCH_LARGE_MIN_N (default 257) up run the large tier (floydwarshall_amd/csrc/fwx_large.hip with the
trace: per block of B pivots one panel launch over column strips of width S and one sweep launch over TR x TC tiles,
(B, S, TR, TC) = fwx_test_batch_large_geometry() = 16, 48, 16, 256).  FWX_BATCH_LARGE_MIN_N=1 puts small orders
through the same kernels, where fwx_dev_solve_batch_mid_traced gives a second answer for the three trace arrays, cell
for cell.  At every order up to 305 the trace arrays are compared with the direct definition (the k-i-j loop that
records `last` on every win and copies column k / row k of it at the start of step k), cell for cell too.  At 1023 and
1024 the numpy definition and the ropes are too slow: the bits are the dense oracle's, and a seeded sample of lists is
compared with a traced single-matrix handle (fwx_matrix_query_exact_batch), which tests/test_gpu_exact_lists_edges.py
and tests/test_gpu_query_kinds.py pin to the rope oracle.

Inputs, the reference objects and the capacity classes are those of tests/test_gpu_batch_mid_lists.py (imported: one
oracle run per input for both files).  Every case asserts its preconditions from the oracle before any GPU call.

Which lists at the default routing: every pair whose src or dst lies in {0, 1, 15, 16, 17, 47, 48, 49, 255, 256,
n-17 ... n-1} -- around a pivot block, a strip, the mid tier's limit and the ragged right / bottom edge -- plus a seeded
sample of 4096 others."""
import ctypes
import functools

import numpy as np
import pytest

import oracle
from floydwarshall_amd import _lib, engine, synth
from floydwarshall_amd._lib import FWX_ERR_CAPACITY, FWX_ERR_INVALID

from helpers import assert_bits_equal, dev, host
from test_gpu_batch_mid_lists import (CALL_INTS, CAP_CLASSES, INT_SENTINEL, MAX_LIST, NAN_SENTINEL, SAMPLE,
                                      _check_device_case, _check_solution, _differ, _hostile_refs, _market_ref,
                                      _not_vacuous, _stack, _synth_refs)

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]


def _geometry():
    out = (ctypes.c_int32 * 4)()
    assert _lib.lib().fwx_test_batch_large_geometry(out) == _lib.FWX_OK
    return tuple(out)


B, S, TR, TC = _geometry()
SMALL_ORDERS = [1, 2, 15, 16, 17, 33, 47, 48, 49, 64, 65, 97]
LARGE_ORDERS = [257, 260, 289, 305]
GUARD_BYTE, GUARD_BYTES = 0xA5, 1 << 16
HOST_FN = {np.float64: "fwx_solve_batch_large_lists_f64", np.float32: "fwx_solve_batch_large_lists_f32"}


def _name(dtype):
    return np.dtype(dtype).name


def test_the_geometry_is_the_one_the_orders_were_chosen_for():
    assert (B, S, TR, TC) == (16, 48, 16, 256)


def _edge_set(n):
    return sorted({v for v in [0, 1, 15, 16, 17, 47, 48, 49, 255, 256] + list(range(n - 17, n)) if 0 <= v < n})


def _items(refs, which=None, all_pairs=False, sample_seed=0):
    """All pairs of the matrices `which` (default: all), or the pairs that touch the edge set plus SAMPLE seeded items
    over the whole batch."""
    n, count = refs[0].n, len(refs)
    which = range(count) if which is None else which
    if all_pairs:
        return [(b, i, j) for b in which for i in range(n) for j in range(n)]
    edge = set(_edge_set(n))
    items = [(b, i, j) for b in which for i in range(n) for j in range(n) if i in edge or j in edge]
    rnd = np.random.default_rng(6600 + n + sample_seed)
    items += [(int(b), int(i), int(j)) for b, i, j in zip(rnd.integers(0, count, SAMPLE), rnd.integers(0, n, SAMPLE),
                                                         rnd.integers(0, n, SAMPLE))]
    return items


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
    st = getattr(_lib.lib(), HOST_FN[rate.dtype.type])(count, n, p(rate), p(nxt), p(hops), p(us), len(items), p(mat),
                                                       p(src), p(dst), p(lens), p(paths), cap, None)
    return st, rate, nxt, hops, None if us is None else [int(u) for u in us], lens, paths


def _ask(refs, items, what, with_hops=True):
    """The lists of `items` through the host form, grouped by capacity class from the ORACLE's lengths; the solution of
    the first call is checked against the dense oracle.  Every list is compared with the ropes'."""
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


def _panel_phase_matters(ref):
    """Cells of at_row / at_col that differ from `last` as it stood at the start of their block of B pivots: the AR / AC
    panels of the panel launch are exercised (a block of one pivot has none)."""
    n = ref.n
    last, at_col, at_row = ref.trace
    moved = 0
    for k0 in range(0, n, B):
        for k in range(k0 + 1, min(k0 + B, n)):
            moved += int((at_row[k, :] >= k0).sum() + (at_col[:, k] >= k0).sum())
    return moved


def _device_case(refs, dtype, stride, with_hops, stream=None, groups_of=None, traced_fn=None):
    """fwx_dev_solve_batch_large_traced (or traced_fn, the mid entry point) on sentinel-filled arrays `stride` apart,
    all six of them; scratch for groups_of matrices (default: all) with a guard region behind it.  Returns the six
    host arrays after the solve, the counters, `inside` (the mask of cells inside a matrix), the device handles for a
    walk and the guard region as it came back."""
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
    guard = None
    if traced_fn is not None:
        traced_fn(d[0], count, n, trace, next_t=d[1], hops_t=d[2] if with_hops else None, stride=stride, updates_t=upd,
                  stream=stream)
        scratch = None
    else:
        per = _lib.batch_large_scratch_bytes(n)
        held = (groups_of or count) * per
        scratch = dev(np.full(held + GUARD_BYTES, GUARD_BYTE, dtype=np.uint8))
        assert scratch.data_ptr() % 16 == 0
        tr = trace.c_struct()
        vp = ctypes.c_void_p
        _lib.check(_lib.lib().fwx_dev_solve_batch_large_traced(
            count, n, _lib.FWX_F64 if dtype == np.float64 else _lib.FWX_F32, vp(d[0].data_ptr()), vp(d[1].data_ptr()),
            vp(d[2].data_ptr()) if with_hops else None, stride, ctypes.byref(tr), vp(upd.data_ptr()),
            vp(scratch.data_ptr()), held + 15, None if stream is None else stream.ptr),      # floor(bytes / per) = groups
            "fwx_dev_solve_batch_large_traced")
    if stream is not None:
        stream.synchronize()
    out = [host(a) for a in d]                            # a blocking copy on the null stream: the solve is over
    if scratch is not None:
        guard = host(scratch)[-GUARD_BYTES:]
    return out, [int(u) for u in host(upd)], inside, (next0, trace), guard


def _walk_device(refs, next0, trace, items, stride, what, stream=None):
    """fwx_dev_exact_paths_batch_large over the device arrays of a _device_case; every list against the ropes."""
    count, n = len(refs), refs[0].n
    cap = max(r.longest for r in refs) + 2
    mat, src, dst = (dev(np.ascontiguousarray([it[f] for it in items], dtype=np.int32)) for f in range(3))
    len_t, path_t = engine.dev_exact_paths_batch_large(next0, count, n, trace, mat, src, dst, cap, stride=stride,
                                                       stream=stream)
    if stream is not None:
        stream.synchronize()
    lens, paths = host(len_t), host(path_t)
    bad = [(it, int(lens[q])) for q, it in enumerate(items)
           if int(lens[q]) != len(refs[it[0]].path(it[1], it[2]))
           or tuple(paths[q, :max(int(lens[q]), 0)].tolist()) != refs[it[0]].path(it[1], it[2])]
    assert not bad, "%s: %d lists differ, first %r" % (what, len(bad), bad[0])
    return lens, paths


# ---- 1. small orders through the large kernels -------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n", SMALL_ORDERS)
def test_small_orders_through_the_large_kernels(n, dtype, monkeypatch):
    """FWX_BATCH_LARGE_MIN_N=1 at 1, 2, around B, 2B + 1, around S, 64, 65, 2S + 1: rate, next, hops and U against the
    oracle; the three trace arrays against fwx_dev_solve_batch_mid_traced on the same input (sentinels in the gaps of
    all six arrays) and against the direct definition, cell for cell with the diagonals; all n^2 lists of every
    matrix against the ropes, with and without hops."""
    count, stride = 3, n * n + 5
    refs = _synth_refs(n, count, _name(dtype))
    _not_vacuous(refs)
    what = "n=%d %s" % (n, _name(dtype))
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    monkeypatch.setenv("FWX_BATCH_LARGE_MIN_N", "1")
    large = _device_case(refs, dtype, stride, True)
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N")
    other = _device_case(refs, dtype, stride, True, traced_fn=engine.dev_solve_batch_mid_traced)
    _check_device_case(refs, dtype, stride, True, large[0], large[1], large[2], what + " large")
    _check_device_case(refs, dtype, stride, True, other[0], other[1], other[2], what + " mid entry point")
    for f, field in enumerate(("rate", "next", "hops", "last", "at_col", "at_row")):
        assert_bits_equal(large[0][f], other[0][f], "%s %s: large kernels against the mid entry point" % (what, field))
    assert (large[4] == GUARD_BYTE).all()
    monkeypatch.setenv("FWX_BATCH_LARGE_MIN_N", "1")
    items = _items(refs, all_pairs=True)
    for with_hops in (True, False):
        _ask(refs, items, "%s through the large kernels hops=%s" % (what, with_hops), with_hops)


def test_forwarded_orders_take_the_mid_path(monkeypatch):
    """A threshold between two orders: the order below it is forwarded (no scratch needed), the one at it is not; the
    same trace and lists either way."""
    n, dtype = 33, np.float64
    refs = _synth_refs(n, 3, _name(dtype))
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    for value in ("34", "33"):
        monkeypatch.setenv("FWX_BATCH_LARGE_MIN_N", value)
        got = _device_case(refs, dtype, n * n, False)
        _check_device_case(refs, dtype, n * n, False, got[0], got[1], got[2], "n=33 FWX_BATCH_LARGE_MIN_N=%s" % value)
        _ask(refs, _items(refs, which=(0,), all_pairs=True), "n=33 FWX_BATCH_LARGE_MIN_N=%s" % value)
    d = [dev(a) for a in _stack(refs)[:2]]
    t = [dev(np.zeros(3 * n * n, dtype=np.int32)) for _ in range(3)]
    trace = engine.Trace(0, 0, _views=tuple(t))
    tr = trace.c_struct()
    vp = ctypes.c_void_p
    call = lambda: _lib.lib().fwx_dev_solve_batch_large_traced(  # noqa: E731
        3, n, _lib.FWX_F64, vp(d[0].data_ptr()), vp(d[1].data_ptr()), None, n * n, ctypes.byref(tr), None, None, 0, None)
    assert call() == FWX_ERR_INVALID                          # routed to the large tier: scratch is required
    monkeypatch.setenv("FWX_BATCH_LARGE_MIN_N", "34")
    assert call() == 0                                        # forwarded: scratch is ignored
    assert_bits_equal(host(d[1]).reshape(3, n, n), np.stack([r.solved[1] for r in refs]), "forwarded without scratch")


# ---- 2. default routing ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n", LARGE_ORDERS)
def test_default_routing_orders_and_fields(n, dtype, monkeypatch):
    """257 (a last block of ONE pivot, a last strip of 17 columns), 260, 289 (one past six strips and eighteen blocks),
    305 (one past nineteen blocks): two synthetic matrices and a market; the trace against the direct definition
    through the device form, the lists of the first matrix's edge pairs and a sample over all three through the host
    form, with and without hops."""
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    refs = _synth_refs(n, 2, _name(dtype)) + (_market_ref(n, _name(dtype)),)
    _not_vacuous(refs)
    assert all(_panel_phase_matters(r) > 0 for r in refs)
    what = "n=%d %s" % (n, _name(dtype))
    for with_hops in (True, False):
        got = _device_case(refs, dtype, n * n, with_hops)
        _check_device_case(refs, dtype, n * n, with_hops, got[0], got[1], got[2], "%s hops=%s" % (what, with_hops))
        assert (got[4] == GUARD_BYTE).all()
    items = _items(refs, which=(0,))
    for with_hops in (True, False):
        _ask(refs, items, "%s hops=%s" % (what, with_hops), with_hops)


# ---- 3. the largest orders -----------------------------------------------------------------------------------------
KINDS_AT_THE_LIMIT = ("d1", "t2", "t1", "d2")


@functools.lru_cache(maxsize=None)
def _limit_case(n, dtype_name):
    """One matrix of order n, the sampled pairs and their lists from a traced single-matrix handle.  The first seed
    whose longest SAMPLED list stays within MAX_LIST -- the handle decides; the dense oracle then gives the bits."""
    dtype = np.dtype(dtype_name).type
    rnd = np.random.default_rng(6650 + n)
    src = np.concatenate([np.zeros(n, np.int32), np.full(n, n - 1, np.int32), rnd.integers(0, n, SAMPLE).astype(np.int32)])
    dst = np.concatenate([np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32),
                          rnd.integers(0, n, SAMPLE).astype(np.int32)])
    cap = MAX_LIST + 2
    for attempt in range(8):
        rate, nxt, hops = synth.make(KINDS_AT_THE_LIMIT[(n + attempt) % 4], n, dtype, seed=synth.BASE_SEED + 5000 + n + attempt)
        lens = np.empty(len(src), dtype=np.int32)
        paths = np.empty((len(src), cap), dtype=np.int32)
        with engine.DeviceMatrix(n, dtype, with_next=True, with_hops=True, device=0) as dm:
            dm.enable_path_log()
            dm.upload(rate, nxt, hops)
            dm.solve()
            _lib.check(_lib.lib().fwx_matrix_query_exact_batch(dm._h, len(src), src.ctypes.data, dst.ctypes.data,
                                                               lens.ctypes.data, paths.ctypes.data, cap),
                       "fwx_matrix_query_exact_batch")
        if int(lens.min()) >= 0 and int(lens.max()) <= MAX_LIST:
            break
    else:
        raise AssertionError("no usable seed at order %d" % n)
    er, en, eh = rate.copy(), nxt.copy(), hops.copy()
    eu = oracle.relax(er, en, eh)
    assert eu > 0
    for a in (rate, nxt, hops, er, en, eh, src, dst, lens, paths):
        a.setflags(write=False)
    return (rate, nxt, hops), (er, en, eh, eu), (src, dst, lens, paths)


@pytest.mark.parametrize("n,dtype", [(1023, np.float64), (1023, np.float32), (1024, np.float64), (1024, np.float32)])
def test_the_largest_orders(n, dtype, monkeypatch):
    """One matrix at the limit and just below it: the bits are the dense oracle's, and the sampled lists (rows 0 and
    n - 1 whole, 4096 seeded pairs) those of a traced single-matrix handle on the same input."""
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    (rate, nxt, hops), (er, en, eh, eu), (src, dst, want_len, want_paths) = _limit_case(n, _name(dtype))
    differ = sum(1 for q in range(0, len(src), 7)
                 if tuple(oracle.follow_path(en, int(src[q]), int(dst[q])) or ()) != tuple(want_paths[q, :want_len[q]].tolist())
                 and want_len[q] > 0)
    print("n=%d %s: longest sampled list %d, %d of %d probed lists are not the next-hop walk" % (
        n, _name(dtype), int(want_len.max()), differ, len(range(0, len(src), 7))))
    r, x, h = rate[None].copy(), nxt[None].copy(), hops[None].copy()
    cap = int(want_len.max()) + 2
    lens = np.full(len(src), -99, dtype=np.int32)
    paths = np.full((len(src), cap), -7, dtype=np.int32)
    us = np.zeros(1, dtype=np.uint64)
    mat = np.zeros(len(src), dtype=np.int32)
    st = getattr(_lib.lib(), HOST_FN[dtype])(1, n, r.ctypes.data, x.ctypes.data, h.ctypes.data, us.ctypes.data, len(src),
                                             mat.ctypes.data, src.ctypes.data, dst.ctypes.data, lens.ctypes.data,
                                             paths.ctypes.data, cap, None)
    assert st == 0
    what = "n=%d %s" % (n, _name(dtype))
    assert_bits_equal(r[0], er, what + " rate")
    assert_bits_equal(x[0], en, what + " next")
    assert_bits_equal(h[0], eh, what + " hops")
    assert int(us[0]) == eu
    assert np.array_equal(lens, want_len), what
    bad = [q for q in range(len(src)) if not np.array_equal(paths[q, :lens[q]], want_paths[q, :lens[q]])]
    assert not bad, "%s: %d lists differ from the handle's, first (%d, %d)" % (what, len(bad), src[bad[0]], dst[bad[0]])


# ---- 4. ties -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n", [257, 300])
def test_market_ties_inside_a_batch(n, dtype, monkeypatch):
    """The reference's own kind of graph between two other matrices: its lists are not the next-hop walk."""
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    others = _synth_refs(n, 2, _name(dtype))
    for seed_offset in range(4):         # the first draw with a tie among the asked lists: the oracle alone decides
        market = _market_ref(n, _name(dtype), seed_offset)
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


# ---- 5. outside the domain ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n", [257, 289])
def test_hostile_batches(n, dtype, monkeypatch):
    """Sixteen draws outside the domain as one batch: updates with an empty ikPath and positive rates with an empty
    list occur, and every list asked for is the reference's."""
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
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
    _ask(refs, _items(refs, which=(0,), sample_seed=100), "hostile n=%d %s" % (n, _name(dtype)))


# ---- 6. groups, gaps, sentinels, a stream --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,n,with_hops,min_n", [(np.float64, 257, True, None), (np.float32, 259, True, None),
                                                     (np.float64, 260, False, None), (np.float64, B + 3, True, "1"),
                                                     (np.float32, S + 1, False, "1")])
def test_device_forms_with_a_stride_counters_a_stream_and_scratch_for_three(dtype, n, with_hops, min_n, monkeypatch):
    """fwx_dev_solve_batch_large_traced and fwx_dev_exact_paths_batch_large on caller-owned device memory and a
    caller's non-default stream, 8 matrices n*n + 37 elements apart (odd n: rows and matrices off 16-byte alignment):
    all six arrays pre-filled with sentinels, the gaps come back untouched, EVERY cell inside a matrix of the three
    trace arrays is overwritten and equals the direct definition's (diagonals -1) -- also in the groups after the
    first: the scratch holds exactly three matrices (groups of 3, 3 and 2) and the guard region behind it comes back
    untouched; scratch for all eight gives the same bits.  The counters are INCREMENTED, and the walk addresses by the
    same stride."""
    from floydwarshall_amd import hip
    if min_n is None:
        monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    else:
        monkeypatch.setenv("FWX_BATCH_LARGE_MIN_N", min_n)
    count, stride = 8, n * n + 37
    refs = _synth_refs(n, count - 1, _name(dtype)) + (_market_ref(n, _name(dtype)),)
    _not_vacuous(refs)
    assert all(_panel_phase_matters(r) > 0 for r in refs)
    s = hip.Stream()
    rnd = np.random.default_rng(6800 + n)
    items = [(int(b), int(i), int(j)) for b, i, j in zip(rnd.integers(0, count, 2000), rnd.integers(0, n, 2000),
                                                         rnd.integers(0, n, 2000))]
    results = []
    for groups_of in (3, count):
        what = "n=%d %s hops=%s scratch for %d" % (n, _name(dtype), with_hops, groups_of)
        got, us, inside, (next0, trace), guard = _device_case(refs, dtype, stride, with_hops, s, groups_of)
        _check_device_case(refs, dtype, stride, with_hops, got, us, inside, what)
        assert guard.size == GUARD_BYTES and (guard == GUARD_BYTE).all(), "%s: the guard region was written" % what
        results.append(_walk_device(refs, next0, trace, items, stride, what, s))
    assert np.array_equal(results[0][0], results[1][0])           # the lists themselves: each against the ropes above
    s.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_the_python_device_wrappers_and_the_host_form_agree(dtype, monkeypatch):
    """engine.dev_solve_batch_large_traced allocates its scratch; its arrays, counters and walked lists are those of
    one fwx_solve_batch_large_lists_* call on the same input and items, bit for bit."""
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    n, count = 260, 3
    refs = _synth_refs(n, 2, _name(dtype)) + (_market_ref(n, _name(dtype)),)
    _not_vacuous(refs)
    rnd = np.random.default_rng(6900 + n)
    items = [(int(b), int(i), int(j)) for b, i, j in zip(rnd.integers(0, count, 3000), rnd.integers(0, n, 3000),
                                                         rnd.integers(0, n, 3000))]
    cap = max(r.longest for r in refs) + 2
    hosted = _raw(refs, items, cap)
    assert hosted[0] == 0
    _check_solution(refs, hosted, "host form n=%d" % n)
    d = [dev(a) for a in _stack(refs)]
    next0 = dev(_stack(refs)[1])
    t = [dev(np.full(count * n * n, INT_SENTINEL, dtype=np.int32)) for _ in range(3)]
    trace = engine.Trace(0, 0, _views=tuple(t))
    upd = dev(np.zeros(count, dtype=np.uint64))
    scratch = engine.dev_solve_batch_large_traced(d[0], count, n, trace, next_t=d[1], hops_t=d[2], updates_t=upd)
    assert scratch.numel() * scratch.element_size() >= count * _lib.batch_large_scratch_bytes(n)
    lens, paths = _walk_device(refs, next0, trace, items, n * n, "device form n=%d" % n)
    for f, field in enumerate(("rate", "next", "hops")):
        assert_bits_equal(host(d[f]).reshape(count, n, n), hosted[f + 1], "device against host form: %s" % field)
    assert [int(u) for u in host(upd)] == hosted[4]
    assert np.array_equal(lens, hosted[5])
    for q in range(len(items)):
        assert np.array_equal(paths[q, :lens[q]], hosted[6][q, :lens[q]]), items[q]


# ---- 7. the capacity rule and bad items -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_capacity_rule_at_the_longest_list(dtype, monkeypatch):
    """The longest list of a matrix of order 257: cap = L and L + 1 return it, cap = L - 1 is FWX_ERR_CAPACITY for that
    item alone; an empty list fits cap = 1."""
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    n = 257
    refs = _synth_refs(n, 2, _name(dtype))
    b = int(np.argmax([r.longest for r in refs]))
    i, j = (int(v) for v in np.unravel_index(int(np.argmax(refs[b].lengths)), (n, n)))
    L = refs[b].longest
    assert L >= 2 and int(refs[b].lengths[i, j]) == L
    short = (b, 0, 0)                                                    # the diagonal's list is empty
    assert refs[b].path(0, 0) == ()
    items = [(b, i, j), short, (1 - b, 1, 0)]
    want = [refs[m].path(s, d) for m, s, d in items]
    for cap in (L - 1, L, L + 1):
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
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    n, count = 260, 2
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


# ---- 8. the binding and chunks ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_python_binding_and_growing_cap(dtype, monkeypatch):
    """engine.solve_batch_large_lists: cap=None grows until every list fits (started at 1 so that it has to); an
    explicit cap is not grown; the arrays come back solved in place; engine.solve_batch_mid_lists still refuses."""
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    monkeypatch.setattr(engine, "BATCH_LISTS_FIRST_CAP", 1)
    n = 257
    refs = _synth_refs(n, 2, _name(dtype))
    longest = max(r.longest for r in refs)
    assert longest >= 2
    b = int(np.argmax([r.longest for r in refs]))
    i, j = (int(v) for v in np.unravel_index(int(np.argmax(refs[b].lengths)), (n, n)))
    some = ([b, 0, 1, 1], [i, 0, n - 1, 5], [j, n - 1, 1, 5])
    rate, nxt, hops = _stack(refs)
    lists, us = engine.solve_batch_large_lists(rate, nxt, hops, items=some, count_updates=True)
    _check_solution(refs, (0, rate, nxt, hops, [int(u) for u in us], None, None), "binding n=%d" % n)
    assert lists == [refs[m].path(s, d) for m, s, d in zip(*some)]
    with pytest.raises(engine.FwxError) as e:
        engine.solve_batch_large_lists(*_stack(refs), items=some, cap=longest - 1)
    assert e.value.status == FWX_ERR_CAPACITY
    with pytest.raises(engine.FwxError) as e:
        engine.solve_batch_mid_lists(*_stack(refs), items=some, cap=longest)
    assert e.value.status == _lib.FWX_ERR_UNSUPPORTED


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_chunked_walk_gives_the_same_answer(dtype, monkeypatch):
    """FWX_BATCH_LISTS_CHUNK=1 walks 40 items of order 257 in forty launches: the same lengths and lists."""
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    n, count = 257, 2
    refs = _synth_refs(n, count, _name(dtype))
    rnd = np.random.default_rng(8800)
    items = [(int(b), int(i), int(j)) for b, i, j in zip(rnd.integers(0, count, 40), rnd.integers(0, n, 40),
                                                         rnd.integers(0, n, 40))]
    cap = max(r.longest for r in refs) + 2
    monkeypatch.delenv("FWX_BATCH_LISTS_CHUNK", raising=False)
    assert _lib.lib().fwx_test_batch_lists_chunk(n, cap) >= 40
    whole = _raw(refs, items, cap)
    monkeypatch.setenv("FWX_BATCH_LISTS_CHUNK", "1")
    assert _lib.lib().fwx_test_batch_lists_chunk(n, cap) == 1
    chunked = _raw(refs, items, cap)
    assert whole[0] == 0 and chunked[0] == 0
    _check_solution(refs, chunked, "chunked")
    assert np.array_equal(whole[5], chunked[5])
    for q, (b, i, j) in enumerate(items):
        w = refs[b].path(i, j)
        for got in (whole, chunked):
            assert int(got[5][q]) == len(w) and tuple(got[6][q, :len(w)].tolist()) == w, (q, b, i, j)
