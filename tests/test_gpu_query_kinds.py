"""The path queries (fwx_matrix_query, fwx_matrix_query_exact, fwx_matrix_query_exact_batch) answer alike on
both handle kinds: a single-device handle and a row-partitioned one address entry (a, b) through the same table
(csrc/fwx_query.h), the first as one partition of all rows.  Expected values come from the CPU alone: the
list-faithful restatement for the exact `_path` lists, the oracle's next-hops for the walk.

Orders, the smallest at which the addressing can go wrong: n = 5 (with 8 partitions most are empty and the
lookup has to step over them), n = 13 (the device pitch is not n: f32 pads to 16, f64 to 14), n = 70 (two fused
blocks, three partitions split at rows that are no multiples of 64).  Inputs are t1: all off-diagonal rates are
non-zero powers of two, so ties abound.  (At these orders the lists coincide with the walks of the final
next-hops; the two queries still read different arrays -- the trace and next0 against next.)

Capacity: cap bounds the list alone -- a list of L entries is returned whenever cap >= L and FWX_ERR_CAPACITY exactly
when L > cap (fwx.h), on every input; the walk's stack is sized by the order.  On these inputs the older rule, a stack
of cap triples, gave the same answers: every sub-entry the walk visits is off-diagonal and has an edge, so each pending
stack item yields at least one list entry and len + pending <= L at every step.  Outside the reference's domain a
pending item can yield nothing and that rule refused lists that fit; tests/test_gpu_exact_lists_edges.py pins the
rule there.  The tests here rely on "cap < L fails" and on lists no longer than cap succeeding next to a failing one,
as the library documents."""
import ctypes
import functools

import numpy as np
import pytest

import oracle
from floydwarshall_amd import engine, synth
from floydwarshall_amd._lib import FWX_ERR_CAPACITY, FWX_ERR_CYCLE, FWX_ERR_INVALID, lib
from oracle import list_faithful as lf

from helpers import assert_bits_equal

pytestmark = pytest.mark.gpu

KINDS = {"single": None, "parts3": [0, 0, 0], "parts8": [0] * 8}
CASES = [(5, "single"), (5, "parts3"), (5, "parts8"), (13, "single"), (13, "parts3"), (70, "single"),
         (70, "parts3")]
PARTITIONED = [(n, kind) for n, kind in CASES if kind != "single"]
DTYPES = [np.float32, np.float64]


@functools.lru_cache(maxsize=None)
def _ref(n, dtype):
    """Input, oracle solution and reference lists of one order: computed once, never modified."""
    rate, nxt, _ = synth.make("t1", n, dtype, seed=100 + n)
    vertices = [("X", "C%03d" % i) for i in range(n)]
    paths = lf.path_indices(lf.run_algo(lf.from_dense(vertices, rate, nxt), dtype))
    er, en = rate.copy(), nxt.copy()
    oracle.relax(er, en)
    walks = [[oracle.follow_path(en, s, d) for d in range(n)] for s in range(n)]
    assert max(len(p) for row in paths for p in row) <= max(4 * n, 64)      # the default cap holds every list
    for a in (rate, nxt, er, en):
        a.setflags(write=False)
    return {"rate": rate, "next": nxt, "er": er, "en": en, "paths": paths, "walks": walks}


def _longest(lists, n):
    """(src, dst, list) of the longest list."""
    s, d = max(((s, d) for s in range(n) for d in range(n)), key=lambda sd: len(lists[sd[0]][sd[1]]))
    return s, d, list(lists[s][d])


def _handle(n, dtype, kind, **kw):
    return engine.DeviceMatrix(n, dtype, with_next=True, devices=KINDS[kind], **kw)


def _traced(n, dtype, kind):
    """A handle of the kind with the traced solve of the reference input done."""
    ref = _ref(n, dtype)
    dm = _handle(n, dtype, kind)
    dm.enable_path_log()
    dm.upload(ref["rate"], ref["next"])
    dm.solve()
    return dm


def _query_raw(fn, dm, s, d, cap):
    """fwx_matrix_query / fwx_matrix_query_exact as the C caller sees it: (status or length, list, rate)."""
    out = np.full(max(cap, 1), -7, dtype=np.int32)
    r = ctypes.c_double(-1.0)
    st = fn(dm._h, int(s), int(d), ctypes.byref(r), out.ctypes.data_as(ctypes.c_void_p), int(cap))
    return st, [int(x) for x in out[:max(st, 0)]], r.value


def _batch_raw(dm, src, dst, cap):
    src = np.ascontiguousarray(src, dtype=np.int32)
    dst = np.ascontiguousarray(dst, dtype=np.int32)
    lens = np.full(len(src), -99, dtype=np.int32)
    paths = np.full((len(src), cap), -7, dtype=np.int32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    st = lib().fwx_matrix_query_exact_batch(dm._h, len(src), ptr(src), ptr(dst), ptr(lens), ptr(paths), cap)
    assert st == 0
    return lens, paths


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,kind", CASES)
def test_three_queries_on_all_pairs(n, kind, dtype):
    ref = _ref(n, dtype)
    er, paths, walks = ref["er"], ref["paths"], ref["walks"]
    with _traced(n, dtype, kind) as dm:
        src = np.repeat(np.arange(n, dtype=np.int32), n)
        dst = np.tile(np.arange(n, dtype=np.int32), n)
        got = dm.query_exact_batch(src, dst)
        assert len(got) == n * n
        for q in range(n * n):
            assert tuple(got[q]) == paths[src[q]][dst[q]], (int(src[q]), int(dst[q]))
        rnd = np.random.default_rng(7)
        pairs = [(int(s), int(d)) for s, d in zip(rnd.integers(0, n, 40), rnd.integers(0, n, 40))]
        exact_rates, walk_rates = [], []
        for s, d in pairs:
            r, p = dm.query_exact(s, d)
            assert tuple(p) == paths[s][d], (s, d)
            exact_rates.append(r)
            r, p = dm.query(s, d)
            assert p == walks[s][d], (s, d)
            walk_rates.append(r)
        want = np.array([er[s, d] for s, d in pairs]).astype(np.float64)      # f32 -> f64 is exact
        assert_bits_equal(np.array(exact_rates), want, "query_exact rates")
        assert_bits_equal(np.array(walk_rates), want, "query rates")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,kind", PARTITIONED)
def test_capacity_rule_is_the_same_on_both_kinds(n, kind, dtype):
    ref = _ref(n, dtype)
    with _traced(n, dtype, "single") as one, _traced(n, dtype, kind) as many:
        for fn, lists in ((lib().fwx_matrix_query_exact, ref["paths"]), (lib().fwx_matrix_query, ref["walks"])):
            s, d, want = _longest(lists, n)
            L = len(want)
            assert L >= 2
            for cap in range(1, L + 3):
                a = _query_raw(fn, one, s, d, cap)
                b = _query_raw(fn, many, s, d, cap)
                assert a == b, (cap, a, b)
                if cap < L:
                    assert a[0] == FWX_ERR_CAPACITY, (cap, a)
                elif a[0] >= 0:
                    assert a[1] == want, (cap, a)
                else:
                    assert a[0] == FWX_ERR_CAPACITY, (cap, a)
                assert_bits_equal(np.array([a[2]]), np.array([ref["er"][s, d]]).astype(np.float64), "rate")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,kind", PARTITIONED)
def test_per_item_errors_in_a_batch(n, kind, dtype):
    ref = _ref(n, dtype)
    paths = ref["paths"]
    ls, ld, longest = _longest(paths, n)
    cap = len(longest) - 1                       # the longest list does not fit; shorter ones do (module docstring)
    assert cap >= 1
    rnd = np.random.default_rng(11)
    valid = [(int(s), int(d)) for s, d in zip(rnd.integers(0, n, 24), rnd.integers(0, n, 24))
             if len(paths[s][d]) <= cap]
    assert len(valid) >= 8
    items = valid[:4] + [(-1, 0)] + valid[4:6] + [(0, n)] + valid[6:] + [(ls, ld), (0, 0)]
    want_len = [FWX_ERR_INVALID if (s, d) in ((-1, 0), (0, n)) else FWX_ERR_CAPACITY if (s, d) == (ls, ld)
                else len(paths[s][d]) for s, d in items]
    src, dst = [s for s, _ in items], [d for _, d in items]
    results = []
    for k in ("single", kind):
        with _traced(n, dtype, k) as dm:
            lens, got = _batch_raw(dm, src, dst, cap)
        assert [int(x) for x in lens] == want_len, k
        lists = [tuple(int(v) for v in got[q, :lens[q]]) if lens[q] >= 0 else None for q in range(len(items))]
        for q, (s, d) in enumerate(items):
            if want_len[q] >= 0:
                assert lists[q] == paths[s][d], (k, s, d)
        results.append(lists)
    assert results[0] == results[1]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,kind", CASES)
def test_a_walk_that_cannot_end_is_an_error_code(n, kind, dtype):
    """An unsolved upload whose next-hops send 0 -> 1 -> 0 for destination 2: the walk is bounded by len >= n."""
    ref = _ref(n, dtype)
    nxt = ref["next"].copy()
    nxt[0, 2], nxt[1, 2] = 1, 0
    nxt[3, 4] = -1
    with _handle(n, dtype, kind) as dm:
        dm.upload(ref["rate"], nxt)
        st, _, r = _query_raw(lib().fwx_matrix_query, dm, 0, 2, n)
        assert st == FWX_ERR_CYCLE
        assert r == float(ref["rate"][0, 2])
        st, _, r = _query_raw(lib().fwx_matrix_query, dm, 3, 4, n)
        assert st == 0 and r == float(ref["rate"][3, 4])
        st, p, _ = _query_raw(lib().fwx_matrix_query, dm, 0, 1, n)      # an ordinary entry of the same upload
        assert (st, p) == (1, [1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,kind", CASES)
def test_lifecycle_is_unchanged(n, kind, dtype):
    ref = _ref(n, dtype)
    rate, nxt, paths = ref["rate"], ref["next"], ref["paths"]
    # the trace enabled AFTER the upload keeps that upload (next0 is copied from the fresh arrays)
    with _handle(n, dtype, kind) as dm:
        dm.upload(rate, nxt)
        dm.enable_path_log()
        with pytest.raises(engine.FwxError) as e:
            dm.query_exact(0, 1)                                   # no traced solve yet
        assert e.value.status == FWX_ERR_INVALID
        with pytest.raises(engine.FwxError) as e:
            dm.query_exact_batch([0], [1])
        assert e.value.status == FWX_ERR_INVALID
        dm.solve()
        src = np.repeat(np.arange(n, dtype=np.int32), n)
        dst = np.tile(np.arange(n, dtype=np.int32), n)
        got = dm.query_exact_batch(src, dst)
        for q in range(n * n):
            assert tuple(got[q]) == paths[src[q]][dst[q]], (int(src[q]), int(dst[q]))
    # the input kept AFTER the upload is that upload: patch + solve == the oracle on the patched matrix
    hops = (nxt >= 0).astype(np.int32)
    index = np.array([0 * n + 3, 4 * n + 1, (n - 1) * n + 2], dtype=np.int64)
    vals = np.array([1.0, 0.0, 1.0], dtype=dtype)                # (rates <= 1: no cycle gains, as in t1)
    pn = np.array([3, -1, 2], dtype=np.int32)
    ph = np.array([1, 0, 1], dtype=np.int32)
    er, en, eh = rate.copy(), nxt.copy(), hops.copy()
    er.reshape(-1)[index], en.reshape(-1)[index], eh.reshape(-1)[index] = vals, pn, ph
    oracle.relax(er, en, eh)
    with _handle(n, dtype, kind, with_hops=True) as dm:
        dm.upload(rate, nxt, hops)
        dm.keep_input()
        dm.patch_input(index, vals, pn, ph)
        dm.solve()
        gr, gn, gh = dm.download()
    assert_bits_equal(gr, er, "rate")
    assert_bits_equal(gn, en, "next")
    assert_bits_equal(gh, eh, "hops")
