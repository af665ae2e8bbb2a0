"""Batched small solves on the GPU: `count` matrices of one order n <= 128 in one launch, every matrix bit for bit
what the oracle's loop (oracle.relax) leaves of that matrix alone -- rates, next, hops (diagonals included) and U.

Two tiers run them: one wave per matrix with the matrix in registers (n <= FWX_BATCH_WAVE_MAX_N <= 16) and
small_solve's body with one workgroup per matrix.  FWX_BATCH_WAVE_MAX_N = 16 / 0 puts the same input through both.

Inputs: matrix b of a batch is synth.make(kind, n, dtype, seed = BASE_SEED + 1000 + b) with the kinds cycling
d1, d2, t1, t3 over b (_synth_batch: the long n = 4 batches pass over the seeds whose matrix the oracle leaves
untouched) -- neighbouring matrices differ -- or hostile_matrix_mix draws from one seeded generator
(NaN, +-inf, negatives, -0.0, subnormals, positive rates without a path).  No case is vacuous: in every batch of
order n >= 4 the ORACLE's U is > 0 for every matrix (n <= 2 has no relaxation at all and n = 3 sometimes none;
those orders pin "nothing is touched" and the diagonal).  The oracle runs once per input and is shared."""
import ctypes
import functools

import numpy as np
import pytest

import oracle
from floydwarshall_amd import _lib, engine, synth
from oracle import list_ropes

from helpers import assert_bits_equal, dev, host
from hostile_inputs import hostile_matrix_mix

pytestmark = pytest.mark.gpu

KINDS = ("d1", "d2", "t1", "t3")
DTYPES = [np.float64, np.float32]
WAVE_ORDERS = [1, 2, 3, 4, 5, 15, 16]
WORKGROUP_ORDERS = [17, 33, 63, 64, 65, 127, 128]
# (n, FWX_BATCH_WAVE_MAX_N): orders up to 16 through both tiers, larger ones through the only tier they have
ORDER_TIERS = [(n, w) for n in WAVE_ORDERS for w in ("16", "0")] + [(n, "16") for n in WORKGROUP_ORDERS]


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _synth_batch(n, count, dtype_name):
    """Matrix b: kind KINDS[b % 4], seeds ascending from BASE_SEED + 1000, one per matrix.  Up to 8 matrices these
    are the seeds BASE_SEED + 1000 + b.  In the long n = 4 batches about one seed in 25 gives a 4 x 4 matrix
    in which the ORACLE relaxes nothing (U = 0: 11 of the first 257); such a seed is passed over and the matrix
    takes the next one, so that every matrix of every batch has work in it and all of them differ."""
    dtype = np.dtype(dtype_name).type
    parts, seed = [], synth.BASE_SEED + 1000
    while len(parts) < count:
        p = synth.make(KINDS[len(parts) % 4], n, dtype, seed=seed)
        seed += 1
        if n >= 4 and count > 8 and oracle.relax(*(a.copy() for a in p)) == 0:
            continue
        parts.append(p)
    return _frozen(*(np.ascontiguousarray(np.stack([p[f] for p in parts])) for f in range(3)))


@functools.lru_cache(maxsize=None)
def _hostile_batch(n, dtype_name):
    """At least 8 draws from one seeded generator, continued until both mixes of hostile_matrix_mix have occurred."""
    dtype = np.dtype(dtype_name).type
    rnd = np.random.default_rng(9000 + n)
    parts, seen = [], set()
    while len(parts) < 8 or len(seen) < 2:
        assert len(parts) < 32, "the seeded draws of order %d never produced both mixes" % n
        r, x, h, heavy = hostile_matrix_mix(rnd, n, dtype)
        parts.append((r, x, h))
        seen.add(heavy)
    assert seen == {False, True}
    return _frozen(*(np.ascontiguousarray(np.stack([p[f] for p in parts])) for f in range(3)))


def _oracle(batch, kb=0, ke=None):
    """oracle.relax over pivots [kb, ke) on each matrix separately: (rate, next, hops, [U_b])."""
    r, x, h = (a.copy() for a in batch)
    us = [oracle.relax(r[b], x[b], h[b], kb, ke) for b in range(r.shape[0])]
    return r, x, h, us


_WANT = {}


def _want(key, batch, kb=0, ke=None):
    """The oracle's answer for an input, computed once and shared by the cases that use it."""
    k = (key, kb, ke)
    if k not in _WANT:
        r, x, h, us = _oracle(batch, kb, ke)
        _WANT[k] = _frozen(r, x, h) + (us,)
    return _WANT[k]


def _solve(batch, fields, kb=0, ke=0):
    """engine.solve_batch on copies of the first `fields` + 1 arrays of the batch: (rate, next, hops, [U_b])."""
    got = [batch[f].copy() if f <= fields else None for f in range(3)]
    us = engine.solve_batch(got[0], got[1], got[2], k_begin=kb, k_end=ke, count_updates=True)
    return got[0], got[1], got[2], [int(u) for u in us]


def _compare(got, want, what):
    """Every matrix of the batch, diagonals included: the arrays are compared whole, (b, i, j) names a difference."""
    for g, w, field in zip(got[:3], want[:3], ("rate", "next", "hops")):
        if g is not None:
            assert_bits_equal(g, w, "%s %s" % (what, field))
    assert got[3] == want[3], "%s: U per matrix %s, the oracle's %s" % (what, got[3], want[3])


def _not_vacuous(n, want):
    if n >= 4:
        assert min(want[3]) > 0, "order %d: the oracle relaxes nothing in matrix %d" % (n, int(np.argmin(want[3])))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,wave", ORDER_TIERS)
def test_orders_and_fields(n, wave, dtype, monkeypatch):
    """Five matrices of every order at which a tile, a row group or a tier changes; rates only, + next, + hops."""
    monkeypatch.setenv("FWX_BATCH_WAVE_MAX_N", wave)
    name = np.dtype(dtype).name
    batch = _synth_batch(n, 5, name)
    want = _want(("synth", n, 5, name), batch)
    _not_vacuous(n, want)
    for fields in (0, 1, 2):
        _compare(_solve(batch, fields), want, "n=%d wave<=%s %s fields=%d" % (n, wave, name, fields))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,count,wave", [(4, c, w) for c in (1, 3, 4, 257, 1025) for w in ("16", "0")]
                         + [(64, c, "16") for c in (1, 2, 257)])
def test_counts(n, count, wave, dtype, monkeypatch):
    """One matrix, a last wave-tier workgroup with 1 or 3 of its 4 waves in use, more workgroups than the chip has
    CUs (257 matrices of one workgroup each; 1025 matrices = 257 wave-tier workgroups)."""
    monkeypatch.setenv("FWX_BATCH_WAVE_MAX_N", wave)
    name = np.dtype(dtype).name
    batch = _synth_batch(n, count, name)
    want = _want(("synth", n, count, name), batch)
    _not_vacuous(n, want)
    _compare(_solve(batch, 2), want, "n=%d count=%d wave<=%s %s" % (n, count, wave, name))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,wave", [(4, "16"), (4, "0"), (5, "16"), (5, "0"), (16, "16"), (16, "0"), (17, "16"),
                                    (65, "16")])
def test_hostile_batches(n, wave, dtype, monkeypatch):
    """Matrices outside the domain side by side with ordinary ones: no domain check, no routing, every one solved by
    the list rule (a positive rate with next = -1 hands the head of kjPath on)."""
    monkeypatch.setenv("FWX_BATCH_WAVE_MAX_N", wave)
    name = np.dtype(dtype).name
    batch = _hostile_batch(n, name)
    assert batch[0].shape[0] >= 8
    want = _want(("hostile", n, name), batch)
    _not_vacuous(n, want)
    _compare(_solve(batch, 2), want, "hostile n=%d wave<=%s %s" % (n, wave, name))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,a,b,wave", [(4, 1, 3, "16"), (4, 1, 3, "0"), (16, 5, 11, "16"), (16, 5, 11, "0"),
                                        (64, 5, 40, "16")])
def test_pivot_ranges(n, a, b, wave, dtype, monkeypatch):
    """One range for every matrix: pivots [a, b) alone equal the oracle over [a, b); [0, a), [a, b), [b, n) by three
    calls equal the whole solve, U included."""
    monkeypatch.setenv("FWX_BATCH_WAVE_MAX_N", wave)
    name = np.dtype(dtype).name
    batch = _synth_batch(n, 5, name)
    tag = "n=%d wave<=%s %s" % (n, wave, name)
    part = _want(("synth", n, 5, name), batch, a, b)
    assert sum(part[3]) > 0
    _compare(_solve(batch, 2, a, b), part, "%s pivots [%d, %d)" % (tag, a, b))
    whole = _want(("synth", n, 5, name), batch)
    _not_vacuous(n, whole)
    state, us = batch, [0] * 5
    for kb, ke in ((0, a), (a, b), (b, n)):
        r, x, h, u = _solve(state, 2, kb, ke)
        state, us = (r, x, h), [p + q for p, q in zip(us, u)]
    _compare(state + (us,), whole, "%s in three ranges" % tag)


NAN_SENTINEL = {np.float64: np.uint64(0x7FF80000DEADBEEF), np.float32: np.uint32(0x7FC0BEEF)}
INT_SENTINEL = 0x5A5A5A5A


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,wave", [(4, "16"), (4, "0"), (16, "16"), (16, "0"), (17, "16")])
def test_device_form_with_a_stride(n, wave, dtype, monkeypatch):
    """fwx_dev_solve_batch on caller-owned device memory, matrices n*n + 7 elements apart: the gaps hold sentinels and
    come back bit-identical, the per-matrix counters are INCREMENTED (pre-loaded with 3)."""
    monkeypatch.setenv("FWX_BATCH_WAVE_MAX_N", wave)
    name = np.dtype(dtype).name
    count, stride = 5, n * n + 7
    batch = _synth_batch(n, count, name)
    want = _want(("synth", n, count, name), batch)
    _not_vacuous(n, want)
    it = np.uint64 if dtype == np.float64 else np.uint32
    flat = [np.full(count * stride, NAN_SENTINEL[dtype], dtype=it).view(dtype),
            np.full(count * stride, INT_SENTINEL, dtype=np.int32), np.full(count * stride, INT_SENTINEL, dtype=np.int32)]
    for f in range(3):
        for b in range(count):
            flat[f][b * stride:b * stride + n * n] = batch[f][b].reshape(-1)
    expect = [a.copy() for a in flat]
    for f in range(3):
        for b in range(count):
            expect[f][b * stride:b * stride + n * n] = want[f][b].reshape(-1)
    d = [dev(a) for a in flat]
    upd = dev(np.full(count, 3, dtype=np.uint64))
    engine.dev_solve_batch(d[0], count, n, next_t=d[1], hops_t=d[2], stride=stride, updates_t=upd)
    for f, field in enumerate(("rate", "next", "hops")):
        assert_bits_equal(host(d[f]), expect[f], "n=%d wave<=%s %s %s with gaps" % (n, wave, name, field))
    assert [int(u) for u in host(upd)] == [3 + u for u in want[3]]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [4, 64, 128])
def test_batch_agrees_with_single_solves(n, dtype, monkeypatch):
    """A second, independent statement: matrix b of the batch equals engine.solve of that matrix alone."""
    monkeypatch.delenv("FWX_BATCH_WAVE_MAX_N", raising=False)
    name = np.dtype(dtype).name
    batch = _synth_batch(n, 3, name)
    _not_vacuous(n, _want(("synth", n, 3, name), batch))
    got = _solve(batch, 2)
    for b in range(3):
        r, x, h = (batch[f][b].copy() for f in range(3))
        u = engine.solve(r, x, h, count_updates=True)
        for g, w, field in zip(got[:3], (r, x, h), ("rate", "next", "hops")):
            assert_bits_equal(g[b], w, "n=%d %s matrix %d %s against engine.solve" % (n, name, b, field))
        assert got[3][b] == u


@pytest.mark.parametrize("dtype", DTYPES)
def test_updates_out_is_the_sum_over_the_batch(dtype, monkeypatch):
    monkeypatch.delenv("FWX_BATCH_WAVE_MAX_N", raising=False)
    name = np.dtype(dtype).name
    n, count = 16, 5
    batch = _synth_batch(n, count, name)
    want = _want(("synth", n, count, name), batch)
    _not_vacuous(n, want)
    r, x, h = (a.copy() for a in batch)
    each = np.full(count, 99, dtype=np.uint64)
    total = ctypes.c_uint64(99)
    o = _lib.FwxOpts()
    o.struct_size, o.device = ctypes.sizeof(_lib.FwxOpts), -1
    o.updates_out = ctypes.pointer(total)
    fn = _lib.lib().fwx_solve_batch_f64 if dtype == np.float64 else _lib.lib().fwx_solve_batch_f32
    _lib.check(fn(count, n, r.ctypes.data, x.ctypes.data, h.ctypes.data, each.ctypes.data, ctypes.byref(o)),
               "fwx_solve_batch")
    assert [int(u) for u in each] == want[3]
    assert total.value == sum(want[3])
    _compare((r, x, h, want[3]), want, "n=16 %s with updates_out" % name)


@pytest.mark.parametrize("dtype", DTYPES)
def test_allocation_failures_leave_the_arrays_alone(dtype, monkeypatch):
    """fwx_test_fail_after walked through the allocation points of the host form (a staged batch with next, hops and
    counters has five: three device reservations, the host counters, the pinned staging): each returns FWX_ERR_OOM
    with the caller's arrays and counters untouched, and the next call works.  A countdown past the last point is
    not reached: that call succeeds."""
    _walk_allocation_points("batch", dtype, monkeypatch)


# Host form -> (orders of the batch, items, cap, allocation points).  The three other forms are the smallest batches
# that reach a reservation the plain form has not: the lists' memory and the large tier's scratch panels (both the
# context's small buffer) and the ragged plan (in the workspace, behind the counters).
FAIL_FORMS = {
    "batch": ((16,) * 5, 0, 0, 5),
    "batch_lists": ((16,) * 5, 4, 16, 6),
    "batch_large": ((257,) * 2, 0, 0, 5),
    "ragged_mid_lists": ((3, 17, 130), 3, 130, 6),
}
LEN_SENTINEL, PATH_SENTINEL = -99, -7


@functools.lru_cache(maxsize=None)
def _fail_case(form, dtype_name):
    """(input, oracle's answer, [U_b], items, their lists) of one form: matrix b is _synth_batch's (kind KINDS[b % 4],
    seed BASE_SEED + 1000 + b) at its own order, the arrays packed back to back -- what a uniform batch is too.  Item
    q asks matrix q for its longest list that fits cap, so every item has vertices to write."""
    orders, items, cap, _ = FAIL_FORMS[form]
    dtype = np.dtype(dtype_name).type
    mats = [synth.make(KINDS[b % 4], n, dtype, seed=synth.BASE_SEED + 1000 + b) for b, n in enumerate(orders)]
    done = [tuple(a.copy() for a in m) for m in mats]
    us = [oracle.relax(*m) for m in done]
    assert all(u > 0 for u, n in zip(us, orders) if n >= 4)
    triples, lists = [], []
    for q in range(items):
        ropes = list_ropes.solve(mats[q][0], mats[q][1])
        fits = np.where(ropes.lengths <= cap, ropes.lengths, 0)
        i, j = (int(v) for v in np.unravel_index(np.argmax(fits), fits.shape))
        assert fits[i, j] >= 1
        triples.append((q, i, j))
        lists.append(ropes.path(i, j))
    pack = lambda ms: _frozen(*(np.concatenate([m[f].reshape(-1) for m in ms]) for f in range(3)))  # noqa: E731
    return pack(mats), pack(done), us, triples, lists


def _walk_allocation_points(form, dtype, monkeypatch):
    for var in ("FWX_BATCH_WAVE_MAX_N", "FWX_BATCH_MID_MIN_N", "FWX_BATCH_LARGE_MIN_N", "FWX_BATCH_LISTS_CHUNK"):
        monkeypatch.delenv(var, raising=False)
    orders, items, cap, points = FAIL_FORMS[form]
    count = len(orders)
    batch, want, want_us, triples, lists = _fail_case(form, np.dtype(dtype).name)
    L = _lib.lib()
    fn = getattr(L, "fwx_solve_%s_%s" % (form, "f64" if dtype == np.float64 else "f32"))
    n_each = np.array(orders, dtype=np.int32)
    mat, src, dst = (np.ascontiguousarray([t[f] for t in triples], dtype=np.int32) for f in range(3))

    def call(arrays, each, total, lens, paths):
        o = _lib.FwxOpts()
        o.struct_size, o.device = ctypes.sizeof(_lib.FwxOpts), -1
        o.updates_out = ctypes.pointer(total)
        head = (count, n_each.ctypes.data) if form.startswith("ragged") else (count, orders[0])
        tail = (items, mat.ctypes.data, src.ctypes.data, dst.ctypes.data, lens.ctypes.data, paths.ctypes.data,
                cap) if items else ()
        return fn(*head, arrays[0].ctypes.data, arrays[1].ctypes.data, arrays[2].ctypes.data, each.ctypes.data, *tail,
                  ctypes.byref(o))

    for countdown in range(1, points + 2):
        arrays = [a.copy() for a in batch]
        each, total = np.full(count, 99, dtype=np.uint64), ctypes.c_uint64(99)
        lens = np.full(max(items, 1), LEN_SENTINEL, dtype=np.int32)
        paths = np.full((max(items, 1), max(cap, 1)), PATH_SENTINEL, dtype=np.int32)
        assert L.fwx_test_fail_after(countdown) == _lib.FWX_OK
        rc = call(arrays, each, total, lens, paths)
        assert L.fwx_test_fail_after(0) == _lib.FWX_OK
        if countdown <= points:
            assert rc == _lib.FWX_ERR_OOM, (countdown, rc)
            for a, b, field in zip(arrays, batch, ("rate", "next", "hops")):
                assert_bits_equal(a, b, "%s after a failure at allocation point %d" % (field, countdown))
            assert [int(u) for u in each] == [99] * count and total.value == 99
            assert (lens == LEN_SENTINEL).all() and (paths == PATH_SENTINEL).all(), countdown
            rc = call(arrays, each, total, lens, paths)         # the next call works
        assert rc == _lib.FWX_OK, (countdown, rc)
        for a, w, field in zip(arrays, want, ("rate", "next", "hops")):
            assert_bits_equal(a, w, "%s after countdown %d" % (field, countdown))
        assert [int(u) for u in each] == want_us and total.value == sum(want_us)
        for q, path in enumerate(lists):
            assert int(lens[q]) == len(path) and tuple(paths[q, :len(path)].tolist()) == path, (countdown, q)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["batch_lists", "batch_large", "ragged_mid_lists"])
def test_allocation_failures_in_the_other_host_forms(form, dtype, monkeypatch):
    """The same walk through the host forms that reserve more than the plain one, each with next, hops, updates_each
    and updates_out; len_out and path_out stay untouched too.  Allocation points counted on the library before the
    batched family moved to fwx_batch.hip, and unchanged since:
      fwx_solve_batch_lists_*       n = 16, count = 5, 4 items, cap = 16           6  the plain form's five and the
                                                                                     lists' memory
      fwx_solve_batch_large_*       n = 257, count = 2                             5  three arrays, the counters, the
                                                                                     scratch panels; at 2 x 257^2 cells
                                                                                     the arrays are past the staging
                                                                                     limit, so no pinned staging
      fwx_solve_ragged_mid_lists_*  orders (3, 17, 130), 3 items, cap = 130        6  three arrays, counters + plan,
                                                                                     staging, the lists' memory
    A countdown of points + 1 is not reached, which pins the counts from above as well."""
    _walk_allocation_points(form, dtype, monkeypatch)
