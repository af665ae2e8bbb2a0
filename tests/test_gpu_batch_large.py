"""Batched large solves on the GPU (fwx_solve_batch_large_f64 / _f32, fwx_dev_solve_batch_large): `count` matrices of
one order n <= 1024, several workgroups per matrix, every matrix bit for bit what the oracle's loop (oracle.relax)
leaves of that matrix alone -- rates, next, hops (diagonals included) and U.

Orders from FWX_BATCH_LARGE_MIN_N (default 257) up run the large tier: per block of B pivots one panel launch over
column strips of width S and one sweep launch over TR x TC tiles, the snapshot panels in device scratch between them
((B, S, TR, TC) = fwx_test_batch_large_geometry()).  FWX_BATCH_LARGE_MIN_N=1 puts small orders through the same
kernels, where the mid entry point gives a second answer.

Inputs as in test_gpu_batch_mid.py: matrix b of a batch is synth.make(kind, n, dtype, seed) with the kinds cycling d1,
d2, t1, t3 and one seed per matrix, or hostile_matrix_mix draws from one seeded generator.  No case is vacuous: in
every batch of order n >= 4 the ORACLE's U is > 0 for every matrix.  The oracle runs once per input and is shared."""
import ctypes
import functools

import numpy as np
import pytest

import oracle
from floydwarshall_amd import _lib, engine, synth

from helpers import assert_bits_equal, dev, host
from hostile_inputs import hostile_matrix_mix

pytestmark = pytest.mark.gpu

KINDS = ("d1", "d2", "t1", "t3")
DTYPES = [np.float64, np.float32]


def _geometry():
    out = (ctypes.c_int32 * 4)()
    assert _lib.lib().fwx_test_batch_large_geometry(out) == _lib.FWX_OK
    return tuple(out)


B, S, TR, TC = _geometry()


def _first_multiple_above(m, floor):
    return (floor // m + 1) * m


# 257, 258; the first multiple of the tile height, of the tile width and of S above 257, each with its two
# neighbours; two tiles and one more, in rows and in columns
LARGE_ORDERS = sorted(n for n in {257, 258}
                      | {_first_multiple_above(m, 257) + d for m in (TR, TC, S) for d in (-1, 0, 1)}
                      | {2 * TR + 1, 2 * TC + 1} if 257 <= n <= 1024)
SMALL_ORDERS = sorted({1, 2, 3, 4, 5, B - 1, B, B + 1, 2 * B + 1, 63, 64, 65, S - 1, S, S + 1, TR - 1, TR + 1, TC - 1,
                       TC + 1, 129, 256} - {0})
EDGE_ORDER = _first_multiple_above(TR, 257) + 1             # one row and one column past a tile edge


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _synth_batch(n, count, dtype_name):
    """Matrix b: kind KINDS[b % 4], seeds ascending from BASE_SEED + 2000, one per matrix; at n >= 4 a seed whose
    matrix the ORACLE leaves untouched (small orders only: about one 4 x 4 draw in 25) is passed over."""
    dtype = np.dtype(dtype_name).type
    parts, seed = [], synth.BASE_SEED + 2000
    while len(parts) < count:
        p = synth.make(KINDS[len(parts) % 4], n, dtype, seed=seed)
        seed += 1
        if 4 <= n <= 16 and oracle.relax(*(a.copy() for a in p)) == 0:
            continue
        parts.append(p)
    return _frozen(*(np.ascontiguousarray(np.stack([p[f] for p in parts])) for f in range(3)))


@functools.lru_cache(maxsize=None)
def _hostile_batch(n, dtype_name, least=8):
    """At least `least` draws from one seeded generator, continued until both mixes of hostile_matrix_mix have
    occurred."""
    dtype = np.dtype(dtype_name).type
    rnd = np.random.default_rng(9500 + n)
    parts, seen = [], set()
    while len(parts) < least or len(seen) < 2:
        assert len(parts) < 32, "the seeded draws of order %d never produced both mixes" % n
        r, x, h, heavy = hostile_matrix_mix(rnd, n, dtype)
        parts.append((r, x, h))
        seen.add(heavy)
    assert seen == {False, True}
    return _frozen(*(np.ascontiguousarray(np.stack([p[f] for p in parts])) for f in range(3)))


_WANT = {}


def _want(key, batch, kb=0, ke=None):
    """oracle.relax over pivots [kb, ke) on each matrix separately, computed once per input and shared:
    (rate, next, hops, [U_b])."""
    k = (key, kb, ke)
    if k not in _WANT:
        r, x, h = (a.copy() for a in batch)
        us = [oracle.relax(r[b], x[b], h[b], kb, ke) for b in range(r.shape[0])]
        _WANT[k] = _frozen(r, x, h) + (us,)
    return _WANT[k]


def _solve(batch, fields, kb=0, ke=0, fn=None):
    """engine.solve_batch_large on copies of the first `fields` + 1 arrays of the batch: (rate, next, hops, [U_b])."""
    got = [batch[f].copy() if f <= fields else None for f in range(3)]
    us = (fn or engine.solve_batch_large)(got[0], got[1], got[2], k_begin=kb, k_end=ke, count_updates=True)
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


def test_the_order_lists_are_what_the_geometry_makes_them():
    assert 1 <= B <= 64 and S >= 1 and TR >= 1 and TC >= 1
    assert {257, 258} <= set(LARGE_ORDERS) and all(257 <= n <= 1024 for n in LARGE_ORDERS)
    for m in (TR, S):
        assert any(n % m == 0 and n - 1 in LARGE_ORDERS and n + 1 in LARGE_ORDERS for n in LARGE_ORDERS), m
    assert any(n > 2 * TR and n % TR == 1 for n in LARGE_ORDERS)
    assert 257 < EDGE_ORDER <= 1024 and EDGE_ORDER % TR == 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", LARGE_ORDERS)
def test_default_routing_orders_and_fields(n, dtype, monkeypatch):
    """Four matrices at 257, 258, around the first tile and strip edges above them and one past two tiles; rates
    only, + next, + hops."""
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    name = np.dtype(dtype).name
    batch = _synth_batch(n, 4, name)
    want = _want(("synth", n, 4, name), batch)
    _not_vacuous(n, want)
    for fields in (0, 1, 2):
        _compare(_solve(batch, fields), want, "n=%d %s fields=%d" % (n, name, fields))


@pytest.mark.parametrize("n,dtype,fields", [(1023, np.float64, 2), (1023, np.float32, 0),
                                            (1024, np.float64, 2), (1024, np.float32, 0)])
def test_the_largest_orders(n, dtype, fields, monkeypatch):
    """Two matrices at the limit and just below it: f64 with next and hops, f32 rates only."""
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    name = np.dtype(dtype).name
    batch = _synth_batch(n, 2, name)
    want = _want(("synth", n, 2, name), batch)
    _not_vacuous(n, want)
    _compare(_solve(batch, fields), want, "n=%d %s fields=%d" % (n, name, fields))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [257, EDGE_ORDER])
def test_hostile_batches(n, dtype, monkeypatch):
    """Matrices outside the domain side by side with ordinary ones: no domain check, no routing, every one solved by
    the list rule (a positive rate with next = -1 hands the head of kjPath on)."""
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    name = np.dtype(dtype).name
    batch = _hostile_batch(n, name, 4)
    assert batch[0].shape[0] >= 4
    want = _want(("hostile", n, name, 4), batch)
    _not_vacuous(n, want)
    _compare(_solve(batch, 2), want, "hostile n=%d %s" % (n, name))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SMALL_ORDERS)
def test_small_orders_through_the_large_kernels(n, dtype, monkeypatch):
    """FWX_BATCH_LARGE_MIN_N=1: the large kernels at orders below a strip, a block or a tile -- against the oracle
    and, up to 256, against engine.solve_batch_mid on the same input; the hostile draws at the same order too."""
    monkeypatch.setenv("FWX_BATCH_LARGE_MIN_N", "1")
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    name = np.dtype(dtype).name
    for key, batch in ((("synth", n, 4, name), _synth_batch(n, 4, name)),
                       (("hostile", n, name, 4), _hostile_batch(n, name, 4))):
        want = _want(key, batch)
        _not_vacuous(n, want)
        for fields in (0, 1, 2):
            _compare(_solve(batch, fields), want, "%s n=%d %s fields=%d" % (key[0], n, name, fields))
        if n <= _lib.FWX_BATCH_MID_MAX_N:
            other = _solve(batch, 2, fn=engine.solve_batch_mid)
            _compare(_solve(batch, 2), other, "%s n=%d %s against solve_batch_mid" % (key[0], n, name))


def test_below_the_threshold_the_call_is_forwarded(monkeypatch):
    """Default routing at n <= 256 and a threshold in between: the same bits as solve_batch_mid's routes."""
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    for n in (64, 130):
        batch = _synth_batch(n, 4, "float64")
        want = _want(("synth", n, 4, "float64"), batch)
        for value in (None, str(n + 1), str(n)):
            if value is None:
                monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
            else:
                monkeypatch.setenv("FWX_BATCH_LARGE_MIN_N", value)
            _compare(_solve(batch, 2), want, "n=%d FWX_BATCH_LARGE_MIN_N=%s" % (n, value))


def _range_cases(n):
    inside = (B + 2, min(B + 7, n)) if n > 2 * B else (2, 7)      # starts and ends inside one block
    return [(0, 1), (5, 5), (7, n - 2), (n - 1, n), inside]


def _split(n):
    """Where the two-range case cuts [0, n): off a block boundary, past the second block where the order allows."""
    return 2 * B + 5 if 2 * B + 5 < n - 1 else (B + 5 if B + 5 < n - 1 else 7)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", sorted({2 * TR + 5, TC + 5, B + 3}))
def test_pivot_ranges(n, dtype, monkeypatch):
    """One range for every matrix, through (k_begin, k_end): each range alone equals the oracle over it; [0, m) then
    [m, n), m off a block boundary, equal the whole solve, U included.  Orders: two row tiles and five, one column
    tile and five, one block and three."""
    m = _split(n)
    monkeypatch.setenv("FWX_BATCH_LARGE_MIN_N", "1")
    assert m % B != 0 and 0 < m < n
    name = np.dtype(dtype).name
    batch = _synth_batch(n, 4, name)
    key, tag = ("synth", n, 4, name), "n=%d %s" % (n, name)
    for kb, ke in _range_cases(n) + [(0, m)]:
        part = _want(key, batch, kb, ke)
        if ke - kb >= 3:
            assert min(part[3]) > 0, "pivots [%d, %d) relax nothing in some matrix" % (kb, ke)
        if ke == kb:
            assert sum(part[3]) == 0
        _compare(_solve(batch, 2, kb, ke), part, "%s pivots [%d, %d)" % (tag, kb, ke))
    whole = _want(key, batch)
    _not_vacuous(n, whole)
    first = _solve(batch, 2, 0, m)
    second_want = [a.copy() for a in first[:3]]
    us = [oracle.relax(second_want[0][b], second_want[1][b], second_want[2][b], m, n) for b in range(4)]
    second = _solve(first[:3], 2, m, n)
    _compare(second, (second_want[0], second_want[1], second_want[2], us), "%s pivots [%d, %d) after [0, %d)" %
             (tag, m, n, m))
    _compare(second[:3] + ([p + q for p, q in zip(first[3], second[3])],), whole, "%s in two ranges" % tag)


NAN_SENTINEL = {np.float64: np.uint64(0x7FF80000DEADBEEF), np.float32: np.uint32(0x7FC0BEEF)}
INT_SENTINEL = 0x5A5A5A5A
GUARD_BYTE, GUARD_BYTES = 0xA5, 1 << 16


@pytest.mark.parametrize("dtype,n,min_n", [(np.float64, 257, None), (np.float32, 259, None),
                                           (np.float64, B + 3, "1"), (np.float32, B + 3, "1")])
def test_device_form_with_a_stride_counters_a_stream_and_scratch_for_three(dtype, n, min_n, monkeypatch):
    """fwx_dev_solve_batch_large on caller-owned device memory and a caller's non-default stream, 8 matrices n*n + 37
    elements apart (f64 with odd n: rows and matrices off 16-byte alignment): the gaps hold sentinels and come back
    bit-identical, the per-matrix counters are INCREMENTED (pre-loaded with 3 + b).  The scratch holds exactly three
    matrices -- groups of 3, 3 and 2 -- and the guard region behind it comes back untouched; scratch for all eight
    gives the same bits."""
    from floydwarshall_amd import hip
    if min_n is None:
        monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    else:
        monkeypatch.setenv("FWX_BATCH_LARGE_MIN_N", min_n)
    name = np.dtype(dtype).name
    count, stride = 8, n * n + 37
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
    per = _lib.batch_large_scratch_bytes(n)
    s = hip.Stream()
    for groups_of in (3, count):
        d = [dev(a) for a in flat]
        upd = dev(np.arange(3, 3 + count, dtype=np.uint64))
        scratch = dev(np.full(groups_of * per + GUARD_BYTES, GUARD_BYTE, dtype=np.uint8))
        assert scratch.data_ptr() % 16 == 0
        lib_status = _lib.lib().fwx_dev_solve_batch_large(
            count, n, _lib.FWX_F64 if dtype == np.float64 else _lib.FWX_F32, ctypes.c_void_p(d[0].data_ptr()),
            ctypes.c_void_p(d[1].data_ptr()), ctypes.c_void_p(d[2].data_ptr()), stride, 0, 0,
            ctypes.c_void_p(upd.data_ptr()), ctypes.c_void_p(scratch.data_ptr()), groups_of * per + 15, s.ptr)     # floor(bytes / per) = groups_of
        _lib.check(lib_status, "fwx_dev_solve_batch_large")
        s.synchronize()
        tag = "n=%d %s scratch for %d" % (n, name, groups_of)
        for f, field in enumerate(("rate", "next", "hops")):
            assert_bits_equal(host(d[f]), expect[f], "%s %s with gaps" % (tag, field))
        assert [int(u) for u in host(upd)] == [3 + b + u for b, u in enumerate(want[3])], tag
        guard = host(scratch)[groups_of * per:]
        assert guard.size == GUARD_BYTES and (guard == GUARD_BYTE).all(), "%s: the guard region was written" % tag
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_python_device_wrapper_allocates_its_scratch(dtype, monkeypatch):
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    from floydwarshall_amd import hip
    name = np.dtype(dtype).name
    n, count = 257, 4
    batch = _synth_batch(n, count, name)
    want = _want(("synth", n, count, name), batch)
    d = [dev(a) for a in batch]
    upd = dev(np.zeros(count, dtype=np.uint64))
    s = hip.Stream()
    scratch = engine.dev_solve_batch_large(d[0], count, n, next_t=d[1], hops_t=d[2], updates_t=upd, stream=s)
    s.synchronize()
    assert scratch.numel() * scratch.element_size() >= count * _lib.batch_large_scratch_bytes(n)
    _compare((host(d[0]), host(d[1]), host(d[2]), [int(u) for u in host(upd)]), want, "n=257 %s wrapper" % name)
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_more_workgroups_than_the_chip_holds(dtype, monkeypatch):
    """4 distinct matrices of order 257 tiled to 64: every copy equals its oracle."""
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    name = np.dtype(dtype).name
    n, count = 257, 64
    batch = _synth_batch(n, 4, name)
    want = _want(("synth", n, 4, name), batch)
    _not_vacuous(n, want)
    tiled = tuple(np.ascontiguousarray(np.tile(a, (count // 4, 1, 1))) for a in batch)
    got = _solve(tiled, 2)
    for f, field in enumerate(("rate", "next", "hops")):
        assert_bits_equal(got[f], np.tile(want[f], (count // 4, 1, 1)), "64 x n=257 %s %s" % (name, field))
    assert got[3] == want[3] * (count // 4)


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_form_updates_each_and_updates_out(dtype, monkeypatch):
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    name = np.dtype(dtype).name
    n, count = 258, 4
    batch = _synth_batch(n, count, name)
    want = _want(("synth", n, count, name), batch)
    _not_vacuous(n, want)
    r, x, h = (a.copy() for a in batch)
    each = np.full(count, 99, dtype=np.uint64)
    total = ctypes.c_uint64(99)
    o = _lib.FwxOpts()
    o.struct_size, o.device = ctypes.sizeof(_lib.FwxOpts), -1
    o.updates_out = ctypes.pointer(total)
    fn = _lib.lib().fwx_solve_batch_large_f64 if dtype == np.float64 else _lib.lib().fwx_solve_batch_large_f32
    _lib.check(fn(count, n, r.ctypes.data, x.ctypes.data, h.ctypes.data, each.ctypes.data, ctypes.byref(o)),
               "fwx_solve_batch_large")
    assert [int(u) for u in each] == want[3]
    assert total.value == sum(want[3])
    _compare((r, x, h, want[3]), want, "n=258 %s with updates_out" % name)
    # updates_out alone, and the mid entry point still refuses the order
    total.value = 99
    r2 = batch[0].copy()
    _lib.check(fn(count, n, r2.ctypes.data, None, None, None, ctypes.byref(o)), "fwx_solve_batch_large")
    assert total.value == sum(want[3])
    assert_bits_equal(r2, want[0], "n=258 %s rates only with updates_out" % name)
    with pytest.raises(engine.FwxError) as e:
        engine.solve_batch_mid(batch[0].copy())
    assert e.value.status == _lib.FWX_ERR_UNSUPPORTED
