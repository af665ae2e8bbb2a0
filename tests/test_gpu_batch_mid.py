"""Batched mid-size solves on the GPU (fwx_solve_batch_mid_f64 / _f32, fwx_dev_solve_batch_mid): `count` matrices of
one order n <= 256 in one launch, every matrix bit for bit what the oracle's loop (oracle.relax) leaves of that
matrix alone -- rates, next, hops (diagonals included) and U.

Orders from FWX_BATCH_MID_MIN_N (default 129) up run the mid tier: one workgroup per matrix, the matrix resident in
device memory, B pivots per pass from snapshot panels in LDS (B = fwx_test_batch_mid_block()).  FWX_BATCH_MID_MIN_N=1
puts small orders through the same kernel, where the existing tiers give a second answer.

Inputs as in test_gpu_batch.py: matrix b of a batch is synth.make(kind, n, dtype, seed) with the kinds cycling d1, d2,
t1, t3 and one seed per matrix, or hostile_matrix_mix draws from one seeded generator.  No case is vacuous: in every
batch of order n >= 4 the ORACLE's U is > 0 for every matrix.  The oracle runs once per input and is shared."""
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
B = _lib.lib().fwx_test_batch_mid_block()


def _nearest_multiple(target):
    """The multiple of B strictly inside (129, 256) nearest `target`."""
    ms = [m for m in range(B, 256, B) if 129 < m < 256]
    return min(ms, key=lambda m: (abs(m - target), m))


MID_ORDERS = sorted({129, 130, 131, 255, 256}
                    | {m + d for m in (_nearest_multiple(144), _nearest_multiple(192)) for d in (-1, 0, 1)})
SMALL_ORDERS = sorted({1, 2, 3, 4, 5, B - 1, B, B + 1, 2 * B + 1, 63, 64, 65, 127, 128} - {0})


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
def _hostile_batch(n, dtype_name):
    """At least 8 draws from one seeded generator, continued until both mixes of hostile_matrix_mix have occurred."""
    dtype = np.dtype(dtype_name).type
    rnd = np.random.default_rng(9500 + n)
    parts, seen = [], set()
    while len(parts) < 8 or len(seen) < 2:
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
    """engine.solve_batch_mid on copies of the first `fields` + 1 arrays of the batch: (rate, next, hops, [U_b])."""
    got = [batch[f].copy() if f <= fields else None for f in range(3)]
    us = (fn or engine.solve_batch_mid)(got[0], got[1], got[2], k_begin=kb, k_end=ke, count_updates=True)
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


def test_the_order_lists_are_what_the_block_width_makes_them():
    assert 1 <= B <= 64
    assert {129, 130, 131, 255, 256} <= set(MID_ORDERS) and all(129 <= n <= 256 for n in MID_ORDERS)
    assert any(n % B == 0 for n in MID_ORDERS)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", MID_ORDERS)
def test_default_routing_orders_and_fields(n, dtype, monkeypatch):
    """Eight matrices at 129, 256, both sides of them and around two multiples of B; rates only, + next, + hops."""
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    name = np.dtype(dtype).name
    batch = _synth_batch(n, 8, name)
    want = _want(("synth", n, 8, name), batch)
    _not_vacuous(n, want)
    for fields in (0, 1, 2):
        _compare(_solve(batch, fields), want, "n=%d %s fields=%d" % (n, name, fields))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [129, 256])
def test_hostile_batches(n, dtype, monkeypatch):
    """Matrices outside the domain side by side with ordinary ones: no domain check, no routing, every one solved by
    the list rule (a positive rate with next = -1 hands the head of kjPath on)."""
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    name = np.dtype(dtype).name
    batch = _hostile_batch(n, name)
    assert batch[0].shape[0] >= 8
    want = _want(("hostile", n, name), batch)
    _not_vacuous(n, want)
    _compare(_solve(batch, 2), want, "hostile n=%d %s" % (n, name))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SMALL_ORDERS)
def test_small_orders_through_the_mid_kernel(n, dtype, monkeypatch):
    """FWX_BATCH_MID_MIN_N=1: the mid kernel at orders the existing tiers also solve -- against the oracle and
    against engine.solve_batch on the same input; the hostile draws at the same order too."""
    monkeypatch.setenv("FWX_BATCH_MID_MIN_N", "1")
    name = np.dtype(dtype).name
    for key, batch in ((("synth", n, 8, name), _synth_batch(n, 8, name)),
                       (("hostile", n, name), _hostile_batch(n, name))):
        want = _want(key, batch)
        _not_vacuous(n, want)
        for fields in (0, 1, 2):
            _compare(_solve(batch, fields), want, "%s n=%d %s fields=%d" % (key[0], n, name, fields))
        other = _solve(batch, 2, fn=engine.solve_batch)
        _compare(_solve(batch, 2), other, "%s n=%d %s against solve_batch" % (key[0], n, name))


def test_below_the_threshold_the_call_is_forwarded(monkeypatch):
    """Default routing at n <= 128 and a threshold in between: the same bits as solve_batch."""
    batch = _synth_batch(64, 8, "float64")
    want = _want(("synth", 64, 8, "float64"), batch)
    for value in (None, "65", "64"):
        if value is None:
            monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
        else:
            monkeypatch.setenv("FWX_BATCH_MID_MIN_N", value)
        _compare(_solve(batch, 2), want, "n=64 FWX_BATCH_MID_MIN_N=%s" % value)


def _range_cases(n):
    inside = (B + 2, min(B + 7, n)) if n > 2 * B else (2, 7)      # starts and ends inside one block
    return [(0, 1), (5, 5), (7, n - 2), (n - 1, n), inside]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m", [(131, 2 * B + 5), (B + 3, 7)])
def test_pivot_ranges(n, m, dtype, monkeypatch):
    """One range for every matrix, through (k_begin, k_end): each range alone equals the oracle over it; [0, m) then
    [m, n), m off a block boundary, equal the whole solve, U included."""
    monkeypatch.setenv("FWX_BATCH_MID_MIN_N", "1")
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


@pytest.mark.parametrize("dtype,n,min_n", [(np.float64, 129, None), (np.float64, 255, None), (np.float32, 131, None),
                                           (np.float64, B + 3, "1"), (np.float32, B + 3, "1")])
def test_device_form_with_a_stride_counters_and_a_stream(dtype, n, min_n, monkeypatch):
    """fwx_dev_solve_batch_mid on caller-owned device memory and a caller's non-default stream, matrices n*n + 37
    elements apart (f64 with odd n: rows and matrices off 16-byte alignment): the gaps hold sentinels and come back
    bit-identical, the per-matrix counters are INCREMENTED (pre-loaded with 3 + b)."""
    from floydwarshall_amd import hip
    if min_n is None:
        monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    else:
        monkeypatch.setenv("FWX_BATCH_MID_MIN_N", min_n)
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
    d = [dev(a) for a in flat]
    upd = dev(np.arange(3, 3 + count, dtype=np.uint64))
    s = hip.Stream()
    engine.dev_solve_batch_mid(d[0], count, n, next_t=d[1], hops_t=d[2], stride=stride, updates_t=upd, stream=s)
    s.synchronize()
    for f, field in enumerate(("rate", "next", "hops")):
        assert_bits_equal(host(d[f]), expect[f], "n=%d %s %s with gaps" % (n, name, field))
    assert [int(u) for u in host(upd)] == [3 + b + u for b, u in enumerate(want[3])]
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_more_workgroups_than_cus(dtype, monkeypatch):
    """8 distinct matrices of order 129 tiled to 520 workgroups: every copy equals its oracle."""
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    name = np.dtype(dtype).name
    n, count = 129, 520
    batch = _synth_batch(n, 8, name)
    want = _want(("synth", n, 8, name), batch)
    _not_vacuous(n, want)
    tiled = tuple(np.ascontiguousarray(np.tile(a, (count // 8, 1, 1))) for a in batch)
    got = _solve(tiled, 2)
    for f, field in enumerate(("rate", "next", "hops")):
        assert_bits_equal(got[f], np.tile(want[f], (count // 8, 1, 1)), "520 x n=129 %s %s" % (name, field))
    assert got[3] == want[3] * (count // 8)


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_form_updates_each_and_updates_out(dtype, monkeypatch):
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    name = np.dtype(dtype).name
    n, count = 130, 8
    batch = _synth_batch(n, count, name)
    want = _want(("synth", n, count, name), batch)
    _not_vacuous(n, want)
    r, x, h = (a.copy() for a in batch)
    each = np.full(count, 99, dtype=np.uint64)
    total = ctypes.c_uint64(99)
    o = _lib.FwxOpts()
    o.struct_size, o.device = ctypes.sizeof(_lib.FwxOpts), -1
    o.updates_out = ctypes.pointer(total)
    fn = _lib.lib().fwx_solve_batch_mid_f64 if dtype == np.float64 else _lib.lib().fwx_solve_batch_mid_f32
    _lib.check(fn(count, n, r.ctypes.data, x.ctypes.data, h.ctypes.data, each.ctypes.data, ctypes.byref(o)),
               "fwx_solve_batch_mid")
    assert [int(u) for u in each] == want[3]
    assert total.value == sum(want[3])
    _compare((r, x, h, want[3]), want, "n=130 %s with updates_out" % name)
    # updates_out alone, and the existing entry points still refuse the order
    total.value = 99
    r2 = batch[0].copy()
    _lib.check(fn(count, n, r2.ctypes.data, None, None, None, ctypes.byref(o)), "fwx_solve_batch_mid")
    assert total.value == sum(want[3])
    assert_bits_equal(r2, want[0], "n=130 %s rates only with updates_out" % name)
    with pytest.raises(engine.FwxError) as e:
        engine.solve_batch(batch[0].copy())
    assert e.value.status == _lib.FWX_ERR_UNSUPPORTED
