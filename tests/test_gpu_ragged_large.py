"""Ragged batches up to order 1024 on the GPU (fwx_solve_ragged_large_f64 / _f32, fwx_dev_solve_ragged_large):
matrices of DIFFERENT orders 0 ... 1024 in one call, every matrix bit for bit what the oracle's loop (oracle.relax)
leaves of that matrix alone -- rates, next, hops (diagonals included) and U.

The four launches of the ragged-mid family run the orders up to 256; the large tier runs the rest as a chain of
launches over its list, sorted by descending order: per block of 16 pivots one panel and one sweep launch over the
ACTIVE PREFIX (the matrices with n > k0), each workgroup finding its slot by binary search in the plan's work table.
FWX_BATCH_LARGE_MIN_N = 1 / 129 / 257 and FWX_BATCH_MID_MIN_N = 1 move the boundaries, so the same input goes through
different tiers.  The PACKED arrays are compared whole: a matrix that wrote into its neighbour shows there.

The orders are the smallest at which the ragged large kernels can go wrong: every smaller tier present (0, 1, 16, 17,
64, 65, 128, 129, 256); 257 and 258; 271 / 272 / 272 / 273 (a matrix that goes inactive exactly at a block edge, a
last block of one pivot, an equal pair); 287 / 288 / 289 (a strip edge); 511 / 512 / 513 / 513 (a tile-column edge,
an equal pair); 1023 and 1024 (the limit, and 1024 alone active over its last blocks).  Inputs as in
test_gpu_ragged_mid.py, whose helpers are used: synth.make with the kinds cycling, at n >= 4 the first seed whose
matrix the ORACLE relaxes (U > 0); hostile batches are draws of hostile_matrix_mix from one seeded generator.  The
oracle runs once per input and is shared."""
import ctypes
import functools

import numpy as np
import pytest

import oracle
from floydwarshall_amd import _lib, engine, hip, synth

from helpers import assert_bits_equal, dev, host
from hostile_inputs import hostile_matrix_mix
from test_gpu_ragged_mid import (INT_SENTINEL, KINDS, _Batch, _Layout, _check_dev, _compare_packed, _empty, _frozen,
                                 _name, _outside_the_domain)

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
EDGE_ORDERS = [0, 1, 16, 17, 64, 65, 128, 129, 256, 257, 258, 271, 272, 272, 273, 287, 288, 289, 511, 512, 513, 513,
               1023, 1024]
HOSTILE_ORDERS = [5, 129, 257, 273, 289]
SETTINGS = ("FWX_BATCH_WAVE_MAX_N", "FWX_BATCH_MID_MIN_N", "FWX_BATCH_LARGE_MIN_N")
GUARD_BYTE, GUARD_BYTES = 0xA5, 1 << 16


def _defaults(monkeypatch):
    for name in SETTINGS:
        monkeypatch.delenv(name, raising=False)


class _Solved:
    """What _Batch(None, of=..., picks=...) reads: inputs with the oracle's solution of each, computed ONCE -- the run
    that picks the seed is the run that is kept."""

    def __init__(self, orders, dtype, seed):
        self.parts, self.solved, self.us = [], [], []
        for b, n in enumerate(orders):
            while True:
                p = _empty(dtype) if n == 0 else synth.make(KINDS[b % 4], n, dtype, seed=seed)
                seed += 1
                r, x, h = (np.ascontiguousarray(a).copy() for a in p)
                u = int(oracle.relax(r, x, h)) if n else 0
                if n < 4 or u > 0:
                    break
            self.parts.append(_frozen(*(np.ascontiguousarray(a) for a in p)))
            self.solved.append(_frozen(r, x, h))
            self.us.append(u)


@functools.lru_cache(maxsize=None)
def _orders_batch(orders, dtype_name, seed=31000):
    base = _Solved(orders, np.dtype(dtype_name).type, synth.BASE_SEED + seed + sum(orders) % 997)
    return _Batch(None, of=base, picks=range(len(orders)))


@functools.lru_cache(maxsize=None)
def _edge_batch(dtype_name):
    """Every edge order in a seeded shuffle."""
    return _orders_batch(tuple(int(n) for n in np.random.default_rng(31).permutation(EDGE_ORDERS)), dtype_name)


@functools.lru_cache(maxsize=None)
def _hostile_batch(dtype_name):
    """Draws from ONE seeded generator at the orders 5, 129, 257, 273, 289 in turn, one round at least, continued
    until both mixes of hostile_matrix_mix have occurred."""
    dtype = np.dtype(dtype_name).type
    rnd = np.random.default_rng(3100)
    parts, seen = [], set()
    while len(parts) < len(HOSTILE_ORDERS) or len(seen) < 2:
        assert len(parts) < 6 * len(HOSTILE_ORDERS), "the seeded draws never produced both mixes"
        r, x, h, heavy = hostile_matrix_mix(rnd, HOSTILE_ORDERS[len(parts) % len(HOSTILE_ORDERS)], dtype)
        parts.append((r, x, h))
        seen.add(heavy)
    assert seen == {False, True}
    return _Batch(parts)


def _solve_packed(batch, fields, each=True):
    """fwx_solve_ragged_large_* as the C caller sees it, on the packed arrays: (rate, next, hops, [U_b])."""
    got = [batch.packed(batch.parts, f) if f <= fields else None for f in range(3)]
    us = np.full(batch.count, 99, dtype=np.uint64) if each else None
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    fn = getattr(_lib.lib(), "fwx_solve_ragged_large_" + ("f64" if got[0].dtype == np.float64 else "f32"))
    _lib.check(fn(batch.count, p(batch.n_each), p(got[0]), p(got[1]), p(got[2]), p(us), None), "fwx_solve_ragged_large")
    return got[0], got[1], got[2], None if us is None else [int(u) for u in us]


def _expected_tier_counts(orders):
    L = _lib.lib()
    wave_max_n, mid_min_n, large_min_n = (L.fwx_test_batch_wave_max_n(), L.fwx_test_batch_mid_min_n(),
                                          L.fwx_test_batch_large_min_n())
    tier = lambda n: (4 if n >= large_min_n else 3 if n >= mid_min_n else 0 if n <= wave_max_n  # noqa: E731
                      else 1 if n <= 64 else 2)
    return [sum(1 for n in orders if n >= 1 and tier(n) == t) for t in range(5)]


# ---- 1. the edge batch --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_edge_orders_in_one_batch(dtype, monkeypatch):
    """Every edge order, shuffled, in one call; rates only, + next, + hops, with and without U."""
    _defaults(monkeypatch)
    batch = _edge_batch(_name(dtype))
    assert sorted(batch.orders) == sorted(EDGE_ORDERS)
    batch.not_vacuous()
    assert all(t > 0 for t in engine.ragged_large_plan(batch.n_each)[2])              # all five tiers are there
    for fields in (2, 1, 0):
        _compare_packed(batch, _solve_packed(batch, fields), "edges %s fields=%d" % (_name(dtype), fields))
    _compare_packed(batch, _solve_packed(batch, 2, each=False), "edges %s no counters" % _name(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("large,mid", [("1", None), ("129", None), ("257", "1")])
def test_tier_routing_changes_no_bit(large, mid, dtype, monkeypatch):
    """The same batch under other boundaries: the tier counts are the plan's, the bits the oracle's (so identical
    among the settings).  large >= 1: every order in the large tier, the orders 1 ... 16 done after one block."""
    _defaults(monkeypatch)
    monkeypatch.setenv("FWX_BATCH_LARGE_MIN_N", large)
    if mid is not None:
        monkeypatch.setenv("FWX_BATCH_MID_MIN_N", mid)
    batch = _edge_batch(_name(dtype))
    batch.not_vacuous()
    tiers = [int(t) for t in engine.ragged_large_plan(batch.n_each)[2]]
    assert tiers == _expected_tier_counts(batch.orders) and sum(tiers) == sum(1 for n in batch.orders if n >= 1)
    if large == "1":
        assert tiers[:4] == [0, 0, 0, 0]
    if mid == "1":
        assert tiers[:3] == [0, 0, 0] and tiers[3] == sum(1 for n in batch.orders if 1 <= n <= 256)
    _compare_packed(batch, _solve_packed(batch, 2), "routing large>=%s mid>=%s %s" % (large, mid, _name(dtype)))


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_python_binding_solves_in_place(dtype, monkeypatch):
    _defaults(monkeypatch)
    batch = _orders_batch((300,), _name(dtype))                                       # a single large matrix
    batch.not_vacuous()
    assert list(engine.ragged_large_plan(batch.n_each)[2]) == [0, 0, 0, 0, 1]
    mats = [[p[f].copy() for p in batch.parts] for f in range(3)]
    us = engine.solve_ragged_large(mats[0], mats[1], mats[2], count_updates=True)
    assert [int(u) for u in us] == batch.us
    for f, field in enumerate(("rate", "next", "hops")):
        assert_bits_equal(mats[f][0], batch.solved[0][f], "binding, one matrix of order 300: %s" % field)


# ---- 2. equal orders: the uniform large call's answer ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_equal_orders_match_the_uniform_large_batch(dtype, monkeypatch):
    _defaults(monkeypatch)
    batch = _orders_batch((289,) * 5, _name(dtype))
    batch.not_vacuous()
    for fields in (0, 1, 2):
        uni = [np.stack([p[f] for p in batch.parts]) if f <= fields else None for f in range(3)]
        us = engine.solve_batch_large(uni[0], uni[1], uni[2], count_updates=True)
        got = _solve_packed(batch, fields)
        for f, field in enumerate(("rate", "next", "hops")):
            if uni[f] is not None:
                assert_bits_equal(got[f], uni[f].reshape(-1), "n=289 %s fields=%d %s" % (_name(dtype), fields, field))
        assert got[3] == [int(u) for u in us]
    _compare_packed(batch, got, "n=289 %s against the oracle" % _name(dtype))


# ---- 3. a long table ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_a_long_table_of_slots_with_equal_strip_counts(dtype, monkeypatch):
    """300 matrices of the orders 257 ... 268 in turn (24 distinct matrices, repeated), three of order 513 among them:
    the slot search runs over 300 slots, most of them with the same number of strips.  U is checked per matrix."""
    _defaults(monkeypatch)
    base = _orders_batch(tuple(257 + b % 12 for b in range(24)) + (513,), _name(dtype))
    base.not_vacuous()
    batch = _Batch(None, of=base, picks=[24 if b in (7, 150, 299) else b % 24 for b in range(300)])
    assert batch.orders[:9] == [257, 258, 259, 260, 261, 262, 263, 513, 265]
    assert list(engine.ragged_large_plan(batch.n_each)[2]) == [0, 0, 0, 0, 300]
    _compare_packed(batch, _solve_packed(batch, 2), "300 matrices %s" % _name(dtype))


# ---- 4. outside the domain ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_hostile_batch(dtype, monkeypatch):
    """Matrices outside the domain in the wave, the mid and the large tier of one batch: no domain check, no routing by
    content."""
    _defaults(monkeypatch)
    batch = _hostile_batch(_name(dtype))
    assert set(batch.orders) == set(HOSTILE_ORDERS)
    batch.not_vacuous()
    assert any(n >= 257 and _outside_the_domain(p[0]) for n, p in zip(batch.orders, batch.parts))
    _compare_packed(batch, _solve_packed(batch, 2), "hostile %s" % _name(dtype))


# ---- 5. the device form ---------------------------------------------------------------------------------------------
def _dev_run(lay, order, tiers, work, *, traced=True, stream=None, preload=3, scratch_bytes=None, table=True):
    """fwx_dev_solve_ragged_large on the layout.  scratch_bytes: the scratch the call is told of, GUARD_BYTES of guard
    behind it (default: room for every slot).  Returns the six arrays, the counters and the guard."""
    batch = lay.batch
    d = [dev(a) for a in lay.flat]
    upd = dev(np.full(batch.count, preload, dtype=np.uint64))
    d_n, d_off, d_order = dev(batch.n_each), dev(lay.offset), dev(np.ascontiguousarray(order, dtype=np.int32))
    trace = engine.Trace(0, 0, _views=(d[3], d[4], d[5])) if traced else None
    work_t = scratch = None
    if table:
        work_t = dev(np.ascontiguousarray(work))
        if scratch_bytes is None:
            scratch_bytes = _lib.batch_large_scratch_bytes(int(work[0, int(tiers[4])]))
        scratch = dev(np.full(scratch_bytes + GUARD_BYTES, GUARD_BYTE, dtype=np.uint8))
    engine.dev_solve_ragged_large(d[0], d_n, d_off, d_order, tiers, work if table else None, work_t, next_t=d[1],
                                  hops_t=d[2], trace=trace, updates_t=upd, scratch_t=scratch,
                                  scratch_bytes=scratch_bytes, stream=stream)
    if stream is not None:
        stream.synchronize()
    guard = host(scratch)[scratch_bytes:] if table else None
    return [host(a) for a in d], [int(u) for u in host(upd)], guard


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_device_form_reverse_layout_gaps_counters_stream_and_groups(dtype, monkeypatch):
    """fwx_dev_solve_ragged_large on caller-owned memory and a caller's stream: reverse memory order, sentinel gaps
    that survive in all six arrays, every trace cell inside a matrix written (none without a trace), counters
    pre-loaded and INCREMENTED by U -- once with scratch for every slot, once with scratch for the largest order alone
    (several groups): the same bits, and the bytes behind the scratch survive."""
    _defaults(monkeypatch)
    batch = _edge_batch(_name(dtype))
    batch.not_vacuous()
    lay = _Layout(batch, dtype)
    _, order, tiers, work = engine.ragged_large_plan(batch.n_each)
    everything = {b for b, n in enumerate(batch.orders) if n >= 1}
    stream = hip.Stream()
    got, us, guard = _dev_run(lay, order, tiers, work, stream=stream)
    stream.close()
    _check_dev(lay, got, us, everything, "device form %s" % _name(dtype))
    assert (guard == GUARD_BYTE).all()
    tight = _lib.batch_large_scratch_bytes(max(batch.orders))
    first = np.zeros(64, dtype=np.int32)
    groups = _lib.lib().fwx_test_ragged_large_schedule(batch.count, int(tiers[4]), work.ctypes.data, tight,
                                                       first.ctypes.data, 64, None)
    assert groups >= 4, groups
    again, us, guard = _dev_run(lay, order, tiers, work, scratch_bytes=tight)
    _check_dev(lay, again, us, everything, "device form, %d groups %s" % (groups, _name(dtype)))
    assert (guard == GUARD_BYTE).all(), "bytes behind the scratch were written"
    for f in range(6):
        assert np.array_equal(got[f].view(np.uint8), again[f].view(np.uint8)), f
    got, us, guard = _dev_run(lay, order, tiers, work, traced=False, preload=0, scratch_bytes=tight)
    _check_dev(lay, got, us, everything, "device form untraced %s" % _name(dtype), preload=0, traced=False)
    assert all((got[f] == INT_SENTINEL).all() for f in (3, 4, 5)), "a trace cell was written without a trace"
    assert (guard == GUARD_BYTE).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_device_form_without_a_large_matrix_needs_no_table(dtype, monkeypatch):
    """Every order at most 256: NULL work table, NULL scratch."""
    _defaults(monkeypatch)
    batch = _orders_batch((129, 5, 17, 256, 0, 64), _name(dtype))
    batch.not_vacuous()
    lay = _Layout(batch, dtype, seed=4)
    _, order, tiers, work = engine.ragged_large_plan(batch.n_each)
    assert list(tiers) == [1, 2, 0, 2, 0] and not work.any()
    got, us, _ = _dev_run(lay, order, tiers, work, table=False)
    _check_dev(lay, got, us, {0, 1, 2, 3, 5}, "no large matrix %s" % _name(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_device_form_hostile_plan_idles_workgroups(dtype, monkeypatch):
    """A large list that holds the ids -1, count and 2^31 - 1 among real ones, the work table the plan's for the
    listed orders: those workgroups leave before touching anything, every matrix not listed stays as it was, and the
    call returns."""
    _defaults(monkeypatch)
    batch = _orders_batch((300, 5, 273, 257, 64, 258), _name(dtype))
    batch.not_vacuous()
    lay = _Layout(batch, dtype, seed=5)
    # slots by descending order: 300 (matrix 0), three slots of nobody's at 290 / 280 / 270, 257 (matrix 3), one at 257
    listed = [300, 290, 280, 270, 257, 257]
    order = np.array([0, -1, batch.count, 2**31 - 1, 3, -1], dtype=np.int32)
    work = engine.ragged_large_plan(listed)[3]
    assert work.shape == (3, batch.count + 1) and work[0, 6] == sum(listed)
    got, us, guard = _dev_run(lay, order, [0, 0, 0, 0, 6], work)
    _check_dev(lay, got, us, {0, 3}, "hostile plan %s" % _name(dtype))
    assert (guard == GUARD_BYTE).all()
