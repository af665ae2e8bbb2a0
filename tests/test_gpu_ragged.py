"""Ragged batched small solves on the GPU (fwx_solve_ragged_f64 / _f32, fwx_dev_solve_ragged): matrices of DIFFERENT
orders in one call, every matrix bit for bit what the oracle's loop (oracle.relax) leaves of that matrix alone --
rates, next, hops (diagonals included) and U.

Three launches run a ragged batch, one per tier: one wave per matrix (n <= FWX_BATCH_WAVE_MAX_N <= 16), small_solve's
body at the 64-wide tile and at the 128-wide tile.  FWX_BATCH_WAVE_MAX_N = 16 / 4 / 0 moves the first boundary, so the
same input goes through different tiers.  The PACKED arrays are compared whole: a matrix that wrote into its
neighbour shows there.

Inputs: matrix b of a batch is synth.make(kind, n_b, dtype, seed) with the kinds cycling d1, d2, t1, t3 over b and the
seeds ascending from one counter; at n_b >= 4 the first seed is taken whose matrix the ORACLE relaxes (U > 0), so no
matrix is vacuous (n <= 2 has no relaxation at all and n = 3 sometimes none; those orders pin "nothing else is
touched").  Hostile batches are draws of hostile_matrix_mix from one seeded generator.  The oracle runs once per input
and is shared."""
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
EDGE_ORDERS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 33, 63, 64, 65, 127, 128]
HOSTILE_ORDERS = [4, 5, 16, 17, 64, 65, 128]
NAN_SENTINEL = {np.float64: np.uint64(0x7FF80000DEADBEEF), np.float32: np.uint32(0x7FC0BEEF)}
INT_SENTINEL = 0x5A5A5A5A


def _name(dtype):
    return np.dtype(dtype).name


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


class _Batch:
    """A ragged batch: the input matrices, the oracle's solution of each and its U; packed forms of both."""

    def __init__(self, parts):
        self.parts = tuple(_frozen(*(np.ascontiguousarray(a) for a in p)) for p in parts)
        self.orders = [p[0].shape[0] for p in self.parts]
        self.count = len(self.parts)
        self.solved, self.us = [], []
        for p in self.parts:
            r, x, h = (a.copy() for a in p)
            self.us.append(int(oracle.relax(r, x, h)) if r.shape[0] else 0)
            self.solved.append(_frozen(r, x, h))
        self.n_each = np.array(self.orders, dtype=np.int32)
        self.offset = np.concatenate([[0], np.cumsum([n * n for n in self.orders])]).astype(np.int64)

    def packed(self, which, f):
        dt = self.parts[0][f].dtype if self.parts else np.float64
        return np.concatenate([p[f].reshape(-1) for p in which] + [np.zeros(0, dtype=dt)])

    def not_vacuous(self):
        for b, (n, u) in enumerate(zip(self.orders, self.us)):
            if n >= 4:
                assert u > 0, "the oracle relaxes nothing in matrix %d (order %d)" % (b, n)


def _empty(dtype):
    return np.zeros((0, 0), dtype=dtype), np.zeros((0, 0), dtype=np.int32), np.zeros((0, 0), dtype=np.int32)


def _synth_parts(orders, dtype, seed):
    parts = []
    for b, n in enumerate(orders):
        if n == 0:
            parts.append(_empty(dtype))
            continue
        while True:
            p = synth.make(KINDS[b % 4], n, dtype, seed=seed)
            seed += 1
            if n < 4 or oracle.relax(*(a.copy() for a in p)) > 0:
                break
        parts.append(p)
    return parts


@functools.lru_cache(maxsize=None)
def _edge_batch(dtype_name):
    """Every order at which a tile, a row group or a tier changes, each twice, in a seeded shuffle."""
    orders = [int(n) for n in np.random.default_rng(31).permutation(EDGE_ORDERS + EDGE_ORDERS)]
    return _Batch(_synth_parts(orders, np.dtype(dtype_name).type, synth.BASE_SEED + 5000))


@functools.lru_cache(maxsize=None)
def _cycle_batch(lo, hi, count, dtype_name):
    orders = [lo + b % (hi - lo + 1) for b in range(count)]
    return _Batch(_synth_parts(orders, np.dtype(dtype_name).type, synth.BASE_SEED + 6000 + lo))


@functools.lru_cache(maxsize=None)
def _orders_batch(orders, dtype_name):
    return _Batch(_synth_parts(list(orders), np.dtype(dtype_name).type, synth.BASE_SEED + 7000 + sum(orders)))


@functools.lru_cache(maxsize=None)
def _hostile_batch(dtype_name):
    """Draws from ONE seeded generator at the orders 4, 5, 16, 17, 64, 65, 128 in turn, two rounds at least, continued
    until both mixes of hostile_matrix_mix have occurred."""
    dtype = np.dtype(dtype_name).type
    rnd = np.random.default_rng(9100)
    parts, seen = [], set()
    while len(parts) < 2 * len(HOSTILE_ORDERS) or len(seen) < 2:
        assert len(parts) < 6 * len(HOSTILE_ORDERS), "the seeded draws never produced both mixes"
        r, x, h, heavy = hostile_matrix_mix(rnd, HOSTILE_ORDERS[len(parts) % len(HOSTILE_ORDERS)], dtype)
        parts.append((r, x, h))
        seen.add(heavy)
    assert seen == {False, True}
    return _Batch(parts)


def _outside_the_domain(rate):
    """An off-diagonal rate that is NaN, infinite or negative: the reference's domain has none."""
    off = ~np.eye(rate.shape[0], dtype=bool)
    with np.errstate(invalid="ignore"):
        return bool((~(rate >= 0) | np.isinf(rate))[off].any())


def _solve_packed(batch, fields, each=True):
    """fwx_solve_ragged_* as the C caller sees it, on the packed arrays: (rate, next, hops, [U_b])."""
    got = [batch.packed(batch.parts, f) if f <= fields else None for f in range(3)]
    us = np.full(batch.count, 99, dtype=np.uint64) if each else None
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    fn = _lib.lib().fwx_solve_ragged_f64 if got[0].dtype == np.float64 else _lib.lib().fwx_solve_ragged_f32
    _lib.check(fn(batch.count, p(batch.n_each), p(got[0]), p(got[1]), p(got[2]), p(us), None), "fwx_solve_ragged")
    return got[0], got[1], got[2], None if us is None else [int(u) for u in us]


def _compare_packed(batch, got, what):
    for f, field in enumerate(("rate", "next", "hops")):
        if got[f] is not None:
            assert_bits_equal(got[f], batch.packed(batch.solved, f), "%s packed %s" % (what, field))
    if got[3] is not None:
        assert got[3] == batch.us, "%s: U per matrix %s, the oracle's %s" % (what, got[3], batch.us)


def _tiers_of(batch):
    wave_max_n = _lib.lib().fwx_test_batch_wave_max_n()
    return [None if n == 0 else 0 if n <= wave_max_n else 1 if n <= 64 else 2 for n in batch.orders]


# ---- 1. tier edges in one batch ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("wave", ["16", "4", "0"])
def test_tier_edges_in_one_batch(wave, dtype, monkeypatch):
    """Thirty matrices of every edge order, shuffled, in one call; rates only, + next, + hops."""
    monkeypatch.setenv("FWX_BATCH_WAVE_MAX_N", wave)
    batch = _edge_batch(_name(dtype))
    assert sorted(batch.orders) == sorted(EDGE_ORDERS + EDGE_ORDERS)
    batch.not_vacuous()
    tiers = _tiers_of(batch)
    assert {t for t in tiers if t is not None} == ({0, 1, 2} if wave != "0" else {1, 2})
    for fields in (0, 1, 2):
        _compare_packed(batch, _solve_packed(batch, fields), "edges wave<=%s %s fields=%d" % (wave, _name(dtype), fields))
    _compare_packed(batch, _solve_packed(batch, 2, each=False), "edges wave<=%s %s no counters" % (wave, _name(dtype)))


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_python_binding_solves_in_place(dtype, monkeypatch):
    """engine.solve_ragged packs a sequence of matrices and writes every one of them back."""
    monkeypatch.delenv("FWX_BATCH_WAVE_MAX_N", raising=False)
    batch = _edge_batch(_name(dtype))
    batch.not_vacuous()
    mats = [[p[f].copy() for p in batch.parts] for f in range(3)]
    us = engine.solve_ragged(mats[0], mats[1], mats[2], count_updates=True)
    assert [int(u) for u in us] == batch.us
    for b in range(batch.count):
        for f, field in enumerate(("rate", "next", "hops")):
            assert_bits_equal(mats[f][b], batch.solved[b][f], "binding matrix %d %s" % (b, field))
    rates = [p[0].copy() for p in batch.parts]
    assert engine.solve_ragged(rates) is None
    for b in range(batch.count):
        assert_bits_equal(rates[b], batch.solved[b][0], "binding, rates only, matrix %d" % b)


# ---- 2. the device form, with gaps and the matrices out of order ------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("wave", ["16", "0"])
def test_device_form_with_gaps(wave, dtype, monkeypatch):
    """fwx_dev_solve_ragged on caller-owned device memory: the matrices lie in a memory order that is not their index
    order, 1 - 7 sentinel elements before each and after the last.  All six arrays are pre-filled with sentinels; the
    gaps come back untouched, every trace cell inside a matrix has been written, the counters are INCREMENTED."""
    monkeypatch.setenv("FWX_BATCH_WAVE_MAX_N", wave)
    batch = _edge_batch(_name(dtype))
    batch.not_vacuous()
    rnd = np.random.default_rng(77)
    memory_order = [int(b) for b in rnd.permutation(batch.count)]
    assert memory_order != sorted(memory_order)
    offset, at = np.zeros(batch.count, dtype=np.int64), 0
    for b in memory_order:
        at += int(rnd.integers(1, 8))
        offset[b] = at
        at += batch.orders[b] ** 2
    total = at + int(rnd.integers(1, 8))
    bits = np.uint64 if dtype == np.float64 else np.uint32
    flat = [np.full(total, NAN_SENTINEL[dtype], dtype=bits).view(dtype)] + [
        np.full(total, INT_SENTINEL, dtype=np.int32) for _ in range(5)]
    inside = np.zeros(total, dtype=bool)
    for b, n in enumerate(batch.orders):
        inside[offset[b]:offset[b] + n * n] = True
        for f in range(3):
            flat[f][offset[b]:offset[b] + n * n] = batch.parts[b][f].reshape(-1)
    assert int(inside.sum()) == int(batch.offset[-1]) and not inside[0] and not inside[-1]
    expect = [a.copy() for a in flat[:3]]
    for b, n in enumerate(batch.orders):
        for f in range(3):
            expect[f][offset[b]:offset[b] + n * n] = batch.solved[b][f].reshape(-1)
    _, order, tiers = engine.ragged_plan(batch.n_each)
    d = [dev(a) for a in flat]
    upd = dev(np.full(batch.count, 3, dtype=np.uint64))
    d_n, d_off, d_order = dev(batch.n_each), dev(offset), dev(order)
    trace = engine.Trace(0, 0, _views=(d[3], d[4], d[5]))
    engine.dev_solve_ragged(d[0], d_n, d_off, d_order, tiers, next_t=d[1], hops_t=d[2], trace=trace, updates_t=upd)
    what = "gaps wave<=%s %s" % (wave, _name(dtype))
    for f, field in enumerate(("rate", "next", "hops")):
        assert_bits_equal(host(d[f]), expect[f], "%s %s" % (what, field))
    assert [int(u) for u in host(upd)] == [3 + u for u in batch.us]
    for f, field in ((3, "last"), (4, "at_col"), (5, "at_row")):
        t = host(d[f])
        assert (t[~inside] == INT_SENTINEL).all(), "%s: the gap of %s was written" % (what, field)
        assert (t[inside] != INT_SENTINEL).all(), "%s: a cell of %s inside a matrix was not written" % (what, field)
    # without the trace and without counters: the same arrays
    d2 = [dev(a) for a in flat[:3]]
    engine.dev_solve_ragged(d2[0], d_n, d_off, d_order, tiers, next_t=d2[1], hops_t=d2[2])
    for f, field in enumerate(("rate", "next", "hops")):
        assert_bits_equal(host(d2[f]), expect[f], "%s untraced %s" % (what, field))


# ---- 3. equal orders: the uniform batch's answer ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n", [4, 16, 17, 64, 65, 128])
def test_equal_orders_match_the_uniform_batch(n, dtype, monkeypatch):
    """A ragged batch whose orders are all n against engine.solve_batch on the same input, bit for bit, U included."""
    monkeypatch.delenv("FWX_BATCH_WAVE_MAX_N", raising=False)
    batch = _orders_batch((n,) * 6, _name(dtype))
    batch.not_vacuous()
    for fields in (0, 1, 2):
        uni = [np.stack([p[f] for p in batch.parts]) if f <= fields else None for f in range(3)]
        us = engine.solve_batch(uni[0], uni[1], uni[2], count_updates=True)
        got = _solve_packed(batch, fields)
        for f, field in enumerate(("rate", "next", "hops")):
            if uni[f] is not None:
                assert_bits_equal(got[f], uni[f].reshape(-1), "n=%d %s fields=%d %s" % (n, _name(dtype), fields, field))
        assert got[3] == [int(u) for u in us]
    _compare_packed(batch, got, "n=%d %s against the oracle" % (n, _name(dtype)))


# ---- 4. counts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("lo,hi,count,wave", [(1, 16, 1025, "16"), (1, 16, 1025, "0"), (17, 64, 257, "16")])
def test_counts(lo, hi, count, wave, dtype, monkeypatch):
    """1025 wave-tier matrices: 257 workgroups, one of the last one's four waves in use.  257 matrices of the 64-wide
    tier: more workgroups than the chip has CUs."""
    monkeypatch.setenv("FWX_BATCH_WAVE_MAX_N", wave)
    batch = _cycle_batch(lo, hi, count, _name(dtype))
    assert batch.count == count and set(batch.orders) == set(range(lo, hi + 1))
    batch.not_vacuous()
    _compare_packed(batch, _solve_packed(batch, 2), "orders %d..%d count=%d wave<=%s %s" % (lo, hi, count, wave,
                                                                                            _name(dtype)))


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("orders,tier", [((7,), 0), ((40,), 1), ((100,), 2), ((5, 0, 3, 16, 9), 0),
                                         ((17, 64, 40), 1), ((65, 128, 0, 99), 2)])
def test_one_matrix_and_one_tier(orders, tier, dtype, monkeypatch):
    """One matrix; a batch with exactly one non-empty tier, for each tier: the other launches are not made."""
    monkeypatch.delenv("FWX_BATCH_WAVE_MAX_N", raising=False)
    batch = _orders_batch(orders, _name(dtype))
    batch.not_vacuous()
    assert {t for t in _tiers_of(batch) if t is not None} == {tier}
    assert [int(t > 0) for t in engine.ragged_plan(batch.n_each)[2]] == [int(t == tier) for t in range(3)]
    _compare_packed(batch, _solve_packed(batch, 2), "orders %r %s" % (orders, _name(dtype)))


# ---- 5. outside the domain --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("wave", ["16", "0"])
def test_hostile_batch(wave, dtype, monkeypatch):
    """Matrices outside the domain at every tier edge in one batch: no domain check, no routing, every one solved by
    the list rule."""
    monkeypatch.setenv("FWX_BATCH_WAVE_MAX_N", wave)
    batch = _hostile_batch(_name(dtype))
    assert set(batch.orders) == set(HOSTILE_ORDERS)
    batch.not_vacuous()
    tiers = _tiers_of(batch)
    for tier in ((0, 1, 2) if wave != "0" else (1, 2)):
        assert any(t == tier and _outside_the_domain(p[0]) for t, p in zip(tiers, batch.parts)), tier
    _compare_packed(batch, _solve_packed(batch, 2), "hostile wave<=%s %s" % (wave, _name(dtype)))
