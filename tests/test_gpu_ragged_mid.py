"""Ragged batches up to order 256 on the GPU (fwx_solve_ragged_mid_f64 / _f32, fwx_dev_solve_ragged_mid): matrices of
DIFFERENT orders 0 ... 256 in one call, every matrix bit for bit what the oracle's loop (oracle.relax) leaves of that
matrix alone -- rates, next, hops (diagonals included) and U.

Four launches run such a batch, one per tier: the three of the ragged small solves and the mid tier (one workgroup per
matrix, the matrix resident in device memory, 16 pivots per pass; mid_solve_ragged reads an order and an offset per
workgroup).  FWX_BATCH_MID_MIN_N = 1 / 65 / 129 and FWX_BATCH_WAVE_MAX_N = 0 / 16 move the boundaries, so the same
input goes through different tiers.  The PACKED arrays are compared whole: a matrix that wrote into its neighbour
shows there.

The orders are the smallest at which the mid kernel can go wrong: 129 (the first mid order), 143 / 144 / 145 (an edge
of the 16-pivot pass), 191 / 192 / 193 (the column width goes from 192 to 256 lanes, 1024 / 192 leaves one wave idle),
255 / 256 (the limit), and the small tiers' own edges.  Inputs as in test_gpu_ragged.py: synth.make with the kinds
cycling, at n >= 4 the first seed whose matrix the ORACLE relaxes (U > 0); hostile batches are draws of
hostile_matrix_mix from one seeded generator.  The oracle runs once per input and is shared."""
import ctypes
import functools

import numpy as np
import pytest

import oracle
from floydwarshall_amd import _lib, engine, hip, synth

from helpers import assert_bits_equal, dev, host
from hostile_inputs import hostile_matrix_mix

pytestmark = pytest.mark.gpu

KINDS = ("d1", "d2", "t1", "t3")
DTYPES = [np.float64, np.float32]
EDGE_ORDERS = [0, 1, 2, 3, 4, 16, 17, 64, 65, 128, 129, 130, 143, 144, 145, 191, 192, 193, 255, 256]
HOSTILE_ORDERS = [5, 17, 65, 129, 145, 192, 256]
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

    def __init__(self, parts, of=None, picks=None):
        if of is not None:                      # matrices picks[b] of the batch `of`, its oracle runs reused
            self.parts = tuple(of.parts[i] for i in picks)
            self.solved, self.us = [of.solved[i] for i in picks], [of.us[i] for i in picks]
        else:
            self.parts = tuple(_frozen(*(np.ascontiguousarray(a) for a in p)) for p in parts)
            self.solved, self.us = [], []
            for p in self.parts:
                r, x, h = (a.copy() for a in p)
                self.us.append(int(oracle.relax(r, x, h)) if r.shape[0] else 0)
                self.solved.append(_frozen(r, x, h))
        self.orders = [p[0].shape[0] for p in self.parts]
        self.count = len(self.parts)
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
    """Every edge order, each twice, in a seeded shuffle."""
    orders = [int(n) for n in np.random.default_rng(22).permutation(EDGE_ORDERS + EDGE_ORDERS)]
    return _Batch(_synth_parts(orders, np.dtype(dtype_name).type, synth.BASE_SEED + 22000))


@functools.lru_cache(maxsize=None)
def _orders_batch(orders, dtype_name):
    return _Batch(_synth_parts(list(orders), np.dtype(dtype_name).type, synth.BASE_SEED + 23000 + sum(orders) % 997))


@functools.lru_cache(maxsize=None)
def _hostile_batch(dtype_name):
    """Draws from ONE seeded generator at the orders 5, 17, 65, 129, 145, 192, 256 in turn, one round at least,
    continued until both mixes of hostile_matrix_mix have occurred."""
    dtype = np.dtype(dtype_name).type
    rnd = np.random.default_rng(2200)
    parts, seen = [], set()
    while len(parts) < len(HOSTILE_ORDERS) or len(seen) < 2:
        assert len(parts) < 6 * len(HOSTILE_ORDERS), "the seeded draws never produced both mixes"
        r, x, h, heavy = hostile_matrix_mix(rnd, HOSTILE_ORDERS[len(parts) % len(HOSTILE_ORDERS)], dtype)
        parts.append((r, x, h))
        seen.add(heavy)
    assert seen == {False, True}
    return _Batch(parts)


def _outside_the_domain(rate):
    off = ~np.eye(rate.shape[0], dtype=bool)
    with np.errstate(invalid="ignore"):
        return bool((~(rate >= 0) | np.isinf(rate))[off].any())


def _solve_packed(batch, fields, each=True):
    """fwx_solve_ragged_mid_* as the C caller sees it, on the packed arrays: (rate, next, hops, [U_b])."""
    got = [batch.packed(batch.parts, f) if f <= fields else None for f in range(3)]
    us = np.full(batch.count, 99, dtype=np.uint64) if each else None
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    fn = _lib.lib().fwx_solve_ragged_mid_f64 if got[0].dtype == np.float64 else _lib.lib().fwx_solve_ragged_mid_f32
    _lib.check(fn(batch.count, p(batch.n_each), p(got[0]), p(got[1]), p(got[2]), p(us), None), "fwx_solve_ragged_mid")
    return got[0], got[1], got[2], None if us is None else [int(u) for u in us]


def _compare_packed(batch, got, what):
    for f, field in enumerate(("rate", "next", "hops")):
        if got[f] is not None:
            assert_bits_equal(got[f], batch.packed(batch.solved, f), "%s packed %s" % (what, field))
    if got[3] is not None:
        assert got[3] == batch.us, "%s: U per matrix %s, the oracle's %s" % (what, got[3], batch.us)


def _expected_tier_counts(orders):
    wave_max_n, mid_min_n = _lib.lib().fwx_test_batch_wave_max_n(), _lib.lib().fwx_test_batch_mid_min_n()
    tier = lambda n: 3 if n >= mid_min_n else 0 if n <= wave_max_n else 1 if n <= 64 else 2  # noqa: E731
    return [sum(1 for n in orders if n >= 1 and tier(n) == t) for t in range(4)]


# ---- 1. the edge batch --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_edge_orders_in_one_batch(dtype, monkeypatch):
    """Forty matrices of every edge order, shuffled, in one call; rates only, + next, + hops, with and without U."""
    monkeypatch.delenv("FWX_BATCH_WAVE_MAX_N", raising=False)
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    batch = _edge_batch(_name(dtype))
    assert sorted(batch.orders) == sorted(EDGE_ORDERS + EDGE_ORDERS)
    batch.not_vacuous()
    assert all(t > 0 for t in engine.ragged_mid_plan(batch.n_each)[2])                # all four launches are made
    for fields in (2, 1, 0):
        _compare_packed(batch, _solve_packed(batch, fields), "edges %s fields=%d" % (_name(dtype), fields))
    _compare_packed(batch, _solve_packed(batch, 2, each=False), "edges %s no counters" % _name(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("mid,wave", [("1", "16"), ("65", "16"), ("129", "0"), ("129", "16"), ("10", "16")])
def test_tier_routing_changes_no_bit(mid, wave, dtype, monkeypatch):
    """The same batch under other boundaries: the tier counts are the plan's, the bits the oracle's (so identical
    among the settings).  ("10", "16"): both settings claim 10 ... 16, the mid tier takes them."""
    monkeypatch.setenv("FWX_BATCH_MID_MIN_N", mid)
    monkeypatch.setenv("FWX_BATCH_WAVE_MAX_N", wave)
    batch = _edge_batch(_name(dtype))
    tiers = [int(t) for t in engine.ragged_mid_plan(batch.n_each)[2]]
    assert tiers == _expected_tier_counts(batch.orders) and sum(tiers) == sum(1 for n in batch.orders if n >= 1)
    if mid == "1":
        assert tiers[:3] == [0, 0, 0]
    if wave == "0":
        assert tiers[0] == 0
    _compare_packed(batch, _solve_packed(batch, 2), "routing mid>=%s wave<=%s %s" % (mid, wave, _name(dtype)))


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_python_binding_solves_in_place(dtype, monkeypatch):
    monkeypatch.delenv("FWX_BATCH_WAVE_MAX_N", raising=False)
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    batch = _edge_batch(_name(dtype))
    mats = [[p[f].copy() for p in batch.parts] for f in range(3)]
    us = engine.solve_ragged_mid(mats[0], mats[1], mats[2], count_updates=True)
    assert [int(u) for u in us] == batch.us
    for b in range(batch.count):
        for f, field in enumerate(("rate", "next", "hops")):
            assert_bits_equal(mats[f][b], batch.solved[b][f], "binding matrix %d %s" % (b, field))


# ---- 2. outside the domain ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("mid", ["129", "1"])
def test_hostile_batch(mid, dtype, monkeypatch):
    """Matrices outside the domain in every tier of one batch: no domain check, no routing by content."""
    monkeypatch.delenv("FWX_BATCH_WAVE_MAX_N", raising=False)
    monkeypatch.setenv("FWX_BATCH_MID_MIN_N", mid)
    batch = _hostile_batch(_name(dtype))
    assert set(batch.orders) == set(HOSTILE_ORDERS)
    batch.not_vacuous()
    assert any(n >= 129 and _outside_the_domain(p[0]) for n, p in zip(batch.orders, batch.parts))
    _compare_packed(batch, _solve_packed(batch, 2), "hostile mid>=%s %s" % (mid, _name(dtype)))


# ---- 3. the device form -------------------------------------------------------------------------------------------
class _Layout:
    """The matrices of a batch in REVERSE index order in memory, 1 - 7 sentinel elements before each and after the
    last; six sentinel-filled arrays (rate, next, hops, last, at_col, at_row) and what the first three must become."""

    def __init__(self, batch, dtype, seed=77):
        rnd = np.random.default_rng(seed)
        self.offset, at = np.zeros(batch.count, dtype=np.int64), 0
        for b in reversed(range(batch.count)):
            at += int(rnd.integers(1, 8))
            self.offset[b] = at
            at += batch.orders[b] ** 2
        total = at + int(rnd.integers(1, 8))
        bits = np.uint64 if dtype == np.float64 else np.uint32
        self.flat = [np.full(total, NAN_SENTINEL[dtype], dtype=bits).view(dtype)] + [
            np.full(total, INT_SENTINEL, dtype=np.int32) for _ in range(5)]
        self.inside = np.zeros(total, dtype=bool)
        self.batch = batch
        for b, n in enumerate(batch.orders):
            self.inside[self.offset[b]:self.offset[b] + n * n] = True
            for f in range(3):
                self.flat[f][self.offset[b]:self.offset[b] + n * n] = batch.parts[b][f].reshape(-1)
        assert int(self.inside.sum()) == int(batch.offset[-1]) and not self.inside[0] and not self.inside[-1]

    def expect(self, solved):
        """The three arrays with the matrices in `solved` (a set of indices) replaced by the oracle's."""
        out = [a.copy() for a in self.flat[:3]]
        for b in solved:
            n = self.batch.orders[b]
            for f in range(3):
                out[f][self.offset[b]:self.offset[b] + n * n] = self.batch.solved[b][f].reshape(-1)
        return out

    def cells_of(self, which):
        m = np.zeros(len(self.inside), dtype=bool)
        for b in which:
            m[self.offset[b]:self.offset[b] + self.batch.orders[b] ** 2] = True
        return m


def _dev_run(lay, order, tiers, *, traced=True, stream=None, preload=3):
    batch = lay.batch
    d = [dev(a) for a in lay.flat]
    upd = dev(np.full(batch.count, preload, dtype=np.uint64))
    d_n, d_off, d_order = dev(batch.n_each), dev(lay.offset), dev(np.ascontiguousarray(order, dtype=np.int32))
    trace = engine.Trace(0, 0, _views=(d[3], d[4], d[5])) if traced else None
    engine.dev_solve_ragged_mid(d[0], d_n, d_off, d_order, tiers, next_t=d[1], hops_t=d[2], trace=trace,
                                updates_t=upd, stream=stream)
    if stream is not None:
        stream.synchronize()
    return [host(a) for a in d], [int(u) for u in host(upd)]


def _check_dev(lay, got, us, solved, what, preload=3, traced=True):
    batch = lay.batch
    for f, (field, want) in enumerate(zip(("rate", "next", "hops"), lay.expect(solved))):
        assert_bits_equal(got[f], want, "%s %s" % (what, field))
    assert us == [preload + (batch.us[b] if b in solved else 0) for b in range(batch.count)], what
    written = lay.cells_of(solved)
    for f, field in ((3, "last"), (4, "at_col"), (5, "at_row")):
        assert (got[f][~written] == INT_SENTINEL).all(), "%s: %s was written outside the solved matrices" % (what, field)
        if traced:
            assert (got[f][written] != INT_SENTINEL).all(), "%s: a cell of %s inside a matrix was not written" % (what,
                                                                                                                field)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_device_form_reverse_layout_gaps_counters_and_stream(dtype, monkeypatch):
    """fwx_dev_solve_ragged_mid on caller-owned memory and a caller's stream: reverse memory order, sentinel gaps that
    survive, every trace cell inside a matrix written, counters pre-loaded and INCREMENTED by U."""
    monkeypatch.delenv("FWX_BATCH_WAVE_MAX_N", raising=False)
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    batch = _edge_batch(_name(dtype))
    batch.not_vacuous()
    lay = _Layout(batch, dtype)
    _, order, tiers = engine.ragged_mid_plan(batch.n_each)
    everything = {b for b, n in enumerate(batch.orders) if n >= 1}
    stream = hip.Stream()
    got, us = _dev_run(lay, order, tiers, stream=stream)
    stream.close()
    _check_dev(lay, got, us, everything, "device form %s" % _name(dtype))
    got, us = _dev_run(lay, order, tiers, traced=False, preload=0)
    _check_dev(lay, got, us, everything, "device form untraced %s" % _name(dtype), preload=0, traced=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_device_form_hostile_plan_idles_workgroups(dtype, monkeypatch):
    """A mid list that holds the ids -1 and count among real ones: those workgroups leave before touching anything,
    every matrix not listed stays as it was, and the call returns."""
    monkeypatch.delenv("FWX_BATCH_WAVE_MAX_N", raising=False)
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    batch = _orders_batch((129, 5, 144, 200, 64, 256), _name(dtype))
    lay = _Layout(batch, dtype, seed=5)
    order = np.array([-1, 0, batch.count, 3, -1, 2**31 - 1], dtype=np.int32)       # mid tier only: matrices 0 and 3
    got, us = _dev_run(lay, order, [0, 0, 0, 6])
    _check_dev(lay, got, us, {0, 3}, "hostile plan %s" % _name(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_device_form_tier_mismatch(dtype, monkeypatch):
    """A mid-order matrix listed in the 128-wide tier is left untouched (its tile does not hold it); small matrices
    listed in the mid tier are solved: its tile holds every order from 1 up."""
    monkeypatch.delenv("FWX_BATCH_WAVE_MAX_N", raising=False)
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    batch = _orders_batch((129, 5, 144, 200, 64, 256), _name(dtype))
    lay = _Layout(batch, dtype, seed=6)
    # wave: none; 64-wide: none; 128-wide: matrix 0 (order 129) and 3 (order 200); mid: 1 (5), 4 (64), 5 (256)
    got, us = _dev_run(lay, [0, 3, 1, 4, 5], [0, 0, 2, 3])
    _check_dev(lay, got, us, {1, 4, 5}, "tier mismatch %s" % _name(dtype))


# ---- 4. more workgroups than CUs ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_more_workgroups_than_compute_units(dtype, monkeypatch):
    """600 matrices of the orders 129 ... 140 in turn (24 distinct matrices, repeated), three of order 256 among them:
    the chip has 256 CUs and a mid workgroup has one to itself.  U is checked per matrix."""
    monkeypatch.delenv("FWX_BATCH_WAVE_MAX_N", raising=False)
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    base = _orders_batch(tuple(129 + b % 12 for b in range(24)) + (256,), _name(dtype))
    base.not_vacuous()
    batch = _Batch(None, of=base, picks=[24 if b in (7, 300, 599) else b % 24 for b in range(600)])
    assert batch.orders[:13] == [129, 130, 131, 132, 133, 134, 135, 256, 137, 138, 139, 140, 129]
    assert list(engine.ragged_mid_plan(batch.n_each)[2]) == [0, 0, 0, 600]
    _compare_packed(batch, _solve_packed(batch, 2), "600 matrices %s" % _name(dtype))


# ---- 5. equal orders: the uniform mid launch's answer -------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_equal_orders_match_the_uniform_mid_batch(dtype, monkeypatch):
    monkeypatch.delenv("FWX_BATCH_WAVE_MAX_N", raising=False)
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    batch = _orders_batch((200,) * 5, _name(dtype))
    batch.not_vacuous()
    for fields in (0, 1, 2):
        uni = [np.stack([p[f] for p in batch.parts]) if f <= fields else None for f in range(3)]
        us = engine.solve_batch_mid(uni[0], uni[1], uni[2], count_updates=True)
        got = _solve_packed(batch, fields)
        for f, field in enumerate(("rate", "next", "hops")):
            if uni[f] is not None:
                assert_bits_equal(got[f], uni[f].reshape(-1), "n=200 %s fields=%d %s" % (_name(dtype), fields, field))
        assert got[3] == [int(u) for u in us]
    _compare_packed(batch, got, "n=200 %s against the oracle" % _name(dtype))
