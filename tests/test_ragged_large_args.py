"""Ragged batches up to order 1024 (fwx_ragged_large_plan, fwx_solve_ragged_large_*, fwx_solve_ragged_large_lists_*,
fwx_dev_solve_ragged_large, fwx_dev_exact_paths_ragged_large, fwx_test_ragged_large_schedule): the symbols exist, the
five-tier plan and its work table are what include/fwx.h says for every setting of FWX_BATCH_WAVE_MAX_N,
FWX_BATCH_MID_MIN_N and FWX_BATCH_LARGE_MIN_N, the schedule hook pins the groups and the active prefix, the smaller
plans are untouched, and every status of the contract is decided before any device call.  CPU only: no launch is made
here."""
import ctypes

import numpy as np
import pytest

from floydwarshall_amd import _lib, engine

OK, INVALID, UNSUPPORTED, NO_DEVICE = (_lib.FWX_OK, _lib.FWX_ERR_INVALID, _lib.FWX_ERR_UNSUPPORTED,
                                      _lib.FWX_ERR_NO_DEVICE)
DTYPES = [np.float64, np.float32]
SUFFIX = {np.float64: "f64", np.float32: "f32"}
NAMES = ("fwx_ragged_large_plan", "fwx_solve_ragged_large_f64", "fwx_solve_ragged_large_f32",
         "fwx_dev_solve_ragged_large", "fwx_dev_exact_paths_ragged_large", "fwx_solve_ragged_large_lists_f64",
         "fwx_solve_ragged_large_lists_f32", "fwx_test_ragged_large_schedule")
FAKE = ctypes.c_void_p(4096)            # a device pointer that is never dereferenced
SCHEDULE_ORDERS = (1024, 513, 513, 273, 272, 257)


def _p(a):
    return None if a is None else a.ctypes.data


def _opts(**kw):
    o = _lib.FwxOpts()
    o.struct_size = ctypes.sizeof(_lib.FwxOpts)
    o.device = -1
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _geometry():
    g = (ctypes.c_int32 * 4)()
    assert _lib.lib().fwx_test_batch_large_geometry(g) == OK
    return tuple(int(v) for v in g)     # B, S, TR, TC


def _ceil(a, b):
    return -(-a // b)


def _batch(orders, dtype):
    """A packed batch: (n_each, rate, next, hops)."""
    cells = sum(n * n for n in orders)
    rate = np.full(cells, 0.5, dtype=dtype)
    nxt = np.concatenate([np.tile(np.arange(n, dtype=np.int32), n) for n in orders] + [np.zeros(0, np.int32)])
    hops = np.ones(cells, dtype=np.int32)
    return np.array(orders, dtype=np.int32), rate, nxt, hops


def _host(dtype, count, n_each, rate, nxt, hops, each=None, opts=None):
    fn = getattr(_lib.lib(), "fwx_solve_ragged_large_" + SUFFIX[dtype])
    return fn(count, _p(n_each), _p(rate), _p(nxt), _p(hops), _p(each), None if opts is None else ctypes.byref(opts))


class _Items:
    def __init__(self, items=2, cap=4):
        self.items, self.cap = items, cap
        self.mat, self.src, self.dst = (np.zeros(max(items, 1), dtype=np.int32) for _ in range(3))
        self.len = np.full(max(items, 1), 77, dtype=np.int32)
        self.path = np.full(max(items, 1) * max(cap, 1), 77, dtype=np.int32)


def _lists(dtype, count, n_each, rate, nxt, hops, it, each=None, opts=None, **null):
    fn = getattr(_lib.lib(), "fwx_solve_ragged_large_lists_" + SUFFIX[dtype])
    a = {k: (None if null.get(k) else _p(getattr(it, k))) for k in ("mat", "src", "dst", "len", "path")}
    return fn(count, _p(n_each), _p(rate), _p(nxt), _p(hops), _p(each), it.items, a["mat"], a["src"], a["dst"],
              a["len"], a["path"], it.cap, None if opts is None else ctypes.byref(opts))


def _tiers(*t):
    return (ctypes.c_int32 * len(t))(*t)


def _trace(last=4096, at_col=4096, at_row=4096):
    t = _lib.FwxTrace()
    t.last, t.at_col, t.at_row = last, at_col, at_row
    return t


def _dev(count, code, rate, nxt, hops, n_each=FAKE, offset=FAKE, order=FAKE, tiers=None, work=None, d_work=FAKE,
         trace=None, upd=None, scratch=FAKE, scratch_bytes=1 << 30):
    return _lib.lib().fwx_dev_solve_ragged_large(count, code, rate, nxt, hops, n_each, offset, order, tiers, _p(work),
                                                 d_work, None if trace is None else ctypes.byref(trace), upd, scratch,
                                                 scratch_bytes, None)


def _walk(count, n_max, items, cap, trace, n_each=FAKE, offset=FAKE, next0=FAKE, mat=FAKE, src=FAKE, dst=FAKE,
          len_out=FAKE, path_out=FAKE, scratch=FAKE):
    return _lib.lib().fwx_dev_exact_paths_ragged_large(count, n_each, offset, n_max, next0,
                                                       None if trace is None else ctypes.byref(trace), items, mat,
                                                       src, dst, len_out, path_out, cap, scratch, None)


def _work_of(large_orders, count):
    """The header's words, restated: three rows of count + 1 prefix sums over the large tier's list."""
    _, S, TR, TC = _geometry()
    rows = [[0], [0], [0]]
    for n in large_orders:
        rows[0].append(rows[0][-1] + n)
        rows[1].append(rows[1][-1] + _ceil(n, S))
        rows[2].append(rows[2][-1] + _ceil(n, TC) * _ceil(n, TR))
    return np.array([r + [r[-1]] * (count - len(large_orders)) for r in rows], dtype=np.int64)


def test_the_ragged_large_symbols_are_exported_and_bound():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
    for name in ("ragged_large_plan", "solve_ragged_large", "solve_ragged_large_lists", "dev_solve_ragged_large",
                 "dev_exact_paths_ragged_large"):
        assert callable(getattr(engine, name)) and name in engine.__all__, name
    assert _lib.lib().fwx_abi_version() == 3           # symbols are only added
    assert _geometry()[0] == 16                        # the schedule below counts blocks of 16 pivots


# ---- the plan ----------------------------------------------------------------------------------------
def _expected_plan(orders, wave_max_n, mid_min_n, large_min_n):
    """The header's words: large wins over mid, mid over wave."""
    tier = lambda n: (4 if n >= large_min_n else 3 if n >= mid_min_n else 0 if n <= wave_max_n else 1 if n <= 64
                      else 2)
    listed = sorted((b for b, n in enumerate(orders) if n >= 1), key=lambda b: (tier(orders[b]), -orders[b], b))
    counts = [sum(1 for b in listed if tier(orders[b]) == t) for t in range(5)]
    return listed, counts


def _order_sets():
    rnd = np.random.default_rng(31)
    return {"empty": [], "all zero": [0, 0, 0],
            "1 to 1024 shuffled": [int(n) for n in rnd.permutation(np.arange(1, 1025))],
            "duplicates": [int(n) for n in rnd.permutation(
                [0, 1, 4, 10, 16, 17, 64, 65, 128, 129, 200, 256, 257, 272, 273, 512, 513, 1023, 1024] * 3)]}


@pytest.mark.parametrize("large", [None, "1", "129", "257", "garbage"])
@pytest.mark.parametrize("mid", [None, "1", "65", "129"])
@pytest.mark.parametrize("wave", [None, "0", "16"])
def test_plan_follows_the_three_settings(wave, mid, large, monkeypatch):
    for name, value in (("FWX_BATCH_WAVE_MAX_N", wave), ("FWX_BATCH_MID_MIN_N", mid), ("FWX_BATCH_LARGE_MIN_N", large)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    L = _lib.lib()
    wave_max_n, mid_min_n, large_min_n = (L.fwx_test_batch_wave_max_n(), L.fwx_test_batch_mid_min_n(),
                                          L.fwx_test_batch_large_min_n())
    assert wave_max_n == (16 if wave is None else int(wave))
    assert mid_min_n == (129 if mid is None else int(mid))
    assert large_min_n == (int(large) if large in ("1", "129", "257") else 257)
    for name, orders in _order_sets().items():
        offset, order, tiers, work = engine.ragged_large_plan(orders)
        assert offset.dtype == np.int64 and order.dtype == np.int32 and tiers.shape == (5,)
        assert work.dtype == np.int64 and work.shape == (3, len(orders) + 1)
        assert list(offset) == [sum(n * n for n in orders[:b]) for b in range(len(orders) + 1)], name
        listed, counts = _expected_plan(orders, wave_max_n, mid_min_n, large_min_n)
        assert list(tiers) == counts, name
        assert list(order[:len(listed)]) == listed, name
        assert list(order[len(listed):]) == [-1] * orders.count(0), name               # order 0 appears in no tier
        assert sorted(listed) == [b for b, n in enumerate(orders) if n >= 1]           # a permutation
        big = [orders[b] for b in listed[len(listed) - counts[4]:]]
        assert big == sorted(big, reverse=True) and all(n >= large_min_n for n in big), name
        assert np.array_equal(work, _work_of(big, len(orders))), name                  # entries past L repeat entry L
        if large == "1":                                                               # large beats mid and wave
            assert counts[:4] == [0, 0, 0, 0]
        if large == "129" and mid in ("1", "65"):
            assert counts[4] == sum(1 for n in orders if n >= 129)
            assert counts[3] == sum(1 for n in orders if mid_min_n <= n <= 128)
        if mid == "1" and large_min_n > 16:                                            # mid beats wave
            assert counts[:3] == [0, 0, 0]


@pytest.mark.parametrize("wave", [None, "0", "4"])
def test_orders_up_to_256_get_the_four_tier_plan_and_the_smaller_plans_are_unchanged(wave, monkeypatch):
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    if wave is None:
        monkeypatch.delenv("FWX_BATCH_WAVE_MAX_N", raising=False)
    else:
        monkeypatch.setenv("FWX_BATCH_WAVE_MAX_N", wave)
    rnd = np.random.default_rng(3)
    orders = [int(n) for n in rnd.integers(0, 257, size=300)] + [256, 256, 129, 1, 0]
    o4, r4, t4 = engine.ragged_mid_plan(orders)
    o5, r5, t5, work = engine.ragged_large_plan(orders)
    assert list(t5) == list(t4) + [0] and np.array_equal(r4, r5) and np.array_equal(o4, o5) and not work.any()
    small = [min(n, 128) for n in orders]
    o3, r3, t3 = engine.ragged_plan(small)
    # FWX_BATCH_LARGE_MIN_N is nothing to the two smaller plans
    monkeypatch.setenv("FWX_BATCH_LARGE_MIN_N", "10")
    o4b, r4b, t4b = engine.ragged_mid_plan(orders)
    assert np.array_equal(o4, o4b) and np.array_equal(r4, r4b) and np.array_equal(t4, t4b)
    o3b, r3b, t3b = engine.ragged_plan(small)
    assert np.array_equal(o3, o3b) and np.array_equal(r3, r3b) and np.array_equal(t3, t3b)
    assert engine.ragged_large_plan(orders)[2][4] == sum(1 for n in orders if n >= 10)


def test_plan_edges_and_statuses(monkeypatch):
    for name in ("FWX_BATCH_WAVE_MAX_N", "FWX_BATCH_MID_MIN_N", "FWX_BATCH_LARGE_MIN_N"):
        monkeypatch.delenv(name, raising=False)
    L = _lib.lib()
    offset, order, tiers, work = engine.ragged_large_plan([])
    assert list(offset) == [0] and len(order) == 0 and list(tiers) == [0] * 5 and work.tolist() == [[0], [0], [0]]
    offset, order, tiers, work = engine.ragged_large_plan([0, 0])
    assert list(offset) == [0, 0, 0] and list(order) == [-1, -1] and list(tiers) == [0] * 5 and not work.any()
    n = np.array([3, 1024, 256, 300], dtype=np.int32)
    t = _tiers(9, 9, 9, 9, 9)
    off = np.zeros(5, dtype=np.int64)
    order = np.zeros(4, dtype=np.int32)
    work = np.full((3, 5), -7, dtype=np.int64)
    assert L.fwx_ragged_large_plan(4, _p(n), None, None, t, None) == OK and list(t) == [1, 0, 0, 1, 2]
    assert L.fwx_ragged_large_plan(4, _p(n), _p(off), None, None, None) == OK          # outputs are optional,
    assert list(off) == [0, 9, 9 + 1024 ** 2, 9 + 1024 ** 2 + 256 ** 2, 9 + 1024 ** 2 + 256 ** 2 + 300 ** 2]
    assert L.fwx_ragged_large_plan(4, _p(n), None, _p(order), None, None) == OK and list(order) == [0, 2, 1, 3]
    assert L.fwx_ragged_large_plan(4, _p(n), None, None, None, _p(work)) == OK         # one at a time
    assert np.array_equal(work, _work_of([1024, 300], 4))
    assert L.fwx_ragged_large_plan(4, _p(n), None, None, None, None) == OK
    assert L.fwx_ragged_large_plan(-1, _p(n), None, None, t, None) == INVALID
    assert L.fwx_ragged_large_plan(2, None, None, None, t, None) == INVALID
    assert L.fwx_ragged_large_plan(0, None, None, None, t, None) == OK and list(t) == [0] * 5
    assert L.fwx_ragged_large_plan(2, _p(np.array([3, -1], dtype=np.int32)), None, None, t, None) == INVALID
    assert L.fwx_ragged_large_plan(2, _p(np.array([3, 1024], dtype=np.int32)), None, None, t, None) == OK
    t = _tiers(9, 9, 9, 9, 9)
    assert L.fwx_ragged_large_plan(2, _p(np.array([3, 1025], dtype=np.int32)), None, None, t, None) == UNSUPPORTED
    assert L.fwx_ragged_large_plan(2, _p(np.array([-1, 1025], dtype=np.int32)), None, None, t, None) == INVALID
    assert list(t) == [9] * 5
    # the smaller plans keep refusing what they refused
    t4 = _tiers(9, 9, 9, 9)
    assert L.fwx_ragged_mid_plan(2, _p(np.array([3, 257], dtype=np.int32)), None, None, t4) == UNSUPPORTED
    assert L.fwx_ragged_plan(2, _p(np.array([3, 129], dtype=np.int32)), None, None, t4) == UNSUPPORTED
    assert list(t4) == [9, 9, 9, 9]
    with pytest.raises(ValueError):
        engine.ragged_large_plan([[1, 2]])


# ---- the schedule ------------------------------------------------------------------------------------
def _schedule(work, large_count, scratch_bytes, cap=16):
    count = work.shape[1] - 1
    first = np.full(cap, -1, dtype=np.int32)
    totals = np.full(3, -1, dtype=np.int64)
    rc = _lib.lib().fwx_test_ragged_large_schedule(count, large_count, _p(work), scratch_bytes, _p(first), cap,
                                                   _p(totals))
    return rc, [int(v) for v in first[:max(rc, 0)]], [int(v) for v in totals]


def _expected_schedule(orders, scratch_bytes):
    """Greedy groups of consecutive slots whose panels (512 bytes per order) fit; per group and block of 16 pivots
    one panel and one sweep launch over the slots with n > 16 q."""
    _, S, TR, TC = _geometry()
    groups, at = [], 0
    while at < len(orders):
        end = at
        while end < len(orders) and 512 * sum(orders[at:end + 1]) <= scratch_bytes:
            end += 1
        groups.append((at, end))
        at = end
    launches = panel = sweep = 0
    for a, b in groups:
        for q in range(_ceil(orders[a], 16)):
            active = [n for n in orders[a:b] if n > 16 * q]
            launches += 2
            panel += sum(_ceil(n, S) for n in active)
            sweep += sum(_ceil(n, TC) * _ceil(n, TR) for n in active)
    return [g[0] for g in groups], [launches, panel, sweep]


def test_schedule_with_ample_scratch_is_one_group(monkeypatch):
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    _, S, TR, TC = _geometry()
    orders = list(SCHEDULE_ORDERS) + [5, 0]                                    # two more that are not large
    _, _, tiers, work = engine.ragged_large_plan(orders)
    assert tiers[4] == 6
    rc, first, totals = _schedule(work, 6, 1 << 30)
    assert rc == 1 and first == [0]
    assert totals == [2 * 64, sum(_ceil(n, S) * _ceil(n, 16) for n in SCHEDULE_ORDERS),
                      sum(_ceil(n, TC) * _ceil(n, TR) * _ceil(n, 16) for n in SCHEDULE_ORDERS)]
    assert (first, totals) == _expected_schedule(list(SCHEDULE_ORDERS), 1 << 30)
    exact = 512 * sum(SCHEDULE_ORDERS)                                         # exactly what one group needs
    assert _schedule(work, 6, exact)[0] == 1 and _schedule(work, 6, exact - 1)[0] == 2
    rc, first, _ = _schedule(work, 6, 1 << 30, cap=0)                          # the groups are counted past cap
    assert rc == 1 and first == []
    assert _schedule(work, 0, 0) == (0, [], [0, 0, 0])                         # nothing listed: nothing judged


def test_schedule_with_scratch_for_the_largest_is_greedy_groups(monkeypatch):
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    _, _, _, work = engine.ragged_large_plan(SCHEDULE_ORDERS)
    rc, first, totals = _schedule(work, 6, 1024 * 512)
    # 1024 | 513 + 513 = 1026 does not fit: 513 | 513 + 273 | 272 + 257
    assert rc == 4 and first == [0, 1, 2, 4]
    assert totals[0] == 2 * (64 + 33 + 33 + 17)                                # each group by its own first order
    assert (first, totals) == _expected_schedule(list(SCHEDULE_ORDERS), 1024 * 512)
    rc, first, _ = _schedule(work, 6, 1024 * 512, cap=2)
    assert rc == 4 and first == [0, 1]                             # the groups are counted past cap
    assert _schedule(work, 6, 1024 * 512 - 1)[0] == INVALID                    # one byte short of the largest


def test_schedule_refuses_what_the_device_form_refuses(monkeypatch):
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    _, _, _, work = engine.ragged_large_plan(SCHEDULE_ORDERS)
    L = _lib.lib()
    assert L.fwx_test_ragged_large_schedule(6, 6, None, 1 << 30, None, 0, None) == INVALID
    assert L.fwx_test_ragged_large_schedule(6, 7, _p(work), 1 << 30, None, 0, None) == INVALID
    assert L.fwx_test_ragged_large_schedule(6, -1, _p(work), 1 << 30, None, 0, None) == INVALID
    assert L.fwx_test_ragged_large_schedule(6, 6, _p(work), 1 << 30, None, 1, None) == INVALID
    assert L.fwx_test_ragged_large_schedule(6, 6, _p(work), 1 << 30, None, 0, None) == 1     # totals are optional
    for bad in _bad_tables(work):
        assert _schedule(bad, 6, 1 << 30)[0] == INVALID


def _bad_tables(work):
    """Host tables the contract refuses, made from a good one of six slots."""
    out = []
    for row in range(3):
        w = work.copy()
        w[row, 3] = w[row, 2] - 1                       # a row that decreases
        out.append(w)
    w = work.copy()
    w[0, 1:] += 1                                       # first order 1025
    out.append(w)
    w = work.copy()
    w[0, 6] = w[0, 5]                                   # an order 0
    out.append(w)
    w = _work_of([513, 1024, 513, 273, 272, 257], 6)    # orders that do not descend
    out.append(w)
    w = work.copy()
    w[1, 4:] += 1                                       # a strip row that is not these orders'
    out.append(w)
    w = work.copy()
    w[2, 2:] -= 1                                       # a tile row that is not these orders'
    out.append(w)
    return out


# ---- statuses ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_host_forms_reject_bad_arguments_before_any_device_call(dtype):
    n_each, rate, nxt, hops = _batch([4, 0, 300], dtype)
    before = rate.copy()
    it = _Items()
    for call in (lambda *a, **k: _host(dtype, *a, **k), lambda *a, **k: _lists(dtype, *a, it=it, **k)):
        assert call(-1, n_each, rate, nxt, hops) == INVALID                        # count < 0
        assert call(3, None, rate, nxt, hops) == INVALID                           # no orders
        assert call(3, np.array([4, -1, 300], dtype=np.int32), rate, nxt, hops) == INVALID
        assert call(3, np.array([-1, 0, 1025], dtype=np.int32), rate, nxt, hops) == INVALID  # negative beats too large
        assert call(3, n_each, None, nxt, hops) == INVALID                         # no rates, some order positive
        assert call(3, n_each, rate, None, hops) == INVALID                        # hops without next
        assert call(3, n_each, rate, nxt, hops, opts=_opts(struct_size=4)) == INVALID
        for kb, ke in ((1, 0), (0, 4), (0, 300), (3, 2), (-1, 0), (0, 301)):       # only the whole range
            assert call(3, n_each, rate, nxt, hops, opts=_opts(k_begin=kb, k_end=ke)) == INVALID, (kb, ke)
        assert call(3, n_each, rate, nxt, hops, opts=_opts(engine=99)) == INVALID
        big = np.array([4, 1025, 0], dtype=np.int32)
        assert call(3, big, rate, nxt, hops) == UNSUPPORTED                        # an order > FWX_BATCH_LARGE_MAX_N
        for eng in (_lib.FWX_ENGINE_PERK, _lib.FWX_ENGINE_FUSED):
            assert call(3, n_each, rate, nxt, hops, opts=_opts(engine=eng)) == UNSUPPORTED, eng
    assert _lists(dtype, 3, n_each, rate, nxt, hops, _Items(items=-1)) == INVALID
    assert _lists(dtype, 3, n_each, rate, None, None, it) == INVALID               # the lists need next
    assert _lists(dtype, 3, n_each, rate, nxt, hops, _Items(cap=0)) == INVALID
    for missing in ("mat", "src", "dst", "len", "path"):
        assert _lists(dtype, 3, n_each, rate, nxt, hops, it, **{missing: True}) == INVALID, missing
    assert np.array_equal(rate, before)
    assert list(it.len) == [77, 77]


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_batches_are_success_and_touch_nothing(dtype):
    n_each, rate, nxt, hops = _batch([4, 5], dtype)
    before = rate.copy(), nxt.copy(), hops.copy()
    each = np.full(2, 77, dtype=np.uint64)
    total = ctypes.c_uint64(55)
    o = _opts(updates_out=ctypes.pointer(total))
    zeros = np.zeros(2, dtype=np.int32)
    it = _Items()
    assert _host(dtype, 0, n_each, rate, nxt, hops, each, o) == OK
    assert _host(dtype, 0, None, None, None, None) == OK
    assert _host(dtype, 2, zeros, rate, nxt, hops, each, o) == OK                  # every order 0
    assert _host(dtype, 2, zeros, None, None, None) == OK                          # ... needs no arrays
    assert _lists(dtype, 0, n_each, rate, nxt, hops, it, each, o) == OK
    assert _lists(dtype, 2, zeros, rate, nxt, hops, it, each, o) == OK
    for got, want in zip((rate, nxt, hops), before):
        assert np.array_equal(got, want)
    assert list(each) == [77, 77] and total.value == 55 and list(it.len) == [77, 77]


def test_device_solve_rejects_bad_arguments_before_any_device_call(monkeypatch):
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    _, _, _, work = engine.ragged_large_plan(SCHEDULE_ORDERS)
    t = _tiers(0, 0, 0, 0, 6)
    for code in (_lib.FWX_F32, _lib.FWX_F64):
        assert _dev(-1, code, FAKE, FAKE, FAKE, tiers=t, work=work) == INVALID
        assert _dev(6, code, FAKE, FAKE, FAKE, tiers=None, work=work) == INVALID
        for neg in range(5):                                                       # a negative tier count
            bad = [1, 0, 0, 0, 0]
            bad[neg] = -1
            assert _dev(6, code, FAKE, FAKE, FAKE, tiers=_tiers(*bad), work=work) == INVALID, neg
        assert _dev(6, code, FAKE, FAKE, FAKE, tiers=_tiers(1, 0, 0, 0, 6), work=work) == INVALID   # the FIFTH count
        assert _dev(6, code, FAKE, FAKE, FAKE, tiers=_tiers(0, 0, 0, 0, 7), work=work) == INVALID   # is summed too
        assert _dev(6, code, FAKE, FAKE, FAKE, tiers=_tiers(2**31 - 1, 2, 2, 2**31 - 1, 2**31 - 1), work=work) == INVALID
        assert _dev(6, code, None, FAKE, FAKE, tiers=t, work=work) == INVALID
        assert _dev(6, code, FAKE, None, FAKE, tiers=t, work=work) == INVALID      # hops without next
        for missing in ("n_each", "offset", "order"):
            assert _dev(6, code, FAKE, FAKE, FAKE, tiers=t, work=work, **{missing: None}) == INVALID, missing
        assert _dev(6, code, FAKE, None, None, tiers=t, work=work, trace=_trace()) == INVALID   # a trace needs next
        for hole in ("last", "at_col", "at_row"):
            assert _dev(6, code, FAKE, FAKE, None, tiers=t, work=work, trace=_trace(**{hole: None})) == INVALID, hole
        # what the large tier runs on, judged when it lists a matrix
        assert _dev(6, code, FAKE, FAKE, FAKE, tiers=t, work=None) == INVALID
        assert _dev(6, code, FAKE, FAKE, FAKE, tiers=t, work=work, d_work=None) == INVALID
        for bad in _bad_tables(work):
            assert _dev(6, code, FAKE, FAKE, FAKE, tiers=t, work=bad) == INVALID
        assert _dev(6, code, FAKE, FAKE, FAKE, tiers=t, work=work, scratch=None) == INVALID
        assert _dev(6, code, FAKE, FAKE, FAKE, tiers=t, work=work, scratch=ctypes.c_void_p(4096 + 8)) == INVALID
        assert _dev(6, code, FAKE, FAKE, FAKE, tiers=t, work=work, scratch_bytes=1024 * 512 - 1) == INVALID
        # ... and ignored when it lists none
        none = _tiers(0, 0, 0, 0, 0)
        assert _dev(0, code, None, None, None, None, None, None, tiers=none, work=None, d_work=None, scratch=None,
                    scratch_bytes=0) == OK
        assert _dev(6, code, None, None, None, None, None, None, tiers=none, work=None, d_work=None, scratch=None,
                    scratch_bytes=0) == OK                                         # every order 0
    assert _dev(6, 7, FAKE, FAKE, FAKE, tiers=t, work=work) == INVALID             # no such dtype


def test_device_walk_rejects_bad_arguments_before_any_device_call():
    tr = _trace()
    assert _walk(-1, 4, 2, 4, tr) == INVALID
    assert _walk(2, -1, 2, 4, tr) == INVALID
    assert _walk(2, 4, -1, 4, tr) == INVALID
    assert _walk(2, 600, 2, 0, tr) == INVALID                                      # cap < 1
    assert _walk(2, 600, 2, 4, None) == INVALID
    for hole in ("last", "at_col", "at_row"):
        assert _walk(2, 600, 2, 4, _trace(**{hole: None})) == INVALID, hole
    for missing in ("n_each", "offset", "next0", "mat", "src", "dst", "len_out", "path_out", "scratch"):
        assert _walk(2, 600, 2, 4, tr, **{missing: None}) == INVALID, missing
    assert _walk(2, 1025, 2, 4, tr) == UNSUPPORTED
    assert _walk(0, 4, 2, 4, None, None, None, None, None, None, None, None, None, None) == OK
    assert _walk(2, 0, 2, 4, None, None, None, None, None, None, None, None, None, None) == OK
    assert _walk(2, 4, 0, 4, None, None, None, None, None, None, None, None, None, None) == OK


@pytest.mark.skipif(engine.device_count() > 0, reason="only meaningful without a GPU")
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_valid_call_without_a_device_reports_it_and_leaves_the_arrays_alone(dtype, monkeypatch):
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    orders = [5, 0, 129, 257, 600]                                                 # 257 and 600 are accepted
    n_each, rate, nxt, hops = _batch(orders, dtype)
    rate[7] = np.nan
    before = rate.copy(), nxt.copy(), hops.copy()
    each = np.full(5, 9, dtype=np.uint64)
    it = _Items()
    assert _host(dtype, 5, n_each, rate, nxt, hops, each) == NO_DEVICE
    assert _host(dtype, 5, n_each, rate, None, None) == NO_DEVICE
    assert _lists(dtype, 5, n_each, rate, nxt, hops, it, each) == NO_DEVICE
    assert _lists(dtype, 5, n_each, rate, nxt, None, _Items(items=0)) == NO_DEVICE   # items == 0: a plain solve
    # ... where the four-tier family still refuses them
    fn4 = getattr(_lib.lib(), "fwx_solve_ragged_mid_" + SUFFIX[dtype])
    assert fn4(5, _p(n_each), _p(rate), _p(nxt), _p(hops), None, None) == UNSUPPORTED
    mats = [np.full((n, n), 0.5, dtype=dtype) for n in orders]
    kept = [m.copy() for m in mats]
    with pytest.raises(engine.FwxError) as e:
        engine.solve_ragged_large(mats, count_updates=True)
    assert e.value.status == NO_DEVICE
    with pytest.raises(engine.FwxError) as e:
        engine.solve_ragged_large_lists(mats, [np.zeros((n, n), dtype=np.int32) for n in orders], items=([0], [0], [0]),
                                        cap=4)
    assert e.value.status == NO_DEVICE
    with pytest.raises(engine.FwxError) as e:
        engine.solve_ragged_large(mats + [np.full((1025, 1025), 0.5, dtype=dtype)])
    assert e.value.status == UNSUPPORTED
    for m, k in zip(mats, kept):
        assert np.array_equal(m, k)
    bits = np.uint64 if dtype == np.float64 else np.uint32
    assert np.array_equal(rate.view(bits), before[0].view(bits))
    assert np.array_equal(nxt, before[1]) and np.array_equal(hops, before[2])
    assert list(each) == [9] * 5 and list(it.len) == [77, 77]
    code = _lib.FWX_F64 if dtype == np.float64 else _lib.FWX_F32
    _, _, tiers, work = engine.ragged_large_plan(orders)
    assert list(tiers) == [1, 0, 0, 1, 2]
    t = _tiers(*[int(v) for v in tiers])
    assert _dev(5, code, FAKE, None, None, tiers=t, work=work) == NO_DEVICE
    assert _dev(5, code, FAKE, FAKE, FAKE, tiers=t, work=work, trace=_trace(), scratch_bytes=600 * 512) == NO_DEVICE
    assert _dev(5, code, FAKE, None, None, tiers=_tiers(1, 0, 0, 1, 0), work=None, d_work=None, scratch=None,
                scratch_bytes=0) == NO_DEVICE                                      # no large matrix: no table needed
    assert _walk(5, 600, 2, 4, _trace()) == NO_DEVICE
    assert _walk(5, 1024, 2, 4, _trace()) == NO_DEVICE


# ---- the Python binding ------------------------------------------------------------------------------
def test_python_binding_checks_what_it_packs():
    sq = lambda n, dtype=np.float64: np.full((n, n), 0.5, dtype=dtype)
    ix = lambda n: np.zeros((n, n), dtype=np.int32)
    for fn in (engine.solve_ragged_large, engine.solve_ragged_large_lists):
        with pytest.raises(ValueError):
            fn([sq(4), np.zeros((3, 4))], [ix(4), np.zeros((3, 4), dtype=np.int32)])       # not square
        with pytest.raises(ValueError):
            fn([sq(4), sq(5, np.float32)], [ix(4), ix(5)])                                  # mixed dtypes
        with pytest.raises(ValueError):
            fn([sq(4), sq(5)], [ix(4), ix(4)])                                              # next shaped unlike its rate
    with pytest.raises(ValueError):
        engine.solve_ragged_large([sq(4)], None, [ix(4)])                                   # hops requires next
    with pytest.raises(ValueError):
        engine.solve_ragged_large_lists([sq(4)], None)                                      # the lists need next
    assert engine.solve_ragged_large([], count_updates=True).shape == (0,)                  # empty: success
    assert list(engine.solve_ragged_large([sq(0), sq(0)], count_updates=True)) == [0, 0]
    assert engine.solve_ragged_large_lists([sq(0)], [ix(0)]) == []
