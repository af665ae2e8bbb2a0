"""Ragged batches up to order 256 (fwx_ragged_mid_plan, fwx_solve_ragged_mid_*, fwx_solve_ragged_mid_lists_*,
fwx_dev_solve_ragged_mid, fwx_dev_exact_paths_ragged_mid): the symbols exist, the four-tier plan is what include/fwx.h
says for every setting of FWX_BATCH_WAVE_MAX_N and FWX_BATCH_MID_MIN_N, the three-tier plan is untouched, and every
status of the contract is decided before any device call.  CPU only: no launch is made here."""
import ctypes

import numpy as np
import pytest

from floydwarshall_amd import _lib, engine

OK, INVALID, UNSUPPORTED, NO_DEVICE = (_lib.FWX_OK, _lib.FWX_ERR_INVALID, _lib.FWX_ERR_UNSUPPORTED,
                                      _lib.FWX_ERR_NO_DEVICE)
DTYPES = [np.float64, np.float32]
SUFFIX = {np.float64: "f64", np.float32: "f32"}
NAMES = ("fwx_ragged_mid_plan", "fwx_solve_ragged_mid_f64", "fwx_solve_ragged_mid_f32", "fwx_dev_solve_ragged_mid",
         "fwx_dev_exact_paths_ragged_mid", "fwx_solve_ragged_mid_lists_f64", "fwx_solve_ragged_mid_lists_f32")
FAKE = ctypes.c_void_p(4096)            # a device pointer that is never dereferenced


def _p(a):
    return None if a is None else a.ctypes.data


def _opts(**kw):
    o = _lib.FwxOpts()
    o.struct_size = ctypes.sizeof(_lib.FwxOpts)
    o.device = -1
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _batch(orders, dtype):
    """A packed batch: (n_each, rate, next, hops)."""
    cells = sum(n * n for n in orders)
    rate = np.full(cells, 0.5, dtype=dtype)
    nxt = np.concatenate([np.tile(np.arange(n, dtype=np.int32), n) for n in orders] + [np.zeros(0, np.int32)])
    hops = np.ones(cells, dtype=np.int32)
    return np.array(orders, dtype=np.int32), rate, nxt, hops


def _host(dtype, count, n_each, rate, nxt, hops, each=None, opts=None):
    fn = getattr(_lib.lib(), "fwx_solve_ragged_mid_" + SUFFIX[dtype])
    return fn(count, _p(n_each), _p(rate), _p(nxt), _p(hops), _p(each), None if opts is None else ctypes.byref(opts))


class _Items:
    def __init__(self, items=2, cap=4):
        self.items, self.cap = items, cap
        self.mat, self.src, self.dst = (np.zeros(max(items, 1), dtype=np.int32) for _ in range(3))
        self.len = np.full(max(items, 1), 77, dtype=np.int32)
        self.path = np.full(max(items, 1) * max(cap, 1), 77, dtype=np.int32)


def _lists(dtype, count, n_each, rate, nxt, hops, it, each=None, opts=None, **null):
    fn = getattr(_lib.lib(), "fwx_solve_ragged_mid_lists_" + SUFFIX[dtype])
    a = {k: (None if null.get(k) else _p(getattr(it, k))) for k in ("mat", "src", "dst", "len", "path")}
    return fn(count, _p(n_each), _p(rate), _p(nxt), _p(hops), _p(each), it.items, a["mat"], a["src"], a["dst"],
              a["len"], a["path"], it.cap, None if opts is None else ctypes.byref(opts))


def _tiers(*t):
    return (ctypes.c_int32 * len(t))(*t)


def _dev(count, code, rate, nxt, hops, n_each=FAKE, offset=FAKE, order=FAKE, tiers=None, trace=None, upd=None):
    return _lib.lib().fwx_dev_solve_ragged_mid(count, code, rate, nxt, hops, n_each, offset, order, tiers,
                                               None if trace is None else ctypes.byref(trace), upd, None)


def _trace(last=4096, at_col=4096, at_row=4096):
    t = _lib.FwxTrace()
    t.last, t.at_col, t.at_row = last, at_col, at_row
    return t


def _walk(count, n_max, items, cap, trace, n_each=FAKE, offset=FAKE, next0=FAKE, mat=FAKE, src=FAKE, dst=FAKE,
          len_out=FAKE, path_out=FAKE, scratch=FAKE):
    return _lib.lib().fwx_dev_exact_paths_ragged_mid(count, n_each, offset, n_max, next0,
                                                     None if trace is None else ctypes.byref(trace), items, mat,
                                                     src, dst, len_out, path_out, cap, scratch, None)


def test_the_ragged_mid_symbols_are_exported_and_bound():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
    for name in ("ragged_mid_plan", "solve_ragged_mid", "solve_ragged_mid_lists", "dev_solve_ragged_mid",
                 "dev_exact_paths_ragged_mid"):
        assert callable(getattr(engine, name)) and name in engine.__all__, name
    assert _lib.lib().fwx_abi_version() == 3           # symbols are only added


# ---- the plan ----------------------------------------------------------------------------------------
def _expected_plan(orders, wave_max_n, mid_min_n):
    """The header's words: the mid tier takes every order from mid_min_n up and wins over the wave tier."""
    tier = lambda n: 3 if n >= mid_min_n else 0 if n <= wave_max_n else 1 if n <= 64 else 2
    listed = sorted((b for b, n in enumerate(orders) if n >= 1), key=lambda b: (tier(orders[b]), -orders[b], b))
    counts = [sum(1 for b in listed if tier(orders[b]) == t) for t in range(4)]
    return listed, counts


def _order_sets():
    rnd = np.random.default_rng(22)
    return {"empty": [], "all zero": [0, 0, 0],
            "1 to 256 shuffled": [int(n) for n in rnd.permutation(np.arange(1, 257))],
            "duplicates": [int(n) for n in rnd.permutation([0, 1, 4, 5, 10, 16, 17, 64, 65, 128, 129, 200, 256] * 3)]}


@pytest.mark.parametrize("mid", [None, "1", "10", "65", "129", "garbage"])
@pytest.mark.parametrize("wave", [None, "0", "4", "16"])
def test_plan_follows_both_settings(wave, mid, monkeypatch):
    for name, value in (("FWX_BATCH_WAVE_MAX_N", wave), ("FWX_BATCH_MID_MIN_N", mid)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    wave_max_n, mid_min_n = _lib.lib().fwx_test_batch_wave_max_n(), _lib.lib().fwx_test_batch_mid_min_n()
    assert wave_max_n == (16 if wave is None else int(wave))
    assert mid_min_n == (int(mid) if mid in ("1", "10", "65", "129") else 129)
    for name, orders in _order_sets().items():
        offset, order, tiers = engine.ragged_mid_plan(orders)
        assert offset.dtype == np.int64 and order.dtype == np.int32 and tiers.shape == (4,)
        assert list(offset) == [sum(n * n for n in orders[:b]) for b in range(len(orders) + 1)], name
        listed, counts = _expected_plan(orders, wave_max_n, mid_min_n)
        assert list(tiers) == counts, name
        assert list(order[:len(listed)]) == listed, name
        assert list(order[len(listed):]) == [-1] * orders.count(0), name
        assert sorted(listed) == [b for b, n in enumerate(orders) if n >= 1]          # a permutation
        if mid == "1":
            assert counts[:3] == [0, 0, 0]
        if mid == "10" and wave == "16":                                              # both claim 10 ... 16: mid wins
            assert counts[0] == sum(1 for n in orders if 1 <= n <= 9)
            assert counts[3] == sum(1 for n in orders if n >= 10) and counts[1] == counts[2] == 0


@pytest.mark.parametrize("wave", [None, "0", "4"])
def test_small_orders_get_the_three_tier_plan_and_the_three_tier_plan_is_unchanged(wave, monkeypatch):
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    if wave is None:
        monkeypatch.delenv("FWX_BATCH_WAVE_MAX_N", raising=False)
    else:
        monkeypatch.setenv("FWX_BATCH_WAVE_MAX_N", wave)
    rnd = np.random.default_rng(3)
    orders = [int(n) for n in rnd.integers(0, 129, size=300)] + [128, 128, 1, 0]
    o3, r3, t3 = engine.ragged_plan(orders)
    o4, r4, t4 = engine.ragged_mid_plan(orders)
    assert list(t4) == list(t3) + [0] and np.array_equal(r3, r4) and np.array_equal(o3, o4)
    # FWX_BATCH_MID_MIN_N is nothing to fwx_ragged_plan
    monkeypatch.setenv("FWX_BATCH_MID_MIN_N", "10")
    o3b, r3b, t3b = engine.ragged_plan(orders)
    assert np.array_equal(o3, o3b) and np.array_equal(r3, r3b) and np.array_equal(t3, t3b)
    assert engine.ragged_mid_plan(orders)[2][3] == sum(1 for n in orders if n >= 10)


def test_plan_edges_and_statuses():
    L = _lib.lib()
    offset, order, tiers = engine.ragged_mid_plan([])
    assert list(offset) == [0] and len(order) == 0 and list(tiers) == [0, 0, 0, 0]
    offset, order, tiers = engine.ragged_mid_plan([0, 0])
    assert list(offset) == [0, 0, 0] and list(order) == [-1, -1] and list(tiers) == [0, 0, 0, 0]
    n = np.array([3, 128, 256], dtype=np.int32)
    t = _tiers(9, 9, 9, 9)
    off = np.zeros(4, dtype=np.int64)
    order = np.zeros(3, dtype=np.int32)
    assert L.fwx_ragged_mid_plan(3, _p(n), None, None, t) == OK and list(t) == [1, 0, 1, 1]   # outputs are optional,
    assert L.fwx_ragged_mid_plan(3, _p(n), _p(off), None, None) == OK                         # one at a time
    assert list(off) == [0, 9, 9 + 128 * 128, 9 + 128 * 128 + 256 * 256]
    assert L.fwx_ragged_mid_plan(3, _p(n), None, _p(order), None) == OK and list(order) == [0, 1, 2]
    assert L.fwx_ragged_mid_plan(3, _p(n), _p(off), _p(order), None) == OK
    assert L.fwx_ragged_mid_plan(3, _p(n), None, None, None) == OK
    assert L.fwx_ragged_mid_plan(-1, _p(n), None, None, t) == INVALID
    assert L.fwx_ragged_mid_plan(2, None, None, None, t) == INVALID
    assert L.fwx_ragged_mid_plan(0, None, None, None, t) == OK and list(t) == [0, 0, 0, 0]
    assert L.fwx_ragged_mid_plan(2, _p(np.array([3, -1], dtype=np.int32)), None, None, t) == INVALID
    assert L.fwx_ragged_mid_plan(2, _p(np.array([3, 129], dtype=np.int32)), None, None, t) == OK
    assert L.fwx_ragged_mid_plan(2, _p(np.array([3, 256], dtype=np.int32)), None, None, t) == OK
    assert L.fwx_ragged_mid_plan(2, _p(np.array([3, 257], dtype=np.int32)), None, None, t) == UNSUPPORTED
    assert L.fwx_ragged_mid_plan(2, _p(np.array([-1, 257], dtype=np.int32)), None, None, t) == INVALID
    # the three-tier plan keeps refusing what it refused
    t3 = _tiers(9, 9, 9)
    assert L.fwx_ragged_plan(2, _p(np.array([3, 129], dtype=np.int32)), None, None, t3) == UNSUPPORTED
    assert list(t3) == [9, 9, 9]
    with pytest.raises(ValueError):
        engine.ragged_mid_plan([[1, 2]])


# ---- statuses ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_host_forms_reject_bad_arguments_before_any_device_call(dtype):
    n_each, rate, nxt, hops = _batch([4, 0, 130], dtype)
    before = rate.copy()
    it = _Items()
    for call in (lambda *a, **k: _host(dtype, *a, **k), lambda *a, **k: _lists(dtype, *a, it=it, **k)):
        assert call(-1, n_each, rate, nxt, hops) == INVALID                        # count < 0
        assert call(3, None, rate, nxt, hops) == INVALID                           # no orders
        assert call(3, np.array([4, -1, 130], dtype=np.int32), rate, nxt, hops) == INVALID
        assert call(3, np.array([-1, 0, 257], dtype=np.int32), rate, nxt, hops) == INVALID   # negative beats too large
        assert call(3, n_each, None, nxt, hops) == INVALID                         # no rates, some order positive
        assert call(3, n_each, rate, None, hops) == INVALID                        # hops without next
        assert call(3, n_each, rate, nxt, hops, opts=_opts(struct_size=4)) == INVALID
        for kb, ke in ((1, 0), (0, 4), (0, 130), (3, 2), (-1, 0), (0, 131)):       # only the whole range
            assert call(3, n_each, rate, nxt, hops, opts=_opts(k_begin=kb, k_end=ke)) == INVALID, (kb, ke)
        assert call(3, n_each, rate, nxt, hops, opts=_opts(engine=99)) == INVALID
        big = np.array([4, 257, 0], dtype=np.int32)
        assert call(3, big, rate, nxt, hops) == UNSUPPORTED                        # an order > FWX_BATCH_MID_MAX_N
        for eng in (_lib.FWX_ENGINE_PERK, _lib.FWX_ENGINE_FUSED):
            assert call(3, n_each, rate, nxt, hops, opts=_opts(engine=eng)) == UNSUPPORTED, eng
    assert _lists(dtype, 3, n_each, rate, nxt, hops, _Items(items=-1)) == INVALID
    assert _lists(dtype, 3, n_each, rate, None, None, it) == INVALID               # the lists need next
    assert _lists(dtype, 3, n_each, rate, nxt, hops, _Items(cap=0)) == INVALID
    assert _lists(dtype, 3, n_each, rate, nxt, hops, _Items(cap=-3)) == INVALID
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


def test_device_solve_rejects_bad_arguments_before_any_device_call():
    t = _tiers(1, 0, 0, 1)
    for code in (_lib.FWX_F32, _lib.FWX_F64):
        assert _dev(-1, code, FAKE, FAKE, FAKE, tiers=t) == INVALID
        assert _dev(2, code, FAKE, FAKE, FAKE, tiers=None) == INVALID
        for neg in range(4):                                                       # a negative tier count
            bad = [1, 0, 0, 0]
            bad[neg] = -1
            assert _dev(2, code, FAKE, FAKE, FAKE, tiers=_tiers(*bad)) == INVALID, neg
        assert _dev(2, code, FAKE, FAKE, FAKE, tiers=_tiers(1, 1, 0, 1)) == INVALID   # more listed than there are:
        assert _dev(2, code, FAKE, FAKE, FAKE, tiers=_tiers(0, 0, 0, 3)) == INVALID   # the FOURTH count is summed too
        assert _dev(2, code, FAKE, FAKE, FAKE, tiers=_tiers(1, 1, 1, 0)) == INVALID
        assert _dev(2, code, FAKE, FAKE, FAKE, tiers=_tiers(2**31 - 1, 2**31 - 1, 2, 2**31 - 1)) == INVALID
        assert _dev(2, code, None, FAKE, FAKE, tiers=t) == INVALID
        assert _dev(2, code, FAKE, None, FAKE, tiers=t) == INVALID                 # hops without next
        for missing in ("n_each", "offset", "order"):
            assert _dev(2, code, FAKE, FAKE, FAKE, tiers=t, **{missing: None}) == INVALID, missing
        assert _dev(2, code, FAKE, None, None, tiers=t, trace=_trace()) == INVALID  # a trace needs next
        for hole in ("last", "at_col", "at_row"):
            assert _dev(2, code, FAKE, FAKE, None, tiers=t, trace=_trace(**{hole: None})) == INVALID, hole
        assert _dev(0, code, None, None, None, None, None, None, tiers=_tiers(0, 0, 0, 0)) == OK
        assert _dev(2, code, None, None, None, None, None, None, tiers=_tiers(0, 0, 0, 0)) == OK   # every order 0
    assert _dev(2, 7, FAKE, FAKE, FAKE, tiers=t) == INVALID                        # no such dtype


def test_device_walk_rejects_bad_arguments_before_any_device_call():
    tr = _trace()
    assert _walk(-1, 4, 2, 4, tr) == INVALID
    assert _walk(2, -1, 2, 4, tr) == INVALID
    assert _walk(2, 4, -1, 4, tr) == INVALID
    assert _walk(2, 200, 2, 0, tr) == INVALID                                      # cap < 1
    assert _walk(2, 200, 2, 4, None) == INVALID
    for hole in ("last", "at_col", "at_row"):
        assert _walk(2, 200, 2, 4, _trace(**{hole: None})) == INVALID, hole
    for missing in ("n_each", "offset", "next0", "mat", "src", "dst", "len_out", "path_out", "scratch"):
        assert _walk(2, 200, 2, 4, tr, **{missing: None}) == INVALID, missing
    assert _walk(2, 257, 2, 4, tr) == UNSUPPORTED
    assert _walk(0, 4, 2, 4, None, None, None, None, None, None, None, None, None, None) == OK
    assert _walk(2, 0, 2, 4, None, None, None, None, None, None, None, None, None, None) == OK
    assert _walk(2, 4, 0, 4, None, None, None, None, None, None, None, None, None, None) == OK


@pytest.mark.skipif(engine.device_count() > 0, reason="only meaningful without a GPU")
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_valid_call_without_a_device_reports_it_and_leaves_the_arrays_alone(dtype):
    orders = [5, 0, 129, 256]                                                      # 129 and 256 are accepted
    n_each, rate, nxt, hops = _batch(orders, dtype)
    rate[7] = np.nan
    before = rate.copy(), nxt.copy(), hops.copy()
    each = np.full(4, 9, dtype=np.uint64)
    it = _Items()
    assert _host(dtype, 4, n_each, rate, nxt, hops, each) == NO_DEVICE
    assert _host(dtype, 4, n_each, rate, None, None) == NO_DEVICE
    assert _lists(dtype, 4, n_each, rate, nxt, hops, it, each) == NO_DEVICE
    assert _lists(dtype, 4, n_each, rate, nxt, None, _Items(items=0)) == NO_DEVICE   # items == 0: a plain solve
    # ... where the three-tier family still refuses them
    fn3 = getattr(_lib.lib(), "fwx_solve_ragged_" + SUFFIX[dtype])
    assert fn3(4, _p(n_each), _p(rate), _p(nxt), _p(hops), None, None) == UNSUPPORTED
    mats = [np.full((n, n), 0.5, dtype=dtype) for n in orders]
    kept = [m.copy() for m in mats]
    with pytest.raises(engine.FwxError) as e:
        engine.solve_ragged_mid(mats, count_updates=True)
    assert e.value.status == NO_DEVICE
    with pytest.raises(engine.FwxError) as e:
        engine.solve_ragged_mid_lists(mats, [np.zeros((n, n), dtype=np.int32) for n in orders])
    assert e.value.status == NO_DEVICE
    with pytest.raises(engine.FwxError) as e:
        engine.solve_ragged_mid(mats + [np.full((257, 257), 0.5, dtype=dtype)])
    assert e.value.status == UNSUPPORTED
    for m, k in zip(mats, kept):
        assert np.array_equal(m, k)
    bits = np.uint64 if dtype == np.float64 else np.uint32
    assert np.array_equal(rate.view(bits), before[0].view(bits))
    assert np.array_equal(nxt, before[1]) and np.array_equal(hops, before[2])
    assert list(each) == [9] * 4 and list(it.len) == [77, 77]
    code = _lib.FWX_F64 if dtype == np.float64 else _lib.FWX_F32
    assert _dev(4, code, FAKE, None, None, tiers=_tiers(1, 0, 0, 2)) == NO_DEVICE
    assert _dev(4, code, FAKE, None, None, tiers=_tiers(0, 0, 0, 4)) == NO_DEVICE
    assert _dev(4, code, FAKE, FAKE, FAKE, tiers=_tiers(1, 1, 1, 1), trace=_trace()) == NO_DEVICE
    assert _walk(4, 129, 2, 4, _trace()) == NO_DEVICE
    assert _walk(4, 256, 2, 4, _trace()) == NO_DEVICE


# ---- the Python binding ------------------------------------------------------------------------------
def test_python_binding_checks_what_it_packs():
    sq = lambda n, dtype=np.float64: np.full((n, n), 0.5, dtype=dtype)
    ix = lambda n: np.zeros((n, n), dtype=np.int32)
    for fn in (engine.solve_ragged_mid, engine.solve_ragged_mid_lists):
        with pytest.raises(ValueError):
            fn([sq(4), np.zeros((3, 4))], [ix(4), np.zeros((3, 4), dtype=np.int32)])       # not square
        with pytest.raises(ValueError):
            fn([sq(4), sq(5, np.float32)], [ix(4), ix(5)])                                  # mixed dtypes
        with pytest.raises(ValueError):
            fn([sq(4), sq(5)], [ix(4), ix(4)])                                              # next shaped unlike its rate
        with pytest.raises(ValueError):
            fn([sq(4), sq(5)], [ix(4), ix(5)], [ix(4), ix(5).astype(np.int64)])             # hops of another type
    with pytest.raises(ValueError):
        engine.solve_ragged_mid([sq(4)], None, [ix(4)])                                     # hops requires next
    with pytest.raises(ValueError):
        engine.solve_ragged_mid_lists([sq(4)], None)                                        # the lists need next
    assert engine.solve_ragged_mid([], count_updates=True).shape == (0,)                    # empty: success
    assert list(engine.solve_ragged_mid([sq(0), sq(0)], count_updates=True)) == [0, 0]
    assert engine.solve_ragged_mid_lists([sq(0)], [ix(0)]) == []
