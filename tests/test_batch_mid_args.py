"""Batched mid-size solves (fwx_solve_batch_mid_f64 / _f32, fwx_dev_solve_batch_mid): the symbols exist, every
argument check of the contract in include/fwx.h is decided before any device call -- the case list of
test_batch_args.py with the limit at 256 -- and FWX_BATCH_MID_MIN_N parses as documented.  CPU only: no launch is
made here."""
import ctypes

import numpy as np
import pytest

from floydwarshall_amd import _lib, engine

OK, INVALID, UNSUPPORTED, NO_DEVICE = (_lib.FWX_OK, _lib.FWX_ERR_INVALID, _lib.FWX_ERR_UNSUPPORTED,
                                      _lib.FWX_ERR_NO_DEVICE)
HOST = {np.float64: "fwx_solve_batch_mid_f64", np.float32: "fwx_solve_batch_mid_f32"}
DTYPES = [np.float64, np.float32]
MID_MIN_N_DEFAULT = 129      # FWX_BATCH_MID_MIN_N unset, as include/fwx.h documents it
NO_GPU = pytest.mark.skipif(engine.device_count() > 0, reason="only meaningful without a GPU")


def _batch(count, n, dtype):
    rate = np.full((count, n, n), 0.5, dtype=dtype)
    nxt = np.tile(np.arange(n, dtype=np.int32), (count, n, 1))
    hops = np.ones((count, n, n), dtype=np.int32)
    return rate, nxt, hops


def _opts(**kw):
    o = _lib.FwxOpts()
    o.struct_size = ctypes.sizeof(_lib.FwxOpts)
    o.device = -1
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _host(dtype, count, n, rate, nxt, hops, each=None, opts=None):
    p = lambda a: None if a is None else a.ctypes.data
    return getattr(_lib.lib(), HOST[dtype])(count, n, p(rate), p(nxt), p(hops), p(each),
                                            None if opts is None else ctypes.byref(opts))


def _dev(count, n, dtype_code, rate, nxt, hops, stride, kb=0, ke=0, upd=None):
    # the pointers are never dereferenced: every case here returns before a device call
    return _lib.lib().fwx_dev_solve_batch_mid(count, n, dtype_code, rate, nxt, hops, stride, kb, ke, upd, None)


def test_the_mid_symbols_are_exported_and_bound():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("fwx_solve_batch_mid_f64", "fwx_solve_batch_mid_f32", "fwx_dev_solve_batch_mid",
                 "fwx_test_batch_mid_min_n", "fwx_test_batch_mid_block"):
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.FWX_BATCH_MID_MAX_N == 256
    assert _lib.FWX_BATCH_MAX_N == 128                  # the existing entry points keep their limit
    assert _lib.lib().fwx_abi_version() == 3           # symbols are only added


def test_the_block_width_is_in_range():
    assert 1 <= _lib.lib().fwx_test_batch_mid_block() <= 64


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_form_rejects_bad_arguments_before_any_device_call(dtype):
    rate, nxt, hops = _batch(2, 4, dtype)
    before = rate.copy()
    assert _host(dtype, -1, 4, rate, nxt, hops) == INVALID                       # count < 0
    assert _host(dtype, 2, -1, rate, nxt, hops) == INVALID                       # n < 0
    assert _host(dtype, -1, 0, rate, nxt, hops) == INVALID                       # negative beats zero
    assert _host(dtype, 0, -1, rate, nxt, hops) == INVALID
    assert _host(dtype, 2, 4, None, nxt, hops) == INVALID                        # no rates
    assert _host(dtype, 2, 4, rate, None, hops) == INVALID                       # hops without next
    assert _host(dtype, 2, 4, rate, nxt, hops, opts=_opts(struct_size=4)) == INVALID
    for kb, ke in ((3, 2), (-1, 4), (0, 5), (5, 0)):                             # bad pivot ranges
        assert _host(dtype, 2, 4, rate, nxt, hops, opts=_opts(k_begin=kb, k_end=ke)) == INVALID, (kb, ke)
    assert _host(dtype, 2, 4, rate, nxt, hops, opts=_opts(engine=99)) == INVALID
    big = np.zeros((1, 257, 257), dtype=dtype)
    assert _host(dtype, 1, 257, big, None, None) == UNSUPPORTED                  # n > FWX_BATCH_MID_MAX_N
    assert _host(dtype, 1, 257, big, None, None, opts=_opts(k_begin=258)) == INVALID   # the range is judged first
    for eng in (_lib.FWX_ENGINE_PERK, _lib.FWX_ENGINE_FUSED):
        assert _host(dtype, 2, 4, rate, nxt, hops, opts=_opts(engine=eng)) == UNSUPPORTED, eng
        assert _host(dtype, 1, 200, big, None, None, opts=_opts(engine=eng)) == UNSUPPORTED, eng
    assert np.array_equal(rate, before)


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_batches_are_success_and_touch_nothing(dtype):
    rate, nxt, hops = _batch(2, 4, dtype)
    before = rate.copy(), nxt.copy(), hops.copy()
    each = np.full(2, 77, dtype=np.uint64)
    total = ctypes.c_uint64(55)
    o = _opts(updates_out=ctypes.pointer(total))
    assert _host(dtype, 0, 4, rate, nxt, hops, each, o) == OK
    assert _host(dtype, 0, 200, rate, nxt, hops, each, o) == OK
    assert _host(dtype, 2, 0, rate, nxt, hops, each, o) == OK
    assert _host(dtype, 0, 0, None, None, None) == OK
    assert _host(dtype, 0, 4096, None, None, None) == OK                         # nothing to solve, whatever n
    for got, want in zip((rate, nxt, hops), before):
        assert np.array_equal(got, want)
    assert list(each) == [77, 77] and total.value == 55


def test_device_form_rejects_bad_arguments_before_any_device_call():
    fake = ctypes.c_void_p(4096)        # never dereferenced
    for code in (_lib.FWX_F32, _lib.FWX_F64):
        assert _dev(-1, 4, code, fake, fake, fake, 16) == INVALID
        assert _dev(2, -1, code, fake, fake, fake, 16) == INVALID
        assert _dev(2, 4, code, None, fake, fake, 16) == INVALID
        assert _dev(2, 4, code, fake, None, fake, 16) == INVALID                 # hops without next
        assert _dev(2, 4, code, fake, fake, fake, 15) == INVALID                 # stride < n*n
        assert _dev(2, 4, code, fake, fake, fake, -16) == INVALID
        assert _dev(2, 200, code, fake, fake, fake, 200 * 200 - 1) == INVALID
        for kb, ke in ((3, 2), (-1, 4), (0, 5), (5, 0)):
            assert _dev(2, 4, code, fake, fake, fake, 16, kb, ke) == INVALID, (kb, ke)
        assert _dev(2, 200, code, fake, fake, fake, 40000, 0, 201) == INVALID
        assert _dev(1, 257, code, fake, None, None, 257 * 257) == UNSUPPORTED
        assert _dev(0, 4, code, None, None, None, 0) == OK
        assert _dev(2, 0, code, None, None, None, 0) == OK
        assert _dev(0, 257, code, None, None, None, 0) == OK
    assert _dev(2, 4, 7, fake, fake, fake, 16) == INVALID                        # no such dtype
    assert _dev(2, 200, 7, fake, fake, fake, 40000) == INVALID


@NO_GPU
def test_every_order_from_129_to_256_is_accepted_by_the_device_form():
    """Past every argument check: without a device that is FWX_ERR_NO_DEVICE, not FWX_ERR_UNSUPPORTED."""
    fake = ctypes.c_void_p(4096)
    for n in range(129, 257):
        for code in (_lib.FWX_F32, _lib.FWX_F64):
            assert _dev(1, n, code, fake, None, None, n * n) == NO_DEVICE, n
            assert _dev(3, n, code, fake, fake, fake, n * n + 5, 7, n - 1) == NO_DEVICE, n


@NO_GPU
@pytest.mark.parametrize("n", [129, 130, 200, 255, 256])
def test_orders_129_to_256_are_accepted_by_the_host_form_only_through_the_mid_entry_points(n):
    fake = ctypes.c_void_p(4096)
    rate = np.zeros((1, n, n))
    assert _host(np.float64, 1, n, rate, None, None) == NO_DEVICE
    # the existing entry points keep their limit
    assert _lib.lib().fwx_dev_solve_batch(1, n, _lib.FWX_F64, fake, None, None, n * n, 0, 0, None, None) == UNSUPPORTED
    assert _lib.lib().fwx_solve_batch_f64(1, n, rate.ctypes.data, None, None, None, None) == UNSUPPORTED


@NO_GPU
@pytest.mark.parametrize("n", [5, 131])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_valid_call_without_a_device_reports_it_and_leaves_the_arrays_alone(dtype, n):
    rate, nxt, hops = _batch(3, n, dtype)
    rate[1, 2, 3] = np.nan
    before = rate.copy(), nxt.copy(), hops.copy()
    each = np.full(3, 9, dtype=np.uint64)
    total = ctypes.c_uint64(55)
    assert _host(dtype, 3, n, rate, nxt, hops, each, _opts(updates_out=ctypes.pointer(total))) == NO_DEVICE
    with pytest.raises(engine.FwxError) as e:
        engine.solve_batch_mid(rate, nxt, hops, count_updates=True)
    assert e.value.status == NO_DEVICE
    it = np.uint64 if dtype == np.float64 else np.uint32
    assert np.array_equal(rate.view(it), before[0].view(it))
    assert np.array_equal(nxt, before[1]) and np.array_equal(hops, before[2])
    assert list(each) == [9, 9, 9] and total.value == 55
    code = _lib.FWX_F64 if dtype == np.float64 else _lib.FWX_F32
    assert _dev(3, n, code, ctypes.c_void_p(4096), None, None, n * n) == NO_DEVICE


def test_python_binding_checks_shapes():
    rate, nxt, hops = _batch(2, 4, np.float64)
    with pytest.raises(ValueError):
        engine.solve_batch_mid(rate[0])                      # one matrix is not a batch
    with pytest.raises(ValueError):
        engine.solve_batch_mid(rate, None, hops)             # hops requires next
    with pytest.raises(ValueError):
        engine.solve_batch_mid(rate, nxt[:, :, :3])
    with pytest.raises(ValueError):
        engine.solve_batch_mid(rate.astype(np.float16))
    with pytest.raises(ValueError):
        engine.solve_batch_mid(np.zeros((2, 130, 131)))
    assert engine.solve_batch_mid(np.zeros((0, 4, 4)), count_updates=True).shape == (0,)     # empty: success
    assert engine.solve_batch_mid(np.zeros((0, 200, 200)), count_updates=True).shape == (0,)
    with pytest.raises(engine.FwxError) as e:
        engine.solve_batch_mid(np.zeros((1, 257, 257)))
    assert e.value.status == UNSUPPORTED


# ---- FWX_BATCH_MID_MIN_N -----------------------------------------------------------------------------
def _parsed():
    return _lib.lib().fwx_test_batch_mid_min_n()


def test_mid_threshold_default(monkeypatch):
    """The documented default (include/fwx.h): only what the small tiers cannot take."""
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    assert _parsed() == MID_MIN_N_DEFAULT


@pytest.mark.parametrize("value", [str(v) for v in range(1, 130)])
def test_mid_threshold_integers_from_1_to_129_are_taken(value, monkeypatch):
    monkeypatch.setenv("FWX_BATCH_MID_MIN_N", value)
    assert _parsed() == int(value)


@pytest.mark.parametrize("value", ["", "0", "130", "256", "1000", "-1", "-0", "+4", " 4", "4 ", "4.0", "4x", "x4", "0x8",
                                   "four", "1 6", "99999999999999999999", "nan"])
def test_mid_threshold_anything_else_is_the_default(value, monkeypatch):
    monkeypatch.setenv("FWX_BATCH_MID_MIN_N", value)
    assert _parsed() == MID_MIN_N_DEFAULT


def test_mid_threshold_is_read_on_every_call(monkeypatch):
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    for value in ("1", "junk", "129", "64", "0"):
        monkeypatch.setenv("FWX_BATCH_MID_MIN_N", value)
        assert _parsed() == (int(value) if value.isdigit() and 1 <= int(value) <= 129 else MID_MIN_N_DEFAULT)
