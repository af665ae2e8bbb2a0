"""Batched large solves (fwx_solve_batch_large_f64 / _f32, fwx_dev_solve_batch_large): the symbols exist, every
argument check of the contract in include/fwx.h is decided before any device call -- the case list of
test_batch_mid_args.py with the limit at 1024, plus the scratch of the device form, which is judged only where it is
used -- and FWX_BATCH_LARGE_MIN_N parses as documented.  CPU only: no launch is made here."""
import ctypes
import os
import re

import numpy as np
import pytest

from floydwarshall_amd import _lib, engine

OK, INVALID, UNSUPPORTED, NO_DEVICE = (_lib.FWX_OK, _lib.FWX_ERR_INVALID, _lib.FWX_ERR_UNSUPPORTED,
                                      _lib.FWX_ERR_NO_DEVICE)
HOST = {np.float64: "fwx_solve_batch_large_f64", np.float32: "fwx_solve_batch_large_f32"}
DTYPES = [np.float64, np.float32]
LARGE_MIN_N_DEFAULT = 257    # FWX_BATCH_LARGE_MIN_N unset, as include/fwx.h documents it
NO_GPU = pytest.mark.skipif(engine.device_count() > 0, reason="only meaningful without a GPU")
FAKE = ctypes.c_void_p(4096)          # never dereferenced; 16-byte aligned
PLENTY = 1 << 30


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


def _dev(count, n, dtype_code, rate, nxt, hops, stride, kb=0, ke=0, upd=None, scratch=FAKE, scratch_bytes=PLENTY):
    # the pointers are never dereferenced: every case here returns before a device call
    return _lib.lib().fwx_dev_solve_batch_large(count, n, dtype_code, rate, nxt, hops, stride, kb, ke, upd, scratch,
                                                scratch_bytes, None)


def _geometry():
    out = (ctypes.c_int32 * 4)()
    assert _lib.lib().fwx_test_batch_large_geometry(out) == OK
    return tuple(out)


def _scratch_bytes_of_the_header(n):
    """FWX_BATCH_LARGE_SCRATCH_BYTES(n) as include/fwx.h spells it: ((size_t)(n) * <integer>)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "fwx.h")).read()
    m = re.search(r"#define\s+FWX_BATCH_LARGE_SCRATCH_BYTES\(n\)\s+\(\(size_t\)\(n\)\s*\*\s*(\d+)\)", src)
    assert m, "the macro is a compile-time expression of n alone"
    return n * int(m.group(1))


def test_the_large_symbols_are_exported_and_bound():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("fwx_solve_batch_large_f64", "fwx_solve_batch_large_f32", "fwx_dev_solve_batch_large",
                 "fwx_test_batch_large_min_n", "fwx_test_batch_large_geometry"):
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.FWX_BATCH_LARGE_MAX_N == 1024
    assert _lib.FWX_BATCH_MID_MAX_N == 256 and _lib.FWX_BATCH_MAX_N == 128     # the existing limits stay
    assert _lib.lib().fwx_abi_version() == 3                                    # symbols are only added


def test_the_geometry_is_in_range_and_the_scratch_holds_the_panels():
    B, S, tr, tc = _geometry()
    assert 1 <= B <= 64 and 1 <= S <= 1024 and 1 <= tr <= 1024 and 1 <= tc <= 1024
    assert _lib.lib().fwx_test_batch_large_geometry(None) == INVALID
    for n in (1, 2, 255, 256, 257, 600, 1023, 1024):
        per = _scratch_bytes_of_the_header(n)
        assert per >= 2 * B * n * 16, n             # 2 panels x B rows x n columns x (f64 + next + hops)
        assert per % 16 == 0, n                     # consecutive matrices stay 16-byte aligned
        assert _lib.batch_large_scratch_bytes(n) == per


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
    big = np.zeros((1, 1025, 1025), dtype=dtype)
    assert _host(dtype, 1, 1025, big, None, None) == UNSUPPORTED                 # n > FWX_BATCH_LARGE_MAX_N
    assert _host(dtype, 1, 1025, big, None, None, opts=_opts(k_begin=1026)) == INVALID   # the range is judged first
    for eng in (_lib.FWX_ENGINE_PERK, _lib.FWX_ENGINE_FUSED):
        assert _host(dtype, 2, 4, rate, nxt, hops, opts=_opts(engine=eng)) == UNSUPPORTED, eng
        assert _host(dtype, 1, 600, big, None, None, opts=_opts(engine=eng)) == UNSUPPORTED, eng
    assert np.array_equal(rate, before)


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_batches_are_success_and_touch_nothing(dtype):
    rate, nxt, hops = _batch(2, 4, dtype)
    before = rate.copy(), nxt.copy(), hops.copy()
    each = np.full(2, 77, dtype=np.uint64)
    total = ctypes.c_uint64(55)
    o = _opts(updates_out=ctypes.pointer(total))
    assert _host(dtype, 0, 4, rate, nxt, hops, each, o) == OK
    assert _host(dtype, 0, 600, rate, nxt, hops, each, o) == OK
    assert _host(dtype, 2, 0, rate, nxt, hops, each, o) == OK
    assert _host(dtype, 0, 0, None, None, None) == OK
    assert _host(dtype, 0, 4096, None, None, None) == OK                         # nothing to solve, whatever n
    for got, want in zip((rate, nxt, hops), before):
        assert np.array_equal(got, want)
    assert list(each) == [77, 77] and total.value == 55


def test_device_form_rejects_bad_arguments_before_any_device_call():
    for code in (_lib.FWX_F32, _lib.FWX_F64):
        assert _dev(-1, 4, code, FAKE, FAKE, FAKE, 16) == INVALID
        assert _dev(2, -1, code, FAKE, FAKE, FAKE, 16) == INVALID
        assert _dev(2, 4, code, None, FAKE, FAKE, 16) == INVALID
        assert _dev(2, 4, code, FAKE, None, FAKE, 16) == INVALID                 # hops without next
        assert _dev(2, 4, code, FAKE, FAKE, FAKE, 15) == INVALID                 # stride < n*n
        assert _dev(2, 4, code, FAKE, FAKE, FAKE, -16) == INVALID
        assert _dev(2, 600, code, FAKE, FAKE, FAKE, 600 * 600 - 1) == INVALID
        for kb, ke in ((3, 2), (-1, 4), (0, 5), (5, 0)):
            assert _dev(2, 4, code, FAKE, FAKE, FAKE, 16, kb, ke) == INVALID, (kb, ke)
        assert _dev(2, 600, code, FAKE, FAKE, FAKE, 360000, 0, 601) == INVALID
        assert _dev(1, 1025, code, FAKE, None, None, 1025 * 1025) == UNSUPPORTED
        assert _dev(1, 1025, code, FAKE, None, None, 1025 * 1025, scratch=None, scratch_bytes=0) == UNSUPPORTED
        assert _dev(0, 4, code, None, None, None, 0, scratch=None, scratch_bytes=0) == OK
        assert _dev(2, 0, code, None, None, None, 0, scratch=None, scratch_bytes=0) == OK
        assert _dev(0, 1025, code, None, None, None, 0) == OK
    assert _dev(2, 4, 7, FAKE, FAKE, FAKE, 16) == INVALID                        # no such dtype
    assert _dev(2, 600, 7, FAKE, FAKE, FAKE, 360000) == INVALID


@pytest.mark.parametrize("n", [257, 600, 1024])
def test_bad_scratch_is_invalid_when_the_call_is_routed_to_the_large_tier(n, monkeypatch):
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    per = _lib.batch_large_scratch_bytes(n)
    for code in (_lib.FWX_F32, _lib.FWX_F64):
        assert _dev(2, n, code, FAKE, None, None, n * n, scratch=None) == INVALID                      # NULL
        assert _dev(2, n, code, FAKE, None, None, n * n, scratch=None, scratch_bytes=0) == INVALID
        for misaligned in (4097, 4100, 4104, 4111):
            assert _dev(2, n, code, FAKE, None, None, n * n, scratch=ctypes.c_void_p(misaligned)) == INVALID, misaligned
        assert _dev(2, n, code, FAKE, None, None, n * n, scratch_bytes=per - 1) == INVALID             # less than one
        assert _dev(2, n, code, FAKE, None, None, n * n, scratch_bytes=0) == INVALID
        # the other checks come first
        assert _dev(2, n, code, None, None, None, n * n, scratch=None) == INVALID
        assert _dev(2, n, 7, FAKE, None, None, n * n, scratch=None) == INVALID


@NO_GPU
def test_scratch_is_judged_only_where_it_is_used(monkeypatch):
    """Past every check the call reports FWX_ERR_NO_DEVICE: bad scratch passes where the order is forwarded to the mid
    entry path and where the pivot range is empty, and only there."""
    bad = dict(scratch=None, scratch_bytes=0)
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    for code in (_lib.FWX_F32, _lib.FWX_F64):
        for n in (1, 5, 128, 129, 256):                                          # below the default threshold
            assert _dev(2, n, code, FAKE, None, None, n * n, **bad) == NO_DEVICE, n
            assert _dev(2, n, code, FAKE, None, None, n * n, scratch=ctypes.c_void_p(4097), scratch_bytes=3) == NO_DEVICE
        assert _dev(2, 257, code, FAKE, None, None, 257 * 257, 5, 5, **bad) == NO_DEVICE            # no pivots
        assert _dev(2, 257, code, FAKE, None, None, 257 * 257, 5, 6, **bad) == INVALID
        assert _dev(2, 257, code, FAKE, None, None, 257 * 257, 5, 6) == NO_DEVICE
    monkeypatch.setenv("FWX_BATCH_LARGE_MIN_N", "1")                             # now everything is routed there
    for n in (1, 5, 256):
        assert _dev(2, n, _lib.FWX_F64, FAKE, None, None, n * n, **bad) == INVALID, n
        assert _dev(2, n, _lib.FWX_F64, FAKE, None, None, n * n, scratch_bytes=_lib.batch_large_scratch_bytes(n) - 1) \
            == INVALID, n
        assert _dev(2, n, _lib.FWX_F64, FAKE, None, None, n * n, scratch_bytes=_lib.batch_large_scratch_bytes(n)) \
            == NO_DEVICE, n
    monkeypatch.setenv("FWX_BATCH_LARGE_MIN_N", "6")
    assert _dev(2, 5, _lib.FWX_F64, FAKE, None, None, 25, **bad) == NO_DEVICE
    assert _dev(2, 6, _lib.FWX_F64, FAKE, None, None, 36, **bad) == INVALID


@NO_GPU
def test_orders_up_to_1024_are_accepted_by_the_device_form():
    """Past every argument check: without a device that is FWX_ERR_NO_DEVICE, not FWX_ERR_UNSUPPORTED."""
    for n in list(range(257, 1025, 59)) + [1023, 1024]:
        per = _lib.batch_large_scratch_bytes(n)
        for code in (_lib.FWX_F32, _lib.FWX_F64):
            assert _dev(1, n, code, FAKE, None, None, n * n, scratch_bytes=per) == NO_DEVICE, n
            assert _dev(3, n, code, FAKE, FAKE, FAKE, n * n + 5, 7, n - 1, scratch_bytes=per) == NO_DEVICE, n


@NO_GPU
@pytest.mark.parametrize("n", [257, 258, 600, 1023, 1024])
def test_orders_257_to_1024_are_accepted_by_the_host_form_only_through_the_large_entry_points(n):
    rate = np.zeros((1, n, n))
    assert _host(np.float64, 1, n, rate, None, None) == NO_DEVICE
    # the existing entry points keep their limits
    L = _lib.lib()
    assert L.fwx_dev_solve_batch_mid(1, n, _lib.FWX_F64, FAKE, None, None, n * n, 0, 0, None, None) == UNSUPPORTED
    assert L.fwx_solve_batch_mid_f64(1, n, rate.ctypes.data, None, None, None, None) == UNSUPPORTED
    assert L.fwx_solve_batch_f64(1, n, rate.ctypes.data, None, None, None, None) == UNSUPPORTED


@NO_GPU
@pytest.mark.parametrize("n", [5, 131, 259])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_valid_call_without_a_device_reports_it_and_leaves_the_arrays_alone(dtype, n):
    rate, nxt, hops = _batch(3, n, dtype)
    rate[1, 2, 3] = np.nan
    before = rate.copy(), nxt.copy(), hops.copy()
    each = np.full(3, 9, dtype=np.uint64)
    total = ctypes.c_uint64(55)
    assert _host(dtype, 3, n, rate, nxt, hops, each, _opts(updates_out=ctypes.pointer(total))) == NO_DEVICE
    with pytest.raises(engine.FwxError) as e:
        engine.solve_batch_large(rate, nxt, hops, count_updates=True)
    assert e.value.status == NO_DEVICE
    it = np.uint64 if dtype == np.float64 else np.uint32
    assert np.array_equal(rate.view(it), before[0].view(it))
    assert np.array_equal(nxt, before[1]) and np.array_equal(hops, before[2])
    assert list(each) == [9, 9, 9] and total.value == 55
    code = _lib.FWX_F64 if dtype == np.float64 else _lib.FWX_F32
    assert _dev(3, n, code, FAKE, None, None, n * n) == NO_DEVICE


def test_python_binding_checks_shapes():
    rate, nxt, hops = _batch(2, 4, np.float64)
    with pytest.raises(ValueError):
        engine.solve_batch_large(rate[0])                      # one matrix is not a batch
    with pytest.raises(ValueError):
        engine.solve_batch_large(rate, None, hops)             # hops requires next
    with pytest.raises(ValueError):
        engine.solve_batch_large(rate, nxt[:, :, :3])
    with pytest.raises(ValueError):
        engine.solve_batch_large(rate.astype(np.float16))
    with pytest.raises(ValueError):
        engine.solve_batch_large(np.zeros((2, 300, 301)))
    assert engine.solve_batch_large(np.zeros((0, 4, 4)), count_updates=True).shape == (0,)     # empty: success
    assert engine.solve_batch_large(np.zeros((0, 600, 600)), count_updates=True).shape == (0,)
    with pytest.raises(engine.FwxError) as e:
        engine.solve_batch_large(np.zeros((1, 1025, 1025)))
    assert e.value.status == UNSUPPORTED


# ---- FWX_BATCH_LARGE_MIN_N ---------------------------------------------------------------------------
def _parsed():
    return _lib.lib().fwx_test_batch_large_min_n()


def test_large_threshold_default(monkeypatch):
    """The documented default (include/fwx.h): only what the mid tier cannot take."""
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    assert _parsed() == LARGE_MIN_N_DEFAULT


def test_large_threshold_integers_from_1_to_257_are_taken(monkeypatch):
    for v in range(1, 258):
        monkeypatch.setenv("FWX_BATCH_LARGE_MIN_N", str(v))
        assert _parsed() == v


@pytest.mark.parametrize("value", ["", "0", "258", "1024", "1000", "-1", "-0", "+4", " 4", "4 ", "4.0", "4x", "x4", "0x8",
                                   "four", "1 6", "99999999999999999999", "nan"])
def test_large_threshold_anything_else_is_the_default(value, monkeypatch):
    monkeypatch.setenv("FWX_BATCH_LARGE_MIN_N", value)
    assert _parsed() == LARGE_MIN_N_DEFAULT


def test_large_threshold_is_read_on_every_call_and_leaves_the_mid_one_alone(monkeypatch):
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    for value in ("1", "junk", "257", "64", "0"):
        monkeypatch.setenv("FWX_BATCH_LARGE_MIN_N", value)
        assert _parsed() == (int(value) if value.isdigit() and 1 <= int(value) <= 257 else LARGE_MIN_N_DEFAULT)
        assert _lib.lib().fwx_test_batch_mid_min_n() == 129
