"""Batched what-if sweeps (fwx_solve_sweep_f64 / _f32, fwx_dev_solve_sweep): the symbols exist and every status rule of
the contract in include/fwx.h is decided before any device call, with every output left as it was.  CPU only: no
launch is made here."""
import ctypes

import numpy as np
import pytest

from floydwarshall_amd import _lib, engine

OK, INVALID, UNSUPPORTED, NO_DEVICE = (_lib.FWX_OK, _lib.FWX_ERR_INVALID, _lib.FWX_ERR_UNSUPPORTED,
                                      _lib.FWX_ERR_NO_DEVICE)
HOST = {np.float64: "fwx_solve_sweep_f64", np.float32: "fwx_solve_sweep_f32"}
CODE = {np.float64: _lib.FWX_F64, np.float32: _lib.FWX_F32}
DTYPES = [np.float64, np.float32]
SENTINEL_RATE, SENTINEL_INT, SENTINEL_U = -77.25, -7777, 4242


def _ptr(a):
    return None if a is None else a.ctypes.data


class Call:
    """A valid sweep of `count` variants of order n, two patches and two items a variant, outputs sentinel-filled.
    Fields are overwritten case by case; what a struct points at stays alive here."""

    def __init__(self, dtype, count=3, n=4):
        self.dtype, self.count, self.n = dtype, count, n
        self.rate = np.full((n, n), 0.5, dtype=dtype)
        self.next = np.tile(np.arange(n, dtype=np.int32), (n, 1))
        self.hops = np.ones((n, n), dtype=np.int32)
        self.pptr = np.arange(count + 1, dtype=np.int64) * 2
        self.pindex = np.tile(np.array([1, n * n - 2], dtype=np.int64), count)
        self.prate = np.full(2 * count, 2.0, dtype=dtype)
        self.pnext = np.zeros(2 * count, dtype=np.int32)
        self.phops = np.ones(2 * count, dtype=np.int32)
        self.iptr = np.arange(count + 1, dtype=np.int64) * 2
        self.src = np.tile(np.array([0, n - 1], dtype=np.int32), count)
        self.dst = np.tile(np.array([n - 1, 0], dtype=np.int32), count)
        self.rate_out = np.full(2 * count, SENTINEL_RATE, dtype=dtype)
        self.next_out = np.full(2 * count, SENTINEL_INT, dtype=np.int32)
        self.hops_out = np.full(2 * count, SENTINEL_INT, dtype=np.int32)
        self.each = np.full(count, SENTINEL_U, dtype=np.uint64)
        self.total = ctypes.c_uint64(SENTINEL_U)
        self.p = _lib.FwxSweepPatches(_ptr(self.pptr), 2 * count, _ptr(self.pindex), _ptr(self.prate),
                                      _ptr(self.pnext), _ptr(self.phops))
        self.it = _lib.FwxSweepItems(_ptr(self.iptr), 2 * count, _ptr(self.src), _ptr(self.dst), _ptr(self.rate_out),
                                     _ptr(self.next_out), _ptr(self.hops_out))
        self.full = _lib.FwxSweepFull(None, None, None, n * n)
        self.base = [_ptr(self.rate), _ptr(self.next), _ptr(self.hops)]
        self.opts = _lib.FwxOpts()
        self.opts.struct_size = ctypes.sizeof(_lib.FwxOpts)
        self.opts.device = -1
        self.opts.updates_out = ctypes.pointer(self.total)
        self.use_patches = self.use_items = self.use_full = True
        self.code = CODE[dtype]

    def _structs(self):
        return (ctypes.byref(self.p) if self.use_patches else None, ctypes.byref(self.it) if self.use_items else None)

    def host(self):
        p, it = self._structs()
        return getattr(_lib.lib(), HOST[self.dtype])(self.count, self.n, *self.base, p, it, _ptr(self.each),
                                                     ctypes.byref(self.opts))

    def dev(self):
        # host memory stands in for device memory: every case here returns before a device call
        p, it = self._structs()
        return _lib.lib().fwx_dev_solve_sweep(self.count, self.n, self.code, *self.base, p, it,
                                              ctypes.byref(self.full) if self.use_full else None, _ptr(self.each), None)

    def untouched(self):
        return (np.all(self.rate_out == SENTINEL_RATE) and np.all(self.next_out == SENTINEL_INT) and
                np.all(self.hops_out == SENTINEL_INT) and np.all(self.each == SENTINEL_U) and
                self.total.value == SENTINEL_U and np.all(self.rate == 0.5))


def _set(obj_name, field, value):
    def change(c):
        setattr(getattr(c, obj_name) if obj_name else c, field, value)
    return change


def _base(i, value):
    def change(c):
        c.base[i] = value
    return change


def _chain(*changes):
    def change(c):
        for f in changes:
            f(c)
    return change


FAKE = 4096     # a non-null pointer that is never dereferenced

# every status rule both forms share: (what, the change to a valid call)
SHARED_INVALID = [
    ("count < 0", _set(None, "count", -1)),
    ("n < 0", _set(None, "n", -1)),
    ("negative beats zero", _chain(_set(None, "count", -1), _set(None, "n", 0))),
    ("base_rate NULL", _base(0, None)),
    ("base_hops without base_next", _chain(_base(1, None), _set("p", "next", None), _set("it", "next_out", None))),
    ("patches->next without base_next",
     _chain(_base(1, None), _base(2, None), _set("p", "hops", None), _set("it", "next_out", None),
            _set("it", "hops_out", None))),
    ("patches->hops without base_hops", _chain(_base(2, None), _set("it", "hops_out", None))),
    ("items->next_out without base_next",
     _chain(_base(1, None), _base(2, None), _set("p", "next", None), _set("p", "hops", None),
            _set("it", "hops_out", None))),
    ("items->hops_out without base_hops", _chain(_base(2, None), _set("p", "hops", None))),
    ("negative patch total", _set("p", "total", -1)),
    ("negative item total", _set("it", "total", -1)),
    ("patches->ptr NULL", _set("p", "ptr", None)),
    ("patches->index NULL", _set("p", "index", None)),
    ("patches->rate NULL", _set("p", "rate", None)),
    ("items->ptr NULL", _set("it", "ptr", None)),
    ("items->src NULL", _set("it", "src", None)),
    ("items->dst NULL", _set("it", "dst", None)),
    ("items->rate_out NULL", _set("it", "rate_out", None)),
]
DEV_ONLY_INVALID = [
    ("a bad dtype", _set(None, "code", 7)),
    ("full->next without base_next",
     _chain(_base(1, None), _base(2, None), _set("p", "next", None), _set("p", "hops", None),
            _set("it", "next_out", None), _set("it", "hops_out", None), _set("full", "next", FAKE))),
    ("full->hops without base_hops",
     _chain(_base(2, None), _set("p", "hops", None), _set("it", "hops_out", None), _set("full", "hops", FAKE))),
    ("full->stride < n*n with a full rate", _chain(_set("full", "rate", FAKE), _set("full", "stride", 15))),
    ("full->stride < n*n with a full next", _chain(_set("full", "next", FAKE), _set("full", "stride", 15))),
    ("full->stride < n*n with full hops", _chain(_set("full", "hops", FAKE), _set("full", "stride", -16))),
]


def _opt(field, value):
    def change(c):
        setattr(c.opts, field, value)
    return change


def _table(name, i, value):
    def change(c):
        getattr(c, name)[i] = value
    return change


HOST_ONLY_INVALID = [
    ("a bad struct_size", _opt("struct_size", 4)),
    ("a pivot range that starts late", _opt("k_begin", 1)),
    ("a pivot range that ends early", _opt("k_end", 3)),
    ("a pivot range past n", _opt("k_end", 5)),
    ("no such engine", _opt("engine", 99)),
    ("patches->ptr[0] != 0", _table("pptr", 0, 1)),
    ("a descending patches->ptr", _table("pptr", 1, 5)),
    ("patches->ptr[count] != total", _table("pptr", 3, 5)),
    ("items->ptr[0] != 0", _table("iptr", 0, 1)),
    ("a descending items->ptr", _table("iptr", 2, 1)),
    ("items->ptr[count] != total", _table("iptr", 3, 7)),
    ("a patch index of -1", _table("pindex", 3, -1)),
    ("a patch index of n*n", _table("pindex", 0, 16)),
    ("an item src of n", _table("src", 2, 4)),
    ("an item src of -1", _table("src", 0, -1)),
    ("an item dst of n", _table("dst", 5, 4)),
    ("an item dst of -1", _table("dst", 1, -1)),
]


def _cases(rules):
    return [pytest.param(what, change, id=what.replace(" ", "_")) for what, change in rules]


def test_the_sweep_symbols_are_exported_and_bound():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("fwx_solve_sweep_f64", "fwx_solve_sweep_f32", "fwx_dev_solve_sweep"):
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.FWX_SWEEP_MAX_N == 128
    assert _lib.lib().fwx_abi_version() == 3           # symbols are only added


def test_the_valid_call_these_cases_start_from_passes_every_check():
    """Without a device the untouched call reaches the device check; with one it is simply a sweep."""
    c = Call(np.float64)
    assert c.host() in (OK, NO_DEVICE)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("what,change", _cases(SHARED_INVALID + HOST_ONLY_INVALID))
def test_host_form_rejects_before_any_device_call(dtype, what, change):
    c = Call(dtype)
    change(c)
    assert c.host() == INVALID, what
    assert c.untouched(), what


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("what,change", _cases(SHARED_INVALID + DEV_ONLY_INVALID))
def test_device_form_rejects_before_any_device_call(dtype, what, change):
    c = Call(dtype)
    change(c)
    assert c.dev() == INVALID, what
    assert c.untouched(), what


@pytest.mark.parametrize("dtype", DTYPES)
def test_orders_above_the_limit_and_other_engines_are_unsupported(dtype):
    c = Call(dtype, n=129)
    assert c.host() == UNSUPPORTED and c.dev() == UNSUPPORTED
    c.full.rate, c.full.stride = FAKE, 129 * 129
    assert c.dev() == UNSUPPORTED
    assert c.untouched()
    c = Call(dtype, n=128)                                 # the limit itself passes the checks
    assert c.host() in (OK, NO_DEVICE)
    for eng in (_lib.FWX_ENGINE_PERK, _lib.FWX_ENGINE_FUSED):
        c = Call(dtype)
        c.opts.engine = eng
        assert c.host() == UNSUPPORTED, eng
        assert c.untouched()


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_sweeps_are_success_and_touch_nothing(dtype):
    for count, n in ((0, 4), (3, 0), (0, 0), (0, 4096)):
        c = Call(dtype)
        c.count, c.n = count, n
        assert c.host() == OK, (count, n)
        assert c.dev() == OK, (count, n)
        assert c.untouched()
    c = Call(dtype)
    c.count, c.base = 0, [None, None, None]
    c.use_patches = c.use_items = c.use_full = False
    assert c.host() == OK and c.dev() == OK


@pytest.mark.parametrize("dtype", DTYPES)
def test_null_structs_and_empty_tables_pass_the_checks(dtype):
    """patches NULL, items NULL, full NULL and tables with total == 0 (whose pointers may be NULL) are valid calls:
    what they return is the device check's answer or success."""
    for change in (_set(None, "use_patches", False), _set(None, "use_items", False), _set(None, "use_full", False),
                   _chain(_set("p", "total", 0), _set("p", "ptr", None), _set("p", "index", None),
                          _set("p", "rate", None)),
                   _chain(_set("it", "total", 0), _set("it", "ptr", None), _set("it", "src", None),
                          _set("it", "dst", None), _set("it", "rate_out", None))):
        c = Call(dtype)
        change(c)
        assert c.host() in (OK, NO_DEVICE)


@pytest.mark.skipif(engine.device_count() > 0, reason="only meaningful without a GPU")
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_valid_call_without_a_device_reports_it_and_leaves_the_outputs_alone(dtype):
    c = Call(dtype)
    assert c.host() == NO_DEVICE
    assert c.dev() == NO_DEVICE
    c.full.rate = FAKE
    assert c.dev() == NO_DEVICE
    assert c.untouched()
    with pytest.raises(engine.FwxError) as e:
        engine.solve_sweep(c.rate, c.next, c.hops, patches=[(np.array([1]), np.array([2.0]))],
                           items=[(np.array([0]), np.array([3]))])
    assert e.value.status == NO_DEVICE


def test_python_binding_checks_shapes():
    rate = np.full((4, 4), 0.5)
    nxt = np.zeros((4, 4), dtype=np.int32)
    one = [(np.array([1]), np.array([2.0]))]
    with pytest.raises(ValueError):
        engine.solve_sweep(rate[0], patches=one, items=[None])             # not a matrix
    with pytest.raises(ValueError):
        engine.solve_sweep(rate, None, nxt, patches=one, items=[None])      # hops requires next
    with pytest.raises(ValueError):
        engine.solve_sweep(rate, patches=one, items=[None, None])           # one entry per variant
    with pytest.raises(ValueError):
        engine.solve_sweep(rate, patches=[(np.array([1, 2]), np.array([2.0]))], items=[None])
    with pytest.raises(ValueError):
        engine.solve_sweep(rate, patches=one + [(np.array([1]), np.array([2.0]), np.array([0]))], items=[None] * 2)
    with pytest.raises(ValueError):
        engine.solve_sweep(rate, patches=None, items=None)
    assert engine.solve_sweep(rate, patches=[], items=[]) == []            # no variants: success
