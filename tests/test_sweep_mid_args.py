"""What-if sweeps up to order 256 (fwx_solve_sweep_mid_f64 / _f32, fwx_dev_solve_sweep_mid): the symbols exist, every
status rule of fwx_solve_sweep_* / fwx_dev_solve_sweep holds word for word with the limit at 256, the scratch rules
apply exactly where a call is routed to the mid tier, and the slot count follows the rule of include/fwx.h.  All of it
is decided before any device call, with every output left as it was.

No launch is made here.  The host form is called with host arrays, which is its contract.  The device form is handed
host memory in place of device memory, so it is called unguarded only where the call returns before the device check
(FWX_ERR_INVALID, FWX_ERR_UNSUPPORTED, an empty sweep); a device-form call that passes every check is made only on a
machine without a device, where it ends at FWX_ERR_NO_DEVICE (Call.dev_valid, the tests marked NO_GPU)."""
import ctypes

import numpy as np
import pytest

from floydwarshall_amd import _lib, engine

import test_sweep_args as small
from test_sweep_args import (DEV_ONLY_INVALID, DTYPES, FAKE, HOST_ONLY_INVALID, INVALID, NO_DEVICE, OK, SHARED_INVALID,
                             UNSUPPORTED, _cases, _ptr)

HOST = {np.float64: "fwx_solve_sweep_mid_f64", np.float32: "fwx_solve_sweep_mid_f32"}
SENTINEL_BYTE = 0xA5
NO_GPU = pytest.mark.skipif(engine.device_count() > 0, reason="only meaningful without a GPU")


class Call(small.Call):
    """test_sweep_args.Call through the mid entry points; the device form is handed a sentinel-filled, 16-byte
    aligned scratch of `slots` slots (host memory stands in for device memory: see dev and dev_valid)."""

    def __init__(self, dtype, count=3, n=4, slots=2):
        super().__init__(dtype, count, n)
        self.slot = _lib.sweep_mid_scratch_bytes(n)
        self._raw = np.full(slots * self.slot + 32, SENTINEL_BYTE, dtype=np.uint8)
        self.scratch_off = (-self._raw.ctypes.data) % 16
        self.scratch = self._raw.ctypes.data + self.scratch_off
        self.scratch_bytes = slots * self.slot

    def host(self):
        p, it = self._structs()
        return getattr(_lib.lib(), HOST[self.dtype])(self.count, self.n, *self.base, p, it, _ptr(self.each),
                                                     ctypes.byref(self.opts))

    def dev(self):
        # host memory stands in for device memory: only for calls that return before the device check (an argument
        # error, an order above the limit, bad scratch, an empty sweep).  A call that passes every check is dev_valid()
        p, it = self._structs()
        return _lib.lib().fwx_dev_solve_sweep_mid(self.count, self.n, self.code, *self.base, p, it,
                                                  ctypes.byref(self.full) if self.use_full else None, _ptr(self.each),
                                                  self.scratch, self.scratch_bytes, None)

    def dev_valid(self):
        """dev() for a call that passes every check: with a device it would launch on these host arrays, so it is made
        only where there is none (the tests that use it are marked NO_GPU) and ends at FWX_ERR_NO_DEVICE."""
        assert engine.device_count() == 0, "a valid device-form call on host memory must not reach a device"
        return self.dev()

    def untouched(self):
        return super().untouched() and bool(np.all(self._raw == SENTINEL_BYTE))


def test_the_mid_sweep_symbols_and_the_hook_are_exported_and_bound():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("fwx_solve_sweep_mid_f64", "fwx_solve_sweep_mid_f32", "fwx_dev_solve_sweep_mid",
                 "fwx_test_sweep_mid_slots"):
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.FWX_SWEEP_MID_MAX_N == 256 and _lib.FWX_SWEEP_MAX_N == 128
    assert _lib.sweep_mid_scratch_bytes(256) == 1 << 20 and _lib.sweep_mid_scratch_bytes(129) == 129 * 129 * 16
    assert _lib.lib().fwx_abi_version() == 3           # symbols are only added
    assert callable(engine.solve_sweep_mid) and callable(engine.dev_solve_sweep_mid)


@pytest.mark.parametrize("min_n", [None, "1"], ids=["default_routing", "mid_from_1"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("what,change", _cases(SHARED_INVALID + HOST_ONLY_INVALID))
def test_host_form_rejects_before_any_device_call(dtype, what, change, min_n, monkeypatch):
    if min_n:
        monkeypatch.setenv("FWX_BATCH_MID_MIN_N", min_n)
    c = Call(dtype)
    change(c)
    assert c.host() == INVALID, what
    assert c.untouched(), what


@pytest.mark.parametrize("min_n", [None, "1"], ids=["default_routing", "mid_from_1"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("what,change", _cases(SHARED_INVALID + DEV_ONLY_INVALID))
def test_device_form_rejects_before_any_device_call(dtype, what, change, min_n, monkeypatch):
    if min_n:
        monkeypatch.setenv("FWX_BATCH_MID_MIN_N", min_n)
    c = Call(dtype)
    change(c)
    assert c.dev() == INVALID, what
    assert c.untouched(), what


@pytest.mark.parametrize("dtype", DTYPES)
def test_orders_above_256_and_other_engines_are_unsupported(dtype):
    c = Call(dtype, n=257, slots=1)
    assert c.host() == UNSUPPORTED and c.dev() == UNSUPPORTED
    c.full.rate, c.full.stride = FAKE, 257 * 257
    assert c.dev() == UNSUPPORTED
    c.scratch = None                                      # the order is judged before the scratch
    assert c.dev() == UNSUPPORTED
    assert c.untouched()
    for n in (129, 256):                                  # what the small entry points refuse passes the checks here
        c = Call(dtype, n=n, slots=1)
        assert c.host() in (OK, NO_DEVICE), n
        s = small.Call(dtype, n=n)
        assert s.host() == UNSUPPORTED and s.dev() == UNSUPPORTED, n
    for eng in (_lib.FWX_ENGINE_PERK, _lib.FWX_ENGINE_FUSED):
        c = Call(dtype)
        c.opts.engine = eng
        assert c.host() == UNSUPPORTED, eng
        assert c.untouched()


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_argument_error_wins_over_the_order_and_the_order_over_the_scratch(dtype):
    c = Call(dtype, n=257, slots=1)
    c.base[0] = None
    assert c.host() == INVALID and c.dev() == INVALID
    c = Call(dtype, n=200, slots=1)
    c.scratch, c.p.total = None, -1
    assert c.dev() == INVALID
    assert c.untouched()


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_sweeps_are_success_and_touch_nothing_whatever_the_scratch(dtype, monkeypatch):
    for min_n in (None, "1"):
        if min_n:
            monkeypatch.setenv("FWX_BATCH_MID_MIN_N", min_n)
        for count, n in ((0, 4), (3, 0), (0, 0), (0, 4096), (0, 200)):
            c = Call(dtype)
            c.count, c.n = count, n
            assert c.host() == OK, (count, n)
            assert c.dev() == OK, (count, n)
            c.scratch, c.scratch_bytes = None, 0
            assert c.dev() == OK, (count, n)
            assert c.untouched()


def _bad_scratches(c):
    """(what, scratch, scratch_bytes) for the three rules, from a call whose scratch is valid."""
    return [("NULL", None, c.scratch_bytes), ("misaligned", c.scratch + 8, c.slot),
            ("misaligned by 4", c.scratch + 4, c.slot), ("one byte short of a slot", c.scratch, c.slot - 1),
            ("no bytes", c.scratch, 0)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [129, 200, 256])
def test_scratch_rules_hold_where_the_order_is_routed_to_the_mid_tier(n, dtype):
    c = Call(dtype, n=n, slots=2)
    for what, ptr, nbytes in _bad_scratches(c):
        c.scratch, c.scratch_bytes = ptr, nbytes
        assert c.dev() == INVALID, what
        assert c.untouched(), what


@pytest.mark.parametrize("dtype", DTYPES)
def test_scratch_rules_hold_for_small_orders_under_the_routing_variable(dtype, monkeypatch):
    """Under FWX_BATCH_MID_MIN_N=1 every order is the mid tier's and the rules hold; at 65 they hold from 65 up."""
    monkeypatch.setenv("FWX_BATCH_MID_MIN_N", "1")
    for n in (1, 4, 64, 128):
        c = Call(dtype, n=n, slots=1)
        for what, ptr, nbytes in _bad_scratches(c):
            c.scratch, c.scratch_bytes = ptr, nbytes
            assert c.dev() == INVALID, (n, what)
            assert c.untouched(), (n, what)
    monkeypatch.setenv("FWX_BATCH_MID_MIN_N", "65")
    c = Call(dtype, n=65, slots=1)
    c.scratch = None
    assert c.dev() == INVALID
    assert c.untouched()


# ---- valid device-form calls: only without a device, where they stop at FWX_ERR_NO_DEVICE --------------------------
@NO_GPU
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [129, 200, 256])
def test_a_scratch_of_one_slot_or_more_passes_the_scratch_rules(n, dtype):
    c = Call(dtype, n=n, slots=2)
    assert c.dev_valid() == NO_DEVICE
    c.scratch_bytes = c.slot                              # exactly one slot is enough
    assert c.dev_valid() == NO_DEVICE
    assert c.untouched()


@NO_GPU
@pytest.mark.parametrize("dtype", DTYPES)
def test_forwarded_orders_ignore_the_scratch(dtype, monkeypatch):
    """n = 64 at the default is forwarded to the small tiers, which need no scratch: NULL, misaligned and short scratch
    all pass the checks.  Under FWX_BATCH_MID_MIN_N=1 a good scratch passes at the same orders (the bad ones are
    refused: test_scratch_rules_hold_for_small_orders_under_the_routing_variable)."""
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    for n in (4, 64, 128):
        c = Call(dtype, n=n, slots=1)
        for what, ptr, nbytes in _bad_scratches(c):
            c.scratch, c.scratch_bytes = ptr, nbytes
            assert c.dev_valid() == NO_DEVICE, (n, what)
    monkeypatch.setenv("FWX_BATCH_MID_MIN_N", "1")
    for n in (1, 4, 64, 128):
        c = Call(dtype, n=n, slots=1)
        assert c.dev_valid() == NO_DEVICE, n
    monkeypatch.setenv("FWX_BATCH_MID_MIN_N", "65")
    c = Call(dtype, n=64, slots=1)
    c.scratch = None
    assert c.dev_valid() == NO_DEVICE


def test_slot_count_follows_the_rule(monkeypatch):
    slots = _lib.lib().fwx_test_sweep_mid_slots
    per = _lib.sweep_mid_scratch_bytes

    def rule(count, n, nbytes, cap):
        return min(count, nbytes // per(n), cap)

    cases = [(1, 130, per(130)), (7, 130, per(130)), (7, 130, 2 * per(130)), (7, 130, 3 * per(130) + 5),
             (7, 130, 3 * per(130) - 1), (5, 130, 8 * per(130)), (600, 20, 600 * per(20)), (4096, 256, 256 << 20),
             (4096, 129, 256 << 20), (10 ** 6, 1, 10 ** 9), (3, 200, per(200) - 1), (3, 200, 0)]
    monkeypatch.delenv("FWX_SWEEP_MID_SLOTS", raising=False)
    for count, n, nbytes in cases:
        assert slots(count, n, nbytes) == rule(count, n, nbytes, 512), (count, n, nbytes)
    assert slots(600, 20, 600 * per(20)) == 512 and slots(4096, 256, 256 << 20) == 256
    for text, cap in (("1", 1), ("2", 2), ("3", 3), ("8", 8), ("512", 512), ("513", 513), ("100000", 100000),
                      ("007", 7)):
        monkeypatch.setenv("FWX_SWEEP_MID_SLOTS", text)
        for count, n, nbytes in cases:
            assert slots(count, n, nbytes) == rule(count, n, nbytes, cap), (text, count, n, nbytes)
    for garbage in ("", "0", "-3", "+4", "4x", "x4", " 4", "4 ", "1e3", "0x10", "99999999999999999999"):
        monkeypatch.setenv("FWX_SWEEP_MID_SLOTS", garbage)
        for count, n, nbytes in cases:
            assert slots(count, n, nbytes) == rule(count, n, nbytes, 512), (garbage, count, n, nbytes)
    # the rule does not look at the routing; nothing to launch is 0; what no call accepts is a status
    monkeypatch.delenv("FWX_SWEEP_MID_SLOTS", raising=False)
    assert slots(0, 130, per(130)) == 0 and slots(5, 0, 1 << 20) == 0
    assert slots(-1, 130, per(130)) == INVALID and slots(5, -1, 1 << 20) == INVALID
    assert slots(5, 257, 1 << 30) == UNSUPPORTED and slots(5, 256, 1 << 30) == 5


def _null_struct_changes():
    from test_sweep_args import _chain, _set
    return (_set(None, "use_patches", False), _set(None, "use_items", False), _set(None, "use_full", False),
            _chain(_set("p", "total", 0), _set("p", "ptr", None), _set("p", "index", None), _set("p", "rate", None)),
            _chain(_set("it", "total", 0), _set("it", "ptr", None), _set("it", "src", None), _set("it", "dst", None),
                   _set("it", "rate_out", None)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_null_structs_and_empty_tables_pass_the_checks_of_the_host_form(dtype):
    for n in (4, 130):
        for change in _null_struct_changes():
            c = Call(dtype, n=n, slots=1)
            change(c)
            assert c.host() in (OK, NO_DEVICE)


@NO_GPU
@pytest.mark.parametrize("dtype", DTYPES)
def test_null_structs_and_empty_tables_pass_the_checks_of_the_device_form(dtype):
    for n in (4, 130):
        for change in _null_struct_changes():
            c = Call(dtype, n=n, slots=1)
            change(c)
            assert c.dev_valid() == NO_DEVICE
            assert c.untouched()


@NO_GPU
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [4, 129, 130, 256])
def test_a_valid_call_without_a_device_reports_it_and_leaves_the_outputs_alone(n, dtype):
    c = Call(dtype, n=n, slots=1)
    assert c.host() == NO_DEVICE
    assert c.dev_valid() == NO_DEVICE
    c.full.rate = FAKE
    assert c.dev_valid() == NO_DEVICE
    assert c.untouched()
    with pytest.raises(engine.FwxError) as e:
        engine.solve_sweep_mid(c.rate, c.next, c.hops, patches=[(np.array([1]), np.array([2.0]))],
                               items=[(np.array([0]), np.array([3]))])
    assert e.value.status == NO_DEVICE


def test_python_binding_checks_shapes_like_the_small_form():
    rate = np.full((4, 4), 0.5)
    nxt = np.zeros((4, 4), dtype=np.int32)
    one = [(np.array([1]), np.array([2.0]))]
    with pytest.raises(ValueError):
        engine.solve_sweep_mid(rate[0], patches=one, items=[None])
    with pytest.raises(ValueError):
        engine.solve_sweep_mid(rate, None, nxt, patches=one, items=[None])
    with pytest.raises(ValueError):
        engine.solve_sweep_mid(rate, patches=one, items=[None, None])
    with pytest.raises(ValueError):
        engine.solve_sweep_mid(rate, patches=None, items=None)
    assert engine.solve_sweep_mid(rate, patches=[], items=[]) == []
