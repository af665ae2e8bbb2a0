"""FWX_PERK_DEEP (whether the ladder of the per-k engine's multi-pivot schedule starts at 32 pivots per streaming pass
where it used to start at 16) is read on every call: `0` gives the schedule before the 32-pivot sweep, anything else,
or unset, the deep pass.  CPU only: the hook needs no device."""
import ctypes

import pytest

from floydwarshall_amd import _lib


def _parsed():
    return _lib.lib().fwx_test_perk_deep(None, 0)


def test_unset_is_on(monkeypatch):
    monkeypatch.delenv("FWX_PERK_DEEP", raising=False)
    assert _parsed() == 1


def test_zero_is_off(monkeypatch):
    monkeypatch.setenv("FWX_PERK_DEEP", "0")
    assert _parsed() == 0


@pytest.mark.parametrize("value", ["1", "32", "16", "", "00", "0 ", " 0", "-0", "+0", "0.0", "0x0", "off", "no", "false",
                                   "junk", "8"])
def test_anything_else_is_on(value, monkeypatch):
    monkeypatch.setenv("FWX_PERK_DEEP", value)
    assert _parsed() == 1


def test_read_on_every_call(monkeypatch):
    for value, want in (("0", 0), ("1", 1), ("0", 0), ("junk", 1), ("0", 0)):
        monkeypatch.setenv("FWX_PERK_DEEP", value)
        assert _parsed() == want
    monkeypatch.delenv("FWX_PERK_DEEP")
    assert _parsed() == 1


def test_the_counter_needs_no_device_and_resets():
    c = ctypes.c_uint64(7)
    _lib.lib().fwx_test_perk_deep(ctypes.byref(c), 1)
    _lib.lib().fwx_test_perk_deep(ctypes.byref(c), 0)
    assert c.value == 0


def test_it_leaves_the_other_knobs_alone(monkeypatch):
    """The deep pass is a choice of schedule: FWX_PERK_WIDE, FWX_PERK_WALK, FWX_PERK_FOLD and FWX_PERK_PIVOTS keep
    their parse beside it, and it keeps its own beside theirs."""
    monkeypatch.setenv("FWX_PERK_DEEP", "0")
    for v in ("FWX_PERK_WIDE", "FWX_PERK_WALK", "FWX_PERK_FOLD", "FWX_PERK_PIVOTS"):
        monkeypatch.delenv(v, raising=False)
    L = _lib.lib()
    assert (L.fwx_test_perk_wide(None, 0), L.fwx_test_perk_walk(), L.fwx_test_perk_fold(),
            L.fwx_test_perk_pivots(None, 0)) == (1, 1, 0, 8)
    monkeypatch.setenv("FWX_PERK_WIDE", "0")
    monkeypatch.setenv("FWX_PERK_WALK", "0")
    monkeypatch.setenv("FWX_PERK_FOLD", "compare")
    monkeypatch.setenv("FWX_PERK_PIVOTS", "4")
    monkeypatch.setenv("FWX_PERK_DEEP", "1")
    assert (L.fwx_test_perk_wide(None, 0), L.fwx_test_perk_walk(), L.fwx_test_perk_fold(),
            L.fwx_test_perk_pivots(None, 0), _parsed()) == (0, 0, 1, 4, 1)
