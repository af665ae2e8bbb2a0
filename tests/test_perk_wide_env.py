"""FWX_PERK_WIDE (the 16-pivot pass of the per-k engine's multi-pivot schedule) is read on every call: `0` turns it
off, anything else, or unset, leaves it on.  CPU only: the hook needs no device."""
import ctypes

import pytest

from floydwarshall_amd import _lib


def _parsed():
    return _lib.lib().fwx_test_perk_wide(None, 0)


def test_unset_is_on(monkeypatch):
    monkeypatch.delenv("FWX_PERK_WIDE", raising=False)
    assert _parsed() == 1


def test_zero_is_off(monkeypatch):
    monkeypatch.setenv("FWX_PERK_WIDE", "0")
    assert _parsed() == 0


@pytest.mark.parametrize("value", ["1", "16", "", "00", "0 ", " 0", "-0", "0.0", "off", "no", "false", "junk", "8"])
def test_anything_else_is_on(value, monkeypatch):
    monkeypatch.setenv("FWX_PERK_WIDE", value)
    assert _parsed() == 1


def test_read_on_every_call(monkeypatch):
    for value, want in (("0", 0), ("1", 1), ("0", 0), ("junk", 1), ("0", 0)):
        monkeypatch.setenv("FWX_PERK_WIDE", value)
        assert _parsed() == want
    monkeypatch.delenv("FWX_PERK_WIDE")
    assert _parsed() == 1


def test_the_counter_reads_and_resets_without_a_device(monkeypatch):
    """No launch is made here, so whatever the counter holds, a reset empties it; FWX_PERK_PIVOTS keeps its parse."""
    c = ctypes.c_uint64(7)
    _lib.lib().fwx_test_perk_wide(ctypes.byref(c), 1)
    _lib.lib().fwx_test_perk_wide(ctypes.byref(c), 0)
    assert c.value == 0
    monkeypatch.setenv("FWX_PERK_PIVOTS", "16")
    monkeypatch.delenv("FWX_PERK_WIDE", raising=False)
    assert _lib.lib().fwx_test_perk_pivots(None, 0) == 8 and _parsed() == 1
