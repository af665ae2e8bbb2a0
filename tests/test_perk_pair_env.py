"""FWX_PERK_PAIR_MIN_N (the smallest order at which a call of the per-k engine that takes the tile sweep applies its full
blocks two at a time, the next pair's panels made beside the 128-pivot launch) is read on every call: digits only; `0`
means never; any other text, or unset, means the default.  CPU only: the hook needs no device."""
import ctypes

import pytest

from floydwarshall_amd import _lib

VAR = "FWX_PERK_PAIR_MIN_N"


def _parsed():
    return _lib.lib().fwx_test_perk_pair(None, 0)


def _default(monkeypatch):
    monkeypatch.delenv(VAR, raising=False)
    return _parsed()


def test_unset_is_the_default(monkeypatch):
    d = _default(monkeypatch)
    assert d == 0 or d >= 512         # never, or an order with four full blocks behind a tile boundary


def test_zero_is_never(monkeypatch):
    monkeypatch.setenv(VAR, "0")
    assert _parsed() == 0


@pytest.mark.parametrize("value,want", [("1", 1), ("128", 128), ("8192", 8192), ("16384", 16384), ("007", 7), ("00", 0),
                                        ("2147483647", 2147483647)])
def test_a_number_is_itself(value, want, monkeypatch):
    monkeypatch.setenv(VAR, value)
    assert _parsed() == want


@pytest.mark.parametrize("value", ["", " ", "-1", "+128", "-0", " 128", "128 ", "8k", "0x80", "1.28e2", "128.0", "off",
                                   "never", "2147483648", "99999999999999999999"])
def test_sign_blank_trailing_text_or_overflow_is_the_default(value, monkeypatch):
    d = _default(monkeypatch)
    monkeypatch.setenv(VAR, value)
    assert _parsed() == d


def test_read_on_every_call(monkeypatch):
    d = _default(monkeypatch)
    for value, want in (("0", 0), ("128", 128), ("junk", d), ("0", 0), ("4096", 4096)):
        monkeypatch.setenv(VAR, value)
        assert _parsed() == want
    monkeypatch.delenv(VAR)
    assert _parsed() == d


def test_the_counter_needs_no_device_and_resets():
    c = ctypes.c_uint64(7)
    _lib.lib().fwx_test_perk_pair(ctypes.byref(c), 1)
    _lib.lib().fwx_test_perk_pair(ctypes.byref(c), 0)
    assert c.value == 0


def test_it_leaves_the_other_knobs_alone(monkeypatch):
    """The pair schedule is a choice of schedule: the older switches keep their parse beside it, and it keeps its own
    beside theirs."""
    monkeypatch.setenv(VAR, "0")
    for v in ("FWX_PERK_TILE_MIN_N", "FWX_PERK_DEEP", "FWX_PERK_WIDE", "FWX_PERK_WALK", "FWX_PERK_FOLD", "FWX_PERK_PIVOTS"):
        monkeypatch.delenv(v, raising=False)
    L = _lib.lib()
    tile_default = L.fwx_test_perk_tile(None, 0)
    assert (L.fwx_test_perk_deep(None, 0), L.fwx_test_perk_wide(None, 0), L.fwx_test_perk_walk(), L.fwx_test_perk_fold(),
            L.fwx_test_perk_pivots(None, 0)) == (1, 1, 1, 0, 8)
    monkeypatch.setenv("FWX_PERK_TILE_MIN_N", "64")
    monkeypatch.setenv("FWX_PERK_DEEP", "0")
    monkeypatch.setenv("FWX_PERK_WIDE", "0")
    monkeypatch.setenv("FWX_PERK_WALK", "0")
    monkeypatch.setenv("FWX_PERK_FOLD", "compare")
    monkeypatch.setenv("FWX_PERK_PIVOTS", "4")
    monkeypatch.setenv(VAR, "512")
    assert (L.fwx_test_perk_tile(None, 0), L.fwx_test_perk_deep(None, 0), L.fwx_test_perk_wide(None, 0),
            L.fwx_test_perk_walk(), L.fwx_test_perk_fold(), L.fwx_test_perk_pivots(None, 0), _parsed()) == (
                64, 0, 0, 0, 1, 4, 512)
    monkeypatch.delenv("FWX_PERK_TILE_MIN_N")
    assert L.fwx_test_perk_tile(None, 0) == tile_default and _parsed() == 512
