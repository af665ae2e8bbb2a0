"""FWX_PERK_PIVOTS (pivots per streaming pass of the per-k engine's rates-only whole-matrix solves) is read on
every call: 1, 2, 4 and 8 are taken, anything else is the default.  CPU only: the hook needs no device."""
import pytest

from floydwarshall_amd import _lib


def _parsed():
    return _lib.lib().fwx_test_perk_pivots(None, 0)


def _default(monkeypatch):
    monkeypatch.delenv("FWX_PERK_PIVOTS", raising=False)
    return _parsed()


def test_default_is_a_supported_width(monkeypatch):
    assert _default(monkeypatch) in (1, 2, 4, 8)


@pytest.mark.parametrize("value", ["1", "2", "4", "8", " 8", "+4"])     # (as strtol reads it: a leading blank or sign)
def test_supported_values_are_taken(value, monkeypatch):
    monkeypatch.setenv("FWX_PERK_PIVOTS", value)
    assert _parsed() == int(value)


@pytest.mark.parametrize("value", ["", "0", "8 ", "3", "5", "6", "7", "16", "64", "-2", "-4", "2.5", "4x", "x4", "0x8",
                                   "four", "8 8", "99999999999999999999", "nan"])
def test_anything_else_is_the_default(value, monkeypatch):
    default = _default(monkeypatch)
    monkeypatch.setenv("FWX_PERK_PIVOTS", value)
    assert _parsed() == default


def test_read_on_every_call(monkeypatch):
    default = _default(monkeypatch)
    for value in ("2", "junk", "8", "1"):
        monkeypatch.setenv("FWX_PERK_PIVOTS", value)
        assert _parsed() == (int(value) if value.isdigit() else default)
