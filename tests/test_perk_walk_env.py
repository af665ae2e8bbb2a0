"""FWX_PERK_WALK (which kernel sweeps the 16-pivot launches of the per-k engine: relax_walk, or round 19's relax_kt)
is read on every call: `0` gives the old kernel, anything else, or unset, relax_walk.  CPU only: the hook needs no
device."""
import pytest

from floydwarshall_amd import _lib


def _parsed():
    return _lib.lib().fwx_test_perk_walk()


def test_unset_is_on(monkeypatch):
    monkeypatch.delenv("FWX_PERK_WALK", raising=False)
    assert _parsed() == 1


def test_zero_is_off(monkeypatch):
    monkeypatch.setenv("FWX_PERK_WALK", "0")
    assert _parsed() == 0


@pytest.mark.parametrize("value", ["1", "32", "", "00", "0 ", " 0", "-0", "+0", "0.0", "0x0", "off", "no", "false",
                                   "junk", "8"])
def test_anything_else_is_on(value, monkeypatch):
    monkeypatch.setenv("FWX_PERK_WALK", value)
    assert _parsed() == 1


def test_read_on_every_call(monkeypatch):
    for value, want in (("0", 0), ("1", 1), ("0", 0), ("junk", 1), ("0", 0)):
        monkeypatch.setenv("FWX_PERK_WALK", value)
        assert _parsed() == want
    monkeypatch.delenv("FWX_PERK_WALK")
    assert _parsed() == 1


def test_it_leaves_the_other_knobs_alone(monkeypatch):
    """The walk is a choice of kernel: FWX_PERK_WIDE, FWX_PERK_FOLD and FWX_PERK_PIVOTS keep their parse beside it."""
    monkeypatch.setenv("FWX_PERK_WALK", "0")
    for v in ("FWX_PERK_WIDE", "FWX_PERK_FOLD", "FWX_PERK_PIVOTS"):
        monkeypatch.delenv(v, raising=False)
    L = _lib.lib()
    assert (L.fwx_test_perk_wide(None, 0), L.fwx_test_perk_fold(), L.fwx_test_perk_pivots(None, 0)) == (1, 0, 8)
    monkeypatch.setenv("FWX_PERK_WIDE", "0")
    monkeypatch.setenv("FWX_PERK_FOLD", "compare")
    monkeypatch.setenv("FWX_PERK_WALK", "1")
    assert (L.fwx_test_perk_wide(None, 0), L.fwx_test_perk_fold(), _parsed()) == (0, 1, 1)
