"""FWX_PERK_FOLD (the fold of relax_kt's non-counting f32 sweeps) is read on every call: `compare`, exactly, forces
the compare form in every tile; anything else, or unset, is automatic.  CPU only: the hook needs no device."""
import pytest

from floydwarshall_amd import _lib


def _parsed():
    return _lib.lib().fwx_test_perk_fold()


def test_unset_is_automatic(monkeypatch):
    monkeypatch.delenv("FWX_PERK_FOLD", raising=False)
    assert _parsed() == 0


def test_compare_is_taken(monkeypatch):
    monkeypatch.setenv("FWX_PERK_FOLD", "compare")
    assert _parsed() == 1


@pytest.mark.parametrize("value", ["", "auto", "max", "Compare", "COMPARE", "compare ", " compare", "compare1", "1", "0"])
def test_anything_else_is_automatic(value, monkeypatch):
    monkeypatch.setenv("FWX_PERK_FOLD", value)
    assert _parsed() == 0


def test_read_on_every_call(monkeypatch):
    for value, want in (("compare", 1), ("junk", 0), ("compare", 1), ("", 0)):
        monkeypatch.setenv("FWX_PERK_FOLD", value)
        assert _parsed() == want
