"""FWX_PERK_GROUP_MAX (the most blocks a main launch of the per-k engine's group schedule applies) is read on every
call: digits only, 2 to 8, an odd value counting as the even one below it; any other text, or unset, means the default
(the hook answers 0: the group size then goes by the order of the matrix).  The group sizes of a call are a pure
function of its number of full blocks and that maximum: 2, then doubling up to the maximum, whatever even number is left
at the end, a single odd block last; group g keeps its panels in half g & 1 of the panel sets, `max` sets per half, so
no group wraps.  CPU only: the hooks need no device."""
import ctypes

import pytest

from floydwarshall_amd import _lib

VAR = "FWX_PERK_GROUP_MAX"


def _parsed():
    return _lib.lib().fwx_test_perk_group(None, 0)


def _plan(nfull, gmax, n=16384, cap=64):
    size, sets = (ctypes.c_int * cap)(), (ctypes.c_int * cap)()
    count = _lib.lib().fwx_test_perk_group_plan(n, nfull, gmax, size, sets, cap)
    assert 0 <= count <= cap
    return list(size[:count]), list(sets[:count])


def test_unset_is_the_default(monkeypatch):
    monkeypatch.delenv(VAR, raising=False)
    assert _parsed() == 0


@pytest.mark.parametrize("value,want", [("2", 2), ("3", 2), ("4", 4), ("5", 4), ("6", 6), ("7", 6), ("8", 8), ("08", 8),
                                        ("004", 4)])
def test_a_number_in_bounds_is_the_even_number_at_or_below_it(value, want, monkeypatch):
    monkeypatch.setenv(VAR, value)
    assert _parsed() == want


@pytest.mark.parametrize("value", ["", " ", "0", "1", "9", "16", "64", "-2", "+4", " 4", "4 ", "4k", "0x8", "8.0", "max",
                                   "2147483648", "99999999999999999999"])
def test_out_of_bounds_or_junk_is_the_default(value, monkeypatch):
    monkeypatch.setenv(VAR, value)
    assert _parsed() == 0


def test_read_on_every_call(monkeypatch):
    for value, want in (("2", 2), ("8", 8), ("junk", 0), ("4", 4)):
        monkeypatch.setenv(VAR, value)
        assert _parsed() == want
    monkeypatch.delenv(VAR)
    assert _parsed() == 0


def test_the_counters_need_no_device_and_reset():
    c = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    _lib.lib().fwx_test_perk_group(c, 1)
    _lib.lib().fwx_test_perk_group(c, 0)
    assert list(c) == [0, 0, 0, 0]


def test_it_leaves_the_pair_threshold_alone(monkeypatch):
    L = _lib.lib()
    monkeypatch.setenv("FWX_PERK_PAIR_MIN_N", "0")
    monkeypatch.setenv(VAR, "8")
    assert (L.fwx_test_perk_pair(None, 0), _parsed()) == (0, 8)
    monkeypatch.setenv("FWX_PERK_PAIR_MIN_N", "512")
    monkeypatch.setenv(VAR, "2")
    assert (L.fwx_test_perk_pair(None, 0), _parsed()) == (512, 2)


# (full blocks, max) -> the sizes, in order
TABLE = {
    (0, 8): [], (1, 8): [1], (2, 8): [2], (3, 8): [2, 1], (4, 8): [2, 2], (5, 8): [2, 2, 1], (6, 8): [2, 4],
    (7, 8): [2, 4, 1], (8, 8): [2, 4, 2], (10, 8): [2, 4, 4], (12, 8): [2, 4, 6], (13, 8): [2, 4, 6, 1],
    (14, 8): [2, 4, 8], (15, 8): [2, 4, 8, 1], (16, 8): [2, 4, 8, 2], (17, 8): [2, 4, 8, 2, 1], (18, 8): [2, 4, 8, 4],
    (22, 8): [2, 4, 8, 8], (32, 8): [2, 4, 8, 8, 8, 2], (256, 8): [2, 4] + [8] * 31 + [2],
    (16, 4): [2, 4, 4, 4, 2], (15, 4): [2, 4, 4, 4, 1], (8, 4): [2, 4, 2], (16, 6): [2, 4, 6, 4],
    (16, 2): [2] * 8, (9, 2): [2, 2, 2, 2, 1],
}


@pytest.mark.parametrize("nfull,gmax", list(TABLE))
def test_the_group_sizes(nfull, gmax, monkeypatch):
    monkeypatch.delenv(VAR, raising=False)
    size, sets = _plan(nfull, gmax)
    assert size == TABLE[(nfull, gmax)]
    assert sum(size) == nfull
    for g, (sz, at) in enumerate(zip(size, sets)):
        assert sz <= gmax and (sz % 2 == 0 or (sz == 1 and g == len(size) - 1))
        assert sz <= 2 * (size[g - 1] if g else 1)                     # the chain beside the launch before is short enough
        half = g & 1
        assert half * gmax <= at and at + sz <= (half + 1) * gmax      # inside its half of the 2 * gmax sets: no wrap


def test_every_count_up_to_300_blocks(monkeypatch):
    monkeypatch.delenv(VAR, raising=False)
    for gmax in (2, 4, 6, 8):
        for nfull in range(300):
            size, sets = _plan(nfull, gmax, cap=200)
            assert sum(size) == nfull and all(s <= gmax for s in size)
            assert all(s % 2 == 0 for s in size[:-1]) and size[:1] in ([], [1], [2])
            assert all(at == (g & 1) * gmax for g, at in enumerate(sets))


def test_max_zero_is_what_a_call_would_take(monkeypatch):
    """0 stands for the call's own choice: the variable if it is set, else the default for the order -- which is a pair
    below every order the larger groups were measured to pay at, and never more than 8."""
    monkeypatch.setenv(VAR, "4")
    assert _plan(16, 0)[0] == TABLE[(16, 4)]
    monkeypatch.setenv(VAR, "2")
    assert _plan(16, 0)[0] == TABLE[(16, 2)]
    monkeypatch.delenv(VAR)
    assert _plan(16, 0, n=1024)[0] == TABLE[(16, 2)]
    assert max(_plan(64, 0, n=1 << 20)[0]) <= 8


def test_arguments_out_of_range():
    L = _lib.lib()
    for nfull, gmax, cap in ((-1, 8, 4), (4, 1, 4), (4, 3, 4), (4, 10, 4), (4, 8, -1)):
        assert L.fwx_test_perk_group_plan(1024, nfull, gmax, None, None, cap) == -1
    assert L.fwx_test_perk_group_plan(1024, 16, 8, None, None, 0) == 4
