"""The per-k engine takes ONE reading of its ten environment variables per call (PerkKnobs, csrc/fwx_perk.hip), and the
test hooks answer from the same reading: with all ten set at once every hook returns its own variable's value, with all
ten set to junk every hook returns its default.  (FWX_PERK_STORE_BYTES and FWX_PERK_TEMPORAL_MIB have no hook; they are
set all the same, so that a reading that mixed the variables up would show in the others.)

The launch counters are one tally behind all the hooks; a hook's reset clears the counters that hook reports and no
other.  The CPU test pins that on whatever the process has counted (nothing, without a device); the GPU test first runs
one small solve through the group schedule, so that every kind of counter holds a number."""
import ctypes

import numpy as np
import pytest

from floydwarshall_amd import _lib

LEGAL = {"FWX_PERK_PIVOTS": "2", "FWX_PERK_WIDE": "0", "FWX_PERK_WALK": "0", "FWX_PERK_DEEP": "0",
         "FWX_PERK_FOLD": "compare", "FWX_PERK_TILE_MIN_N": "192", "FWX_PERK_PAIR_MIN_N": "384",
         "FWX_PERK_GROUP_MAX": "6", "FWX_PERK_STORE_BYTES": "32", "FWX_PERK_TEMPORAL_MIB": "1.5"}
JUNK = {"FWX_PERK_PIVOTS": "8 ", "FWX_PERK_WIDE": "00", "FWX_PERK_WALK": "off", "FWX_PERK_DEEP": " 0",
        "FWX_PERK_FOLD": "Compare", "FWX_PERK_TILE_MIN_N": "+1", "FWX_PERK_PAIR_MIN_N": "1k",
        "FWX_PERK_GROUP_MAX": "9", "FWX_PERK_STORE_BYTES": "48", "FWX_PERK_TEMPORAL_MIB": "x"}
# hook -> how many counters it reports (0: it takes no arguments)
HOOKS = {"pivots": 5, "wide": 1, "fold": 0, "walk": 0, "deep": 1, "tile": 1, "pair": 1, "group": 4}


def _answers():
    """What every hook returns right now, and the group sizes a call of 16 full blocks would take at n = 16384."""
    L = _lib.lib()
    out = {h: getattr(L, "fwx_test_perk_" + h)(*((None, 0) if k else ())) for h, k in HOOKS.items()}
    size = (ctypes.c_int * 16)()
    count = L.fwx_test_perk_group_plan(16384, 16, 0, size, None, 16)
    out["plan"] = list(size[:count])
    return out


def _counters(hook, reset=0):
    c = (ctypes.c_uint64 * HOOKS[hook])()
    getattr(_lib.lib(), "fwx_test_perk_" + hook)(c, reset)
    return [int(v) for v in c]


def _tally():
    return {h: _counters(h) for h, k in HOOKS.items() if k}


def test_every_hook_answers_from_one_reading(monkeypatch):
    assert set(LEGAL) == set(JUNK) and len(LEGAL) == 10
    for v in LEGAL:
        monkeypatch.delenv(v, raising=False)
    default = _answers()
    assert (default["wide"], default["walk"], default["deep"], default["fold"], default["group"]) == (1, 1, 1, 0, 0)
    assert default["pivots"] in (1, 2, 4, 8) and default["tile"] >= 0 and default["pair"] >= 0
    assert default["plan"] == [2, 4, 8, 2]             # (the default at n = 16384: eight blocks)
    for v, text in LEGAL.items():
        monkeypatch.setenv(v, text)
    assert _answers() == {"pivots": 2, "wide": 0, "fold": 1, "walk": 0, "deep": 0, "tile": 192, "pair": 384, "group": 6,
                          "plan": [2, 4, 6, 4]}
    for v, text in JUNK.items():
        monkeypatch.setenv(v, text)
    assert _answers() == default
    # and one at a time: each variable moves its own hook's answer and no other's
    moved = {"FWX_PERK_PIVOTS": ("pivots",), "FWX_PERK_WIDE": ("wide",), "FWX_PERK_WALK": ("walk",),
             "FWX_PERK_DEEP": ("deep",), "FWX_PERK_FOLD": ("fold",), "FWX_PERK_TILE_MIN_N": ("tile",),
             "FWX_PERK_PAIR_MIN_N": ("pair",), "FWX_PERK_GROUP_MAX": ("group", "plan"), "FWX_PERK_STORE_BYTES": (),
             "FWX_PERK_TEMPORAL_MIB": ()}
    for v, text in LEGAL.items():
        monkeypatch.setenv(v, text)
        got = _answers()
        assert {h for h in got if got[h] != default[h]} == set(moved[v]), v
        monkeypatch.setenv(v, JUNK[v])


def _check_resets_are_separate():
    """Hook by hook: reset returns what was counted, clears that hook's counters and leaves every other hook's."""
    for hook in (h for h, k in HOOKS.items() if k):
        before = _tally()
        assert _counters(hook, reset=1) == before[hook], hook
        want = dict(before)
        want[hook] = [0] * HOOKS[hook]
        assert _tally() == want, hook


def test_a_reset_clears_its_own_counters_only():
    _check_resets_are_separate()
    assert all(not any(c) for c in _tally().values())


@pytest.mark.gpu
def test_a_reset_clears_its_own_counters_only_after_launches(monkeypatch):
    """n = 1024, pivots [0, 967) in one call under FWX_PERK_GROUP_MAX=8: main launches of 2, 4 and 8 blocks, an odd last
    block and a 7-pivot tail (a 4-, a 2- and a single-pivot launch), so every counter but the 6-block one moves."""
    from floydwarshall_amd import engine, synth
    from helpers import dev, host

    for v in LEGAL:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("FWX_PERK_TILE_MIN_N", "1")
    monkeypatch.setenv("FWX_PERK_PAIR_MIN_N", "1")
    monkeypatch.setenv("FWX_PERK_GROUP_MAX", "8")
    for hook in (h for h, k in HOOKS.items() if k):
        _counters(hook, reset=1)
    n = 1024
    r_t = dev(synth.make("d1", n, np.float32, seed=33)[0])
    engine.dev_relax(r_t, n, 0, 0, n - 57)
    host(r_t)                                          # (waits for the launches)
    t = _tally()
    assert t["group"][0] > 0 and t["group"][1] > 0 and t["group"][3] > 0
    assert all(t["pivots"]) and t["wide"][0] and t["deep"][0] and t["tile"][0] and t["pair"][0]
    _check_resets_are_separate()
