"""The group schedule of the per-k engine (round 30, FWX_PERK_GROUP_MAX): a call that takes the pair schedule applies its
full blocks in groups that grow inside the call -- 2, 4, 8 blocks per main launch -- while a chain on the look-ahead
stream takes the band of the next group (its tile rows and tile columns) through the group being applied, then through
every block of its own group, panels first.  A main launch steps over the band that its chain has finished and over the
band that the chain beside it is working on.  It must end at the bits of the sequential fold for every input.

Every case sets FWX_PERK_PAIR_MIN_N=1, FWX_PERK_TILE_MIN_N=1 and FWX_PERK_GROUP_MAX itself (nothing depends on the
shipped defaults), compares the rates bit for bit with the C oracle and with the same call under FWX_PERK_GROUP_MAX=2,
and reads the hooks: the main launches by group size (fwx_test_perk_group) are exactly what the shape names, and the
five older counters read what they read under FWX_PERK_GROUP_MAX=2.

Shapes.  n = 1024, one call: groups 2, 4, 8, 2 -- bands 1, 2, 4 and 1 tile rows wide, the last at the matrix edge, both
halves of the panel sets.  n = 1152 and 1092: the last tile row and column are ragged (0 and 68 entries past a multiple
of 128: 1152 = 9 x 128 has 18 blocks, groups 2, 4, 8, 4; 1092 has 17 blocks and 4 ragged pivots, groups 2, 4, 8, 2, 1).
Two calls of 512 pivots: 2, 4, 2 each.  k_begin = 64: a leading block, then 2, 4, 8 from pivot 128.
k_end = 1024 - 40: 2, 4, 8, an odd last block and 24 ragged pivots.  FWX_PERK_GROUP_MAX=4: 2, 4, 4, 4, 2.
n = 8192, two calls of 1024 pivots, against the serial schedule on the device: main launches of several rounds of
workgroups, which run beside all of the chain (the only shape here at which a main launch that strays into the chain's
band, or reads the panel half the chain is filling, shows).
"""
import ctypes

import numpy as np
import pytest

from floydwarshall_amd import _lib, engine, hip, synth

from helpers import assert_bits_equal, dev, host, perk_launches, perk_oracle
from test_gpu_perk_deep import _deep
from test_gpu_perk_pair import _pair
from test_gpu_perk_tile import _tile
from test_gpu_perk_wide import _reset, _want, _wide

pytestmark = pytest.mark.gpu

F32 = np.float32
KNOBS = ("FWX_PERK_PIVOTS", "FWX_PERK_WIDE", "FWX_PERK_WALK", "FWX_PERK_DEEP", "FWX_PERK_FOLD", "FWX_PERK_STORE_BYTES",
         "FWX_PERK_TEMPORAL_MIB", "FWX_PERK_TILE_MIN_N", "FWX_PERK_PAIR_MIN_N", "FWX_PERK_GROUP_MAX")
# (n, [(k_begin, k_end) of each call], FWX_PERK_GROUP_MAX) -> main launches of 2, 4, 6 and 8 blocks, all calls together
SHAPES = {
    "whole 1024": (1024, [(0, 1024)], "8", [2, 1, 0, 1]),
    "ragged tile 1152": (1152, [(0, 1152)], "8", [1, 2, 0, 1]),
    "ragged tile 1092": (1092, [(0, 1092)], "8", [2, 1, 0, 1]),
    "two calls of 512": (1024, [(0, 512), (512, 1024)], "8", [4, 2, 0, 0]),
    "leading block": (1024, [(64, 1024)], "8", [1, 1, 0, 1]),
    "odd block and ragged tail": (1024, [(0, 1024 - 40)], "8", [1, 1, 0, 1]),
    "max 4": (1024, [(0, 1024)], "4", [2, 3, 0, 0]),
}
KINDS = ["d1", "t3", "t4"]


def _group(reset=True):
    """(what FWX_PERK_GROUP_MAX parses to, main launches of 2, 4, 6 and 8 blocks since the last reset)."""
    c = (ctypes.c_uint64 * 4)()
    g = _lib.lib().fwx_test_perk_group(c, 1 if reset else 0)
    return g, [int(v) for v in c]


def _defaults(monkeypatch, gmax):
    for v in KNOBS:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("FWX_PERK_TILE_MIN_N", "1")
    monkeypatch.setenv("FWX_PERK_PAIR_MIN_N", "1")
    monkeypatch.setenv("FWX_PERK_GROUP_MAX", gmax)


def _reset_all():
    _reset()
    _deep()
    _tile()
    _pair()
    _group()


def _older_hooks():
    return perk_launches(), _wide()[1], _deep()[1], _tile()[1], _pair()[1]


def _run(rate, calls, stream=None):
    """(rates, the five older hooks, main launches by group size) of the uncounted calls, one behind the other."""
    n = rate.shape[0]
    _reset_all()
    r_t = dev(rate)
    for kb, ke in calls:
        engine.dev_relax(r_t, n, 0, kb, ke, stream=stream)
    return host(r_t), _older_hooks(), _group()[1]


def _matrix(kind, n):
    return synth.make(kind, n, F32, seed=n + 30)[0]


def _oracle(key, rate, calls):
    """The oracle over the whole pivot range of the calls (they are contiguous): once per (input, range)."""
    return _want(("group",) + key, rate, calls[0][0], calls[-1][1])[0]


def _check(monkeypatch, rate, calls, gmax, by_size, want, tag):
    _defaults(monkeypatch, gmax)
    assert _group(reset=False)[0] == int(gmax)
    got, older, groups = _run(rate, calls)
    assert_bits_equal(got, want, tag)
    assert groups == by_size, tag
    monkeypatch.setenv("FWX_PERK_GROUP_MAX", "2")
    got2, older2, groups2 = _run(rate, calls)
    assert_bits_equal(got2, want, tag + " at FWX_PERK_GROUP_MAX=2")
    assert older == older2, tag
    assert groups2 == [sum((i + 1) * c for i, c in enumerate(by_size)), 0, 0, 0], tag
    return got


def test_the_shapes_are_what_the_rule_gives():
    """The table above against the rule itself (fwx_test_perk_group_plan), call by call."""
    L = _lib.lib()
    for tag, (n, calls, gmax, by_size) in SHAPES.items():
        want = [0, 0, 0, 0]
        for kb, ke in calls:
            assert kb % 64 == 0
            ka = (kb + 127) // 128 * 128
            size = (ctypes.c_int * 16)()
            count = L.fwx_test_perk_group_plan(n, (ke - ka) // 64, int(gmax), size, None, 16)
            for sz in size[:count]:
                if sz >= 2:
                    want[sz // 2 - 1] += 1
        assert want == by_size, tag
    size, sets = (ctypes.c_int * 16)(), (ctypes.c_int * 16)()
    assert L.fwx_test_perk_group_plan(1024, 16, 8, size, sets, 16) == 4
    assert list(size[:4]) == [2, 4, 8, 2] and list(sets[:4]) == [0, 8, 0, 8]      # both halves of the sets
    assert (1152 % 128, 1092 % 128, 1092 // 64, 1092 % 64) == (0, 68, 17, 4)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_group_shapes(shape, kind, monkeypatch):
    n, calls, gmax, by_size = SHAPES[shape]
    rate = _matrix(kind, n)
    want = _oracle((kind, n), rate, calls)
    _check(monkeypatch, rate, calls, gmax, by_size, want, "%s %s" % (shape, kind))


@pytest.mark.parametrize("shape", ["whole 1024", "ragged tile 1092"])
def test_compare_fold(shape, monkeypatch):
    """FWX_PERK_FOLD=compare: every tile folds in the compare form from its first stage, through all 32 stages."""
    n, calls, gmax, by_size = SHAPES[shape]
    rate = _matrix("t3", n)
    want = _oracle(("t3", n), rate, calls)
    _defaults(monkeypatch, gmax)
    monkeypatch.setenv("FWX_PERK_FOLD", "compare")
    got, _, groups = _run(rate, calls)
    assert_bits_equal(got, want, shape + " compare")
    assert groups == by_size


# ---- the only sign-set operands sit in the last block of a group -------------------------------------------------------
SB_N, SB_COL = 1024, 1000
SB_ROWS = (128 + 3 * 64 + 5, 384 + 7 * 64 + 5)


def _last_block_case():
    """D1 (every entry positive) with two -0.0, both at column SB_COL (tile column 7), as W operands of pivot 325 --
    stage 12 = 4 * 4 - 4 of the group [128, 384), in its last block: the main launch of that group sees it, tile column
    7 lies outside its two bands -- and of pivot 837 -- stage 28 = 4 * 8 - 4 of the group [384, 896): tile column 7 is
    the next group's band, so the 32-stage cross launch of the chain sees it.  Both rows are NaN left of their diagonal,
    so no earlier pivot moves them (their Ct operands are NaN) and the -0.0 is still there at its time: the tiles of
    tile column 7 whose entries are clean fold in the max form up to that stage and in the compare form from it."""
    rate = synth.make("d1", SB_N, F32, seed=SB_N + 37)[0]
    for k in SB_ROWS:
        rate[k, :k] = F32(np.nan)
        rate[k, SB_COL] = F32(-0.0)
    return rate


def test_sign_set_operand_in_the_last_block_of_a_group(monkeypatch):
    assert [(SB_ROWS[0] - 128) // 16, (SB_ROWS[1] - 384) // 16] == [4 * 4 - 4, 4 * 8 - 4] and SB_COL // 128 == 7
    rate = _last_block_case()
    want = _oracle(("last block",), rate, [(0, SB_N)])
    # the case itself on the oracle: up to each of the two pivots no pivot's row or column carries a sign bit (r[k][k]
    # apart, which the NaN patch hides) except the planted zero in its own row
    state, at, found = rate, 0, set()
    for stop in SB_ROWS:
        while at <= stop:
            for side, line in (("row", state[at, :]), ("col", state[:, at])):
                found.update((at, side, int(v)) for v in np.flatnonzero(np.signbit(line)) if v != at)
            state, at = perk_oracle(state, at, at + 1)[0], at + 1
    assert found == {(k, "row", SB_COL) for k in SB_ROWS}, found
    _check(monkeypatch, rate, [(0, SB_N)], "8", [2, 1, 0, 1], want, "last block of a group")


# ---- main launches of several rounds of workgroups ----------------------------------------------------------------------
BIG_N = 8192


def test_main_launches_that_outlast_the_chain(monkeypatch):
    """At the orders above a main launch is a single round of workgroups (at most 81 tiles on 256 CUs) and ends about
    when the chain's first launch does, so nothing there shows whether the two really keep apart.  At n = 8192 a main
    launch is up to 3969 tiles, more than five rounds, and runs beside all of the chain: a main launch that touched a
    tile of the chain's band, or read the panel half that the chain is filling, would end with other bits.  Two calls
    of 1024 pivots, as the benchmark issues them.  The reference is the serial schedule (FWX_PERK_PAIR_MIN_N=0) on the
    same device -- no look-ahead stream, one panel set, pinned to the oracle by tests/test_gpu_perk_tile.py; an oracle
    solve of these pivots at this order is 1.4e11 relaxations on the CPU, far past a test's few seconds."""
    calls, by_size = [(0, 1024), (1024, 2048)], {"8": [4, 2, 0, 2], "4": [4, 6, 0, 0], "2": [16, 0, 0, 0]}
    rate = _matrix("d1", BIG_N)
    _defaults(monkeypatch, "8")
    monkeypatch.setenv("FWX_PERK_PAIR_MIN_N", "0")
    want, older0, groups = _run(rate, calls)
    assert groups == [0, 0, 0, 0] and older0[4] == 0
    monkeypatch.setenv("FWX_PERK_PAIR_MIN_N", "1")
    for gmax in ("8", "4", "2"):
        monkeypatch.setenv("FWX_PERK_GROUP_MAX", gmax)
        got, older, groups = _run(rate, calls)
        assert_bits_equal(got, want, "n=%d at FWX_PERK_GROUP_MAX=%s against the serial schedule" % (BIG_N, gmax))
        assert groups == by_size[gmax] and older[:4] == older0[:4] and older[4] == 16, gmax


# ---- streams -----------------------------------------------------------------------------------------------------------
def test_two_streams_at_once(monkeypatch):
    """Two different matrices, each on a stream of its own, the calls interleaved without any synchronisation in
    between: the panel halves, the look-ahead stream and the events of a call are its stream's own."""
    _defaults(monkeypatch, "8")
    n = 1024
    a, b = _matrix("d1", n), _matrix("t4", n)
    calls = SHAPES["two calls of 512"][1]
    want_a, want_b = _oracle(("d1", n), a, calls), _oracle(("t4", n), b, calls)
    sa, sb = hip.Stream(), hip.Stream()
    hip.default_stream().synchronize()
    a_t, b_t = dev(a), dev(b)
    hip.default_stream().synchronize()
    _reset_all()
    for lo, hi in calls:
        engine.dev_relax(a_t, n, 0, lo, hi, stream=sa)
        engine.dev_relax(b_t, n, 0, lo, hi, stream=sb)
    sa.synchronize()
    sb.synchronize()
    assert_bits_equal(host(a_t), want_a, "stream a")
    assert_bits_equal(host(b_t), want_b, "stream b")
    assert _group()[1] == [8, 4, 0, 0]
