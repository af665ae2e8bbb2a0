"""The deep pass of the per-k engine's multi-pivot schedule (round 25, FWX_PERK_DEEP, on unless `0`): where the ladder
of an uncounted f32 call at the default width started at 16 pivots per streaming pass, it starts at 32.  The sweep is
relax_walk with 8 bytes of a row per lane: strips of 512 columns, DEEP_R rows per workgroup, DEEP_SLOTS rows per batch,
32 snapshots folded per visit -- in the max form (the maximum of 32 candidates, one compare) where a wave's operands are
all NaN or sign-clear, in the 32-step compare form elsewhere and in every chunk that is no multiple of the slots, which
ends in a row-by-row tail.  The diagonal component of row r is r % 2.  It must end at the bits of the sequential fold
for every loaded entry.

Every case compares the rates bit for bit with the C oracle and reads the three launch hooks: a 32-pivot launch counts
as four 8-pivot groups in fwx_test_perk_pivots, as two in fwx_test_perk_wide and as one in fwx_test_perk_deep.

Orders.  512 + e ends both strips with a chunk of e % DEEP_R rows (a whole one at 64), the second strip with e / 2
owning lanes beside clamped ones: e = 4 the tail alone, 8 the last batch alone, 12 head and tail, 16, 24, 32, 40 and 64
batches with a reload behind them (one to seven) and the last one.  The chunks from row 512 on hold the diagonal in
strip 1.  64 and 72: one strip, the diagonal in every tile.  264 for the fold cases, 452 for two streams.
"""
import ctypes

import numpy as np
import pytest

from floydwarshall_amd import _lib, engine, hip, synth

from helpers import MIB, assert_bits_equal, dev, host, perk_expected_launches, perk_launches, perk_oracle
from test_gpu_perk_wide import (FOLD_KB, FOLD_KE, FOLD_N, STORE_BYTES, _expected_wide, _fold_case, _matrix, _reset,
                                _run, _want, _wide)

pytestmark = pytest.mark.gpu

F32 = np.float32
DEEP_R, DEEP_SLOTS = 64, 8          # FWX_PERK_DEEP_RPB, FWX_PERK_DEEP_UNROLL of fwx_kernels.h
STRIP = 512                         # 256 lanes x 2 floats
ENDS = [4, 8, 12, 16, 24, 32, 40, 64]
KNOBS = ("FWX_PERK_PIVOTS", "FWX_PERK_WIDE", "FWX_PERK_WALK", "FWX_PERK_DEEP", "FWX_PERK_FOLD", "FWX_PERK_STORE_BYTES",
         "FWX_PERK_TEMPORAL_MIB")


def _deep(reset=True):
    """(what FWX_PERK_DEEP parses to, 32-pivot launches since the last reset)."""
    c = ctypes.c_uint64(0)
    on = _lib.lib().fwx_test_perk_deep(ctypes.byref(c), 1 if reset else 0)
    return on, int(c.value)


def _expected_deep(kb, ke):
    """32-groups of the schedule over pivots [kb, ke): per block of <= 64 pivots from kb, the whole 32s."""
    return sum(min(64, ke - k0) // 32 for k0 in range(kb, ke, 64) if min(64, ke - k0) >= 2)


def _defaults(monkeypatch):
    for v in KNOBS:
        monkeypatch.delenv(v, raising=False)


def _run_deep(rate, kb, ke, serp=True):
    """(rates, the five counters, wide launches, deep launches) of one uncounted fwx_dev_relax."""
    _deep()
    got, _, launches, wide = _run(rate, kb, ke, serp)
    return got, launches, wide, _deep()[1]


def _check(rate, kb, ke, want, tag, serps=(True, False), deep_on=True):
    """Oracle bits and the three hooks.  deep_on False: a switch is off, no 32-pivot launch, the rest as before."""
    for serp in serps:
        got, launches, wide, deep = _run_deep(rate, kb, ke, serp)
        what = "%s serp=%s pivots [%d, %d)" % (tag, serp, kb, ke)
        assert_bits_equal(got, want[0], what)
        assert deep == (_expected_deep(kb, ke) if deep_on else 0), what
        assert wide == _expected_wide(kb, ke), what
        assert launches == perk_expected_launches(kb, ke, 8), what


def test_the_orders_cover_every_chunk_shape():
    """(a batch is loaded at the start, a row-by-row tail, batches with a reload behind them) of the last chunk: every
    combination the geometry has."""
    assert DEEP_R % DEEP_SLOTS == 0 and DEEP_R in ENDS
    shapes = set()
    for e in ENDS:
        rows = e % DEEP_R or DEEP_R
        head, tail = rows >= DEEP_SLOTS, rows % DEEP_SLOTS != 0
        shapes.add((head, tail, 0 if tail else rows // DEEP_SLOTS - 1))
    want = {(False, True, 0), (True, False, 0), (True, True, 0)}
    want |= {(True, False, DEEP_R // DEEP_SLOTS - 1)}                # a whole chunk
    assert shapes >= want and len({s for s in shapes if s[2]}) >= 4  # and several lengths of the reload loop
    assert all(0 < e // 2 < 256 for e in ENDS)             # owning lanes beside clamped ones in the second strip


# ---- every chunk shape at the end of both strips ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hostile", "d1", "d1_diag"])
@pytest.mark.parametrize("end", ENDS)
def test_uncounted_relax_chunk_shapes(end, kind, monkeypatch):
    _defaults(monkeypatch)
    n = STRIP + end
    rate = _matrix(kind, n)
    # from 0 (nearly every row stores), 32 + 16 + 8 off a block's first panel rows, the patched columns across the
    # strip boundary to the end of the row (32 + 4)
    ranges = [(0, 32), (40, 96), (n - 36, n)]
    assert [_expected_deep(*r) for r in ranges] == [1, 1, 1]
    assert [_expected_wide(*r) for r in ranges] == [2, 3, 2]
    assert STRIP < n and (n - 36 < STRIP or end >= 40)      # from 40 on the 36 columns lie in the second strip alone
    monkeypatch.setenv("FWX_PERK_TEMPORAL_MIB", repr(rate.nbytes / 2 / MIB))       # a budget that splits the matrix
    for kb, ke in ranges:
        want = _want((kind, n), rate, kb, ke)
        for store in STORE_BYTES:
            monkeypatch.setenv("FWX_PERK_STORE_BYTES", store)
            _check(rate, kb, ke, want, "%s n=%d G=%s" % (kind, n, store))


# ---- one strip, short blocks, the diagonal in every tile ------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hostile", "d1", "d1_diag"])
@pytest.mark.parametrize("n", [64, 72])
def test_one_strip_whole_solve(n, kind, monkeypatch):
    _defaults(monkeypatch)
    rate = _matrix(kind, n)
    want = _want((kind, n), rate, 0, n)
    assert_bits_equal(np.diagonal(want[0]).copy(), np.diagonal(rate).copy(), "oracle: the diagonal")
    assert _expected_deep(0, n) == 2
    for store in STORE_BYTES:
        monkeypatch.setenv("FWX_PERK_STORE_BYTES", store)
        _check(rate, 0, n, want, "%s n=%d G=%s" % (kind, n, store))


# ---- the fold at 32 steps, n = 264: pivots [8, 56) are one 32-group and one 16-group ---------------------------------
LATE_ROW, LATE_COLS, LATE_CT_T = 100, slice(110, 150), 25      # a Ct operand of the group's second half: one tile
LATE_ROWS, LATE_COL, LATE_W_T = slice(200, 216), 259, 27         # a W operand: one column of the strip's third wave


def _deep_fold_case(kind):
    n, kb = FOLD_N, FOLD_KB
    d1 = synth.make("d1", n, F32, seed=n + 29)[0]
    if kind == "ties_t_and_t_plus_16":
        # pivots t and t + 16 of the 32-group get the same row and the same column, in powers of two: their candidates
        # are equal bit for bit wherever neither snapshot has moved -- the pair that two 16-pivot launches separated
        rnd = np.random.default_rng(n + 7)
        rate = np.ldexp(F32(1.0), -rnd.integers(1, 6, size=(n, n))).astype(F32)
        for t in range(16):
            rate[kb + t + 16, :] = rate[kb + t, :]
            rate[:, kb + t + 16] = rate[:, kb + t]
        return rate
    if kind == "negative_late_in_w_and_in_ct":
        # tests/test_gpu_perk_wide.py's negative_in_w_and_in_ct with both operands among pivots 16 .. 31 of the group,
        # which no 16-pivot kernel stages or votes on: a -0.0 followed by +0.0 at the next pivot, against entries
        # x = -1 whose every other candidate is NaN.  The sequential fold ends at -0.0; a max form taken in spite of the
        # -0.0 ends at +0.0.  A wave spans 128 columns here: LATE_COLS lies in waves 0 and 1, LATE_COL in wave 2.
        rate, nan, ke = d1.copy(), F32(np.nan), FOLD_KE
        a = kb + LATE_CT_T
        rate[LATE_ROW, kb:ke] = nan
        rate[LATE_ROW, a], rate[LATE_ROW, a + 1] = F32(-0.0), F32(0.0)
        for k in (a, a + 1):
            rate[k, kb:ke] = nan
            rate[k, LATE_COLS] = F32(1.0)
        rate[a, a + 1] = rate[a + 1, a] = F32(0.0)
        rate[LATE_ROW, LATE_COLS] = F32(-1.0)
        b = kb + LATE_W_T
        rate[kb:ke, LATE_COL] = nan
        rate[b, LATE_COL], rate[b + 1, LATE_COL] = F32(-0.0), F32(0.0)
        rate[LATE_ROWS, b] = rate[LATE_ROWS, b + 1] = F32(1.0)
        rate[b, b + 1] = rate[b + 1, b] = F32(0.0)
        rate[LATE_ROWS, LATE_COL] = F32(-1.0)
        return rate
    return _fold_case(kind)


@pytest.mark.parametrize("kind", ["sign_clear_operands_hostile_x", "negative_in_w_and_in_ct", "underflow_to_zero",
                                  "ties_t_and_t_plus_8", "hostile_pivot_diagonal", "ties_t_and_t_plus_16",
                                  "negative_late_in_w_and_in_ct"])
def test_fold_constructions(kind, monkeypatch):
    _defaults(monkeypatch)
    assert (_expected_deep(FOLD_KB, FOLD_KE), _expected_wide(FOLD_KB, FOLD_KE)) == (1, 3)
    rate = _deep_fold_case(kind)
    want = _want(("deep fold", kind), rate, FOLD_KB, FOLD_KE)
    if kind == "negative_in_w_and_in_ct":
        from test_gpu_perk_wide import VOTE_COL, VOTE_COLS, VOTE_ROW, VOTE_ROWS
        for got in (want[0][VOTE_ROW, VOTE_COLS], want[0][VOTE_ROWS, VOTE_COL]):
            assert np.all(got == 0) and np.all(np.signbit(got)), "the oracle must end at -0.0 there"
    if kind == "negative_late_in_w_and_in_ct":
        for got in (want[0][LATE_ROW, LATE_COLS], want[0][LATE_ROWS, LATE_COL]):
            assert np.all(got == 0) and np.all(np.signbit(got)), "the oracle must end at -0.0 there"
        # the case itself, replayed on the oracle pivot by pivot: at its own time each pivot's row and column (but
        # r[k][k], which the NaN patch hides) carry no sign bit except the two planted -0.0, so only the tile of
        # LATE_ROW and the wave of LATE_COL are disqualified
        planted = {(FOLD_KB + LATE_CT_T, "col", LATE_ROW), (FOLD_KB + LATE_W_T, "row", LATE_COL)}
        state, found = rate.copy(), set()
        for k in range(FOLD_KB, FOLD_KE):
            for side, line in (("row", state[k, :]), ("col", state[:, k])):
                for at in np.flatnonzero(np.signbit(line)):
                    if at != k:
                        assert line[at] == 0, (k, side, at)
                        found.add((k, side, int(at)))
            state = perk_oracle(state, k, k + 1)[0]
        assert found == planted, found
        assert_bits_equal(state, want[0], "the replay")
    if kind == "ties_t_and_t_plus_16":
        t = np.arange(16) + FOLD_KB
        assert_bits_equal(rate[t, :5].copy(), rate[t + 16, :5].copy(), "the case itself")
    for fold in (None, "compare"):
        if fold:
            monkeypatch.setenv("FWX_PERK_FOLD", fold)
        for store in ("64", "16"):
            monkeypatch.setenv("FWX_PERK_STORE_BYTES", store)
            _check(rate, FOLD_KB, FOLD_KE, want, "%s fold=%s G=%s" % (kind, fold, store))


# ---- the switches -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hostile", "d1"])
def test_each_switch_off_is_the_same_solve(kind, monkeypatch):
    _defaults(monkeypatch)
    n, kb, ke = STRIP + 24, 60, 130
    rate = _matrix(kind, n)
    want = _want((kind, n), rate, kb, ke)
    assert (_expected_deep(kb, ke), _expected_wide(kb, ke)) == (2, 4)
    assert _deep(reset=False)[0] == 1
    _check(rate, kb, ke, want, "deep on")
    monkeypatch.setenv("FWX_PERK_DEEP", "0")
    assert _deep(reset=False)[0] == 0
    _check(rate, kb, ke, want, "deep off", deep_on=False)
    monkeypatch.delenv("FWX_PERK_DEEP")
    monkeypatch.setenv("FWX_PERK_WALK", "0")
    assert _deep(reset=False)[0] == 1
    _check(rate, kb, ke, want, "walk off", deep_on=False)      # the deep pass is relax_walk's: without it, round 19's launches
    monkeypatch.delenv("FWX_PERK_WALK")
    monkeypatch.setenv("FWX_PERK_WIDE", "0")
    got, launches, wide, deep = _run_deep(rate, kb, ke)
    assert_bits_equal(got, want[0], "wide off")
    assert (wide, deep) == (0, 0) and launches == perk_expected_launches(kb, ke, 8)
    assert (_wide(reset=False)[0], _deep(reset=False)[0]) == (0, 1)


# ---- two streams ------------------------------------------------------------------------------------------------------
def test_two_streams_interleaved(monkeypatch):
    """Two different matrices, each solved in slices on a stream of its own, the calls interleaved without any
    synchronisation in between; 32-pivot, 16-pivot and narrower launches alternate on both streams."""
    _defaults(monkeypatch)
    n = 452
    a = synth.make("d1", n, F32, seed=1)[0]
    b = synth.make("t2", n, F32, seed=2)[0]
    want_a, want_b = _want(("streams a",), a, 0, n)[0], _want(("streams b",), b, 0, n)[0]
    cuts = [0, 16, 21, 53, 54, 134, 150, 230, 231, 400, n]
    sa, sb = hip.Stream(), hip.Stream()
    hip.default_stream().synchronize()
    a_t, b_t = dev(a), dev(b)
    hip.default_stream().synchronize()
    _reset()
    _deep()
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        engine.dev_relax(a_t, n, 0, lo, hi, stream=sa)
        engine.dev_relax(b_t, n, 0, lo, hi, stream=sb)
    sa.synchronize()
    sb.synchronize()
    assert_bits_equal(host(a_t), want_a, "stream a")
    assert_bits_equal(host(b_t), want_b, "stream b")
    slices = list(zip(cuts[:-1], cuts[1:]))
    assert _deep()[1] == 2 * sum(_expected_deep(lo, hi) for lo, hi in slices) > 0
    assert _wide()[1] == 2 * sum(_expected_wide(lo, hi) for lo, hi in slices)
    want_l = [2 * sum(perk_expected_launches(lo, hi, 8)[i] for lo, hi in slices) for i in range(5)]
    assert perk_launches() == want_l
