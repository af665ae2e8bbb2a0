"""The kernel of the 16-pivot sweep since round 23 (relax_walk, FWX_PERK_WALK, on unless `0`): one body for every
tile, the diagonal as a run-time term of the fold, three waves per SIMD.  A workgroup owns WALK_R rows of its strip,
keeps the 16 pivot rows for all of them and folds WALK_SLOTS rows per batch, the last batch without a reload behind
it; a chunk that is no multiple of the slots takes the compare form with a row-by-row tail.  It must end at the bits
of the sequential fold for every loaded entry, like the kernel it replaces.

Every case compares the rates bit for bit with the C oracle and reads both launch hooks, fwx_test_perk_pivots and
fwx_test_perk_wide: the walk changes the kernel of a 16-pivot launch, never the schedule.

Orders.  1024 + e ends both strips with a chunk of e % WALK_R rows (a whole one at 16 and 32), the second strip with
e / 4 owning lanes and clamped ones: e = 4 no head (the tail alone), 8 and 24 the last batch alone, 12 head and tail,
16 and 32 a batch with a reload behind it and the last one.  The chunks from row 1024 on hold the diagonal in strip 1,
those above it in strip 0; the others do not.  64 and 72: one strip, the diagonal in every tile.  264 for the fold
cases (sixteen whole chunks and one of 8 rows), 452 for two streams.
"""
import numpy as np
import pytest

from floydwarshall_amd import _lib, engine, hip, synth

from helpers import MIB, assert_bits_equal, dev, host, perk_expected_launches, perk_launches
from test_gpu_perk_wide import (FOLD_KB, FOLD_KE, FOLD_N, STORE_BYTES, _expected_wide, _fold_case, _matrix, _reset,
                                _run, _want, _wide)

pytestmark = pytest.mark.gpu

F32 = np.float32
WALK_R, WALK_SLOTS = 16, 8          # FWX_PERK_WALK_RPB, FWX_PERK_WALK_UNROLL of fwx_kernels.h
ENDS = [4, 8, 12, 16, 24, 32]


def _walk():
    return _lib.lib().fwx_test_perk_walk()


def _defaults(monkeypatch):
    for v in ("FWX_PERK_PIVOTS", "FWX_PERK_WIDE", "FWX_PERK_WALK", "FWX_PERK_FOLD", "FWX_PERK_STORE_BYTES",
              "FWX_PERK_TEMPORAL_MIB"):
        monkeypatch.delenv(v, raising=False)


def _check(rate, kb, ke, want, tag, serps=(True, False), walk=1):
    """Oracle bits, the wide counter, the five counters of the width 8, whichever kernel sweeps."""
    for serp in serps:
        assert _walk() == walk
        got, _, launches, wide = _run(rate, kb, ke, serp)
        what = "%s serp=%s pivots [%d, %d)" % (tag, serp, kb, ke)
        assert_bits_equal(got, want[0], what)
        assert wide == _expected_wide(kb, ke), what
        assert launches == perk_expected_launches(kb, ke, 8), what


def test_the_orders_cover_every_chunk_shape():
    """(a batch is loaded at the start, a row-by-row tail, batches with a reload behind them) of the last chunk: every
    combination the geometry has."""
    assert WALK_R % WALK_SLOTS == 0 and WALK_R in ENDS
    shapes = set()
    for e in ENDS:
        rows = e % WALK_R or WALK_R
        head, tail = rows >= WALK_SLOTS, rows % WALK_SLOTS != 0
        shapes.add((head, tail, 0 if tail else rows // WALK_SLOTS - 1))
    want = {(False, True, 0), (True, False, 0), (True, True, 0)}
    want |= {(True, False, i) for i in range(1, WALK_R // WALK_SLOTS)}
    assert shapes == want


# ---- every chunk shape at the end of both strips ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hostile", "d1", "d1_diag"])
@pytest.mark.parametrize("end", ENDS)
def test_uncounted_relax_chunk_shapes(end, kind, monkeypatch):
    _defaults(monkeypatch)
    n = 1024 + end
    rate = _matrix(kind, n)
    # from 0 (nearly every row stores: a slot is reloaded behind its store), the middle of a block (three 16-groups
    # off the block's first panel rows), the patched columns across the strip boundary to the end of the row
    ranges = [(0, 32), (40, 40 + 48), (n - 20, n)]
    assert [_expected_wide(*r) for r in ranges] == [2, 3, 1]
    for kb, ke in ranges:
        want = _want((kind, n), rate, kb, ke)
        for budget in (repr(rate.nbytes / 2 / MIB), "1e12"):       # one that splits the matrix, one that does not
            monkeypatch.setenv("FWX_PERK_TEMPORAL_MIB", budget)
            for store in STORE_BYTES:
                monkeypatch.setenv("FWX_PERK_STORE_BYTES", store)
                _check(rate, kb, ke, want, "%s n=%d budget=%s G=%s" % (kind, n, budget, store))


# ---- one strip, short blocks, the diagonal in every tile ------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hostile", "d1", "d1_diag"])
@pytest.mark.parametrize("n", [64, 72])
def test_one_strip_whole_solve(n, kind, monkeypatch):
    _defaults(monkeypatch)
    rate = _matrix(kind, n)
    want = _want((kind, n), rate, 0, n)
    for store in STORE_BYTES:
        monkeypatch.setenv("FWX_PERK_STORE_BYTES", store)
        _check(rate, 0, n, want, "%s n=%d G=%s" % (kind, n, store))


# ---- the fold constructions of round 14 at 16 steps, n = 264 ----------------------------------------------------------
@pytest.mark.parametrize("kind", ["sign_clear_operands_hostile_x", "negative_in_w_and_in_ct", "underflow_to_zero",
                                  "ties_t_and_t_plus_8", "hostile_pivot_diagonal"])
def test_fold_constructions(kind, monkeypatch):
    """negative_in_w_and_in_ct: a -0.0 in one W row and in one Ct row, so waves in the max form and waves in the compare
    form meet in one launch (what the case is, is checked against the oracle by tests/test_gpu_perk_wide.py)."""
    _defaults(monkeypatch)
    rate = _fold_case(kind)
    want = _want(("fold", kind), rate, FOLD_KB, FOLD_KE)
    if kind == "negative_in_w_and_in_ct":
        from test_gpu_perk_wide import VOTE_COL, VOTE_COLS, VOTE_ROW, VOTE_ROWS
        for got in (want[0][VOTE_ROW, VOTE_COLS], want[0][VOTE_ROWS, VOTE_COL]):
            assert np.all(got == 0) and np.all(np.signbit(got)), "the oracle must end at -0.0 there"
    for fold in (None, "compare"):
        if fold:
            monkeypatch.setenv("FWX_PERK_FOLD", fold)
        for store in ("64", "16"):
            monkeypatch.setenv("FWX_PERK_STORE_BYTES", store)
            _check(rate, FOLD_KB, FOLD_KE, want, "%s fold=%s G=%s" % (kind, fold, store))


# ---- the switches -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hostile", "d1"])
def test_walk_off_and_wide_off_are_the_same_solve(kind, monkeypatch):
    _defaults(monkeypatch)
    n, kb, ke = 1024 + 24, 60, 130
    rate = _matrix(kind, n)
    want = _want((kind, n), rate, kb, ke)
    _check(rate, kb, ke, want, "walk on")
    assert _expected_wide(kb, ke) == 4
    monkeypatch.setenv("FWX_PERK_WALK", "0")
    _check(rate, kb, ke, want, "walk off", walk=0)              # round 19's kernel: the same launches, the same counts
    monkeypatch.setenv("FWX_PERK_WIDE", "0")
    for walk in ("0", "1"):
        monkeypatch.setenv("FWX_PERK_WALK", walk)
        got, _, launches, wide = _run(rate, kb, ke)
        assert_bits_equal(got, want[0], "wide off, walk %s" % walk)
        assert wide == 0 and launches == perk_expected_launches(kb, ke, 8)
        assert (_wide(reset=False)[0], _walk()) == (0, int(walk))


# ---- two streams ------------------------------------------------------------------------------------------------------
def test_two_streams_interleaved(monkeypatch):
    """Two different matrices, each solved in slices on a stream of its own, the calls interleaved without any
    synchronisation in between; walks and narrower launches alternate on both streams."""
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
    assert _walk() == 1
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        engine.dev_relax(a_t, n, 0, lo, hi, stream=sa)
        engine.dev_relax(b_t, n, 0, lo, hi, stream=sb)
    sa.synchronize()
    sb.synchronize()
    assert_bits_equal(host(a_t), want_a, "stream a")
    assert_bits_equal(host(b_t), want_b, "stream b")
    slices = list(zip(cuts[:-1], cuts[1:]))
    assert _wide()[1] == 2 * sum(_expected_wide(lo, hi) for lo, hi in slices) > 0
    want_l = [2 * sum(perk_expected_launches(lo, hi, 8)[i] for lo, hi in slices) for i in range(5)]
    assert perk_launches() == want_l
