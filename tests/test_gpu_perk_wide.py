"""The wide pass of the per-k engine's multi-pivot schedule: an uncounted f32 call at the default width issues ONE
16-pivot relax_kt sweep wherever it would issue two consecutive 8-pivot ones inside a block (FWX_PERK_WIDE, on unless
`0`).  The sweep folds 16 snapshots per visit, in the max form where a wave's operands are all NaN or sign-clear and
in the 16-step compare form elsewhere, and must end at the bits of the sequential fold for every loaded entry.

Every case compares the rates bit for bit with the C oracle and reads both hooks: fwx_test_perk_pivots (a 16-pivot
launch counts as two 8-pivot groups, so the five counters are what the width 8 gives) and fwx_test_perk_wide (the
16-pivot launches themselves).

Orders: 1036 = two column strips, the second with 3 owning lanes and clamped ones, and a ragged last row chunk (the
compare form with 16 steps); 64 and 72 = one strip, a block shorter than 64, the diagonal in every tile; 264 for
the fold cases; 452 for two interleaved streams.

The vote.  With 16 rows x 16 pivots staged per workgroup a wave holds the staged Ct of only four pivots in its own
lanes; the other twelve reach its vote through a read-back from LDS, a branch that only the 16-pivot kernel has.
`negative_in_w_and_in_ct` is the case that pins it: hostile matrices disqualify every wave through W whatever the
read-back does, and D1 disqualifies none.
"""
import ctypes

import numpy as np
import pytest

from floydwarshall_amd import _lib, engine, hip, synth

from helpers import (MIB, assert_bits_equal, dev, dev_zeros, host, perk_expected_launches, perk_launches,
                     perk_oracle)
from hostile_inputs import hostile_matrix

pytestmark = pytest.mark.gpu

F32 = np.float32
STORE_BYTES = ["16", "32", "64", "128"]
_ORACLE = {}     # key -> the oracle's (rates, U): computed once, shared, never modified


def _want(key, rate, kb, ke):
    k = key + (kb, ke)
    if k not in _ORACLE:
        _ORACLE[k] = perk_oracle(rate, kb, ke)
    return _ORACLE[k]


def _wide(reset=True):
    """(what FWX_PERK_WIDE parses to, 16-pivot launches since the last reset)."""
    c = ctypes.c_uint64(0)
    on = _lib.lib().fwx_test_perk_wide(ctypes.byref(c), 1 if reset else 0)
    return on, int(c.value)


def _expected_wide(kb, ke):
    """16-groups of the schedule over pivots [kb, ke): per block of <= 64 pivots from kb, the whole 16s."""
    return sum(min(64, ke - k0) // 16 for k0 in range(kb, ke, 64) if min(64, ke - k0) >= 2)


def _reset():
    perk_launches()
    _wide()


def _defaults(monkeypatch):
    for v in ("FWX_PERK_PIVOTS", "FWX_PERK_WIDE", "FWX_PERK_FOLD", "FWX_PERK_STORE_BYTES", "FWX_PERK_TEMPORAL_MIB"):
        monkeypatch.delenv(v, raising=False)


def _run(rate, kb, ke, serp=True, counted=False):
    """fwx_dev_relax on the whole matrix in place: (rates, U or None, the five counters, wide launches)."""
    n = rate.shape[0]
    _reset()
    r_t = dev(rate)
    upd = dev_zeros((engine.FWX_UPDATE_SHARDS,), np.int64) if counted else None
    engine.dev_relax(r_t, n, 0, kb, ke, serpentine=serp, updates_t=upd)
    got = host(r_t)
    u = int(host(upd).sum()) if counted else None
    return got, u, perk_launches(), _wide()[1]


def _check_wide(rate, kb, ke, want, tag, serps=(True, False)):
    """The default uncounted call goes wide: oracle bits, the wide counter, the five counters of the width 8."""
    for serp in serps:
        got, _, launches, wide = _run(rate, kb, ke, serp)
        what = "%s serp=%s pivots [%d, %d)" % (tag, serp, kb, ke)
        assert_bits_equal(got, want[0], what)
        assert wide == _expected_wide(kb, ke), what
        assert launches == perk_expected_launches(kb, ke, 8), what


def _matrix(kind, n, dtype=F32):
    """hostile: awkward values everywhere (it saturates to inf and NaN within a few pivots); d1: the benchmark's
    distribution; d1_diag: d1 with a diagonal that every pivot's own column would improve from (r[k][k] > 1, +inf,
    the largest finite value) if the NaN at column k + t were missing for any of the 16 t."""
    if kind == "hostile":
        return hostile_matrix(np.random.default_rng(11 * n + 3), n, dtype)[0]
    rate = synth.make("d1", n, dtype, seed=n + 19)[0]
    if kind == "d1_diag":
        vals = np.array([3.0, np.inf, np.finfo(dtype).max, 1.5, -2.0, 7.0, np.nan], dtype=dtype)
        rate[np.arange(n), np.arange(n)] = vals[np.arange(n) % len(vals)]
    return rate


# ---- n = 1036: ranges, sweep orders, temporal budgets, store widths -------------------------------------------------
RANGES_1036 = [(0, 16),            # one wide launch and nothing else
               (3, 3 + 31),        # 16 + 8 + 4 + 2 + 1
               (1016, 1036),       # the 16 patched columns straddle the strip boundary and run to the end
               (60, 60 + 70)]      # a block counted from k_begin that ends ragged, then a second block


@pytest.mark.parametrize("kb,ke", RANGES_1036)
@pytest.mark.parametrize("kind", ["hostile", "d1", "d1_diag"])
def test_uncounted_relax_n1036(kind, kb, ke, monkeypatch):
    _defaults(monkeypatch)
    n = 1036
    rate = _matrix(kind, n)
    want = _want((kind, n), rate, kb, ke)
    assert _expected_wide(kb, ke) == {(0, 16): 1, (3, 34): 1, (1016, 1036): 1, (60, 130): 4}[(kb, ke)]
    for budget in (repr(rate.nbytes / 2 / MIB), "1e12"):       # one that splits the matrix, one that does not
        monkeypatch.setenv("FWX_PERK_TEMPORAL_MIB", budget)
        for store in STORE_BYTES:
            monkeypatch.setenv("FWX_PERK_STORE_BYTES", store)
            _check_wide(rate, kb, ke, want, "%s n=%d budget=%s G=%s" % (kind, n, budget, store))


# ---- one strip, short blocks, the diagonal in every tile ------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hostile", "d1", "d1_diag"])
@pytest.mark.parametrize("n", [64, 72])
def test_one_strip_whole_solve(n, kind, monkeypatch):
    _defaults(monkeypatch)
    rate = _matrix(kind, n)
    want = _want((kind, n), rate, 0, n)
    assert_bits_equal(np.diagonal(want[0]).copy(), np.diagonal(rate).copy(), "oracle: the diagonal")
    for store in STORE_BYTES:
        monkeypatch.setenv("FWX_PERK_STORE_BYTES", store)
        _check_wide(rate, 0, n, want, "%s n=%d G=%s" % (kind, n, store))


# ---- the fold at 16 steps, n = 264 ----------------------------------------------------------------------------------
FOLD_N, FOLD_KB, FOLD_KE = 264, 8, 8 + 48        # three 16-groups; a wave spans 256 columns, a tile 8 or 16 rows


VOTE_ROW, VOTE_COLS, VOTE_CT_T = 100, slice(120, 160), 9       # the Ct operand: one row, entries in the first wave
VOTE_ROWS, VOTE_COL, VOTE_W_T = slice(200, 216), 259, 11         # the W operand: one column of the second wave


def _nan32(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def _fold_case(kind):
    n, kb, ke = FOLD_N, FOLD_KB, FOLD_KE
    d1 = synth.make("d1", n, F32, seed=n + 23)[0]
    if kind == "sign_clear_operands_hostile_x":
        # pivot rows and columns from D1, every other entry hostile: NaN payloads, +-0, +-inf, negative denormals
        rate = hostile_matrix(np.random.default_rng(n + 1), n, F32)[0]
        rnd = np.random.default_rng(n + 2)
        extra = np.array([_nan32(0x7FC01234), _nan32(0xFFC00001), F32(-1e-40), F32(-0.0), F32(np.inf),
                          F32(-np.inf)], dtype=F32)
        where = rnd.random((n, n)) < 0.3
        rate[where] = rnd.choice(extra, size=int(where.sum()))
        rate[kb:ke, :] = d1[kb:ke, :]
        rate[:, kb:ke] = d1[:, kb:ke]
        return rate
    rate = d1.copy()
    if kind == "negative_in_w_and_in_ct":
        # Two operands with a sign bit, both -0.0, each followed by +0.0 at the next pivot, against entries x = -1
        # whose every other candidate is NaN: the sequential fold ends at -0.0 (+0.0 does not beat it), a max form taken
        # in spite of the -0.0 ends at +0.0.  Everything that could move an operand before its pivot's time is NaN or
        # zero, so each is still there when its snapshot is taken (test_fold_at_16_steps replays that on the oracle).
        nan = F32(np.nan)
        # Ct: r[VOTE_ROW][kb + 9] = -0.0.  Pivot t = 9 of the first 16-group is staged by the workgroup's third wave, so
        # the wave over columns 0 .. 255 learns of it through the read-back of the staged values alone; only the tile
        # of that row is disqualified, the waves over columns 0 .. 255 of every other tile keep the max form.
        a = kb + VOTE_CT_T
        rate[VOTE_ROW, kb:ke] = nan
        rate[VOTE_ROW, a], rate[VOTE_ROW, a + 1] = F32(-0.0), F32(0.0)
        for k in (a, a + 1):
            rate[k, kb:ke] = nan                   # nothing moves rows a, a + 1 before their time
            rate[k, VOTE_COLS] = F32(1.0)
        rate[a, a + 1] = rate[a + 1, a] = F32(0.0)  # pivot a leaves row and column a + 1 alone at those places
        rate[VOTE_ROW, VOTE_COLS] = F32(-1.0)
        # W: r[kb + 11][VOTE_COL] = -0.0 in a column that only the second wave holds (columns 256 ...): that wave
        # folds with the compare in every tile.
        b = kb + VOTE_W_T
        rate[kb:ke, VOTE_COL] = nan
        rate[b, VOTE_COL], rate[b + 1, VOTE_COL] = F32(-0.0), F32(0.0)
        rate[VOTE_ROWS, b] = rate[VOTE_ROWS, b + 1] = F32(1.0)
        rate[b, b + 1] = rate[b + 1, b] = F32(0.0)
        rate[VOTE_ROWS, VOTE_COL] = F32(-1.0)
    elif kind == "underflow_to_zero":
        # every candidate of the entries (i >= 200, j = 120 .. 122) is tiny * tiny = +0, against stored -0.0
        # (kept), +0.0 (kept) and a negative denormal (becomes +0); all operands sign-clear
        tiny = F32(1e-30)
        rate[200:, kb:ke] = tiny
        rate[kb:ke, 120:123] = tiny
        rate[200:, 120] = F32(-0.0)
        rate[200:, 121] = F32(0.0)
        rate[200:, 122] = F32(-1e-40)
    elif kind == "ties_t_and_t_plus_8":
        # pivots t and t + 8 of every 16-group get the same row and the same column, in powers of two, so that
        # their candidates are equal bit for bit wherever neither snapshot has moved: the pair that two 8-pivot
        # launches used to separate
        rnd = np.random.default_rng(n + 5)
        rate = np.ldexp(F32(1.0), -rnd.integers(1, 6, size=(n, n))).astype(F32)
        for g in range(kb, ke, 16):
            for t in range(8):
                rate[g + t + 8, :] = rate[g + t, :]
                rate[:, g + t + 8] = rate[:, g + t]
    elif kind == "hostile_pivot_diagonal":
        vals = [_nan32(0xFFC00001), F32(-np.inf), F32(-0.0), F32(-3.0), _nan32(0x7FC01234), F32(np.inf)]
        for k in range(kb, ke):
            rate[k, k] = vals[k % len(vals)]
    else:
        raise AssertionError(kind)
    return rate


@pytest.mark.parametrize("kind", ["sign_clear_operands_hostile_x", "negative_in_w_and_in_ct", "underflow_to_zero",
                                  "ties_t_and_t_plus_8", "hostile_pivot_diagonal"])
def test_fold_at_16_steps(kind, monkeypatch):
    _defaults(monkeypatch)
    n, kb, ke = FOLD_N, FOLD_KB, FOLD_KE
    rate = _fold_case(kind)
    want = _want(("fold", kind), rate, kb, ke)
    if kind == "sign_clear_operands_hostile_x":
        ok = lambda a: bool(np.all(np.isnan(a) | ~np.signbit(a)))
        assert ok(want[0][kb:ke, :]) and ok(want[0][:, kb:ke]), "the case itself: operands stay NaN or sign-clear"
    if kind == "negative_in_w_and_in_ct":
        # the case itself, replayed on the oracle pivot by pivot: at its own time each pivot's row and column (but
        # r[k][k], which the NaN patch hides) carry no sign bit except the two -0.0, which are still there, each
        # followed by a +0.0; and the entries they decide end at -0.0
        planted = {(kb + VOTE_CT_T, "col", VOTE_ROW), (kb + VOTE_W_T, "row", VOTE_COL)}
        state, found = rate.copy(), set()
        for k in range(kb, ke):
            for side, line in (("row", state[k, :]), ("col", state[:, k])):
                for at in np.flatnonzero(np.signbit(line)):
                    if at != k:
                        assert line[at] == 0, (k, side, at)
                        found.add((k, side, int(at)))
            if k == kb + VOTE_CT_T + 1:
                assert state[VOTE_ROW, k] == 0 and not np.signbit(state[VOTE_ROW, k])
                assert np.all(state[k, VOTE_COLS] == 1) and np.all(state[k - 1, VOTE_COLS] == 1)
            if k == kb + VOTE_W_T + 1:
                assert state[k, VOTE_COL] == 0 and not np.signbit(state[k, VOTE_COL])
            state = perk_oracle(state, k, k + 1)[0]
        assert found == planted, found
        assert_bits_equal(state, want[0], "the replay")
        for got in (want[0][VOTE_ROW, VOTE_COLS], want[0][VOTE_ROWS, VOTE_COL]):
            assert np.all(got == 0) and np.all(np.signbit(got)), "the oracle must end at -0.0 there"
    if kind == "underflow_to_zero":
        got = want[0][200:, 120:123]
        assert np.all(got == 0) and np.all(np.signbit(got[:, 0])) and not np.any(np.signbit(got[:, 1:]))
    for fold in (None, "compare"):
        if fold:
            monkeypatch.setenv("FWX_PERK_FOLD", fold)
        for store in ("64", "16"):
            monkeypatch.setenv("FWX_PERK_STORE_BYTES", store)
            _check_wide(rate, kb, ke, want, "%s fold=%s G=%s" % (kind, fold, store))


# ---- the switch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hostile", "d1"])
def test_wide_off_is_the_same_solve_launch_for_launch(kind, monkeypatch):
    _defaults(monkeypatch)
    n, kb, ke = 1036, 60, 130
    rate = _matrix(kind, n)
    want = _want((kind, n), rate, kb, ke)
    on_r, _, on_launches, on_wide = _run(rate, kb, ke)
    assert _wide(reset=False)[0] == 1
    monkeypatch.setenv("FWX_PERK_WIDE", "0")
    assert _wide(reset=False)[0] == 0
    off_r, _, off_launches, off_wide = _run(rate, kb, ke)
    assert_bits_equal(on_r, want[0], "wide on")
    assert_bits_equal(off_r, want[0], "wide off")
    assert on_wide == _expected_wide(kb, ke) == 4 and off_wide == 0
    assert on_launches == off_launches == perk_expected_launches(kb, ke, 8)


# ---- calls that must not go wide --------------------------------------------------------------------------------------
def test_a_counted_call_stays_8_wide(monkeypatch):
    _defaults(monkeypatch)
    n, kb, ke = 1036, 60, 130
    for kind in ("hostile", "d1"):
        rate = _matrix(kind, n)
        want = _want((kind, n), rate, kb, ke)
        got, u, launches, wide = _run(rate, kb, ke, counted=True)
        assert_bits_equal(got, want[0], kind)
        assert u == want[1] and wide == 0 and launches == perk_expected_launches(kb, ke, 8), kind


def test_an_f64_call_stays_8_wide(monkeypatch):
    _defaults(monkeypatch)
    n, kb, ke = 518, 60, 130
    for kind in ("hostile", "d1"):
        rate = _matrix(kind, n, np.float64)
        want = _want((kind, n, "f64"), rate, kb, ke)
        got, _, launches, wide = _run(rate, kb, ke)
        assert_bits_equal(got, want[0], kind)
        assert wide == 0 and launches == perk_expected_launches(kb, ke, 8), kind


@pytest.mark.parametrize("width", [4, 2, 1])
def test_narrower_widths_stay_as_they_are(width, monkeypatch):
    _defaults(monkeypatch)
    monkeypatch.setenv("FWX_PERK_PIVOTS", str(width))
    n, kb, ke = 1036, 60, 130
    rate = _matrix("d1", n)
    want = _want(("d1", n), rate, kb, ke)
    got, _, launches, wide = _run(rate, kb, ke)
    assert_bits_equal(got, want[0], "width %d" % width)
    assert wide == 0 and launches == perk_expected_launches(kb, ke, width)


# ---- two streams ------------------------------------------------------------------------------------------------------
def test_two_streams_interleaved_wide_and_narrow(monkeypatch):
    """Two different matrices, each solved in slices on a stream of its own, the calls interleaved without any
    synchronisation in between; the cuts make 16-pivot and narrower launches alternate on both streams."""
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
