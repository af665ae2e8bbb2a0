"""relax_kt's max form of the fold: a wave whose loaded pivot operands (its slices of W after the NaN patch, the tile's
staged Ct) are all NaN or sign-clear takes m = maxNum of its NP candidates and then `x < m ? m : x`, every other wave
and every counting launch folds with a compare and a select per pivot.  Both must give the bits of the sequential
fold for EVERY loaded x, so everything here is compared bit for bit with the C oracle, U too
where the call counts, with FWX_PERK_FOLD unset (automatic) and `compare` (the compare form in every tile):

  1. pivot rows and columns from D1 (operands qualify in every tile), every other entry hostile;
  2. one disqualifying operand in a D1 matrix, so that tiles of both forms meet in one launch, and products that
     underflow to +0 against entries equal to -0.0, +0.0 and a negative denormal; and cases that a wrong vote
     fails: a single -0.0 operand, in W or in Ct, followed by +0.0 in the same group against a negative entry;
  3. hostile matrices whole (the compare form nearly everywhere);
  4. diagonals that every pivot would improve, at every store width;
  5. exact ties.

Orders: one partial strip with clamped lanes, a second strip with a single owning lane (and a ragged last row
chunk), three strips.
"""
import numpy as np
import pytest

from floydwarshall_amd import engine, synth

from helpers import MIB, assert_bits_equal, dev, host, perk_check, perk_oracle
from hostile_inputs import hostile_matrix

pytestmark = pytest.mark.gpu

WIDTHS = [2, 4, 8]
FOLDS = ["auto", "compare"]
STORE_BYTES = ["16", "32", "64", "128"]
ORDERS = [(12, np.float32), (1028, np.float32), (2056, np.float32),
          (6, np.float64), (514, np.float64), (1030, np.float64)]
MID = [(1028, np.float32), (514, np.float64)]
BIG = [(2056, np.float32), (1030, np.float64)]
_ORACLE = {}     # key -> the oracle's (rates, U): computed once, shared, never modified


def _want(key, rate, kb, ke):
    k = key + (kb, ke)
    if k not in _ORACLE:
        _ORACLE[k] = perk_oracle(rate, kb, ke)
    return _ORACLE[k]


def _ranges(n):
    """Three blocks from an odd start, the last one 27 = 8 + 8 + 8 + 2 + 1 pivots, and the last pivots of the
    matrix; whole solves at the tiny orders."""
    return [(0, n)] if n < 160 else [(5, 160), (n - 77, n)]


def _set_fold(monkeypatch, fold):
    if fold == "auto":
        monkeypatch.delenv("FWX_PERK_FOLD", raising=False)
    else:
        monkeypatch.setenv("FWX_PERK_FOLD", fold)


def _both_calls(rate, kb, ke, monkeypatch, want, what, serps=(True, False)):
    """The counted call (U and the launch counters too) and the uncounted one, the instantiation bench.py times, at
    every width, with a temporal budget that splits the matrix."""
    want_r, _ = want
    n = rate.shape[0]
    budget = repr(rate.nbytes / 2 / MIB)
    perk_check(rate, kb, ke, monkeypatch, what, budgets=[budget], serps=serps, pivots=WIDTHS, want=want)
    monkeypatch.setenv("FWX_PERK_TEMPORAL_MIB", budget)
    for np_ in WIDTHS:
        monkeypatch.setenv("FWX_PERK_PIVOTS", str(np_))
        for serp in serps:
            r_t = dev(rate)
            engine.dev_relax(r_t, n, 0, kb, ke, serpentine=serp)
            assert_bits_equal(host(r_t), want_r, "%s NP=%d serp=%s pivots [%d, %d), not counting"
                              % (what, np_, serp, kb, ke))


def _sign_clear_or_nan(a):
    return bool(np.all(np.isnan(a) | ~np.signbit(a)))


def _nan_bits(dtype, bits32, bits64):
    if np.dtype(dtype) == np.float32:
        return np.array([bits32], dtype=np.uint32).view(np.float32)[0]
    return np.array([bits64], dtype=np.uint64).view(np.float64)[0]


# ---- 1: operands qualify everywhere, the folded entries are anything -----------------------------------------------
def _hostile_x(n, dtype, kb, ke):
    rate = hostile_matrix(np.random.default_rng(7 * n + kb), n, dtype)[0]
    d1 = synth.make("d1", n, dtype, seed=n + 1)[0]
    rate[kb:ke, :] = d1[kb:ke, :]
    rate[:, kb:ke] = d1[:, kb:ke]
    return rate


@pytest.mark.parametrize("fold", FOLDS)
@pytest.mark.parametrize("n,dtype", ORDERS)
def test_max_form_with_hostile_x(n, dtype, fold, monkeypatch):
    monkeypatch.delenv("FWX_PERK_STORE_BYTES", raising=False)
    _set_fold(monkeypatch, fold)
    for kb, ke in _ranges(n):
        rate = _hostile_x(n, dtype, kb, ke)
        want = _want(("hostile x", n, np.dtype(dtype).name), rate, kb, ke)
        # the premise held at every pivot time: rows and columns of the range stayed NaN or sign-clear
        assert _sign_clear_or_nan(want[0][kb:ke, :]) and _sign_clear_or_nan(want[0][:, kb:ke])
        _both_calls(rate, kb, ke, monkeypatch, want, "hostile x n=%d fold=%s" % (n, fold))


# ---- 2: tiles of both forms in one launch ---------------------------------------------------------------------------
def _mixed(kind, n, dtype):
    """A D1 matrix with one disqualifying operand for the pivots [5, 160) (strips are 1024 f32 / 512 f64 columns)."""
    rate = synth.make("d1", n, dtype, seed=n + 3)[0]
    strip = 1024 if np.dtype(dtype) == np.float32 else 512
    tiny = dtype(1e-30) if np.dtype(dtype) == np.float32 else dtype(1e-200)
    if kind == "negzero_in_pivot_row":
        rate[21, strip + 5] = dtype(-0.0)
    elif kind == "negative_in_pivot_column":
        rate[8 + 3, 37] = dtype(-0.75)
    elif kind == "negative_nan_in_pivot_row":
        rate[90, 3] = _nan_bits(dtype, 0xFFC00001, 0xFFF8000000000001)
    else:
        # every candidate of the entries (i >= 200, j = 300 .. 302) is tiny * tiny, which underflows to +0, against
        # loaded entries of -0.0 (kept), +0.0 (kept) and a negative denormal (becomes +0); all operands sign-clear
        rate[200:, 5:160] = tiny
        rate[5:160, 300:303] = tiny
        rate[200:, 300] = dtype(-0.0)
        rate[200:, 301] = dtype(0.0)
        rate[200:, 302] = dtype(-1e-40) if np.dtype(dtype) == np.float32 else dtype(-1e-320)
    return rate


@pytest.mark.parametrize("fold", FOLDS)
@pytest.mark.parametrize("kind", ["negzero_in_pivot_row", "negative_in_pivot_column", "negative_nan_in_pivot_row",
                                  "underflow_to_zero"])
@pytest.mark.parametrize("n,dtype", BIG)
def test_mixed_tiles_in_one_launch(n, dtype, kind, fold, monkeypatch):
    monkeypatch.delenv("FWX_PERK_STORE_BYTES", raising=False)
    _set_fold(monkeypatch, fold)
    rate = _mixed(kind, n, dtype)
    kb, ke = 5, 160
    want = _want(("mixed", kind, n, np.dtype(dtype).name), rate, kb, ke)
    _both_calls(rate, kb, ke, monkeypatch, want, "%s n=%d fold=%s" % (kind, n, fold))


# ---- 2b: cases a wrong vote fails -------------------------------------------------------------------------------------
def _vote(side, n, dtype, comp):
    """Pivots 8 and 9 lie in one group of 2, 4 or 8 pivots of the range [8, 16).  At the entries x[i][j] = -1 below,
    pivot 8's candidate is -0.0 and pivot 9's is +0.0, every other candidate of the group is NaN.  The sequential
    fold ends at -0.0 (+0.0 does not beat it); a max form taken in spite of the -0.0 operand ends at +0.0.  The only
    sign bit among the operands of those waves is the -0.0: on the W side r[8][j] for ONE column j = 2000 + comp
    (every component of a lane's vector in turn), on the Ct side r[i][8] for one row i."""
    rate = synth.make("d1", n, dtype, seed=n + 9)[0]
    nan = dtype(np.nan)
    rows, cols = np.arange(300, 340), np.arange(1990, 2030)
    if side == "w":
        cols = np.array([2000 + comp])
        rate[np.ix_(rows, cols)] = dtype(-1.0)
        rate[rows, 8] = dtype(1.0)
        rate[rows, 9] = dtype(1.0)
        rate[8, cols] = dtype(-0.0)
        rate[9, cols] = dtype(0.0)
        for k in range(10, 16):
            rate[k, cols] = nan
    else:
        rows = np.array([300 + comp])
        rate[np.ix_(rows, cols)] = dtype(-1.0)
        rate[8, cols] = dtype(1.0)
        rate[9, cols] = dtype(1.0)
        rate[rows, 8] = dtype(-0.0)
        rate[rows, 9] = dtype(0.0)
        for k in range(10, 16):
            rate[rows, k] = nan
    rate[8, 9] = rate[9, 8] = dtype(0.0)       # pivot 8 must not change row 9 or column 9 at those places
    return rate, rows, cols


@pytest.mark.parametrize("fold", FOLDS)
@pytest.mark.parametrize("comp", [0, 1, 2, 3])
@pytest.mark.parametrize("side", ["w", "ct"])
def test_a_single_negative_zero_operand_decides_the_form(side, comp, fold, monkeypatch):
    monkeypatch.delenv("FWX_PERK_STORE_BYTES", raising=False)
    _set_fold(monkeypatch, fold)
    n, dtype = 2056, np.float32
    rate, rows, cols = _vote(side, n, dtype, comp)
    kb, ke = 8, 16
    want = _want(("vote", side, comp), rate, kb, ke)
    got = want[0][np.ix_(rows, cols)]
    assert np.all(got == 0) and np.all(np.signbit(got)), "the case itself: the oracle must end at -0.0 there"
    _both_calls(rate, kb, ke, monkeypatch, want, "vote %s comp=%d fold=%s" % (side, comp, fold), serps=(True,))


# ---- 3: hostile everything ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fold", FOLDS)
@pytest.mark.parametrize("n,dtype", ORDERS)
def test_hostile_everything(n, dtype, fold, monkeypatch):
    monkeypatch.delenv("FWX_PERK_STORE_BYTES", raising=False)
    _set_fold(monkeypatch, fold)
    rate = hostile_matrix(np.random.default_rng(5 * n + 2), n, dtype)[0]
    for kb, ke in _ranges(n):
        want = _want(("hostile", n, np.dtype(dtype).name), rate, kb, ke)
        _both_calls(rate, kb, ke, monkeypatch, want, "hostile n=%d fold=%s" % (n, fold))


# ---- 4 and 5: the diagonal and exact ties, at every store width -----------------------------------------------------
def _tempting(kind, n, dtype):
    """A matrix whose diagonal every pivot would improve if nothing guarded it: r[i][k] * r[k][i] > r[i][i]."""
    rnd = np.random.default_rng(n + len(kind))
    if kind == "half_under_large":
        rate = (0.8 + rnd.random((n, n)) / 5.0).astype(dtype)     # products in (0.64, 1): no cycle gains
        np.fill_diagonal(rate, 0.5)
        return rate
    rate = synth.make("d1", n, dtype, seed=n + 5)[0]
    diag = np.where(np.arange(n) % 2 == 0, dtype(-0.0),
                    _nan_bits(dtype, 0x7FC01234, 0x7FF8000000012345)).astype(dtype)
    rate[np.arange(n), np.arange(n)] = diag
    return rate


@pytest.mark.parametrize("fold", FOLDS)
@pytest.mark.parametrize("store", STORE_BYTES)
@pytest.mark.parametrize("kind", ["half_under_large", "negzero_and_nan", "t1"])
@pytest.mark.parametrize("n,dtype", MID)
def test_diagonal_and_ties_at_every_store_width(n, dtype, kind, store, fold, monkeypatch):
    monkeypatch.setenv("FWX_PERK_STORE_BYTES", store)
    _set_fold(monkeypatch, fold)
    rate = synth.make("t1", n, dtype, seed=n + 13)[0] if kind == "t1" else _tempting(kind, n, dtype)
    kb, ke = 5, 160
    want = _want(("every store width", kind, n, np.dtype(dtype).name), rate, kb, ke)
    assert_bits_equal(np.diagonal(want[0]).copy(), np.diagonal(rate).copy(), "oracle %s: the diagonal" % kind)
    _both_calls(rate, kb, ke, monkeypatch, want, "%s n=%d G=%s fold=%s" % (kind, n, store, fold))
