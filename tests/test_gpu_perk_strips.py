"""relax_kt at column-strip boundaries.  A strip is 256 sixteen-byte vectors wide (1024 f32 / 512 f64 columns), a
wave covers 64 of them, and four things the kernel does depend on where a strip, a wave or a store group ends:

  * the NaN at column k + t of its pivot-row registers (skip j == k) and in every component of a clamped lane (a
    lane past the end of the row in the ragged last strip), patched in by selects in every strip;
  * the store rule: a group of 1, 2, 4 or 8 lanes stores when one of its lanes changed.  The counting kernel
    evaluates it on the wave mask of the compares in scalar registers and uses the result as the exec mask of the
    store, so a wrong shift or group mask shows at the first and last lane of a group, of a wave and of a strip, and
    where a group is partly clamped; the uncounted kernel rebuilds the flag per lane from the ballot;
  * U, the number of updates: the set bits of every compare mask of the fold, counted per wave in scalar registers --
    a clamped lane or a NaN column that compared true would be counted;
  * the tile index, split into strip and row chunk by a multiply-high where the matrix has two strips or more (here:
    2 and 3 strips, a power of two and not).

The shapes are those at which a rule "which strips need the NaN patch" would go wrong (leaving the selects out of the
other strips was tried and measured slower; the cases stay as its regression tests):

  * a group of 8 pivots across a strip boundary;
  * a pivot in the last column of a strip and one in the first column of the next;
  * three strips, pivots in the first and across the second boundary, a diagonal tile that is also the pivot strip;
  * a ragged last strip (4 columns past the boundary, 255 lanes clamped), the pivots outside it and inside it, at
    the default store width, at 16 bytes (the group of one lane, whose store rule has no owner term) and at 128.

Every width 1 / 2 / 4 / 8, both temporal budgets and both sweep orders through helpers.perk_check: rates, U and the
launch counters bit for bit against the C oracle, on a uniform matrix and on a hostile one (NaN, +-0, +-inf,
negatives).  perk_check always counts; the uncounted kernel is the one whole solves run, so each case is also run
once without counting."""
import numpy as np
import pytest

from floydwarshall_amd import engine, synth

from helpers import assert_bits_equal, dev, host, perk_check, perk_oracle
from hostile_inputs import hostile_matrix

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
# (dtype, n, pivot ranges, the last strip is ragged)
CASES = {
    "f32 straddle": (F32, 2048, [(1020, 1036)], False),
    "f32 last and first column": (F32, 2048, [(1016, 1024), (1024, 1032)], False),
    "f32 three strips": (F32, 3072, [(0, 24), (2040, 2064)], False),
    "f32 ragged": (F32, 2052, [(1020, 1036), (2040, 2052)], True),
    "f64 straddle": (F64, 1024, [(508, 524)], False),
    "f64 ragged": (F64, 1028, [(1016, 1028)], True),
}
RAGGED = [c for c, v in CASES.items() if v[3]]
KINDS = ["d1", "hostile"]
_INPUT, _ORACLE = {}, {}      # computed once, shared between the tests, never modified


def _input(case, kind):
    dtype, n = CASES[case][:2]
    if (case, kind) not in _INPUT:
        if kind == "hostile":
            rate = hostile_matrix(np.random.default_rng(n + 13), n, dtype)[0]
        else:
            rate = synth.make("d1", n, dtype, seed=n + 5)[0]
        rate.setflags(write=False)
        _INPUT[case, kind] = rate
    return _INPUT[case, kind]


def _want(case, kind, kb, ke):
    if (case, kind, kb, ke) not in _ORACLE:
        _ORACLE[case, kind, kb, ke] = perk_oracle(_input(case, kind), kb, ke)
    return _ORACLE[case, kind, kb, ke]


def _check_case(case, kind, monkeypatch):
    rate = _input(case, kind)
    for kb, ke in CASES[case][2]:
        perk_check(rate, kb, ke, monkeypatch, "%s, %s" % (case, kind), want=_want(case, kind, kb, ke))


def test_the_cases_sit_on_the_boundaries_they_claim():
    """Arithmetic of the cases themselves (no GPU work): every case has a pivot group of 8 that meets two strips or
    touches a strip's first or last column, the ragged ones end 4 columns past a strip boundary, and every order is
    a multiple of the vector width (or the multi-pivot schedule would not run at all)."""
    for case, (dtype, n, ranges, ragged) in CASES.items():
        w = 16 // np.dtype(dtype).itemsize
        sw = 256 * w
        assert n % w == 0, case
        assert (n % sw != 0) == ragged and (not ragged or n % sw == 4), case
        groups = [(k, min(k + 8, ke)) for kb, ke in ranges for k in range(kb, ke, 8)]
        assert any(lo // sw != (hi - 1) // sw or lo % sw == 0 or hi % sw == 0 for lo, hi in groups), case
        assert all(hi <= n for lo, hi in groups), case


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", list(CASES))
def test_strip_boundaries_equal_the_oracle(case, kind, monkeypatch):
    monkeypatch.delenv("FWX_PERK_STORE_BYTES", raising=False)
    _check_case(case, kind, monkeypatch)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("store", ["16", "128"])
@pytest.mark.parametrize("case", RAGGED)
def test_ragged_strip_at_the_narrowest_and_widest_store_group(case, store, kind, monkeypatch):
    """16 bytes: a lane stores when it changed, with no owner term -- a clamped lane must never have changed.
    128 bytes: groups of 8 lanes, the last group of the row partly clamped."""
    monkeypatch.setenv("FWX_PERK_STORE_BYTES", store)
    _check_case(case, kind, monkeypatch)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", list(CASES))
def test_without_counting(case, kind, monkeypatch):
    """The uncounted instantiation (what a whole solve launches), widths 2, 4 and 8, the default budget."""
    monkeypatch.delenv("FWX_PERK_STORE_BYTES", raising=False)
    monkeypatch.delenv("FWX_PERK_TEMPORAL_MIB", raising=False)
    rate = _input(case, kind)
    n = CASES[case][1]
    for np_ in (2, 4, 8):
        monkeypatch.setenv("FWX_PERK_PIVOTS", str(np_))
        for kb, ke in CASES[case][2]:
            r_t = dev(rate)
            engine.dev_relax(r_t, n, 0, kb, ke)
            assert_bits_equal(host(r_t), _want(case, kind, kb, ke)[0], "%s, %s, NP=%d [%d, %d)" % (case, kind, np_, kb, ke))
