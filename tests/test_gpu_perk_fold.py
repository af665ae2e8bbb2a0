"""relax_kt's fold without a per-step diagonal term or changed flag: the diagonal component folds from +inf
and gets its loaded bits back, `changed` is an integer comparison of the folded vector with the loaded one, and
a workgroup picks one of four stream instantiations, (non-temporal | default loads) x (tile holds diagonal
elements | it does not).  Everything is compared bit for bit with the C oracle, U too where the call counts:

  1. orders that put the diagonal on the edges of the tile choice -- one vector per row; a full 8-row chunk plus
     a 4-row tail; a second strip with a single owning lane, whose diagonal rows sit in the tail chunk; three
     strips -- at widths 2, 4, 8, both sweep orders and a temporal budget that splits the matrix;
  2. the counted call (the counting instantiation) and the uncounted call (the one bench.py times), separately,
     on every case of 1;
  3. inputs on which a missing diagonal guard or a wrong `changed` shows -- hostile values, exact ties, and
     diagonals that every pivot would improve (0.5 under off-diagonals in (0.8, 1), -0.0, NaN with a payload) -- for
     every store width, so that the unchanged lanes of a store group write back exactly what they loaded.
"""
import numpy as np
import pytest

from floydwarshall_amd import engine, synth

from helpers import MIB, assert_bits_equal, dev, host, perk_check, perk_oracle
from hostile_inputs import hostile_matrix

pytestmark = pytest.mark.gpu

WIDTHS = [2, 4, 8]
STORE_BYTES = ["16", "32", "64", "128"]
ORDERS = [(4, np.float32), (12, np.float32), (1028, np.float32), (2056, np.float32),
          (2, np.float64), (6, np.float64), (514, np.float64), (1030, np.float64)]
_ORACLE = {}     # (what, n, dtype, kb, ke) -> the oracle's (rates, U): computed once, shared, never modified


def _want(key, rate, kb, ke):
    k = key + (kb, ke)
    if k not in _ORACLE:
        _ORACLE[k] = perk_oracle(rate, kb, ke)
    return _ORACLE[k]


def _ranges(n):
    """Three blocks from an odd start, the last one 27 = 8 + 8 + 8 + 2 + 1 pivots, and the last pivots of the
    matrix; whole solves at the tiny orders."""
    return [(0, n)] if n < 160 else [(5, 160), (n - 77, n)]


def _input(kind, n, dtype, seed):
    if kind == "hostile":
        return hostile_matrix(np.random.default_rng(seed), n, dtype)[0]
    return synth.make(kind, n, dtype, seed=seed)[0]


def _nan_with_payload(dtype):
    if np.dtype(dtype) == np.float32:
        return np.array([0x7FC01234], dtype=np.uint32).view(np.float32)[0]
    return np.array([0x7FF8000000012345], dtype=np.uint64).view(np.float64)[0]


def _tempting(kind, n, dtype):
    """A matrix whose diagonal every pivot would improve if nothing guarded it: r[i][k] * r[k][i] > r[i][i]."""
    rnd = np.random.default_rng(n + len(kind))
    if kind == "half_under_large":
        rate = (0.8 + rnd.random((n, n)) / 5.0).astype(dtype)     # products in (0.64, 1): no cycle gains
        np.fill_diagonal(rate, 0.5)
        return rate
    rate = synth.make("d1", n, dtype, seed=n + 5)[0]
    diag = np.where(np.arange(n) % 2 == 0, dtype(-0.0), _nan_with_payload(dtype)).astype(dtype)
    rate[np.arange(n), np.arange(n)] = diag
    return rate


def _uncounted(rate, kb, ke, monkeypatch, want_r, what, widths=WIDTHS, serps=(True, False)):
    """fwx_dev_relax without an update counter: the instantiation bench.py times."""
    monkeypatch.setenv("FWX_PERK_TEMPORAL_MIB", repr(rate.nbytes / 2 / MIB))
    n = rate.shape[0]
    for np_ in widths:
        monkeypatch.setenv("FWX_PERK_PIVOTS", str(np_))
        for serp in serps:
            r_t = dev(rate)
            engine.dev_relax(r_t, n, 0, kb, ke, serpentine=serp)
            assert_bits_equal(host(r_t), want_r, "%s NP=%d serp=%s pivots [%d, %d), not counting"
                              % (what, np_, serp, kb, ke))


def _diagonal_kept(rate, got, what):
    assert_bits_equal(np.diagonal(got).copy(), np.diagonal(rate).copy(), what + ": the diagonal")


# ---- 1 and 2: the diagonal on the edges of the tile choice, counted and uncounted ---------------------------------
@pytest.mark.parametrize("kind", ["d1", "hostile"])
@pytest.mark.parametrize("n,dtype", ORDERS)
def test_counted_calls_at_the_edges_of_the_tile_choice(n, dtype, kind, monkeypatch):
    monkeypatch.delenv("FWX_PERK_STORE_BYTES", raising=False)
    rate = _input(kind, n, dtype, 3 * n + 1)
    for kb, ke in _ranges(n):
        want = _want((kind, n, np.dtype(dtype).name), rate, kb, ke)
        perk_check(rate, kb, ke, monkeypatch, "%s n=%d" % (kind, n), budgets=[repr(rate.nbytes / 2 / MIB)],
                   pivots=WIDTHS, want=want)
        _diagonal_kept(rate, want[0], "oracle %s n=%d" % (kind, n))


@pytest.mark.parametrize("kind", ["d1", "hostile"])
@pytest.mark.parametrize("n,dtype", ORDERS)
def test_uncounted_calls_at_the_edges_of_the_tile_choice(n, dtype, kind, monkeypatch):
    monkeypatch.delenv("FWX_PERK_STORE_BYTES", raising=False)
    rate = _input(kind, n, dtype, 3 * n + 1)
    for kb, ke in _ranges(n):
        want_r = _want((kind, n, np.dtype(dtype).name), rate, kb, ke)[0]
        _uncounted(rate, kb, ke, monkeypatch, want_r, "%s n=%d" % (kind, n))


# ---- 3: inputs on which a missing diagonal guard or a wrong `changed` shows ---------------------------------------
@pytest.mark.parametrize("store", STORE_BYTES)
@pytest.mark.parametrize("kind", ["hostile", "t1", "half_under_large", "negzero_and_nan"])
@pytest.mark.parametrize("n,dtype", [(1028, np.float32), (514, np.float64)])
def test_diagonal_and_write_back_at_every_store_width(n, dtype, kind, store, monkeypatch):
    monkeypatch.setenv("FWX_PERK_STORE_BYTES", store)
    rate = _input(kind, n, dtype, n + 13) if kind in ("hostile", "t1") else _tempting(kind, n, dtype)
    kb, ke = 5, 160
    want_r, want_u = _want(("every store width", kind, n, np.dtype(dtype).name), rate, kb, ke)
    _diagonal_kept(rate, want_r, "oracle " + kind)
    what = "%s n=%d G=%s" % (kind, n, store)
    perk_check(rate, kb, ke, monkeypatch, what, budgets=[repr(rate.nbytes / 2 / MIB)], serps=(True,), pivots=WIDTHS,
               want=(want_r, want_u))
    _uncounted(rate, kb, ke, monkeypatch, want_r, what, serps=(True,))
