"""The per-k engine's multi-pivot schedule: a rates-only solve of the whole matrix in place applies
FWX_PERK_PIVOTS = NP pivots per streaming pass (relax_kt) from the time-k snapshots of one panel launch per
64-pivot block.  For every NP (1 = one relax_k launch per pivot) and both dtypes the rates, and U where the call
counts, must equal the C oracle's bit for bit:

  * orders with ragged strips, ragged row chunks and clamped lanes (260, 324, 452, 1036: the orders of the
    kernel-forms tests), pivot ranges that start and end inside a 64-block and inside an NP-group;
  * uniform, tie-heavy, sparse and hostile inputs (+-inf, NaN, negatives, -0.0: the reason the fold is the strict
    compare and never max);
  * both sweep orders, a temporal budget that splits the matrix (both load instantiations run) and one that
    does not, every FWX_PERK_STORE_BYTES;
  * the headline order N = 16384 against the committed digest of the whole oracle solve;
  * two solves interleaved on two streams of one process (the snapshot scratch is keyed by stream).

The launch counters of the test hook show that the sweeps really were NP wide."""
import numpy as np
import pytest

from floydwarshall_amd import _lib, engine, hip, synth

from helpers import (MIB, PERK_PIVOTS as PIVOTS, assert_bits_equal, dev, digest, host, load_golden,
                     perk_check as _check, perk_expected_launches as _expected_launches, perk_launches as _launches,
                     perk_oracle as _oracle)
from hostile_inputs import hostile_matrix

pytestmark = pytest.mark.gpu

ORDERS = [260, 324, 452, 1036]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", ORDERS)
def test_every_width_equals_the_oracle_at_ragged_orders(n, dtype, monkeypatch):
    """Pivots [5, 5 + 64 + 64 + 27): three blocks from an odd start (blocks are counted from k_begin, so every
    group straddles an aligned group of NP pivots), the last one ragged with 27 = 8 + 8 + 8 + 2 + 1 pivots; and
    the last pivots of the matrix, where a group ends at n."""
    rate = synth.make("d1", n, dtype, seed=n + 7)[0]
    _check(rate, 5, 5 + 155, monkeypatch, "d1 n=%d" % n)
    _check(rate, n - 77, n, monkeypatch, "d1 n=%d tail" % n, budgets=[repr(rate.nbytes / 2 / MIB)], serps=(True,))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kb,ke", [(0, 64), (63, 65), (64, 131), (30, 33), (17, 18), (100, 228), (7, 260)])
def test_pivot_ranges_that_cut_blocks_and_groups(kb, ke, dtype, monkeypatch):
    """A whole block; two pivots across an aligned block boundary; 67 = 64 + 2 + 1; three pivots = 2 + 1; a
    single pivot (relax_k, no panel); two whole blocks off the 64 grid; 253 pivots up to the end of the matrix."""
    n = 260
    rate = synth.make("d2", n, dtype, seed=kb * 1000 + ke)[0]
    _check(rate, kb, ke, monkeypatch, "d2", budgets=[repr(rate.nbytes / 2 / MIB)], serps=(True,))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["t1", "t2", "hostile"])
def test_ties_sparse_and_hostile_inputs(kind, dtype, monkeypatch):
    """t1: exact ties everywhere (the earliest pivot must win: ascending fold order, strict compare); t2: 15 %
    density; hostile: NaN, +-inf, negatives, -0.0, subnormals, overflowing products -- two draws per order (the
    generator picks a mostly-ordinary or an all-odd mix at random)."""
    rnd = np.random.default_rng(452)
    for n in (324, 452):
        for rep in range(2 if kind == "hostile" else 1):
            rate = hostile_matrix(rnd, n, dtype)[0] if kind == "hostile" else synth.make(kind, n, dtype, seed=n + 3)[0]
            _check(rate, 3, 3 + 150, monkeypatch, "%s n=%d" % (kind, n), budgets=[repr(rate.nbytes / 2 / MIB)])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_store_width(dtype, monkeypatch):
    """n = 1036: clamped lanes beside the owner of the last vector, rows that are not whole 64-byte sectors."""
    n = 1036
    rnd = np.random.default_rng(1036)
    for rate, what in ((synth.make("d1", n, dtype, seed=61)[0], "d1"), (hostile_matrix(rnd, n, dtype)[0], "hostile")):
        for g in ("16", "32", "64", "128"):
            monkeypatch.setenv("FWX_PERK_STORE_BYTES", g)
            _check(rate, 9, 9 + 90, monkeypatch, "%s G=%s" % (what, g), budgets=[repr(rate.nbytes / 3 / MIB)],
                   serps=(True,))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_whole_solves_through_the_handle_and_host_entry_points(dtype, monkeypatch):
    """fwx_solve_* with the per-k engine (counting) and a whole uncounted solve on device memory."""
    n = 324
    rate = synth.make("t1", n, dtype, seed=5)[0]
    want_r, want_u = _oracle(rate, 0, n)
    for np_ in PIVOTS:
        monkeypatch.setenv("FWX_PERK_PIVOTS", str(np_))
        got = rate.copy()
        u = engine.solve(got, None, None, engine=engine.FWX_ENGINE_PERK, count_updates=True)
        assert_bits_equal(got, want_r, "fwx_solve NP=%d" % np_)
        assert u == want_u, np_
        r_t = dev(rate)
        engine.dev_relax(r_t, n, 0, 0, n)
        assert_bits_equal(host(r_t), want_r, "fwx_dev_relax NP=%d, not counting" % np_)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_two_streams_interleaved(dtype, monkeypatch):
    """Two different matrices, each solved in slices on a stream of its own, the calls interleaved without any
    synchronisation in between: every call rewrites the snapshot scratch of ITS stream only."""
    n = 452
    a = synth.make("d1", n, dtype, seed=1)[0]
    b = synth.make("t2", n, dtype, seed=2)[0]
    want_a, want_b = _oracle(a, 0, n)[0], _oracle(b, 0, n)[0]
    for np_ in (2, 4, 8):
        monkeypatch.setenv("FWX_PERK_PIVOTS", str(np_))
        sa, sb = hip.Stream(), hip.Stream()
        hip.default_stream().synchronize()
        a_t, b_t = dev(a), dev(b)
        hip.default_stream().synchronize()
        cuts = [0, 37, 101, 230, 231, 400, n]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            engine.dev_relax(a_t, n, 0, lo, hi, stream=sa)
            engine.dev_relax(b_t, n, 0, lo, hi, stream=sb)
        sa.synchronize()
        sb.synchronize()
        assert_bits_equal(host(a_t), want_a, "stream a NP=%d" % np_)
        assert_bits_equal(host(b_t), want_b, "stream b NP=%d" % np_)


def test_headline_order_n16384_against_the_whole_oracle_solve(monkeypatch):
    """BASELINE config 4, the matrix bench.py's headline figure is measured on, through fwx_dev_relax at the
    default width: the digest of all 2^28 rates is that of the whole oracle solve (tests/golden)."""
    monkeypatch.delenv("FWX_PERK_PIVOTS", raising=False)
    n = 16384
    gold = load_golden("config4_n16384_digests.json")
    rate_h = synth.d1_uniform(n, np.float32, synth.BASE_SEED + 3)[0]
    r_t = dev(rate_h)
    del rate_h
    _launches()
    engine.dev_relax(r_t, n, 0, 0, n)
    assert digest(host(r_t)) == gold["rate_digest"]
    np_ = _lib.lib().fwx_test_perk_pivots(None, 0)
    assert _launches() == _expected_launches(0, n, np_)
