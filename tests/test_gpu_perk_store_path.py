"""relax_k's rates-only store path: when any lane of an aligned group of G / 16 lanes improved, every lane of
the group stores its vector, the others writing back the bits they loaded (FWX_PERK_STORE_BYTES = G).  For
every G the rates and the update count U must equal the oracle's bit for bit: clamped lanes past the end of a
row (n % 1024 != 0) never store beside the owner of the last vector, groups straddle 64-byte sectors
(n % 16 != 0), slab heights are not multiples of 4, slabs start at row0 != 0 with pivot rows from an external
panel and skip a row range, inputs are hostile (NaN payloads, -0.0, inf, subnormals), both sweep orders run,
and the temporal split of the streaming loads falls inside the slab."""
import numpy as np
import pytest

import oracle
from floydwarshall_amd import engine, synth

from helpers import assert_bits_equal, dev, dev_empty, dev_zeros, host
from hostile_inputs import hostile_matrix

pytestmark = pytest.mark.gpu

MIB = float(1 << 20)
STORE_BYTES = ["16", "32", "64", "128"]


def _budgets(slab_bytes):
    """FWX_PERK_TEMPORAL_MIB: the split in the middle of the slab, and all default policy."""
    return [repr(slab_bytes / 2 / MIB), "1e12"]


def _oracle(rate, k_begin, k_end):
    er = rate.copy()
    u = oracle.relax_mt(er, None, k_begin, k_end, threads=16, fast=True)
    return er, u


def _check_solves(rate, kb, ke, monkeypatch):
    want_r, want_u = _oracle(rate, kb, ke)
    for g in STORE_BYTES:
        monkeypatch.setenv("FWX_PERK_STORE_BYTES", g)
        for budget in _budgets(rate.nbytes):
            monkeypatch.setenv("FWX_PERK_TEMPORAL_MIB", budget)
            for serp in (True, False):
                got = rate.copy()
                u = engine.solve(got, None, None, engine=engine.FWX_ENGINE_PERK, count_updates=True,
                                 k_begin=kb, k_end=ke, serpentine=serp)
                assert_bits_equal(got, want_r, "rate G=%s budget=%s serp=%s" % (g, budget, serp))
                assert u == want_u, (g, budget, serp)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [1000, 1036, 2056])
def test_store_widths_equal_the_oracle(n, dtype, monkeypatch):
    """n = 1000, 1036: clamped lanes and rows that are not whole sectors; 2056: several strips, the last one
    a single partial group.  An odd k_begin starts in the reversed sweep direction."""
    rate, _, _ = synth.make("d1", n, dtype, seed=n + 11)
    _check_solves(rate, 5, 5 + (160 if n > 2000 else 300), monkeypatch)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_store_widths_on_hostile_inputs(dtype, monkeypatch):
    rnd = np.random.default_rng(1036)
    for n in (1000, 1036):
        rate, _, _ = hostile_matrix(rnd, n, dtype)
        _check_solves(rate, 3, 3 + 160, monkeypatch)


def _updates_in_rows(rate, k0, k1, lo, hi):
    """The oracle's updates in rows [lo, hi) over pivots [k0, k1), in place on `rate`."""
    u = 0
    for k in range(k0, k1):
        before = rate[lo:hi].copy()
        oracle.relax(rate, None, None, k, k + 1)
        u += int(np.count_nonzero(rate[lo:hi] != before))
    return u


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_store_widths_on_row_slabs(dtype, monkeypatch):
    """fwx_dev_relax on a slab of 767 rows starting at row 257 (height not a multiple of 4), pivot rows from a
    time-k snapshot panel, with and without a skipped row range; the budget puts the split inside the slab."""
    n, lo, hi, k0, k1 = 1036, 257, 1024, 301, 365
    rate = synth.make("d2", n, dtype, seed=43)[0]
    want_r = rate.copy()
    oracle.relax(want_r, None, None, k0, k1)
    su = _updates_in_rows(rate.copy(), k0, k1, lo, hi)
    slab = (hi - lo) * n * np.dtype(dtype).itemsize
    for g in STORE_BYTES:
        monkeypatch.setenv("FWX_PERK_STORE_BYTES", g)
        monkeypatch.setenv("FWX_PERK_TEMPORAL_MIB", repr(slab / 3 / MIB))
        for serp in (True, False):
            for skip in (None, (64, 128)):
                full_t = dev(rate)
                w = dev_empty((k1 - k0, n), dtype)
                engine.dev_panel_snap(full_t[k0:k1], n, k0, w)
                r_t = dev(rate[lo:hi])
                upd = dev_zeros((engine.FWX_UPDATE_SHARDS,), np.int64)
                engine.dev_relax(r_t, n, lo, k0, k1, pivots_t=w, serpentine=serp, updates_t=upd, skip=skip)
                got = host(r_t)
                keep = np.ones(hi - lo, dtype=bool)
                if skip:
                    keep[skip[0]:skip[1]] = False
                    assert_bits_equal(got[~keep], rate[lo:hi][~keep], "skipped rows G=%s" % g)
                assert_bits_equal(got[keep], want_r[lo:hi][keep], "slab G=%s serp=%s skip=%s" % (g, serp, skip))
                if skip is None:
                    assert int(host(upd).sum()) == su, (g, serp)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_store_widths_whole_matrix_in_place(dtype, monkeypatch):
    """The whole matrix as one slab, pivot rows read in place (row k is never stored, column k is rewritten
    with its own bits under the pivot-column gathers of the other strips)."""
    n = 1000
    rate = synth.make("t1", n, dtype, seed=29)[0]
    want_r = rate.copy()
    eu = oracle.relax_mt(want_r, None, 0, n, threads=16, fast=True)
    for g in STORE_BYTES:
        monkeypatch.setenv("FWX_PERK_STORE_BYTES", g)
        monkeypatch.setenv("FWX_PERK_TEMPORAL_MIB", repr(rate.nbytes / 2 / MIB))
        r_t = dev(rate)
        upd = dev_zeros((engine.FWX_UPDATE_SHARDS,), np.int64)
        engine.dev_relax(r_t, n, 0, 0, n, updates_t=upd)
        assert_bits_equal(host(r_t), want_r, "rate G=%s" % g)
        assert int(host(upd).sum()) == eu, g
