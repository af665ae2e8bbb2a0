"""relax_k's cache-policy split: the workgroups before the temporal tail of a launch stream r[i][j] with
non-temporal loads, the tail with default-policy loads (RelaxArgs::temporal_bytes, FWX_PERK_TEMPORAL_MIB).
A cache hint only: wherever the split falls -- the whole slab non-temporal, a tail smaller than one
workgroup's rows, the middle of the slab -- every result bit, the update count U and the path trace
must equal the oracle's and the all-default-policy run's."""
import numpy as np
import pytest

import oracle
from floydwarshall_amd import engine, synth

from helpers import assert_bits_equal, dev, dev_empty, dev_zeros, host
from hostile_inputs import hostile_matrix

pytestmark = pytest.mark.gpu

MIB = float(1 << 20)
ALL_DEFAULT = "1e12"       # MiB: no slab is that large -> today's all-default-policy launches


def _budgets(slab_bytes):
    """FWX_PERK_TEMPORAL_MIB values that put the split inside a slab of `slab_bytes`: none (all nt), a
    tail smaller than one workgroup's 4 rows, half and a third of the slab."""
    return ["0", "0.001", repr(slab_bytes / 2 / MIB), repr(slab_bytes / 3 / MIB)]


def _oracle(rate, nxt, hops, k_begin, k_end):
    er = rate.copy()
    en = None if nxt is None else nxt.copy()
    eh = None if hops is None else hops.copy()
    u = oracle.relax_mt(er, en, k_begin, k_end, threads=16, hops=eh, fast=True)
    return er, en, eh, u


def _updates_in_rows(rate, nxt, k0, k1, lo, hi):
    """Updates the oracle makes in rows [lo, hi) over pivots [k0, k1) (in place on rate / nxt): an update
    strictly raises an entry, so per step it is the number of entries of those rows that changed."""
    u = 0
    for k in range(k0, k1):
        before = rate[lo:hi].copy()
        oracle.relax(rate, nxt, None, k, k + 1)
        u += int(np.count_nonzero(rate[lo:hi] != before))
    return u


def _check_solve(rate, nxt, hops, want, **kw):
    er, en, eh, eu = want
    gr = rate.copy()
    gn = None if nxt is None else nxt.copy()
    gh = None if hops is None else hops.copy()
    u = engine.solve(gr, gn, gh, engine=engine.FWX_ENGINE_PERK, count_updates=True, **kw)
    assert_bits_equal(gr, er, "rate %r" % (kw,))
    if nxt is not None:
        assert np.array_equal(gn, en), "next %r" % (kw,)
    if hops is not None:
        assert np.array_equal(gh, eh), "hops %r" % (kw,)
    assert u == eu, kw


@pytest.mark.parametrize("fields", ["rates", "next", "next+hops"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [1000, 1024, 1030, 2052])
def test_split_solves_equal_the_oracle(n, dtype, fields, monkeypatch):
    """n = 1030 is not a multiple of the vector width (scalar relax_k); n = 2052 runs several strips.
    An odd k_begin puts the first launch in the reversed direction."""
    rate, nxt, hops = synth.make("d1", n, dtype, seed=n + 5)
    if fields == "rates":
        nxt = hops = None
    elif fields == "next":
        hops = None
    elif hops is None:
        hops = (nxt >= 0).astype(np.int32)
    kb, ke = 7, 7 + (300 if n > 2000 else n // 2)
    want = _oracle(rate, nxt, hops, kb, ke)
    slab = n * n * np.dtype(dtype).itemsize
    for budget in _budgets(slab) + [ALL_DEFAULT]:
        monkeypatch.setenv("FWX_PERK_TEMPORAL_MIB", budget)
        for serp in (True, False):
            _check_solve(rate, nxt, hops, want, k_begin=kb, k_end=ke, serpentine=serp)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_whole_solve_with_the_split_in_the_middle(dtype, monkeypatch):
    n = 1024
    rate, nxt, _ = synth.make("d1", n, dtype, seed=77)
    hops = (nxt >= 0).astype(np.int32)
    want = _oracle(rate, nxt, hops, 0, n)
    monkeypatch.setenv("FWX_PERK_TEMPORAL_MIB", repr(n * n * np.dtype(dtype).itemsize / 2 / MIB))
    _check_solve(rate, nxt, hops, want)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_hostile_inputs_under_the_split(dtype, monkeypatch):
    """Zeros of both signs, subnormals, overflowing products, infinities, NaN, negatives."""
    rnd = np.random.default_rng(2052)
    for n in (1000, 1030):
        rate, nxt, hops = hostile_matrix(rnd, n, dtype)
        kb, ke = 3, 3 + 180
        want = _oracle(rate, nxt, hops, kb, ke)
        for budget in _budgets(n * n * np.dtype(dtype).itemsize):
            monkeypatch.setenv("FWX_PERK_TEMPORAL_MIB", budget)
            for serp in (True, False):
                _check_solve(rate, nxt, hops, want, k_begin=kb, k_end=ke, serpentine=serp)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_row_slabs_and_skipped_rows_under_the_split(dtype, monkeypatch):
    """fwx_dev_relax_skip on a row slab that does not start at row 0 (pivot rows from time-k
    snapshots), with and without a skipped row range inside it; the budget is sized to the slab."""
    n, lo, hi, k0, k1 = 1024, 256, 1024, 301, 365
    rate, nxt, _ = synth.make("d2", n, dtype, seed=41)
    want_r, want_n = rate.copy(), nxt.copy()
    # U of the slab = the oracle's updates in rows [lo, hi)
    su = _updates_in_rows(rate.copy(), nxt.copy(), k0, k1, lo, hi)
    assert su == oracle.relax(want_r, want_n, None, k0, k1) - _updates_in_rows(rate.copy(), nxt.copy(), k0, k1, 0, lo)
    slab = (hi - lo) * n * np.dtype(dtype).itemsize
    for budget in _budgets(slab):
        monkeypatch.setenv("FWX_PERK_TEMPORAL_MIB", budget)
        for serp in (True, False):
            for skip in (None, (64, 128)):
                full_t, full_n = dev(rate), dev(nxt)
                w = dev_empty((k1 - k0, n), dtype)
                engine.dev_panel_snap(full_t[k0:k1], n, k0, w)
                r_t, n_t = dev(rate[lo:hi]), dev(nxt[lo:hi])
                upd = dev_zeros((engine.FWX_UPDATE_SHARDS,), np.int64)
                engine.dev_relax(r_t, n, lo, k0, k1, pivots_t=w, next_t=n_t, serpentine=serp,
                                 updates_t=upd, skip=skip)
                got_r, got_n = host(r_t), host(n_t)
                keep = np.ones(hi - lo, dtype=bool)
                if skip:
                    keep[skip[0]:skip[1]] = False
                    assert_bits_equal(got_r[~keep], rate[lo:hi][~keep], "skipped rows")
                assert_bits_equal(got_r[keep], want_r[lo:hi][keep], "slab rate %s %s %s" % (budget, serp, skip))
                assert np.array_equal(got_n[keep], want_n[lo:hi][keep])
                if skip is None:
                    assert int(host(upd).sum()) == su


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_update_counts_of_a_whole_slab(dtype, monkeypatch):
    """A slab that is the whole matrix, pivots read in place: U equals the oracle's exactly."""
    n = 1030
    rate, nxt, _ = synth.make("d1", n, dtype, seed=19)
    want_r, want_n = rate.copy(), nxt.copy()
    eu = oracle.relax(want_r, want_n, None, 0, n)
    for budget in ("0", repr(n * n * np.dtype(dtype).itemsize / 2 / MIB)):
        monkeypatch.setenv("FWX_PERK_TEMPORAL_MIB", budget)
        r_t, n_t = dev(rate), dev(nxt)
        upd = dev_zeros((engine.FWX_UPDATE_SHARDS,), np.int64)
        engine.dev_relax(r_t, n, 0, 0, n, next_t=n_t, updates_t=upd)
        assert_bits_equal(host(r_t), want_r, "rate")
        assert np.array_equal(host(n_t), want_n)
        assert int(host(upd).sum()) == eu


@pytest.mark.parametrize("dtype,n", [(np.float32, 1030), (np.float64, 1024)])
def test_path_trace_under_the_split(dtype, n, monkeypatch):
    """The traced per-k solve: rates, next-hops and U equal the oracle's, and the exact `_path` lists
    rebuilt from the trace equal those of the all-default-policy run."""
    rate, nxt, _ = synth.make("t1", n, dtype, seed=23)
    er, en = rate.copy(), nxt.copy()
    eu = oracle.relax(er, en)
    rnd = np.random.default_rng(n)
    src = rnd.integers(0, n, 3000).astype(np.int32)
    dst = rnd.integers(0, n, 3000).astype(np.int32)
    lists = {}
    for budget in (ALL_DEFAULT, "0", "0.001", repr(n * n * np.dtype(dtype).itemsize / 2 / MIB)):
        monkeypatch.setenv("FWX_PERK_TEMPORAL_MIB", budget)
        with engine.DeviceMatrix(n, dtype, with_next=True) as dm:
            dm.enable_path_log()
            dm.upload(rate, nxt)
            u = dm.solve(engine=engine.FWX_ENGINE_PERK, count_updates=True)
            assert u == eu == dm.path_log_count()
            gr, gn, _ = dm.download()
            assert_bits_equal(gr, er, "traced rate, budget " + budget)
            assert np.array_equal(gn, en)
            lists[budget] = dm.query_exact_batch(src, dst, cap=4 * n)
    for budget, got in lists.items():
        assert got == lists[ALL_DEFAULT], budget
