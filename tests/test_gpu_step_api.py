"""The device-pointer step API of include/fwx.h on slabs, pinned bit for bit to the CPU oracle: fwx_dev_relax[_skip],
fwx_dev_panel, fwx_dev_panel_snap, fwx_dev_relax_fused[_skip], fwx_dev_check_nonneg, fwx_pivots.next and FWX_FLAG_NONNEG,
with the caller choosing row0, rows, the pass, the skip range, the scratch pointers and the domain flag.

1. One pass on one slab (tests/step_api_worker.py has the case runner and the reference, helpers.pass_reference): f32 and
   f64, every field set, slabs above / below / around the pass, cut through the pivot block, off every grain, short and
   unaligned passes -- fused and per-k, the per-k kernel's scalar instantiation included (n = 261 / 259).
2. Skip ranges through the public calls, and the refusals of check_slab / the argument checks, nothing written.
3. The large-tile forms on slabs, in child processes (the tile thresholds are read once per process).
4. Whole solves built from the public calls alone: a fused partitioned schedule with look-ahead whose stacked traces
   give all n^2 exact `_path` lists of the rope oracle; a per-k solve outside the domain with fwx_pivots.next;
   fwx_dev_panel on short blocks and on a hostile block.
5. Scratch and slabs off 16-byte alignment: the element-wise staging loops of the max-form and arg kernels
   (ct_vec == 0) and the scalar domain check.

Every case asserts, before it looks at the device result, that the oracle changes what the case compares (teeth), and
through fwx_test_kernel_forms that the launch form it is about ran.  The seeds below are the first of 1, 2, 3, ... for
which every case of this file has teeth (decided by the oracle alone: worker.teeth)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from floydwarshall_amd import _lib, engine, hip, synth

import step_api_worker as worker
from helpers import (assert_bits_equal, dev, dev_empty, dev_zeros, host, pass_reference, path_from_trace)
from hostile_inputs import hostile_matrix, market_rates

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = ("f32", "f64")
NP_DTYPE = {"f32": np.float32, "f64": np.float64}

# seed per (kind, dtype): the first of 1, 2, 3, ... with which EVERY one-pass, skip, large-tile and unaligned case of
# this file has teeth (tests/step_api_worker.py teeth(): rates, next-hops and trace entries change in the rows relaxed
# and, with a skip range, in the rows skipped)
SEEDS = {("d2", "f32"): 1, ("d2", "f64"): 1, ("t1", "f32"): 1, ("t1", "f64"): 1,
         ("hostile", "f32"): 1, ("hostile", "f64"): 1}

# (row0, rows, k0, bt) at n = 260 = 2 * 128 + 4: 65 f32 vectors, a pivot tail of 4
GEOMETRIES = [
    (0, 64, 64, 64), (128, 64, 0, 64), (0, 260, 192, 64),         # the slab above, below and around the pass
    (64, 64, 0, 64),                                              # exactly the next panel's rows: the look-ahead launch
    (100, 67, 64, 64), (61, 40, 64, 64),                          # part of the pivot block at the slab's start / end
    (3, 129, 128, 64), (127, 133, 0, 64), (252, 8, 192, 64), (259, 1, 0, 64),     # off every grain
    (0, 260, 256, 4), (0, 260, 128, 1), (4, 213, 96, 48), (4, 213, 37, 27),       # short and unaligned passes
]
# one of each group, scaled by hand to the orders that take the per-k kernel's scalar instantiation
GEOMETRIES_SCALAR = {
    261: [(0, 64, 64, 64), (64, 64, 0, 64), (100, 67, 64, 64), (3, 129, 128, 64), (260, 1, 0, 64), (0, 261, 256, 5),
          (4, 213, 37, 27)],
    259: [(128, 64, 0, 64), (64, 64, 0, 64), (61, 40, 64, 64), (127, 132, 0, 64), (258, 1, 0, 64), (0, 259, 256, 3),
          (4, 213, 37, 27)],
}
FUSED_FIELDS = ("r", "ru", "n", "nh", "nhu", "nt")
UNCOUNTED = ("r", "n", "nh", "nt")
PERK_FIELDS = ("n", "nh", "nhu")


def _case(kind, n, dt, fields, geo, eng, **extra):
    row0, rows, k0, bt = geo
    return dict(kind=kind, n=n, dtype=dt, fields=fields, seed=SEEDS[(kind, dt)], row0=row0, rows=rows, k0=k0, bt=bt,
                engine=eng, **extra)


def fused_cases(n, geo, dt, fields=FUSED_FIELDS, **extra):
    """Every field set on t1 (ties) and d2, without the flag and -- uncounted fields -- with it; the hostile draw for
    r / ru (with next-hops the fused kernels require the domain by contract)."""
    out = []
    for kind in ("t1", "d2"):
        for f in fields:
            out.append(_case(kind, n, dt, f, geo, "fused", nonneg=False, **extra))
            if f in UNCOUNTED:
                out.append(_case(kind, n, dt, f, geo, "fused", nonneg=True, **extra))
    out += [_case("hostile", n, dt, f, geo, "fused", nonneg=False, **extra) for f in fields if f in ("r", "ru")]
    return out


def perk_cases(n, geo, dt, fields=PERK_FIELDS, **extra):
    """t1 and d2 with NULL fwx_pivots.next (the caller vouches for the domain), the hostile draw with the next-hop
    panel."""
    return [_case(kind, n, dt, f, geo, "perk", **extra) for kind in ("t1", "d2", "hostile") for f in fields]


def _stop_on_device_error(e):
    if worker.is_device_error(e):
        pytest.exit("HIP error in tests/test_gpu_step_api.py: stopping the GPU tests\n%r" % (e,), returncode=3)


def _run(cases, **thresholds):
    """The cases in this process: no mismatch, and every case reached the forms it is about."""
    try:
        results = worker.run_cases(cases)
    except Exception as e:
        _stop_on_device_error(e)
        raise
    _check(results, **thresholds)


def _check(results, **thresholds):
    bad = []
    for res in results:
        c, forms = res["case"], set(res["forms"])
        want = worker.expected_forms(c, **thresholds)
        if res["error"]:
            bad.append("%r: %s" % (c, res["error"]))
        elif not want <= forms:
            bad.append("%r: forms %s not reached (saw %s)" % (c, sorted(want - forms), sorted(forms)))
    assert not bad, "%d of %d cases:\n%s" % (len(bad), len(results), "\n".join(bad[:12]))


_IDS = ["%d-%d-%d-%d" % g for g in GEOMETRIES]


# ---- 1. one pass on one slab --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("geo", GEOMETRIES, ids=_IDS)
def test_fused_pass_on_a_slab(geo, dt):
    _run(fused_cases(260, geo, dt))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("geo", GEOMETRIES, ids=_IDS)
def test_perk_pass_on_a_slab(geo, dt):
    _run(perk_cases(260, geo, dt))


@pytest.mark.parametrize("n,dt", [(261, "f32"), (259, "f64")])
def test_perk_pass_scalar_instantiation(n, dt):
    """Rows that are no multiple of 16 bytes: relax_k<T, 1, ...> with next-hops and hops."""
    assert n % (16 // np.dtype(NP_DTYPE[dt]).itemsize) != 0
    for geo in GEOMETRIES_SCALAR[n]:
        _run(perk_cases(n, geo, dt))


# ---- 2. skip ranges, refusals -----------------------------------------------------------------------------------------
SKIP_SLABS = [(4, 213, 96, 48), (0, 260, 96, 48)]
SKIP_FIELDS = ("r", "ru", "n", "nh", "nhu")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("geo", SKIP_SLABS, ids=["slab", "whole"])
def test_fused_skip_range(geo, dt):
    """All but the ragged tail skipped, a range in the middle (rows above and below it are relaxed), and an empty
    range with unaligned ends."""
    for skip in ((0, geo[1] & ~7), (64, 128), (6, 6)):
        _run(fused_cases(260, geo, dt, fields=SKIP_FIELDS + ("nt",), skip=list(skip)))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("geo", SKIP_SLABS, ids=["slab", "whole"])
def test_perk_skip_range(geo, dt):
    for skip in ((0, 8), (64, 128), (208, 212), (200, 208), (6, 6)):
        _run(perk_cases(260, geo, dt, fields=SKIP_FIELDS, skip=list(skip)))


def _ptr(t):
    return None if t is None else t.data_ptr()


def _status_fused(rate_t, n, row0, k0, k1, w_t, ws, *, next_t=None, hops_t=None, wh_t=None, trace=None, skip=(0, 0),
                  stride=None):
    """fwx_dev_relax_fused_skip with exactly these pointers: its status."""
    s, p, sc = _lib.FwxSlab(), _lib.FwxPivots(), _lib.FwxFusedScratch()
    s.n, s.row0, s.rows, s.dtype = n, row0, rate_t.shape[0], engine._tensor_dtype_code(rate_t)
    s.rate, s.next, s.hops = _ptr(rate_t), _ptr(next_t), _ptr(hops_t)
    p.k_begin, p.k_end, p.rate, p.hops, p.stride = k0, k1, _ptr(w_t), _ptr(wh_t), n if stride is None else stride
    sc.col_rate, sc.col_next, sc.col_hops = _ptr(ws.ct), _ptr(ws.cnt), _ptr(ws.cht)
    tr = ctypes.byref(trace.c_struct()) if trace is not None else None
    return _lib.lib().fwx_dev_relax_fused_skip(ctypes.byref(s), ctypes.byref(p), ctypes.byref(sc), tr, None, 0,
                                               skip[0], skip[1], hip.default_stream().ptr)


def _status_perk(rate_t, n, row0, k0, k1, w_t, *, next_t=None, hops_t=None, wh_t=None, skip=(0, 0)):
    s, p = _lib.FwxSlab(), _lib.FwxPivots()
    s.n, s.row0, s.rows, s.dtype = n, row0, rate_t.shape[0], engine._tensor_dtype_code(rate_t)
    s.rate, s.next, s.hops = _ptr(rate_t), _ptr(next_t), _ptr(hops_t)
    p.k_begin, p.k_end, p.rate, p.hops, p.stride = k0, k1, _ptr(w_t), _ptr(wh_t), n
    return _lib.lib().fwx_dev_relax_skip(ctypes.byref(s), ctypes.byref(p), 1, None, skip[0], skip[1],
                                         hip.default_stream().ptr)


@pytest.mark.parametrize("dt", DTYPES)
def test_refusals_write_nothing(dt):
    """Each call returns the FWX_ERR_INVALID its argument check gives, and no array on the device changes."""
    n, row0, rows, k0, k1 = 260, 4, 213, 96, 144
    (rate, nxt, hops), ref = worker.reference("d2", n, np.dtype(NP_DTYPE[dt]).name, SEEDS[("d2", dt)], k0, k1 - k0)
    r_t, n_t, h_t = dev(rate), dev(nxt), dev(hops)
    tr = engine.Trace(n, n)
    w, wh = dev(ref.W), dev(ref.WH)
    w65, wh65 = dev_zeros((65, n), rate.dtype), dev_zeros((65, n), np.int32)
    ws = worker.fused_scratch(rows, rate.dtype, True, True)
    sl = slice(row0, row0 + rows)
    full = dict(next_t=n_t[sl], hops_t=h_t[sl], wh_t=wh, trace=tr.rows(row0, row0 + rows))
    INVALID = _lib.FWX_ERR_INVALID
    assert _status_fused(r_t[sl], n, row0, k0, k1, w, ws, skip=(4, 12), **full) == INVALID      # not multiples of 8
    assert _status_fused(r_t[sl], n, row0, k0, k1, w, ws, skip=(208, 216), **full) == INVALID   # skip_hi > rows
    assert _status_fused(r_t[sl], n, row0, k0, k0 + 65, w65, ws, next_t=n_t[sl], hops_t=h_t[sl], wh_t=wh65) == INVALID
    assert _status_fused(r_t[sl], n, row0, k0, k1, w, ws, stride=n + 4, **full) == INVALID
    assert _status_fused(r_t[sl], n, row0, k0, k1, w, ws, trace=tr.rows(row0, row0 + rows)) == INVALID   # no next
    assert _status_fused(r_t[sl], n, row0, k0, k1, w, ws, next_t=n_t[sl], hops_t=h_t[sl]) == INVALID     # no piv->hops
    assert _status_perk(r_t[sl], n, row0, k0, k1, w, next_t=n_t[sl], hops_t=h_t[sl], wh_t=wh, skip=(2, 8)) == INVALID
    assert _status_perk(r_t[sl], n, row0, k0, k1, w, next_t=n_t[sl], hops_t=h_t[sl], wh_t=wh, skip=(212, 216)) == INVALID
    assert _status_perk(r_t[sl], n, row0, k0, k1, w, next_t=n_t[sl], hops_t=h_t[sl]) == INVALID          # no piv->hops
    assert _status_perk(r_t[sl], n, row0, k0, k1, w, hops_t=h_t[sl], wh_t=wh) == INVALID                 # hops, no next
    # rows that are no multiple of 16 bytes: the fused call refuses an order the per-k call takes
    odd = 261
    ro_t, wo_t = dev_zeros((64, odd), rate.dtype), dev_zeros((64, odd), rate.dtype)
    assert _status_fused(ro_t, odd, 0, 0, 64, wo_t, worker.fused_scratch(64, rate.dtype, False, False)) == INVALID
    assert not host(ro_t).any()
    # the accepted twins of the first two, so that the refusals above are about the argument they name
    assert _status_fused(r_t[sl], n, row0, k0, k1, w, ws, skip=(8, 16), **full) == 0
    hip.default_stream().synchronize()
    done = np.zeros(n, dtype=bool)
    done[row0:row0 + 8] = done[row0 + 16:row0 + rows] = True
    pick = lambda after, before: np.where(done[:, None], after, before)  # noqa: E731
    none = np.full((n, n), -1, dtype=np.int32)
    assert_bits_equal(host(r_t), pick(ref.rate, rate), "rate")
    assert_bits_equal(host(n_t), pick(ref.next, nxt), "next")
    assert_bits_equal(host(h_t), pick(ref.hops, hops), "hops")
    assert_bits_equal(host(tr.last), pick(ref.last, none), "last")
    assert_bits_equal(host(tr.at_col), pick(ref.at_col, none), "at_col")
    assert_bits_equal(host(tr.at_row), none, "at_row")
    assert_bits_equal(host(w), ref.W, "w")
    assert_bits_equal(host(wh), ref.WH, "wh")
    assert not host(w65).any() and not host(wh65).any()


# ---- 3. the large-tile forms on slabs: child processes ------------------------------------------------------------------
LARGE = {"FWX_SMALL_TILES_BELOW": "0", "FWX_MID_TILES_BELOW": "0", "FWX_ARG_SMALL_TILES_BELOW": "0"}
KNOBS = tuple(LARGE) + ("FWX_DOUBLE_PASS_MIN_N", "FWX_DOUBLE_PASS_NEXT_MIN_N", "FWX_LOOKAHEAD_MIN_N",
                        "FWX_ARG_GENERAL_STAGING", "FWX_ARG_F64_SHORT_TILES", "FWX_PANELS_TIGHT", "FWX_PANELS_32_ROWS",
                        "FWX_SPLIT_MAIN", "FWX_SYMMETRIC_MIN_N")
# slabs of 8, 127, 128, 133 and 200 rows: below, at and just past one 128-row tile, and two ragged tiles
LARGE_GEOMETRIES = {
    260: [(252, 8, 192, 64), (3, 127, 64, 64), (128, 128, 0, 64), (127, 133, 256, 4), (60, 200, 64, 64)],
    452: [(444, 8, 384, 64), (1, 127, 64, 64), (320, 128, 128, 64), (319, 133, 448, 4), (252, 200, 192, 64)],
}


def _run_child(env_over, cases, timeout):
    """One worker process; nothing more starts on the card if it dies by a signal, reports a HIP error or overruns."""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(env_over)
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "step_api_worker.py"), json.dumps(cases)],
                           env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        pytest.exit("step_api_worker overran %d s with %r: stopping the GPU tests" % (timeout, env_over), returncode=3)
    if r.returncode < 0 or r.returncode in (134, 139, worker.DEVICE_ERROR_STATUS):
        pytest.exit("step_api_worker ended with status %d (%r): stopping the GPU tests\n%s"
                    % (r.returncode, env_over, r.stderr[-3000:]), returncode=3)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("STEP_API_RESULT ")]
    assert r.returncode == 0 and line, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    return json.loads(line[-1][len("STEP_API_RESULT "):])


@pytest.mark.parametrize("n", sorted(LARGE_GEOMETRIES))
def test_large_tile_forms_on_slabs(n):
    """Every tile threshold 0: MAIN_LARGE_*, MAX_LARGE_F32, MAX_LARGE_F64, ARG_RI8_NP1_F32, ARG_F64_RI4_NP1."""
    cases = [c for geo in LARGE_GEOMETRIES[n] for dt in DTYPES for c in fused_cases(n, geo, dt)]
    _check(_run_child(LARGE, cases, 240), large=True)


def test_mid_tile_max_form_on_slabs():
    """FWX_MID_TILES_BELOW at its default: the f32 max form on 128 x 64 tiles, MAX_MID_F32."""
    env = {k: v for k, v in LARGE.items() if k != "FWX_MID_TILES_BELOW"}
    cases = [c for n in sorted(LARGE_GEOMETRIES) for geo in LARGE_GEOMETRIES[n]
             for c in fused_cases(n, geo, "f32", fields=("r",)) if c["nonneg"]]
    assert cases
    _check(_run_child(env, cases, 120), large=True, mid_default=True)


# ---- 4. whole solves from the public calls alone --------------------------------------------------------------------------
def _market(n, dtype):
    from oracle import list_faithful as lf
    n_ccy = 8
    m0 = lf.build_matrix(market_rates(-(-n // n_ccy) + 1, n_ccy, seed=23 + n), dtype)
    assert len(m0) >= n
    _, rate, nxt, hops = lf.to_dense(m0, dtype)          # the leading n vertices: a market on fewer vertices
    return tuple(np.ascontiguousarray(a[:n, :n]) for a in (rate, nxt, hops))


# the second set of bounds puts look-ahead rows on the fused skip grain (multiples of 8 inside their slab): with the
# first, no block of 48 pivots ever does, and every owner relaxes above and below its look-ahead rows instead
BOUNDS = {"ragged": (0, 61, 100, 233, 260), "on-grain": (0, 64, 104, 232, 260)}


@pytest.mark.parametrize("nonneg", [True, False], ids=["flag", "counting"])
@pytest.mark.parametrize("kind,bounds", [("t1", "ragged"), ("market", "ragged"), ("t1", "on-grain"), ("market", "on-grain")])
@pytest.mark.parametrize("dt", DTYPES)
def test_fused_partitioned_solve_and_lists(dt, kind, bounds, nonneg):
    """An emulated partitioned solve, rate + next + hops + trace, blocks of 48 pivots cut across owners, with the
    look-ahead schedule of dist.relax_skipping: the owners of the next block's rows relax those first (then their panel
    is taken), everyone sweeps its slab skipping them -- in one skip launch where they lie on the grain of 8, above and
    below them otherwise.  Rate, next, hops and U against oracle.relax, and from the stacked traces all n^2 exact
    `_path` lists against the rope oracle."""
    from oracle import list_ropes
    n, block, dtype = 260, 48, NP_DTYPE[dt]
    bounds = BOUNDS[bounds]
    rate, nxt, hops = _market(n, dtype) if kind == "market" else synth.make("t1", n, dtype, seed=41)
    er, en, eh = rate.copy(), nxt.copy(), hops.copy()
    eu = oracle.relax(er, en, eh)
    assert eu > 0
    r_t, n_t, h_t = dev(rate), dev(nxt), dev(hops)
    tr = engine.Trace(n, n)
    upd = None if nonneg else dev_zeros((engine.FWX_UPDATE_SHARDS,), np.int64)
    parts = len(bounds) - 1
    wss = [engine.FusedWorkspace(n, bounds[p + 1] - bounds[p], dtype, with_next=True, with_hops=True)
           for p in range(parts)]
    W = [dev_empty((engine.FWX_FUSED_BLOCK, n), dtype) for _ in range(2)]
    WH = [dev_empty((engine.FWX_FUSED_BLOCK, n), np.int32) for _ in range(2)]
    blocks = [(k0, min(k0 + block, n)) for k0 in range(0, n, block)]
    launches = {"skip": 0, "split": 0}

    def panel(b):
        k0, k1 = blocks[b]
        engine.dev_panel_snap(r_t[k0:k1], n, k0, W[b % 2][:k1 - k0], block_next_t=n_t[k0:k1], block_hops_t=h_t[k0:k1],
                              w_hops_t=WH[b % 2][:k1 - k0], trace=tr.rows(k0, k1))

    def relax(p, lo, hi, b, skip=None):          # rows [lo, hi) of partition p, pivots of block b
        if hi <= lo:
            return
        k0, k1 = blocks[b]
        engine.dev_relax_fused(r_t[lo:hi], n, lo, k0, k1, W[b % 2][:k1 - k0], wss[p], next_t=n_t[lo:hi],
                               hops_t=h_t[lo:hi], wh_t=WH[b % 2][:k1 - k0], trace=tr.rows(lo, hi), updates_t=upd,
                               nonneg=nonneg, skip=skip)

    try:
        panel(0)
        for b in range(len(blocks)):
            ahead = {}
            if b + 1 < len(blocks):
                for p in range(parts):
                    lo, hi = max(bounds[p], blocks[b + 1][0]), min(bounds[p + 1], blocks[b + 1][1])
                    if lo < hi:
                        relax(p, lo, hi, b)
                        ahead[p] = (lo, hi)
                panel(b + 1)
            for p in range(parts):
                s0, s1 = bounds[p], bounds[p + 1]
                if p not in ahead:
                    relax(p, s0, s1, b)
                elif (ahead[p][0] - s0) % 8 == 0 and (ahead[p][1] - s0) % 8 == 0:
                    relax(p, s0, s1, b, skip=(ahead[p][0] - s0, ahead[p][1] - s0))
                    launches["skip"] += 1
                else:
                    relax(p, s0, ahead[p][0], b)
                    relax(p, ahead[p][1], s1, b)
                    launches["split"] += 1
        got = host(r_t), host(n_t), host(h_t)
        last, at_col, at_row = host(tr.last), host(tr.at_col), host(tr.at_row)
        u = None if nonneg else int(host(upd).sum())
    except Exception as e:
        _stop_on_device_error(e)
        raise
    assert launches["split"] > 0 and (launches["skip"] > 0) == (bounds == BOUNDS["on-grain"]), launches
    assert_bits_equal(got[0], er, "rate")
    assert_bits_equal(got[1], en, "next")
    assert_bits_equal(got[2], eh, "hops")
    assert u is None or u == eu, (u, eu)
    ropes = list_ropes.solve(rate, nxt)
    assert_bits_equal(ropes.rate, er, "rope oracle vs dense oracle: rate")
    want = ropes.all_paths()
    walks_differ = 0
    for i in range(n):
        for j in range(n):
            path = path_from_trace(last, at_col, at_row, nxt, i, j)
            assert tuple(path) == tuple(want[i][j]), "exact list (%d, %d): %r vs %r" % (i, j, path, want[i][j])
            walks_differ += len(path) != (1 if nxt[i, j] >= 0 else 0)
    assert walks_differ > 0, "no list of this solve was ever concatenated"


HOSTILE_SOLVE_SEED = {"f32": 1, "f64": 1}       # first seed of 1, 2, ... whose solve has an update with an empty ikPath


@pytest.mark.parametrize("dt", DTYPES)
def test_perk_solve_outside_the_domain_with_pivot_next(dt):
    """A hostile draw with next-hops and hops on three slabs, blocks of ONE row: fwx_dev_panel on the owner's row gives
    the snapshot, a device copy of the owner's live next-hop row stands in for the broadcast of fwx_pivots.next (step
    k leaves row k alone), every slab relaxes with the three.  Teeth: some update of the solve has next[i][k] < 0 at
    its step -- the case fwx_pivots.next exists for."""
    n, bounds, dtype = 68, (0, 23, 45, 68), NP_DTYPE[dt]
    rate, nxt, hops = hostile_matrix(np.random.default_rng(HOSTILE_SOLVE_SEED[dt]), n, dtype)
    ref = pass_reference(rate, nxt, hops, 0, n)
    eu = int(ref.u_rows.sum())
    assert _updates_with_empty_left(rate, nxt, hops) > 0, "no update of this solve has an empty ikPath"
    slabs = [tuple(dev(a[bounds[p]:bounds[p + 1]]) for a in (rate, nxt, hops)) for p in range(3)]
    upd = dev_zeros((engine.FWX_UPDATE_SHARDS,), np.int64)
    w, wh = dev_empty((1, n), dtype), dev_empty((1, n), np.int32)
    try:
        engine.kernel_forms_seen(reset=True)
        for k in range(n):
            owner = max(p for p in range(3) if bounds[p] <= k)
            r_o, n_o, h_o = (t[k - bounds[owner]:k - bounds[owner] + 1] for t in slabs[owner])
            engine.dev_panel(r_o, n, k, w, next_t=n_o, hops_t=h_o, w_hops_t=wh, updates_t=upd)
            wn = n_o.clone()
            for p in range(3):
                engine.dev_relax(slabs[p][0], n, bounds[p], k, k + 1, pivots_t=w, pivot_hops_t=wh, pivot_next_t=wn,
                                 next_t=slabs[p][1], hops_t=slabs[p][2], updates_t=upd)
        got = [np.concatenate([host(s[f]) for s in slabs]) for f in range(3)]
        u = int(host(upd).sum())
        assert "RELAX_K" in engine.kernel_forms_seen(reset=True)
    except Exception as e:
        _stop_on_device_error(e)
        raise
    assert_bits_equal(got[0], ref.rate, "rate")
    assert_bits_equal(got[1], ref.next, "next")
    assert_bits_equal(got[2], ref.hops, "hops")
    assert u == eu, (u, eu)


def _updates_with_empty_left(rate, nxt, hops, k0=0, k1=None):
    """Updates of the pivots [k0, k1) whose ikPath is empty (next[i][k] < 0 at the start of step k), by the oracle."""
    r, nx, hp = rate.copy(), nxt.copy(), hops.copy()
    it = np.uint64 if r.dtype.itemsize == 8 else np.uint32
    count = 0
    for k in range(k0, r.shape[0] if k1 is None else k1):
        before, empty = r.view(it).copy(), nx[:, k] < 0
        oracle.relax(r, nx, hp, k, k + 1)
        count += int(((r.view(it) != before) & empty[:, None]).sum())
    return count


def _panel_block(rate, nxt, hops, k0, bt):
    """fwx_dev_panel on the rows [k0, k0 + bt) of the uploaded state: (rate, next, hops of the whole matrix, w, w_hops,
    U) afterwards."""
    n = rate.shape[0]
    r_t, n_t, h_t = dev(rate), dev(nxt), dev(hops)
    w, wh = dev_empty((bt, n), rate.dtype), dev_empty((bt, n), np.int32)
    upd = dev_zeros((engine.FWX_UPDATE_SHARDS,), np.int64)
    try:
        engine.kernel_forms_seen(reset=True)
        engine.dev_panel(r_t[k0:k0 + bt], n, k0, w, next_t=n_t[k0:k0 + bt], hops_t=h_t[k0:k0 + bt], w_hops_t=wh,
                         updates_t=upd)
        out = host(r_t), host(n_t), host(h_t), host(w), host(wh), int(host(upd).sum())
        assert "RELAX_K" in engine.kernel_forms_seen(reset=True)
    except Exception as e:
        _stop_on_device_error(e)
        raise
    return out


def _check_panel_block(state, ref, k0, bt, got):
    """The block's rows are at time k0 + bt, every other row keeps its bits; w / w_hops are the snapshots; U is the
    block's."""
    inside = np.zeros(state[0].shape[0], dtype=bool)
    inside[k0:k0 + bt] = True
    for g, after, before, what in zip(got[:3], (ref.rate, ref.next, ref.hops), state, ("rate", "next", "hops")):
        assert_bits_equal(g, np.where(inside[:, None], after, before), what)
    assert_bits_equal(got[3], ref.W, "w")
    assert_bits_equal(got[4], ref.WH, "w_hops")
    assert got[5] == int(ref.u_rows[inside].sum()), (got[5], int(ref.u_rows[inside].sum()))


@pytest.mark.parametrize("k0,bt", [(64, 32), (100, 20), (256, 4)])
@pytest.mark.parametrize("dt", DTYPES)
def test_dev_panel_short_blocks(dt, k0, bt):
    """fwx_dev_panel with next + hops + w_hops + U on blocks shorter than 64 and on the pivot tail, in the domain."""
    state, ref = worker.reference("t1", 260, np.dtype(NP_DTYPE[dt]).name, SEEDS[("t1", dt)], k0, bt)
    inside = slice(k0, k0 + bt)
    assert (ref.next[inside] != state[1][inside]).any() and (ref.hops[inside] != state[2][inside]).any()
    _check_panel_block(state, ref, k0, bt, _panel_block(*state, k0, bt))


HOSTILE_PANEL_SEED = {"f32": 1, "f64": 1}       # first seed of 1, 2, ... whose block has an update with an empty ikPath


@pytest.mark.parametrize("dt", DTYPES)
def test_dev_panel_hostile_block(dt):
    """Outside the domain fwx_dev_panel follows the list rule in full: an update inside the block whose ikPath is empty
    (next[i][k] < 0) takes next[k][j] -- the block's own row k, which step k leaves alone."""
    n, k0, bt = 68, 16, 16
    state, ref = worker.reference("hostile", n, np.dtype(NP_DTYPE[dt]).name, HOSTILE_PANEL_SEED[dt], k0, bt)
    inside = np.zeros(n, dtype=bool)
    inside[k0:k0 + bt] = True
    # teeth: an update of a block row by a block pivot with an empty ikPath whose kjPath is not empty -- storing
    # next[i][k] = -1 there instead of next[k][j] would go unnoticed otherwise
    r, nx, hp = (a.copy() for a in state)
    it = np.uint64 if r.dtype.itemsize == 8 else np.uint32
    telling = 0
    for k in range(k0, k0 + bt):
        before, empty = r.view(it).copy(), nx[:, k] < 0
        row_k = nx[k].copy()
        oracle.relax(r, nx, hp, k, k + 1)
        hit = (r.view(it) != before) & empty[:, None] & (row_k >= 0)[None, :] & inside[:, None]
        telling += int(hit.sum())
    assert telling > 0, "no update of a block row has an empty ikPath and a non-empty kjPath"
    _check_panel_block(state, ref, k0, bt, _panel_block(*state, k0, bt))


# ---- 5. scratch and slabs off 16-byte alignment -----------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("geo", [(0, 260, 192, 64), (3, 129, 128, 64), (4, 213, 37, 27)], ids=["whole", "3-129", "4-213"])
def test_fused_scratch_off_16_bytes(geo, dt):
    """ct, cnt and cht one element past a 16-byte boundary: the column panel's stores are element-wise, and the max-form
    and arg kernels then stage the pivot columns through their element-wise loops (ct_vec == 0) -- every access on
    that path is a scalar one or guarded by the alignment test, so the call is valid."""
    cases = [c for c in fused_cases(260, geo, dt, fields=("r", "nh"), offset=1) if c["nonneg"]]
    assert len(cases) == 4
    _run(cases)


def test_domain_bits_of_an_unaligned_slab():
    """fwx_dev_check_nonneg on rows [1, 261) of an n = 261 f32 matrix (4 bytes off 16-byte alignment: the scalar kernel):
    one NaN, one -0.0 and one orphan next-hop in the first, a middle and the last element of the slab, one at a
    time; a NaN in row 0, outside the slab, is not seen."""
    n = 261
    rate, nxt, _ = synth.make("d2", n, np.float32, seed=9)
    first, mid, last = (1, 0), (130, 131), (n - 1, n - 1)
    try:
        def bits(r, nx):
            r_t, n_t = dev(r), dev(nx)
            assert r_t[1:n].data_ptr() % 16 == 4 and n_t[1:n].data_ptr() % 16 == 4
            return engine.dev_domain_bits(r_t[1:n], n, 1, n_t[1:n]), engine.dev_domain_bits(r_t[1:n], n, 1)
        assert bits(rate, nxt) == (3, 3)
        r = rate.copy()
        r[0, 5] = np.nan
        r[0, n - 1] = -1.0
        assert bits(r, nxt) == (3, 3)
        for at in (first, mid, last):
            for value in (np.float32(np.nan), np.float32(-0.0), np.float32(-2.0)):
                r, nx = rate.copy(), nxt.copy()
                r[at], nx[at] = value, at[1]              # (the diagonal has no path: give it one, so only D1 breaks)
                assert bits(r, nx) == (2, 2), (at, value)
            r, nx = rate.copy(), nxt.copy()
            r[at], nx[at] = 0.5, -1                       # a positive rate without a path
            assert bits(r, nx) == (1, 3), at
            r[at] = 0.0                                   # no route: rate 0.0 and no path is inside the domain
            assert bits(r, nx) == (3, 3), at
    except Exception as e:
        _stop_on_device_error(e)
        raise
