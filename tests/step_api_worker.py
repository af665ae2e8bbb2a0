"""One pass of the device step API on one slab, against the one-pass reference (helpers.pass_reference): the cases of
tests/test_gpu_step_api.py.  No test functions here.  The test module imports run_case for the cases it runs in its
own process; for the large-tile forms it starts this module as a child process, because the tile thresholds of the
fused engine are read once per process: the knobs in the environment, a JSON list of cases as argv[1], one child at a
time.  The child prints one line, STEP_API_RESULT and a JSON list: per case an error message or null and the launch
forms seen.  It imports numpy, the oracle and floydwarshall_amd only -- never torch.

A case: {"kind": d2 | t1 | hostile, "n", "dtype": f32 | f64, "fields", "seed", "row0", "rows", "k0", "bt",
"engine": fused | perk, "nonneg": bool, "skip": [lo, hi] or null, "offset": elements by which the fused scratch is
moved off a 16-byte boundary}.  fields as in kernel_forms_worker.py: r (rates), ru (rates, counting U), n (+ next),
nh (+ next + hops), nhu (+ next + hops, counting U), nt (+ next + path trace).

What a case does.  The whole matrix at time k0 (state_at) is uploaded; the slab is a row view of it.
(1) fused cases without a skip range: fwx_dev_panel_snap on the rows [k0, k0 + bt) -- w, w_hops and the trace's at_row
    rows against the reference's W / WH / at_row, the matrix and `last` unchanged.
(2) fwx_dev_relax_fused[_skip] or fwx_dev_relax[_skip] on the slab, fed the REFERENCE panel so that a wrong panel cannot
    mask a wrong sweep: rate, next, hops, last and at_col of the slab's rows outside the skip range equal the reference
    at time k0 + bt, every other cell of every array keeps its uploaded bits, and the 256 U shards sum to the
    reference's updates in the rows relaxed.
Teeth, decided on the oracle alone before the device result is looked at: the rows relaxed differ from the upload in
rate, for fields with next in at least one next entry, for nt at least one `last` entry is >= 0; and with a skip range
the same holds for the rows skipped (they would have changed)."""
import functools
import json
import os
import sys
import traceback
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import oracle  # noqa: E402
from floydwarshall_amd import engine, hip, synth  # noqa: E402

from helpers import assert_bits_equal, dev, dev_empty, dev_zeros, host, pass_reference  # noqa: E402
from hostile_inputs import hostile_matrix  # noqa: E402

# The state handed to a pass.  d2: the input after the pivots [0, k0), the state a solve holds at time k0.  t1 and the
# hostile draw converge within a few pivots (ties: every rate is 1.0 after a handful; hostile: infinities spread), so a
# state with their whole history leaves a pass at k0 >= 37 nothing to update: they get the newest HISTORY pivots
# [k0 - HISTORY, k0) only -- a state the oracle produced, with paths of two and three hops in it, and work left.
HISTORY = 2


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=64)
def state_at(kind, n, dtype_name, seed, k0):
    dtype = np.dtype(dtype_name).type
    if kind == "hostile":
        rate, nxt, hops = hostile_matrix(np.random.default_rng(seed), n, dtype)
    else:
        rate, nxt, hops = synth.make(kind, n, dtype, seed=seed)
    oracle.relax(rate, nxt, hops, 0 if kind == "d2" else max(0, k0 - HISTORY), k0)
    return _frozen(rate, nxt, hops)


@functools.lru_cache(maxsize=8)
def reference(kind, n, dtype_name, seed, k0, bt):
    """(state at k0, pass_reference of [k0, k0 + bt)) with every field: the rates and the update mask of a pass do not
    depend on which other fields are carried, so every field set of a case shares it."""
    state = state_at(kind, n, dtype_name, seed, k0)
    return state, pass_reference(*state, k0, k0 + bt)


def _dtype_name(c):
    return "float32" if c["dtype"] == "f32" else "float64"


def case_reference(c):
    return reference(c["kind"], c["n"], _dtype_name(c), c["seed"], c["k0"], c["bt"])


def _row_sets(c):
    """Boolean masks over the n rows: the rows the call relaxes, and the rows of the slab it skips."""
    lo, hi = c.get("skip") or (0, 0)
    done = np.zeros(c["n"], dtype=bool)
    done[c["row0"]:c["row0"] + c["rows"]] = True
    skipped = np.zeros(c["n"], dtype=bool)
    skipped[c["row0"] + lo:c["row0"] + hi] = True
    done &= ~skipped
    return done, skipped


def teeth(c):
    """What the case could not catch, by the oracle alone: a list of complaints, empty when the case has teeth."""
    (rate, nxt, _), ref = case_reference(c)
    it = np.uint64 if rate.dtype.itemsize == 8 else np.uint32
    done, skipped = _row_sets(c)
    out = []
    for rows, what in ((done, "relaxed"), (skipped, "skipped")):
        if not rows.any():
            if what == "relaxed":
                out.append("no row is relaxed")
            continue
        if not (ref.rate[rows].view(it) != rate[rows].view(it)).any():
            out.append("no rate of the %s rows changes" % what)
        if c["fields"] not in ("r", "ru") and not (ref.next[rows] != nxt[rows]).any():
            out.append("no next-hop of the %s rows changes" % what)
        if c["fields"] == "nt" and not (ref.last[rows] >= 0).any():
            out.append("no trace entry of the %s rows is written" % what)
    return out


def expected_forms(c, large=False, mid_default=False):
    """The launch forms the case is about, for the thresholds of the process it runs in: default (64 x 64 tiles at these
    orders), every tile threshold 0 (large), or those with FWX_MID_TILES_BELOW left alone (mid_default)."""
    if c["engine"] == "perk":
        return {"RELAX_K"}
    sfx = "F32" if c["dtype"] == "f32" else "F64"
    want = {"COLPANEL_" + sfx}
    if not c.get("skip"):
        want.add("ROWPANEL_" + sfx)
    if not c.get("nonneg") or c["fields"] in ("ru", "nhu"):
        want.add(("MAIN_LARGE_" if large else "MAIN_SMALL_") + sfx)
    elif c["fields"] == "r":
        if not large:
            want.add("MAX_SMALL_" + sfx)
        elif sfx == "F64":
            want.add("MAX_LARGE_F64")
        else:
            want.add("MAX_MID_F32" if mid_default else "MAX_LARGE_F32")
    elif sfx == "F32":
        want.add("ARG_RI8_NP1_F32" if large else "ARG_RI4_NP1_F32")
    else:
        want.add("ARG_F64_RI4_NP1")
    return want


def offset_view(shape, dtype, offset):
    """A device array `offset` elements past the start of a 16-byte aligned allocation."""
    dtype = np.dtype(dtype)
    count = int(np.prod(shape))
    buf = dev_empty((count + offset + 16 // dtype.itemsize,), dtype)
    assert buf.data_ptr() % 16 == 0
    return hip.DeviceArray(shape, dtype, _ptr=buf.data_ptr() + offset * dtype.itemsize, _base=buf)


POISON_NEXT, POISON_HOPS = 123456, 1 << 20


def fused_scratch(rows, dtype, with_next, with_hops, offset=0):
    """What engine.dev_relax_fused reads of a FusedWorkspace, each array `offset` elements off a 16-byte boundary, and
    poisoned: +inf rates (they would win every fold), a next-hop and a path length no matrix holds.  The kernels write
    the cells of the rows they relax before they read them; a cell of a skipped row or of the padding that leaks into
    a result shows."""
    ld = (max(rows, 1) + 3) & ~3
    shape = (engine.FWX_FUSED_BLOCK, ld)
    ws = types.SimpleNamespace(ct=offset_view(shape, dtype, offset),
                               cnt=offset_view(shape, np.int32, offset) if with_next else None,
                               cht=offset_view(shape, np.int32, offset) if with_hops else None)
    ws.ct.copy_from_host(np.full(shape, np.inf, dtype=dtype))
    if with_next:
        ws.cnt.copy_from_host(np.full(shape, POISON_NEXT, dtype=np.int32))
    if with_hops:
        ws.cht.copy_from_host(np.full(shape, POISON_HOPS, dtype=np.int32))
    if offset:
        assert ws.ct.data_ptr() % 16 != 0
    return ws


def run_case(c):
    """Runs one case (see the module docstring); raises AssertionError on a mismatch."""
    complaints = teeth(c)
    assert not complaints, "the case has no teeth: " + "; ".join(complaints)
    (rate, nxt, hops), ref = case_reference(c)
    n, row0, rows, k0, bt, fields = c["n"], c["row0"], c["rows"], c["k0"], c["bt"], c["fields"]
    k1 = k0 + bt
    fused = c["engine"] == "fused"
    with_next = fields not in ("r", "ru")
    with_hops = fields in ("nh", "nhu")
    count = fields in ("ru", "nhu")
    traced = fields == "nt"
    skip = tuple(c["skip"]) if c.get("skip") else None
    dtype = rate.dtype
    assert fused or not traced
    assert not c.get("nonneg") or (fused and not count and c["kind"] != "hostile")
    assert with_next <= (c["kind"] != "hostile" or not fused), "the fused kernels need the domain for next-hops"

    r_t = dev(rate)
    n_t = dev(nxt) if with_next else None
    h_t = dev(hops) if with_hops else None
    tr = engine.Trace(n, n) if traced else None
    none = np.full((n, n), -1, dtype=np.int32)
    cut = lambda t, lo, hi: None if t is None else t[lo:hi]  # noqa: E731

    # (1) the snapshot panel of the block's rows; nothing but w, w_hops and the at_row rows is written
    if fused and skip is None:
        w = dev_empty((bt, n), dtype)
        wh = dev_empty((bt, n), np.int32) if with_hops else None
        engine.dev_panel_snap(r_t[k0:k1], n, k0, w, block_next_t=cut(n_t, k0, k1), block_hops_t=cut(h_t, k0, k1),
                              w_hops_t=wh, trace=tr.rows(k0, k1) if traced else None)
        assert_bits_equal(host(w), ref.W, "panel w")
        if with_hops:
            assert_bits_equal(host(wh), ref.WH, "panel w_hops")
        assert_bits_equal(host(r_t), rate, "rate after the panel")
        if with_next:
            assert_bits_equal(host(n_t), nxt, "next after the panel")
        if with_hops:
            assert_bits_equal(host(h_t), hops, "hops after the panel")
        if traced:
            assert_bits_equal(host(tr.at_row), ref.at_row, "panel at_row")
            assert_bits_equal(host(tr.last), none, "last after the panel")
            assert_bits_equal(host(tr.at_col), none, "at_col after the panel")

    # (2) the sweep of the slab, from the reference's panel
    w_ref = dev(ref.W)
    wh_ref = dev(ref.WH) if with_hops else None
    upd = dev_zeros((engine.FWX_UPDATE_SHARDS,), np.int64) if count else None
    lo, hi = row0, row0 + rows
    if fused:
        ws = fused_scratch(rows, dtype, with_next, with_hops, c.get("offset", 0))
        engine.dev_relax_fused(r_t[lo:hi], n, row0, k0, k1, w_ref, ws, next_t=cut(n_t, lo, hi), hops_t=cut(h_t, lo, hi),
                               wh_t=wh_ref, trace=tr.rows(lo, hi) if traced else None, updates_t=upd,
                               nonneg=bool(c.get("nonneg")), skip=skip)
    else:
        pn = dev(ref.WN) if with_next and c["kind"] == "hostile" else None     # outside the domain: fwx_pivots.next
        engine.dev_relax(r_t[lo:hi], n, row0, k0, k1, pivots_t=w_ref, pivot_hops_t=wh_ref, pivot_next_t=pn,
                         next_t=cut(n_t, lo, hi), hops_t=cut(h_t, lo, hi), updates_t=upd, skip=skip)

    done, _ = _row_sets(c)
    pick = lambda after, before: np.where(done[:, None], after, before)  # noqa: E731
    assert_bits_equal(host(r_t), pick(ref.rate, rate), "rate")
    if with_next:
        assert_bits_equal(host(n_t), pick(ref.next, nxt), "next")
    if with_hops:
        assert_bits_equal(host(h_t), pick(ref.hops, hops), "hops")
    if traced:
        assert_bits_equal(host(tr.last), pick(ref.last, none), "last")
        assert_bits_equal(host(tr.at_col), pick(ref.at_col, none), "at_col")
        assert_bits_equal(host(tr.at_row), ref.at_row if skip is None else none, "at_row")
    if count:
        got = host(upd)
        assert got.shape == (engine.FWX_UPDATE_SHARDS,)
        assert int(got.sum()) == int(ref.u_rows[done].sum()), "U %d vs %d" % (int(got.sum()), int(ref.u_rows[done].sum()))
    assert_bits_equal(host(w_ref), ref.W, "the pivot panel was written to")


DEVICE_ERROR_STATUS = 70        # exit status of the child after a HIP error: the parent starts nothing more on the card


def is_device_error(e):
    return isinstance(e, hip.HipError) or (isinstance(e, engine.FwxError) and e.status == -3)     # FWX_ERR_HIP


def run_cases(cases):
    """[{case, error, forms}]: every case on its own, the launch forms it reached beside it.  A HIP error ends the
    run: it is raised, not recorded."""
    out = []
    engine.kernel_forms_seen(reset=True)
    for c in cases:
        err = None
        try:
            run_case(c)
        except AssertionError as e:
            err = "mismatch: %s" % e
        except Exception as e:
            if is_device_error(e):
                raise
            err = traceback.format_exc(limit=4)
        out.append({"case": c, "error": err, "forms": sorted(engine.kernel_forms_seen(reset=True))})
    return out


if __name__ == "__main__":
    try:
        results = run_cases(json.loads(sys.argv[1]))
    except Exception as e:
        traceback.print_exc()
        sys.exit(DEVICE_ERROR_STATUS if is_device_error(e) else 1)
    print("STEP_API_RESULT " + json.dumps(results), flush=True)
