#!/usr/bin/env python3
"""The traced large-tier batch solve (257 <= n <= 1024) and the batch walk of the exact `_path` lists, against the
untraced large-tier solve and against what a host had before for the same answer: one traced handle per matrix
(f64 + next + hops, market inputs).

Device forms, HIP events on one stream over device-resident data, per cell (n, count):
  (a) one fwx_dev_solve_batch_large call, scratch for the whole batch
  (b) one fwx_dev_solve_batch_large_traced call on the same scratch, alternated with (a) repetition by repetition in
      this process
  (c) one fwx_dev_exact_paths_batch_large launch over ITEMS seeded items (mat, src, dst), cap = the oracle's longest
      list + 2, on the trace (b) left
  (d) host clock, per matrix over the first D_MATRICES matrices: on ONE DeviceMatrix with enable_path_log (created
      outside the clock) upload, solve and query_exact_batch of that matrix's share of the items.  Reported per
      matrix next to ((b) + (c)) / count; it is not extrapolated to a total.
Every timed solve runs on unsolved data: a pristine copy of the batch stays on the device and is copied over the
working arrays before every repetition, outside the events.  One warm-up repetition per cell and variant, then the
median of REPS with minimum and maximum.

Host form, host clock around the blocking C call: fwx_solve_batch_large_lists_f64 with all ITEMS items, per matrix,
next to (d) (cells up to --host-max-count matrices).

Inputs after tools/measure_batch_mid_lists.py: matrix b is the market of 8 currencies on n / 8 + 4 exchanges (the leading
n vertices) with seed 23 + n + (b mod 8).  Building the eight markets of an order and the oracle's longest list takes the CPU minutes at
n = 1024: --inputs DIR keeps them (market_<n>.npz), and --prepare-only fills DIR without touching a device.  No torch
in the process.
usage: measure_batch_large_lists.py [--out FILE.json] [--reps 5] [--cells n:count,...] [--inputs DIR] [--prepare-only]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from floydwarshall_amd import _lib, engine, hip  # noqa: E402
import measure_batch_lists  # noqa: E402,F401
from hostile_inputs import market_rates  # noqa: E402  (measure_batch_lists put tests/ on the path)
from measure_batch_lists import ptr, stats  # noqa: E402
from oracle import list_faithful as lf  # noqa: E402
from oracle import list_ropes  # noqa: E402

ITEMS = 65536
D_MATRICES = 16


def market(n, seed):
    """measure_batch_lists.market with four spare exchanges: a currency nobody quotes on an exchange is no vertex
    (about one in 128), and at these orders one spare exchange does not always make up for them."""
    n_exch = -(-n // 8) + 4
    m0 = lf.build_matrix(market_rates(n_exch, 8, seed=seed), np.float64)
    assert len(m0) >= n, (n, len(m0))
    _, rate, nxt, hops = lf.to_dense(m0, np.float64)
    return [np.ascontiguousarray(a[:n, :n]) for a in (rate, nxt, hops)]


def markets_of(n, inputs):
    """The eight distinct markets of order n, (rate, next, hops) each of shape (8, n, n), and the oracle's longest
    list over them."""
    path = os.path.join(inputs, "market_%d.npz" % n) if inputs else None
    if path and os.path.exists(path):
        z = np.load(path)
        return [z["rate"], z["next"], z["hops"]], int(z["longest"])
    parts = [market(n, 23 + n + b) for b in range(8)]
    longest = max(int(list_ropes.solve(p[0], p[1]).lengths.max()) for p in parts)
    eight = [np.ascontiguousarray(np.stack([p[f] for p in parts])) for f in range(3)]
    if path:
        os.makedirs(inputs, exist_ok=True)
        np.savez_compressed(path, rate=eight[0], next=eight[1], hops=eight[2], longest=longest)
    return eight, longest


def cell_of(n, count, reps, host_max_count, inputs):
    eight, longest = markets_of(n, inputs)
    host = [np.ascontiguousarray(a[np.arange(count) % 8]) for a in eight]
    cap = longest + 2
    cells = count * n * n
    pristine = [hip.DeviceArray.from_numpy(a.reshape(-1)) for a in host]
    d = [hip.DeviceArray(p.shape, p.dtype) for p in pristine]
    scratch = hip.DeviceArray((count * _lib.batch_large_scratch_bytes(n),), np.uint8)
    s = hip.Stream()
    e0, e1 = hip.Event(), hip.Event()

    def prepare():
        for da, p in zip(d, pristine):
            da.copy_(p)
        hip.synchronize()

    def timed(fn):
        e0.record(s)
        out = fn()
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1), out

    cell = {"n": n, "count": count, "items": ITEMS, "cap": cap}
    trace = engine.Trace(1, cells)
    variants = [("a_untraced", lambda: engine.dev_solve_batch_large(d[0], count, n, next_t=d[1], hops_t=d[2],
                                                                     scratch_t=scratch, stream=s)),
                ("b_traced", lambda: engine.dev_solve_batch_large_traced(d[0], count, n, trace, next_t=d[1], hops_t=d[2],
                                                                         scratch_t=scratch, stream=s))]
    samples = {name: [] for name, _ in variants}
    for rep in range(reps + 1):                       # repetition 0 is the warm-up
        for name, fn in variants:
            prepare()
            t = timed(fn)[0]
            if rep:
                samples[name].append(t)
    for name, _ in variants:
        cell[name] = stats(samples[name])
    cell["b_over_a"] = cell["b_traced"]["ms"] / cell["a_untraced"]["ms"]
    rnd = np.random.default_rng(9100 + n)
    items = [rnd.integers(0, hi, ITEMS).astype(np.int32) for hi in (count, n, n)]
    d_items = [hip.DeviceArray.from_numpy(a) for a in items]

    def walk():
        return engine.dev_exact_paths_batch_large(pristine[1], count, n, trace, d_items[0], d_items[1], d_items[2], cap,
                                                  stream=s)

    c_ms = [timed(walk)[0] for _ in range(reps + 1)][1:]
    lens = timed(walk)[1][0].numpy(s)
    assert int(lens.min()) >= 0 and int(lens.max()) <= longest, (int(lens.min()), int(lens.max()), longest)
    cell["c_walk"] = stats(c_ms)
    cell["batch_per_matrix_ms"] = (cell["b_traced"]["ms"] + cell["c_walk"]["ms"]) / count

    # (d): one traced handle, matrix after matrix
    share = [np.nonzero(items[0] == b)[0] for b in range(min(D_MATRICES, count))]
    d_src = [np.ascontiguousarray(items[1][sel]) for sel in share]
    d_dst = [np.ascontiguousarray(items[2][sel]) for sel in share]
    lens_out = np.empty(ITEMS, dtype=np.int32)              # the C entry points, outputs allocated once: no Python
    paths_out = np.empty((ITEMS, cap), dtype=np.int32)      #   list is built inside a timed region
    query = _lib.lib().fwx_matrix_query_exact_batch
    d_ms = []
    with engine.DeviceMatrix(n, np.float64, with_next=True, with_hops=True) as dm:
        dm.enable_path_log()
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            for b, sel in enumerate(share):
                dm.upload(host[0][b], host[1][b], host[2][b])
                dm.solve()
                if len(sel):
                    rc = query(dm._h, len(sel), ptr(d_src[b]), ptr(d_dst[b]), ptr(lens_out), ptr(paths_out), cap)
                    assert rc == 0, rc
            if rep:
                d_ms.append(1e3 * (time.perf_counter() - t0) / len(share))
    cell["d_handle_per_matrix"] = stats(d_ms)
    cell["d_over_batch"] = cell["d_handle_per_matrix"]["ms"] / cell["batch_per_matrix_ms"]

    if count <= host_max_count:                             # the host form, everything in one call
        h_ms = []
        for rep in range(reps + 1):
            work = [a.copy() for a in host]
            t0 = time.perf_counter()
            rc = _lib.lib().fwx_solve_batch_large_lists_f64(count, n, ptr(work[0]), ptr(work[1]), ptr(work[2]), None,
                                                            ITEMS, ptr(items[0]), ptr(items[1]), ptr(items[2]),
                                                            ptr(lens_out), ptr(paths_out), cap, None)
            assert rc == 0, rc
            if rep:
                h_ms.append(1e3 * (time.perf_counter() - t0) / count)
        assert np.array_equal(lens_out, lens)               # the host form and the device walk agree on every length
        cell["host_form_per_matrix"] = stats(h_ms)
        cell["d_over_host_form"] = cell["d_handle_per_matrix"]["ms"] / cell["host_form_per_matrix"]["ms"]
    for da in d + pristine + d_items + [scratch, trace.last, trace.at_col, trace.at_row]:
        da.free()
    s.close()
    return cell


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cells", default=",".join("%d:%d" % (n, c) for n in (257, 384, 512, 768, 1024)
                                                for c in (1, 16, 256)))
    ap.add_argument("--host-max-count", type=int, default=16)
    ap.add_argument("--inputs", help="directory that keeps the markets of every order between runs")
    ap.add_argument("--prepare-only", action="store_true", help="fill --inputs and stop; needs no device")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    specs = [tuple(int(v) for v in spec.split(":")) for spec in args.cells.split(",")]
    if args.prepare_only:
        if not args.inputs:
            ap.error("--prepare-only needs --inputs")
        for n in sorted({n for n, _ in specs}):
            print("n=%d: longest list %d" % (n, markets_of(n, args.inputs)[1]), flush=True)
        return
    if engine.device_count() < 1:
        sys.exit("measure_batch_large_lists.py: no HIP device (nothing is measured without one)")
    os.environ.pop("FWX_BATCH_LARGE_MIN_N", None)
    os.environ.pop("FWX_BATCH_MID_MIN_N", None)
    geometry = (4 * _lib.c_i32)()
    _lib.lib().fwx_test_batch_large_geometry(geometry)
    result = {"what": "f64 + next + hops, market inputs; ms; median (min, max) of %d repetitions after one warm-up; "
                      "(a), (b), (c) HIP events per call, (d) and the host form host clock per matrix" % args.reps,
              "library": os.path.relpath(_lib.LIB_PATH, ROOT),
              "geometry": {"B": geometry[0], "S": geometry[1], "tile_rows": geometry[2], "tile_cols": geometry[3]},
              "cells": []}
    print("library: %s" % result["library"], flush=True)
    print("ms: (a) untraced   (b) traced   (b)/(a)   (c) walk of %d items | per matrix: ((b)+(c))/count   host form   "
          "(d) handle   (d)/batch   (d)/host form" % ITEMS, flush=True)
    for n, count in specs:
        c = cell_of(n, count, args.reps, args.host_max_count, args.inputs)
        result["cells"].append(c)
        print("n=%4d count=%4d  %9.4f [%.4f, %.4f]  %9.4f [%.4f, %.4f]  %5.3f  %9.4f [%.4f, %.4f] | %10.6f  %s  "
              "%9.4f [%.4f, %.4f]  %8.1f  %s" % (
                  n, count, c["a_untraced"]["ms"], c["a_untraced"]["min_ms"], c["a_untraced"]["max_ms"],
                  c["b_traced"]["ms"], c["b_traced"]["min_ms"], c["b_traced"]["max_ms"], c["b_over_a"],
                  c["c_walk"]["ms"], c["c_walk"]["min_ms"], c["c_walk"]["max_ms"], c["batch_per_matrix_ms"],
                  "%10.6f" % c["host_form_per_matrix"]["ms"] if "host_form_per_matrix" in c else "         -",
                  c["d_handle_per_matrix"]["ms"], c["d_handle_per_matrix"]["min_ms"], c["d_handle_per_matrix"]["max_ms"],
                  c["d_over_batch"], "%8.1f" % c["d_over_host_form"] if "d_over_host_form" in c else "       -"),
              flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
