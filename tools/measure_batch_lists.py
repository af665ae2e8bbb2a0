#!/usr/bin/env python3
"""The traced batch solve and the batch walk of the exact `_path` lists, against the untraced batch solve and against
what a host had before for the same answer: one traced handle per matrix (f64 + next + hops, market inputs).

Device forms, HIP events on one stream over device-resident data, per cell (n, count):
  (a) one fwx_dev_solve_batch launch
  (b) one fwx_dev_solve_batch_traced launch, alternated with (a) repetition by repetition in this process
  (c) one fwx_dev_exact_paths_batch launch over ITEMS seeded items (mat, src, dst), cap = the oracle's longest
      list + 2, on the trace (b) left
  (d) host clock, per matrix over the first D_MATRICES matrices: on ONE DeviceMatrix with enable_path_log (created
      outside the clock) upload, solve and query_exact_batch of that matrix's share of the items.  Reported per
      matrix next to ((b) + (c)) / count; it is not extrapolated to a total.
Every timed solve runs on unsolved data: the device holds `inner` pristine copies of the batch (as many as fit
512 MiB, at most 16), re-uploaded before every repetition; (a) and (b) launch once per copy between the two events
and report the time per launch.  One warm-up repetition per cell and variant, then the median of REPS with minimum
and maximum.

Host form, host clock around the blocking C call: fwx_solve_batch_lists_f64 with all ITEMS items, per matrix, next to
(d).  Both call the C entry points with outputs allocated once: no Python list is built inside a timed region.

Inputs: matrix b is the market of tests/test_gpu_exact_lists_edges.py (8 currencies, the leading n vertices) with seed
23 + n + (b mod 8).  No torch in the process.
usage: measure_batch_lists.py [--out FILE.json] [--reps 5] [--cells n:count,...]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from floydwarshall_amd import _lib, engine, hip  # noqa: E402
from hostile_inputs import market_rates  # noqa: E402
from oracle import list_faithful as lf  # noqa: E402
from oracle import list_ropes  # noqa: E402

ITEMS = 65536
D_MATRICES = 64


def market(n, seed):
    n_exch = -(-n // 8) + 1
    _, rate, nxt, hops = lf.to_dense(lf.build_matrix(market_rates(n_exch, 8, seed=seed), np.float64), np.float64)
    return [np.ascontiguousarray(a[:n, :n]) for a in (rate, nxt, hops)]


def batch_of(n, count):
    """(rate, next, hops) of shape (count, n, n), eight distinct markets repeated, and the oracle's longest list."""
    parts = [market(n, 23 + n + b) for b in range(8)]
    longest = max(int(list_ropes.solve(p[0], p[1]).lengths.max()) for p in parts)
    return [np.ascontiguousarray(np.stack([parts[b % 8][f] for b in range(count)])) for f in range(3)], longest


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def stats(samples):
    return {"ms": statistics.median(samples), "min_ms": min(samples), "max_ms": max(samples)}


def cell_of(n, count, reps):
    host, longest = batch_of(n, count)
    cap = longest + 2
    cells = count * n * n
    inner = max(1, min(16, (512 << 20) // sum(a.nbytes for a in host)))
    tiled = [np.ascontiguousarray(np.tile(a.reshape(-1), inner)) for a in host]
    d = [hip.DeviceArray(a.shape, a.dtype) for a in tiled]
    next0 = hip.DeviceArray.from_numpy(host[1].reshape(-1))
    trace = engine.Trace(1, cells)
    rnd = np.random.default_rng(9100 + n)
    items = [rnd.integers(0, hi, ITEMS).astype(np.int32) for hi in (count, n, n)]
    d_items = [hip.DeviceArray.from_numpy(a) for a in items]
    s = hip.Stream()
    e0, e1 = hip.Event(), hip.Event()

    def prepare():
        for da, a in zip(d, tiled):
            da.copy_from_host(a)
        hip.synchronize()

    def copy(i):
        return [hip.DeviceArray((cells,), da.dtype, _ptr=da.data_ptr() + i * cells * da.element_size(), _base=da)
                for da in d]

    def solves(traced):
        e0.record(s)
        for i in range(inner):
            r, x, h = copy(i)
            if traced:
                engine.dev_solve_batch_traced(r, count, n, trace, next_t=x, hops_t=h, stream=s)
            else:
                engine.dev_solve_batch(r, count, n, next_t=x, hops_t=h, stream=s)
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1) / inner

    def walk():
        e0.record(s)
        out = engine.dev_exact_paths_batch(next0, count, n, trace, d_items[0], d_items[1], d_items[2], cap, stream=s)
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1), out

    a_ms, b_ms = [], []
    for rep in range(reps + 1):                       # repetition 0 is the warm-up
        for traced, into in ((False, a_ms), (True, b_ms)):
            prepare()
            t = solves(traced)
            if rep:
                into.append(t)
    c_ms = [walk()[0] for _ in range(reps + 1)][1:]
    lens = walk()[1][0].numpy(s)
    assert int(lens.min()) >= 0 and int(lens.max()) <= longest, (int(lens.min()), int(lens.max()), longest)

    # (d): one traced handle, matrix after matrix
    share = [np.nonzero(items[0] == b)[0] for b in range(min(D_MATRICES, count))]
    d_ms = []
    d_src = [np.ascontiguousarray(items[1][sel]) for sel in share]
    d_dst = [np.ascontiguousarray(items[2][sel]) for sel in share]
    lens_out = np.empty(ITEMS, dtype=np.int32)              # the C entry points, outputs allocated once: no Python
    paths_out = np.empty((ITEMS, cap), dtype=np.int32)      #   list is built inside a timed region
    query = _lib.lib().fwx_matrix_query_exact_batch
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

    # the host form, everything in one call
    h_ms = []
    for rep in range(reps + 1):
        work = [a.copy() for a in host]
        t0 = time.perf_counter()
        rc = _lib.lib().fwx_solve_batch_lists_f64(count, n, ptr(work[0]), ptr(work[1]), ptr(work[2]), None, ITEMS,
                                                  ptr(items[0]), ptr(items[1]), ptr(items[2]), ptr(lens_out),
                                                  ptr(paths_out), cap, None)
        assert rc == 0, rc
        if rep:
            h_ms.append(1e3 * (time.perf_counter() - t0) / count)

    assert np.array_equal(lens_out, lens)                   # the host form and the device walk agree on every length
    for da in d + d_items + [next0, trace.last, trace.at_col, trace.at_row]:
        da.free()
    s.close()
    cell = {"n": n, "count": count, "items": ITEMS, "cap": cap, "launches_per_window": inner,
            "a_untraced": stats(a_ms), "b_traced": stats(b_ms), "c_walk": stats(c_ms),
            "d_handle_per_matrix": stats(d_ms), "host_form_per_matrix": stats(h_ms)}
    cell["b_over_a"] = cell["b_traced"]["ms"] / cell["a_untraced"]["ms"]
    cell["batch_per_matrix_ms"] = (cell["b_traced"]["ms"] + cell["c_walk"]["ms"]) / count
    cell["d_over_batch"] = cell["d_handle_per_matrix"]["ms"] / cell["batch_per_matrix_ms"]
    cell["d_over_host_form"] = cell["d_handle_per_matrix"]["ms"] / cell["host_form_per_matrix"]["ms"]
    return cell


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cells", default="4:4096,16:4096,64:256,64:4096,128:256")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if engine.device_count() < 1:
        sys.exit("measure_batch_lists.py: no HIP device (nothing is measured without one)")
    result = {"what": "f64 + next + hops, market inputs; ms; median (min, max) of %d repetitions after one warm-up; "
                      "(a), (b), (c) HIP events per launch, (d) and the host form host clock per matrix" % args.reps,
              "cells": []}
    print("ms: (a) untraced   (b) traced   (b)/(a)   (c) walk of %d items | per matrix: ((b)+(c))/count   host form   "
          "(d) handle   (d)/batch   (d)/host form" % ITEMS, flush=True)
    for spec in args.cells.split(","):
        n, count = (int(v) for v in spec.split(":"))
        c = cell_of(n, count, args.reps)
        result["cells"].append(c)
        print("n=%3d count=%4d  %9.4f [%.4f, %.4f]  %9.4f [%.4f, %.4f]  %5.2f  %9.4f [%.4f, %.4f] | %10.6f  %10.6f  "
              "%9.4f [%.4f, %.4f]  %8.1f  %8.1f" % (
                  n, count, c["a_untraced"]["ms"], c["a_untraced"]["min_ms"], c["a_untraced"]["max_ms"],
                  c["b_traced"]["ms"], c["b_traced"]["min_ms"], c["b_traced"]["max_ms"], c["b_over_a"],
                  c["c_walk"]["ms"], c["c_walk"]["min_ms"], c["c_walk"]["max_ms"], c["batch_per_matrix_ms"],
                  c["host_form_per_matrix"]["ms"], c["d_handle_per_matrix"]["ms"], c["d_handle_per_matrix"]["min_ms"],
                  c["d_handle_per_matrix"]["max_ms"], c["d_over_batch"], c["d_over_host_form"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
