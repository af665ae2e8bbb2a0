#!/usr/bin/env python3
"""Batched mid-size solves (129 <= n <= 256) against the loop over single-matrix solves they replace
(f64 + next + hops).

Device form, HIP events on one stream over device-resident data, per cell (n, count):
  (a) one fwx_dev_solve_batch_mid call
  (b) `count` consecutive fwx_dev_solve calls (engine AUTO) on the same stream: what a host had before.
      fwx_dev_solve BLOCKS: every call ends in a host synchronisation, so (b) holds the fused engine's launch chain
      and a host round trip per matrix.  This path is the baseline, never the code under test
  (c) n = 128 only: (a) with FWX_BATCH_MID_MIN_N=1 -- the mid kernel, matrix resident in device memory -- against
      fwx_dev_solve_batch's workgroup tier, matrix in registers, on the same input: what the global-resident scheme
      costs, and so whether 129 is the right threshold
Every timed launch runs on unsolved data: the device holds `inner` pristine copies of the batch (as many as fit
1 GiB, at most 32), re-uploaded before every repetition; the batch forms launch once per copy between the two
events and report the time per launch, (b) loops over the matrices of the first copy.  One warm-up repetition per
cell and variant, then the median of REPS.

Host form, host clock around blocking calls: fwx_solve_batch_mid_f64 against `count` calls of fwx_solve_f64
(cells up to --host-max-count matrices: the arrays of a larger batch exceed what a host call stages).

No torch in the process.  usage: measure_batch_mid.py [--out FILE.json] [--reps 5] [--cells n:count,...]"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from floydwarshall_amd import _lib, engine, hip  # noqa: E402
from measure_batch import batch_of, median_ms  # noqa: E402


def device_cell(n, count, reps):
    host = batch_of(n, count)
    per_copy = sum(a.nbytes for a in host)
    inner = max(1, min(32, (1 << 30) // per_copy))
    tiled = [np.ascontiguousarray(np.tile(a, (inner, 1))) for a in host] if inner > 1 else host
    d = [hip.DeviceArray(a.shape, a.dtype) for a in tiled]
    s = hip.Stream()
    e0, e1 = hip.Event(), hip.Event()
    rows = count * n

    def prepare():
        for da, a in zip(d, tiled):
            da.copy_from_host(a)
        hip.synchronize()

    def batch_with(fn):
        def run():
            e0.record(s)
            for i in range(inner):
                r, x, h = (da.rows(i * rows, (i + 1) * rows) for da in d)
                fn(r, count, n, next_t=x, hops_t=h, stream=s)
            e1.record(s)
            e1.synchronize()
            return e0.elapsed_time(e1) / inner
        return run

    slabs = []
    for b in range(count):
        sl = _lib.FwxSlab()
        sl.n, sl.row0, sl.rows, sl.dtype = n, 0, n, _lib.FWX_F64
        sl.rate, sl.next, sl.hops = (da.data_ptr() + b * n * n * da.element_size() for da in d)
        slabs.append(sl)
    o, _ = engine._opts(stream=s)
    dev_solve = _lib.lib().fwx_dev_solve

    def loop():
        e0.record(s)
        for sl in slabs:
            rc = dev_solve(ctypes.byref(sl), ctypes.byref(o))
            if rc:
                _lib.check(rc, "fwx_dev_solve")
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1)

    cell = {"n": n, "count": count, "launches_per_window": inner}
    if n <= _lib.FWX_BATCH_MAX_N:
        os.environ["FWX_BATCH_MID_MIN_N"] = "1"
    else:
        os.environ.pop("FWX_BATCH_MID_MIN_N", None)
    cell["batch_ms"], cell["batch_min_ms"], cell["batch_max_ms"] = \
        median_ms(batch_with(engine.dev_solve_batch_mid), prepare, reps)
    os.environ.pop("FWX_BATCH_MID_MIN_N", None)
    cell["loop_ms"], cell["loop_min_ms"], cell["loop_max_ms"] = median_ms(loop, prepare, reps)
    cell["loop_over_batch"] = cell["loop_ms"] / cell["batch_ms"]
    if n <= _lib.FWX_BATCH_MAX_N:
        cell["workgroup_tier_ms"], cell["workgroup_tier_min_ms"], cell["workgroup_tier_max_ms"] = \
            median_ms(batch_with(engine.dev_solve_batch), prepare, reps)
        cell["mid_over_workgroup_tier"] = cell["batch_ms"] / cell["workgroup_tier_ms"]
    for da in d:
        da.free()
    s.close()
    return cell


def host_cell(n, count, reps):
    pristine = [a.reshape(count, n, n) for a in batch_of(n, count)]
    work = [a.copy() for a in pristine]

    def prepare():
        for w, p in zip(work, pristine):
            np.copyto(w, p)

    def batch():
        t0 = time.perf_counter()
        engine.solve_batch_mid(*work)
        return 1e3 * (time.perf_counter() - t0)

    solve = _lib.lib().fwx_solve_f64
    ptrs = [[a[b].ctypes.data for a in work] for b in range(count)]

    def loop():
        t0 = time.perf_counter()
        for r, x, h in ptrs:
            rc = solve(n, r, x, h, None)
            if rc:
                _lib.check(rc, "fwx_solve_f64")
        return 1e3 * (time.perf_counter() - t0)

    cell = {"n": n, "count": count}
    cell["host_batch_ms"], cell["host_batch_min_ms"], cell["host_batch_max_ms"] = median_ms(batch, prepare, reps)
    cell["host_loop_ms"], cell["host_loop_min_ms"], cell["host_loop_max_ms"] = median_ms(loop, prepare, reps)
    cell["host_loop_over_batch"] = cell["host_loop_ms"] / cell["host_batch_ms"]
    return cell


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cells", default=",".join("%d:%d" % (n, c) for n in (129, 192, 256, 128)
                                                for c in (8, 64, 256, 4096)))
    ap.add_argument("--host-max-count", type=int, default=256)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if engine.device_count() < 1:
        sys.exit("measure_batch_mid.py: no HIP device (nothing is measured without one)")
    cells = [tuple(int(v) for v in c.split(":")) for c in args.cells.split(",")]
    result = {"what": "f64 + next + hops; ms; median of %d repetitions after one warm-up; batch_ms = one "
                      "fwx_dev_solve_batch_mid call (n <= 128: FWX_BATCH_MID_MIN_N=1); loop_ms = count blocking "
                      "fwx_dev_solve calls, a host synchronisation per matrix included; workgroup_tier_ms = one "
                      "fwx_dev_solve_batch call" % args.reps,
              "block": _lib.lib().fwx_test_batch_mid_block(), "device": [], "host": []}
    print("(b) = count blocking fwx_dev_solve calls: the fused engine's launches and a host synchronisation per matrix",
          flush=True)
    print("device form (HIP events)      mid batch (a)    loop (b)   (b)/(a)   workgroup tier (c)   (a)/(c)", flush=True)
    for n, count in cells:
        c = device_cell(n, count, args.reps)
        result["device"].append(c)
        wg = c.get("workgroup_tier_ms")
        print("n=%3d count=%4d   %15.4f %11.3f %9.1f   %s" % (
            n, count, c["batch_ms"], c["loop_ms"], c["loop_over_batch"],
            "%12.4f %12.2f" % (wg, c["batch_ms"] / wg) if wg is not None else "           -            -"), flush=True)
    if not args.skip_host:
        print("host form (host clock)        fwx_solve_batch_mid_f64   count x fwx_solve_f64   ratio", flush=True)
        for n, count in cells:
            if count > args.host_max_count or n <= _lib.FWX_BATCH_MAX_N:
                continue
            c = host_cell(n, count, args.reps)
            result["host"].append(c)
            print("n=%3d count=%4d   %24.3f %23.3f %7.1f" % (n, count, c["host_batch_ms"], c["host_loop_ms"],
                                                             c["host_loop_over_batch"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
