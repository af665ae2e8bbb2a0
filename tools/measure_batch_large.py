#!/usr/bin/env python3
"""Batched large solves (257 <= n <= 1024) against the loop over single-matrix solves they replace
(f64 + next + hops).

Device form, HIP events on one stream over device-resident data, per cell (n, count):
  (a) one fwx_dev_solve_batch_large call, scratch for the whole batch
  (b) `count` consecutive fwx_dev_solve calls (engine AUTO) on the same stream: what a host had before.
      fwx_dev_solve BLOCKS: every call ends in a host synchronisation, so (b) holds the fused engine's launch chain
      and a host round trip per matrix.  This path is the baseline, never the code under test
  (c) n = 257 only: one fwx_dev_solve_batch_mid call on `count` matrices of order 256, the mid kernel's neighbour
Every timed launch runs on unsolved data: the device holds a pristine copy of `inner` batches (as many as fit
1 GiB, at most 8) and a working copy restored from it, device to device, before every repetition; the batch forms
launch once per batch between the two events and report the time per launch, (b) loops over the matrices of the
first batch.  One warm-up repetition per cell and variant, then the median of REPS; min and max are kept, and
`earns` says whether (b) - (a) exceeds twice (b)'s own spread (max - min).  Cells whose arrays exceed 8 GB are
skipped.

Host form, host clock around blocking calls: fwx_solve_batch_large_f64 against `count` calls of fwx_solve_f64
(cells up to --host-max-count matrices).

Every order is measured by a child process of its own under a time limit (--step-timeout); after a child that
failed or ran out of time nothing more is started.  No torch in the process.  With FWX_LIB_PATH pointing at a build of
an earlier commit the same cells give that commit's side of an A/B (symbols it lacks are not bound).
usage: measure_batch_large.py [--out FILE.json] [--reps 5] [--orders 257,384,...] [--counts 1,2,...]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from floydwarshall_amd import _lib, engine, hip  # noqa: E402
from measure_batch import batch_of, median_ms  # noqa: E402

MAX_CELL_BYTES = 8 << 30


def cell_bytes(n, count):
    return count * n * n * 16


def device_cell(n, count, reps):
    host = batch_of(n, count)
    per_copy = sum(a.nbytes for a in host)
    inner = max(1, min(8, (1 << 30) // per_copy))
    tiled = [np.ascontiguousarray(np.tile(a, (inner, 1))) for a in host] if inner > 1 else host
    pristine = [hip.DeviceArray.from_numpy(a) for a in tiled]
    d = [hip.DeviceArray(a.shape, a.dtype) for a in tiled]
    scratch = hip.DeviceArray((count * _lib.batch_large_scratch_bytes(n),), np.uint8)
    s = hip.Stream()
    e0, e1 = hip.Event(), hip.Event()
    rows = count * n

    def prepare():
        for da, p in zip(d, pristine):
            da.copy_(p)
        hip.synchronize()

    def batch_with(fn, order, **kw):
        def run():
            e0.record(s)
            for i in range(inner):
                r, x, h = (da.rows(i * rows, (i + 1) * rows) for da in d)
                fn(r, count, order, next_t=x, hops_t=h, stream=s, **kw)
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

    launches = 2 * ((n + 15) // 16)
    cell = {"n": n, "count": count, "launches_per_window": inner, "kernel_launches_per_call": launches}
    cell["batch_ms"], cell["batch_min_ms"], cell["batch_max_ms"] = \
        median_ms(batch_with(engine.dev_solve_batch_large, n, scratch_t=scratch), prepare, reps)
    cell["batch_us_per_kernel_launch"] = 1e3 * cell["batch_ms"] / launches
    cell["loop_ms"], cell["loop_min_ms"], cell["loop_max_ms"] = median_ms(loop, prepare, reps)
    cell["loop_over_batch"] = cell["loop_ms"] / cell["batch_ms"]
    cell["loop_spread_ms"] = cell["loop_max_ms"] - cell["loop_min_ms"]
    cell["earns"] = bool(cell["loop_ms"] - cell["batch_ms"] > 2 * cell["loop_spread_ms"])
    if n == 257:
        # the first 256 x 256 elements per matrix of the same buffers, read as matrices of order 256, stride n*n
        def mid(r, cnt, order, next_t, hops_t, stream):
            engine.dev_solve_batch_mid(r, cnt, 256, next_t=next_t, hops_t=hops_t, stride=n * n, stream=stream)
        cell["mid_256_ms"], cell["mid_256_min_ms"], cell["mid_256_max_ms"] = median_ms(batch_with(mid, 256), prepare, reps)
    for da in d + pristine + [scratch]:
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
        engine.solve_batch_large(*work)
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


def worker(args, n, counts):
    """One order: every count, device form then host form.  Prints the table lines, writes the cells to args.out."""
    if engine.device_count() < 1:
        sys.exit("measure_batch_large.py: no HIP device (nothing is measured without one)")
    os.environ.pop("FWX_BATCH_LARGE_MIN_N", None)
    os.environ.pop("FWX_BATCH_MID_MIN_N", None)
    out = {"device": [], "host": []}
    for count in counts:
        if cell_bytes(n, count) > MAX_CELL_BYTES:
            print("n=%4d count=%4d   skipped: %.1f GB" % (n, count, cell_bytes(n, count) / 1e9), flush=True)
            continue
        c = device_cell(n, count, args.reps)
        out["device"].append(c)
        print("dev  n=%4d count=%4d   batch %9.4f [%9.4f, %9.4f]   loop %9.3f [%9.3f, %9.3f]   loop/batch %6.2f   "
              "earns %-5s  %5.1f us/launch%s" % (
                  n, count, c["batch_ms"], c["batch_min_ms"], c["batch_max_ms"], c["loop_ms"], c["loop_min_ms"],
                  c["loop_max_ms"], c["loop_over_batch"], c["earns"], c["batch_us_per_kernel_launch"],
                  "   mid n=256: %.4f" % c["mid_256_ms"] if "mid_256_ms" in c else ""), flush=True)
    for count in counts:
        if args.skip_host or count > args.host_max_count or cell_bytes(n, count) > MAX_CELL_BYTES:
            continue
        c = host_cell(n, count, args.reps)
        out["host"].append(c)
        print("host n=%4d count=%4d   fwx_solve_batch_large_f64 %9.3f   count x fwx_solve_f64 %9.3f   ratio %6.2f" % (
            n, count, c["host_batch_ms"], c["host_loop_ms"], c["host_loop_over_batch"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--orders", default="257,384,512,768,1024")
    ap.add_argument("--counts", default="1,2,4,8,16,64,256")
    ap.add_argument("--host-max-count", type=int, default=64)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds per order")
    ap.add_argument("--worker", type=int, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if os.environ.get("FWX_LIB_PATH"):      # an older build of the same ABI lacks the symbols later rounds added: the
        have = ctypes.CDLL(_lib.LIB_PATH)   # parent's side of an A/B of this call, alternated with this tree's in one job
        for name in [name for name in _lib.SIGNATURES if not hasattr(have, name)]:
            del _lib.SIGNATURES[name]
    counts = [int(v) for v in args.counts.split(",")]
    if args.worker is not None:
        return worker(args, args.worker, counts)
    geometry = (ctypes.c_int32 * 4)()
    _lib.lib().fwx_test_batch_large_geometry(geometry)
    result = {"what": "f64 + next + hops; ms; median of %d repetitions after one warm-up, min and max kept; batch_ms = "
                      "one fwx_dev_solve_batch_large call; loop_ms = count blocking fwx_dev_solve calls, a host "
                      "synchronisation per matrix included; mid_256_ms = one fwx_dev_solve_batch_mid call at n = 256; "
                      "earns = loop_ms - batch_ms > 2 * (loop_max_ms - loop_min_ms)" % args.reps,
              "geometry": {"B": geometry[0], "S": geometry[1], "tile_rows": geometry[2], "tile_cols": geometry[3]},
              "device": [], "host": []}
    print("(b) = count blocking fwx_dev_solve calls: the fused engine's launches and a host synchronisation per matrix",
          flush=True)
    for n in (int(v) for v in args.orders.split(",")):
        with tempfile.TemporaryDirectory() as tmp:
            part = os.path.join(tmp, "part.json")
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", str(n), "--out", part, "--reps", str(args.reps),
                   "--counts", args.counts, "--host-max-count", str(args.host_max_count)]
            if args.skip_host:
                cmd.append("--skip-host")
            try:
                rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print("n=%d: the step ended with status %d; nothing more is started" % (n, rc), flush=True)
                result["stopped_at"] = {"n": n, "status": rc}
                break
            with open(part) as f:
                got = json.load(f)
            result["device"] += got["device"]
            result["host"] += got["host"]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 1 if "stopped_at" in result else 0


if __name__ == "__main__":
    sys.exit(main())
