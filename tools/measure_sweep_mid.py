#!/usr/bin/env python3
"""What-if sweeps on the mid tier against the mid batch call on materialised variants (f64 + next + hops).

Every cell (n, count): the base is synth d2 of order n; variant b multiplies one quote by 4 and divides the opposite
quote by 4 (two patches) and asks for four entries, the patched pair among them (tools/measure_sweep.py's cell).

Device form, HIP events on one stream over device-resident data:
  (a) one fwx_dev_solve_sweep_mid call, items only: slots x n*n x 16 bytes of scratch, whatever the count
  (b) one fwx_dev_solve_batch_mid call on the same variants materialised on the device beforehand: count x n*n x 16
      bytes.  It solves in place, so a pristine copy of the batch stays on the device and is copied over the working
      one (device to device, outside the timed window) before every repetition.
The two are timed ALTERNATELY, repetition by repetition; one warm-up repetition, then the median of REPS and the
spread (min, max) of each.  The expectation: (a) adds one read of the base and one write of the slot per variant to
the ceil(n / 16) read passes the body makes over the matrix, so (a) <= (b) * (1 + 2 / ceil(n / 16)) + twice (b)'s
spread.

Host form, host clock around blocking calls:
  (c) fwx_solve_sweep_mid_f64 on the base and the tables
  (d) numpy builds the `count` matrices, fwx_solve_batch_mid_f64 solves them, numpy indexes the answers
with the bytes each moves to and from the device.  The expectation: (c) beats (d) in every cell, by more as count grows.

No torch in the process.  usage: measure_sweep_mid.py [--out FILE.json] [--reps 7] [--cells n:count,...]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from floydwarshall_amd import _lib, engine, hip  # noqa: E402
from measure_sweep import materialise, spread, sweep_of  # noqa: E402


def bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


def device_cell(n, count, reps):
    t = sweep_of(n, count)
    mats = [a.reshape(count * n, n) for a in materialise(t, n, count)]
    pristine = [hip.DeviceArray.from_numpy(a) for a in mats]
    work = [hip.DeviceArray(a.shape, a.dtype) for a in mats]
    dbase = [hip.DeviceArray.from_numpy(a) for a in t["base"]]
    dt = {k: hip.DeviceArray.from_numpy(t[k]) for k in ("pptr", "pindex", "prate", "pnext", "phops", "iptr", "src", "dst")}
    outs = [hip.DeviceArray((4 * count,), np.float64), hip.DeviceArray((4 * count,), np.int32),
            hip.DeviceArray((4 * count,), np.int32)]
    per_slot = _lib.sweep_mid_scratch_bytes(n)
    slots = min(count, 512)
    scratch = hip.DeviceArray((slots * per_slot,), np.uint8)
    L = _lib.lib()
    slots = L.fwx_test_sweep_mid_slots(count, n, scratch.numel())
    s = hip.Stream()
    e0, e1 = hip.Event(), hip.Event()
    vp = ctypes.c_void_p
    sp = vp(s.ptr.value if isinstance(s.ptr, ctypes.c_void_p) else s.ptr)

    def prepare():
        for w, p in zip(work, pristine):
            w.copy_(p)
        hip.synchronize()

    batch_args = (count, n, _lib.FWX_F64, vp(work[0].data_ptr()), vp(work[1].data_ptr()), vp(work[2].data_ptr()),
                  n * n, 0, 0, None, sp)

    def batch():
        e0.record(s)
        rc = L.fwx_dev_solve_batch_mid(*batch_args)
        if rc:
            _lib.check(rc, "fwx_dev_solve_batch_mid")
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1)

    p = _lib.FwxSweepPatches(dt["pptr"].data_ptr(), 2 * count, dt["pindex"].data_ptr(), dt["prate"].data_ptr(),
                             dt["pnext"].data_ptr(), dt["phops"].data_ptr())
    it = _lib.FwxSweepItems(dt["iptr"].data_ptr(), 4 * count, dt["src"].data_ptr(), dt["dst"].data_ptr(),
                            outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr())
    sweep_args = (count, n, _lib.FWX_F64, vp(dbase[0].data_ptr()), vp(dbase[1].data_ptr()), vp(dbase[2].data_ptr()),
                  ctypes.byref(p), ctypes.byref(it), None, None, vp(scratch.data_ptr()), scratch.numel(), sp)

    def sweep():
        e0.record(s)
        rc = L.fwx_dev_solve_sweep_mid(*sweep_args)
        if rc:
            _lib.check(rc, "fwx_dev_solve_sweep_mid")
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1)

    prepare()
    sweep()
    batch()                                  # warm-up: code objects
    got = [o.numpy(s) for o in outs]
    solved = [w.numpy(s).reshape(count, n, n) for w in work]
    b = np.repeat(np.arange(count), 4)
    same = all(np.array_equal(bits(g), bits(m[b, t["src"], t["dst"]])) for g, m in zip(got, solved))
    del solved
    a_ms, b_ms = [], []
    for _ in range(reps):
        prepare()
        a_ms.append(sweep())
        b_ms.append(batch())
    passes = -(-n // 16)
    cell = {"n": n, "count": count, "slots": int(slots), "answers_equal_the_batch_call": bool(same)}
    cell["sweep_ms"], cell["sweep_min_ms"], cell["sweep_max_ms"] = spread(a_ms)
    cell["batch_ms"], cell["batch_min_ms"], cell["batch_max_ms"] = spread(b_ms)
    cell["sweep_over_batch"] = cell["sweep_ms"] / cell["batch_ms"]
    cell["expected_ratio_at_most"] = 1 + 2 / passes
    cell["within_expectation"] = bool(
        cell["sweep_ms"] <= cell["batch_ms"] * (1 + 2 / passes) + 2 * (cell["batch_max_ms"] - cell["batch_min_ms"]))
    tables = sum(t[k].nbytes for k in ("pptr", "pindex", "prate", "pnext", "phops", "iptr", "src", "dst"))
    cell["sweep_device_bytes"] = int(slots * per_slot + n * n * 16 + tables + 4 * count * 16)
    cell["batch_device_bytes"] = int(count * n * n * 16)
    for da in pristine + work + dbase + list(dt.values()) + outs + [scratch]:
        da.free()
    s.close()
    return cell


def host_cell(n, count, reps):
    t = sweep_of(n, count)
    p = _lib.FwxSweepPatches(t["pptr"].ctypes.data, 2 * count, t["pindex"].ctypes.data, t["prate"].ctypes.data,
                             t["pnext"].ctypes.data, t["phops"].ctypes.data)
    out = [np.zeros(4 * count), np.zeros(4 * count, dtype=np.int32), np.zeros(4 * count, dtype=np.int32)]
    it = _lib.FwxSweepItems(t["iptr"].ctypes.data, 4 * count, t["src"].ctypes.data, t["dst"].ctypes.data,
                            out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data)
    base = [a.ctypes.data for a in t["base"]]
    sweep_fn = _lib.lib().fwx_solve_sweep_mid_f64

    def sweep():
        t0 = time.perf_counter()
        rc = sweep_fn(count, n, *base, ctypes.byref(p), ctypes.byref(it), None, None)
        if rc:
            _lib.check(rc, "fwx_solve_sweep_mid_f64")
        return 1e3 * (time.perf_counter() - t0)

    b = np.repeat(np.arange(count), 4)
    parts = {}

    def batch():
        t0 = time.perf_counter()
        mats = materialise(t, n, count)
        t1 = time.perf_counter()
        engine.solve_batch_mid(*mats)
        t2 = time.perf_counter()
        parts["answers"] = [m[b, t["src"], t["dst"]] for m in mats]
        t3 = time.perf_counter()
        parts.setdefault("build_ms", []).append(1e3 * (t1 - t0))
        parts.setdefault("solve_ms", []).append(1e3 * (t2 - t1))
        parts.setdefault("index_ms", []).append(1e3 * (t3 - t2))
        return 1e3 * (t3 - t0)

    sweep()
    batch()                                  # warm-up: code objects, the per-call context
    same = all(np.array_equal(bits(g), bits(w)) for g, w in zip(out, parts["answers"]))
    parts = {}
    a_ms, b_ms = [], []
    for _ in range(reps):
        a_ms.append(sweep())
        b_ms.append(batch())
    cell = {"n": n, "count": count, "answers_equal_the_batch_call": bool(same)}
    cell["host_sweep_ms"], cell["host_sweep_min_ms"], cell["host_sweep_max_ms"] = spread(a_ms)
    cell["host_batch_ms"], cell["host_batch_min_ms"], cell["host_batch_max_ms"] = spread(b_ms)
    for k in ("build_ms", "solve_ms", "index_ms"):
        cell["host_batch_" + k] = spread(parts[k])[0]
    cell["host_batch_over_sweep"] = cell["host_batch_ms"] / cell["host_sweep_ms"]
    tables = sum(t[k].nbytes for k in ("pptr", "pindex", "prate", "pnext", "phops", "iptr", "src", "dst"))
    cell["sweep_bytes_up"] = int(sum(a.nbytes for a in t["base"]) + tables)
    cell["sweep_bytes_down"] = int(sum(a.nbytes for a in out))
    cell["batch_bytes_up"] = cell["batch_bytes_down"] = int(count * n * n * 16)
    return cell


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cells", default=",".join("%d:%d" % (n, c) for n in (129, 192, 256) for c in (256, 2048)))
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if engine.device_count() < 1:
        sys.exit("measure_sweep_mid.py: no HIP device (nothing is measured without one)")
    for k in ("FWX_BATCH_MID_MIN_N", "FWX_SWEEP_MID_SLOTS"):
        os.environ.pop(k, None)
    cells = [tuple(int(v) for v in c.split(":")) for c in args.cells.split(",")]
    result = {"what": "f64 + next + hops; two patches and four items a variant; ms; median (min, max) of %d alternating "
                      "repetitions after one warm-up" % args.reps, "device": [], "host": []}
    print(result["what"], flush=True)
    print("device form (HIP events)   slots   sweep_mid (a) [min, max]          batch_mid (b) [min, max]        (a)/(b)  "
          "bound   within   device bytes (a) / (b)", flush=True)
    for n, count in cells:
        c = device_cell(n, count, args.reps)
        result["device"].append(c)
        print("n=%3d count=%4d   %4d   %9.4f [%8.4f, %8.4f]   %9.4f [%8.4f, %8.4f]   %6.3f  %6.3f   %s   %11d / %11d%s" % (
            n, count, c["slots"], c["sweep_ms"], c["sweep_min_ms"], c["sweep_max_ms"], c["batch_ms"], c["batch_min_ms"],
            c["batch_max_ms"], c["sweep_over_batch"], c["expected_ratio_at_most"],
            "yes" if c["within_expectation"] else "NO ", c["sweep_device_bytes"], c["batch_device_bytes"],
            "" if c["answers_equal_the_batch_call"] else "   ANSWERS DIFFER"), flush=True)
    if not args.skip_host:
        print("host form (host clock)      fwx_solve_sweep_mid_f64 (c)   numpy build + fwx_solve_batch_mid_f64 + index (d) "
              "[build, solve, index]   (d)/(c)   bytes up / down (c)   bytes each way (d)", flush=True)
        for n, count in cells:
            c = host_cell(n, count, args.reps)
            result["host"].append(c)
            print("n=%3d count=%4d   %10.3f   %10.3f [%9.3f, %9.3f, %8.3f]   %7.1f   %9d / %7d   %11d%s" % (
                n, count, c["host_sweep_ms"], c["host_batch_ms"], c["host_batch_build_ms"], c["host_batch_solve_ms"],
                c["host_batch_index_ms"], c["host_batch_over_sweep"], c["sweep_bytes_up"], c["sweep_bytes_down"],
                c["batch_bytes_up"], "" if c["answers_equal_the_batch_call"] else "   ANSWERS DIFFER"), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
