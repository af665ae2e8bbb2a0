#!/usr/bin/env python3
"""Batched what-if sweeps against the batch call on materialised variants (f64 + next + hops).

Every cell (n, count): the base is synth d2 of order n; variant b multiplies one quote by 4 and divides the opposite
quote by 4 (two patches) and asks for four entries, the patched pair among them.

Device form, HIP events on one stream over device-resident data:
  (a) one fwx_dev_solve_sweep launch, items only (reads the base and the tables, writes 4 * count answers)
  (b) one fwx_dev_solve_batch launch on the same variants materialised on the device beforehand
The two are timed ALTERNATELY, repetition by repetition.  (b) solves in place, so the device holds `inner` pristine
copies of the materialised batch (as many as fit 1 GiB, at most 32), re-uploaded before every repetition; both calls
launch `inner` times between the two events and report the time per launch.  One warm-up repetition, then the median
of REPS and the spread (min, max) of each.  The expectation: (a) is not slower than (b) by more than twice (b)'s spread.

Host form, host clock around blocking calls:
  (c) fwx_solve_sweep_f64 on the base and the tables
  (d) numpy builds the `count` matrices, fwx_solve_batch_f64 solves them, numpy indexes the answers
with the bytes each moves to and from the device.

--resources FILE: kernel resource usage recorded at build time (-Rpass-analysis=kernel-resource-usage of the parent
and of this tree, a JSON object {"old": {kernel: {...}}, "new": {...}}); the small-solve and wave-solve kernels of it
are copied into the result and printed.

No torch in the process.  usage: measure_sweep.py [--out FILE.json] [--reps 7] [--cells n:count,...]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from floydwarshall_amd import _lib, engine, hip, synth  # noqa: E402


def sweep_of(n, count):
    """The base and the tables of a cell: dict of numpy arrays."""
    base = synth.make("d2", n, np.float64, seed=synth.BASE_SEED + 3000)
    rnd = np.random.default_rng(1000 * n + count)
    i = rnd.integers(n, size=count)
    j = (i + 1 + rnd.integers(n - 1, size=count)) % n
    r = base[0]
    t = {"base": base, "pptr": 2 * np.arange(count + 1, dtype=np.int64), "iptr": 4 * np.arange(count + 1, dtype=np.int64)}
    t["pindex"] = np.stack([i * n + j, j * n + i], axis=1).reshape(-1).astype(np.int64)
    t["prate"] = np.stack([r[i, j] * 4.0, r[j, i] / 4.0], axis=1).reshape(-1)
    t["pnext"] = np.stack([j, i], axis=1).reshape(-1).astype(np.int32)
    t["phops"] = np.ones(2 * count, dtype=np.int32)
    t["src"] = np.stack([i, j, rnd.integers(n, size=count), rnd.integers(n, size=count)], axis=1).reshape(-1).astype(np.int32)
    t["dst"] = np.stack([j, i, rnd.integers(n, size=count), rnd.integers(n, size=count)], axis=1).reshape(-1).astype(np.int32)
    return t


def materialise(t, n, count):
    """What a host without the sweep call builds: count copies of the base with the patches applied."""
    out = [np.ascontiguousarray(np.broadcast_to(a, (count, n, n))).reshape(count, n * n) for a in t["base"]]
    b = np.repeat(np.arange(count), 2)
    out[0][b, t["pindex"]] = t["prate"]
    out[1][b, t["pindex"]] = t["pnext"]
    out[2][b, t["pindex"]] = t["phops"]
    return [a.reshape(count, n, n) for a in out]


def spread(samples):
    return statistics.median(samples), min(samples), max(samples)


def device_cell(n, count, reps):
    t = sweep_of(n, count)
    mats = materialise(t, n, count)
    per_copy = sum(a.nbytes for a in mats)
    inner = max(1, min(32, (1 << 30) // per_copy))
    tiled = [np.ascontiguousarray(np.tile(a.reshape(count * n, n), (inner, 1))) for a in mats]
    d = [hip.DeviceArray(a.shape, a.dtype) for a in tiled]
    dbase = [hip.DeviceArray.from_numpy(a) for a in t["base"]]
    dt = {k: hip.DeviceArray.from_numpy(t[k]) for k in ("pptr", "pindex", "prate", "pnext", "phops", "iptr", "src", "dst")}
    outs = [hip.DeviceArray((4 * count,), np.float64), hip.DeviceArray((4 * count,), np.int32),
            hip.DeviceArray((4 * count,), np.int32)]
    s = hip.Stream()
    e0, e1 = hip.Event(), hip.Event()
    rows = count * n

    def prepare():
        for da, a in zip(d, tiled):
            da.copy_from_host(a)
        hip.synchronize()

    # both calls straight through ctypes with their arguments built once: at the small orders a launch is shorter
    # than what a Python wrapper spends checking its arguments, and the window would time the wrapper
    L = _lib.lib()
    vp = ctypes.c_void_p
    sp = vp(s.ptr.value if isinstance(s.ptr, ctypes.c_void_p) else s.ptr)
    batch_args = []
    for k in range(inner):
        r, x, h = (da.rows(k * rows, (k + 1) * rows) for da in d)
        batch_args.append((count, n, _lib.FWX_F64, vp(r.data_ptr()), vp(x.data_ptr()), vp(h.data_ptr()), n * n, 0, 0,
                           None, sp))

    def batch():
        e0.record(s)
        for a in batch_args:
            rc = L.fwx_dev_solve_batch(*a)
            if rc:
                _lib.check(rc, "fwx_dev_solve_batch")
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1) / inner

    p = _lib.FwxSweepPatches(dt["pptr"].data_ptr(), 2 * count, dt["pindex"].data_ptr(), dt["prate"].data_ptr(),
                             dt["pnext"].data_ptr(), dt["phops"].data_ptr())
    it = _lib.FwxSweepItems(dt["iptr"].data_ptr(), 4 * count, dt["src"].data_ptr(), dt["dst"].data_ptr(),
                            outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr())
    sweep_args = (count, n, _lib.FWX_F64, vp(dbase[0].data_ptr()), vp(dbase[1].data_ptr()), vp(dbase[2].data_ptr()),
                  ctypes.byref(p), ctypes.byref(it), None, None, sp)

    def sweep():
        e0.record(s)
        for _ in range(inner):
            rc = L.fwx_dev_solve_sweep(*sweep_args)
            if rc:
                _lib.check(rc, "fwx_dev_solve_sweep")
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1) / inner

    os.environ.pop("FWX_BATCH_WAVE_MAX_N", None)
    prepare()
    sweep()
    batch()                                  # warm-up: code objects
    got = [o.numpy(s) for o in outs]
    solved = [da.rows(0, rows).numpy(s).reshape(count, n, n) for da in d]
    b = np.repeat(np.arange(count), 4)
    same = all(np.array_equal(g.view(np.uint64) if g.dtype == np.float64 else g,
                              (m[b, t["src"], t["dst"]]).view(np.uint64) if g.dtype == np.float64 else m[b, t["src"], t["dst"]])
               for g, m in zip(got, solved))
    a_ms, b_ms = [], []
    for _ in range(reps):
        prepare()
        a_ms.append(sweep())
        b_ms.append(batch())
    cell = {"n": n, "count": count, "launches_per_window": inner, "answers_equal_the_batch_call": bool(same)}
    cell["sweep_ms"], cell["sweep_min_ms"], cell["sweep_max_ms"] = spread(a_ms)
    cell["batch_ms"], cell["batch_min_ms"], cell["batch_max_ms"] = spread(b_ms)
    cell["sweep_over_batch"] = cell["sweep_ms"] / cell["batch_ms"]
    cell["within_twice_the_batch_spread"] = bool(
        cell["sweep_ms"] <= cell["batch_ms"] + 2 * (cell["batch_max_ms"] - cell["batch_min_ms"]))
    for da in d + dbase + list(dt.values()) + outs:
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
    sweep_fn = _lib.lib().fwx_solve_sweep_f64

    def sweep():
        t0 = time.perf_counter()
        rc = sweep_fn(count, n, *base, ctypes.byref(p), ctypes.byref(it), None, None)
        if rc:
            _lib.check(rc, "fwx_solve_sweep_f64")
        return 1e3 * (time.perf_counter() - t0)

    b = np.repeat(np.arange(count), 4)
    parts = {}

    def batch():
        t0 = time.perf_counter()
        mats = materialise(t, n, count)
        t1 = time.perf_counter()
        engine.solve_batch(*mats)
        t2 = time.perf_counter()
        parts["answers"] = [m[b, t["src"], t["dst"]] for m in mats]
        t3 = time.perf_counter()
        parts.setdefault("build_ms", []).append(1e3 * (t1 - t0))
        parts.setdefault("solve_ms", []).append(1e3 * (t2 - t1))
        parts.setdefault("index_ms", []).append(1e3 * (t3 - t2))
        return 1e3 * (t3 - t0)

    sweep()
    batch()                                  # warm-up: code objects, the per-call context
    same = all(np.array_equal(g.view(np.uint64) if g.dtype == np.float64 else g,
                              w.view(np.uint64) if w.dtype == np.float64 else w) for g, w in zip(out, parts["answers"]))
    parts = {}
    a_ms, b_ms = [], []
    for _ in range(reps):
        a_ms.append(sweep())
        b_ms.append(batch())
    cell = {"n": n, "count": count, "answers_equal_the_batch_call": bool(same)}
    cell["host_sweep_ms"], cell["host_sweep_min_ms"], cell["host_sweep_max_ms"] = spread(a_ms)
    cell["host_batch_ms"], cell["host_batch_min_ms"], cell["host_batch_max_ms"] = spread(b_ms)
    for k in ("build_ms", "solve_ms", "index_ms"):
        cell["host_batch_" + k] = statistics.median(parts[k])
    cell["host_batch_over_sweep"] = cell["host_batch_ms"] / cell["host_sweep_ms"]
    tables = sum(t[k].nbytes for k in ("pptr", "pindex", "prate", "pnext", "phops", "iptr", "src", "dst"))
    cell["sweep_bytes_up"] = int(sum(a.nbytes for a in t["base"]) + tables)
    cell["sweep_bytes_down"] = int(sum(a.nbytes for a in out))
    cell["batch_bytes_up"] = cell["batch_bytes_down"] = int(count * n * n * 16)
    return cell


def resource_lines(path):
    with open(path) as f:
        usage = json.load(f)
    keep = {}
    for side in ("old", "new"):
        keep[side] = {k: v for k, v in usage.get(side, {}).items()
                      if any(s in k for s in ("small_solve", "wave_solve"))}
    return keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cells", default=",".join("%d:%d" % (n, c) for n in (4, 16, 64, 128) for c in (256, 4096)))
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--resources")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if engine.device_count() < 1:
        sys.exit("measure_sweep.py: no HIP device (nothing is measured without one)")
    cells = [tuple(int(v) for v in c.split(":")) for c in args.cells.split(",")]
    result = {"what": "f64 + next + hops; two patches and four items a variant; ms; median (min, max) of %d alternating "
                      "repetitions after one warm-up" % args.reps, "device": [], "host": []}
    print(result["what"], flush=True)
    print("device form (HIP events)    sweep (a) [min, max]            batch (b) [min, max]           (a)/(b)  within 2x spread of (b)",
          flush=True)
    for n, count in cells:
        c = device_cell(n, count, args.reps)
        result["device"].append(c)
        print("n=%3d count=%4d   %9.4f [%8.4f, %8.4f]   %9.4f [%8.4f, %8.4f]   %6.3f   %s%s" % (
            n, count, c["sweep_ms"], c["sweep_min_ms"], c["sweep_max_ms"], c["batch_ms"], c["batch_min_ms"],
            c["batch_max_ms"], c["sweep_over_batch"], "yes" if c["within_twice_the_batch_spread"] else "NO",
            "" if c["answers_equal_the_batch_call"] else "   ANSWERS DIFFER"), flush=True)
    if not args.skip_host:
        print("host form (host clock)      fwx_solve_sweep_f64 (c)   numpy build + fwx_solve_batch_f64 + index (d) "
              "[build, solve, index]   (d)/(c)   bytes up / down (c)   bytes each way (d)", flush=True)
        for n, count in cells:
            c = host_cell(n, count, args.reps)
            result["host"].append(c)
            print("n=%3d count=%4d   %10.3f   %10.3f [%9.3f, %9.3f, %8.3f]   %7.1f   %9d / %7d   %11d%s" % (
                n, count, c["host_sweep_ms"], c["host_batch_ms"], c["host_batch_build_ms"], c["host_batch_solve_ms"],
                c["host_batch_index_ms"], c["host_batch_over_sweep"], c["sweep_bytes_up"], c["sweep_bytes_down"],
                c["batch_bytes_up"], "" if c["answers_equal_the_batch_call"] else "   ANSWERS DIFFER"), flush=True)
    if args.resources:
        result["kernel_resources"] = resource_lines(args.resources)
        print("kernel resources (gfx950): TotalSGPRs VGPRs LDS[bytes/block] scratch[bytes/lane] occupancy; old = the parent, "
              "new = this tree", flush=True)
        for side in ("old", "new"):
            for k, v in sorted(result["kernel_resources"][side].items()):
                print("%s  %-4d %-4d %-7d %-3d %-2d  %s" % (
                    side, v.get("TotalSGPRs", -1), v.get("VGPRs", -1), v.get("LDS Size [bytes/block]", -1),
                    v.get("ScratchSize [bytes/lane]", -1), v.get("Occupancy [waves/SIMD]", -1), k.split("(")[0]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
