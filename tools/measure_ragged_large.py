#!/usr/bin/env python3
"""Ragged batches up to order 1024 against what a caller with such a history could do before (f64 + next + hops).

(a) A ramp, device forms, HIP events on one stream over device-resident data: `count` matrices whose orders follow a
seeded ramp from 4 to 1024 (a price history whose vertex set grows past 256), solved by
  (r) one fwx_dev_solve_ragged_large call on the packed batch, scratch for every slot (one group)
  (p) the same matrices padded to 1024 -- NaN rates, next -1, hops 0 -- in ONE fwx_dev_solve_batch_large call
  (h) the split by hand: fwx_dev_solve_ragged_mid over the matrices of order <= 256 (packed) plus ONE
      fwx_dev_solve_batch_large call over the others padded to 1024
and the host forms, host clock around blocking calls: fwx_solve_ragged_large_f64 on the packed batch against
fwx_solve_batch_large_f64 on the batch padded to 1024.
(b) Equal orders: a ragged batch whose orders are all n against fwx_dev_solve_batch_large on the same input, per cell
(n, count) -- what the slot search and the per-workgroup indirection cost.  Both through ctypes with arguments built
once; the difference stands beside the uniform call's own spread (max - min).

Method as tools/measure_ragged_mid.py, whose helpers this tool uses: every timed launch on unsolved data (re-uploaded
before every repetition), one warm-up per variant, then REPS repetitions in which the variants alternate; median,
minimum and maximum of each.

No torch in the process.
usage: measure_ragged_large.py [--out FILE.json] [--reps 5] [--count 512] [--cells n:count,...] [--skip-host]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from floydwarshall_amd import _lib, engine, hip, synth  # noqa: E402
from measure_ragged import KINDS, DeviceBatch, alternate, matrices_of, packed, padded, put, timed  # noqa: E402
from measure_ragged_mid import report, synced  # noqa: E402

SETTINGS = ("FWX_BATCH_WAVE_MAX_N", "FWX_BATCH_MID_MIN_N", "FWX_BATCH_LARGE_MIN_N")


def ramp_orders(count, seed=31):
    """Orders rising from 4 to 1024 over the batch with a seeded jitter of +-3."""
    rnd = np.random.default_rng(seed)
    base = 4 + 1020 * np.arange(count) / max(count - 1, 1)
    return np.clip(np.round(base + rnd.integers(-3, 4, count)), 4, 1024).astype(np.int32)


def scratch_for(orders):
    return hip.DeviceArray((_lib.batch_large_scratch_bytes(int(sum(int(n) for n in orders))),), np.uint8)


def ramp(count, reps):
    orders = ramp_orders(count)
    mats = matrices_of(orders)
    offset, order, tiers, work = engine.ragged_large_plan(orders)
    d_n, d_off, d_order, d_work = put(orders), put(offset[:-1]), put(order), put(work)
    s = hip.Stream()
    e0, e1 = hip.Event(), hip.Event()
    cell = {"count": count, "orders": "seeded ramp 4..1024", "tier_count": [int(t) for t in tiers],
            "cells_packed": int(offset[-1]), "cells_padded_1024": count * 1024 * 1024}

    # the variants one after the other: the padded batch is 16 bytes x count x 2^20 on the device
    ragged = DeviceBatch(packed(mats))
    sc_r = scratch_for(n for n in orders if n > 256)

    def run_ragged():
        r, x, h = ragged.dev
        return timed(s, e0, e1, lambda: engine.dev_solve_ragged_large(r, d_n, d_off, d_order, tiers, work, d_work,
                                                                       next_t=x, hops_t=h, scratch_t=sc_r, stream=s))

    small = [m for m, n in zip(mats, orders) if n <= 256]
    large = [m for m, n in zip(mats, orders) if n > 256]
    small_orders = np.array([m[0].shape[0] for m in small], dtype=np.int32)
    s_offset, s_order, s_tiers = engine.ragged_mid_plan(small_orders)
    s_n, s_off, s_ord = put(small_orders), put(s_offset[:-1]), put(s_order)
    hand_small, hand_large = DeviceBatch(packed(small)), DeviceBatch(padded(large, 1024))
    sc_h = scratch_for([1024] * len(large))

    def launch_by_hand():
        r, x, h = hand_large.dev
        engine.dev_solve_batch_large(r, len(large), 1024, next_t=x, hops_t=h, scratch_t=sc_h, stream=s)
        r, x, h = hand_small.dev
        engine.dev_solve_ragged_mid(r, s_n, s_off, s_ord, s_tiers, next_t=x, hops_t=h, stream=s)

    def prepare_by_hand():
        hand_small.prepare()
        hand_large.prepare()
        hip.synchronize()

    pad = DeviceBatch(padded(mats, 1024))
    sc_p = scratch_for([1024] * count)

    def run_padded():
        r, x, h = pad.dev
        return timed(s, e0, e1, lambda: engine.dev_solve_batch_large(r, count, 1024, next_t=x, hops_t=h,
                                                                      scratch_t=sc_p, stream=s))

    got = alternate({"ragged_large": (synced(ragged.prepare), run_ragged),
                     "padded_1024": (synced(pad.prepare), run_padded),
                     "split_by_hand": (prepare_by_hand, lambda: timed(s, e0, e1, launch_by_hand))}, reps)
    cell["split_by_hand"] = {"ragged_mid_tier_count": [int(t) for t in s_tiers], "padded_to_1024": len(large)}
    first = np.zeros(4, dtype=np.int32)
    totals = np.zeros(3, dtype=np.int64)
    cell["groups"] = int(_lib.lib().fwx_test_ragged_large_schedule(count, int(tiers[4]), work.ctypes.data,
                                                                   sc_r.numel(), first.ctypes.data, 4, totals.ctypes.data))
    cell["launches"], cell["panel_workgroups"], cell["sweep_workgroups"] = (int(v) for v in totals)
    report(cell, got)
    cell["padded_1024_over_ragged_large"] = cell["padded_1024_ms"] / cell["ragged_large_ms"]
    cell["split_by_hand_over_ragged_large"] = cell["split_by_hand_ms"] / cell["ragged_large_ms"]
    cell["ragged_large_beats_padded_1024"] = cell["ragged_large_max_ms"] < cell["padded_1024_min_ms"]
    cell["ragged_large_beats_split_by_hand"] = cell["ragged_large_max_ms"] < cell["split_by_hand_min_ms"]
    for b in (ragged, pad, hand_small, hand_large):
        b.free()
    for a in (sc_r, sc_h, sc_p):
        a.free()
    s.close()
    return cell, mats, orders


def host_pair(mats, orders, reps):
    count = len(mats)
    pristine_r, pristine_p = packed(mats), padded(mats, 1024)
    work_r, work_p = [a.copy() for a in pristine_r], [a.copy() for a in pristine_p]
    rates_p = [a.reshape(count, 1024, 1024) for a in work_p]
    n_each = np.ascontiguousarray(orders, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def restore(work, pristine):
        def go():
            for w, q in zip(work, pristine):
                np.copyto(w, q)
        return go

    def run_ragged():
        t0 = time.perf_counter()
        _lib.check(_lib.lib().fwx_solve_ragged_large_f64(count, p(n_each), p(work_r[0]), p(work_r[1]), p(work_r[2]),
                                                         None, None), "fwx_solve_ragged_large_f64")
        return 1e3 * (time.perf_counter() - t0)

    def run_padded():
        t0 = time.perf_counter()
        engine.solve_batch_large(*rates_p)
        return 1e3 * (time.perf_counter() - t0)

    got = alternate({"host_ragged_large": (restore(work_r, pristine_r), run_ragged),
                     "host_padded_1024": (restore(work_p, pristine_p), run_padded)}, reps)
    cell = {"count": count, "bytes_packed": sum(a.nbytes for a in pristine_r),
            "bytes_padded_1024": sum(a.nbytes for a in pristine_p)}
    report(cell, got)
    cell["host_padded_1024_over_ragged_large"] = cell["host_padded_1024_ms"] / cell["host_ragged_large_ms"]
    return cell


def equal_orders(n, count, reps):
    mats = [synth.make(KINDS[b % 4], n, np.float64, seed=synth.BASE_SEED + 1000 + b) for b in range(8)]
    mats = [mats[b % 8] for b in range(count)]
    flat = packed(mats)
    inner = max(1, min(8, (1 << 30) // sum(a.nbytes for a in flat)))
    batch = DeviceBatch(flat, inner)
    orders = np.full(count, n, dtype=np.int32)
    offset, order, tiers, work = engine.ragged_large_plan(orders)
    assert list(tiers) == [0, 0, 0, 0, count]
    d_n, d_off, d_order, d_work = put(orders), put(offset[:-1]), put(order), put(work)
    scratch = scratch_for(orders)
    s = hip.Stream()
    e0, e1 = hip.Event(), hip.Event()
    vp = ctypes.c_void_p
    L = _lib.lib()
    tiers_p, work_p = vp(tiers.ctypes.data), vp(work.ctypes.data)
    ptrs = [[vp(a.data_ptr()) for a in batch.copy(i)] for i in range(inner)]
    index = [vp(a.data_ptr()) for a in (d_n, d_off, d_order, d_work)]
    sc, sc_bytes = vp(scratch.data_ptr()), scratch.numel()

    def ragged():
        for r, x, h in ptrs:
            L.fwx_dev_solve_ragged_large(count, _lib.FWX_F64, r, x, h, index[0], index[1], index[2], tiers_p, work_p,
                                         index[3], None, None, sc, sc_bytes, s.ptr)

    def uniform():
        for r, x, h in ptrs:
            L.fwx_dev_solve_batch_large(count, n, _lib.FWX_F64, r, x, h, n * n, 0, 0, None, sc, sc_bytes, s.ptr)

    batch.prepare()
    r, x, h = ptrs[0]                        # statuses once, outside the windows
    _lib.check(L.fwx_dev_solve_ragged_large(count, _lib.FWX_F64, r, x, h, index[0], index[1], index[2], tiers_p, work_p,
                                            index[3], None, None, sc, sc_bytes, s.ptr), "fwx_dev_solve_ragged_large")
    _lib.check(L.fwx_dev_solve_batch_large(count, n, _lib.FWX_F64, r, x, h, n * n, 0, 0, None, sc, sc_bytes, s.ptr),
               "fwx_dev_solve_batch_large")
    s.synchronize()
    got = alternate({"ragged_large": (synced(batch.prepare), lambda: timed(s, e0, e1, ragged, inner)),
                     "uniform": (synced(batch.prepare), lambda: timed(s, e0, e1, uniform, inner))}, reps)
    cell = {"n": n, "count": count, "launches_per_window": inner}
    report(cell, got)
    cell["uniform_spread_ms"] = cell["uniform_max_ms"] - cell["uniform_min_ms"]
    cell["ragged_large_minus_uniform_ms"] = cell["ragged_large_ms"] - cell["uniform_ms"]
    cell["ragged_large_over_uniform"] = cell["ragged_large_ms"] / cell["uniform_ms"]
    cell["within_twice_the_uniform_spread"] = cell["ragged_large_minus_uniform_ms"] <= 2 * cell["uniform_spread_ms"]
    batch.free()
    scratch.free()
    s.close()
    return cell


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--count", type=int, default=512)
    ap.add_argument("--cells", default=",".join("%d:%d" % (n, c) for n in (257, 512, 1024) for c in (16, 256)))
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--skip-ramp", action="store_true")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if engine.device_count() < 1:
        sys.exit("measure_ragged_large.py: no HIP device (nothing is measured without one)")
    for name in SETTINGS:
        os.environ.pop(name, None)
    result = {"what": "f64 + next + hops; ms; median (min, max) of %d repetitions after one warm-up, the variants "
                      "taking turns; every timed launch on unsolved data" % args.reps}

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")

    result["equal_orders"] = []
    print("equal orders (device forms, ms)  ragged_large    uniform   difference   uniform spread   within twice it",
          flush=True)
    for n, count in (tuple(int(v) for v in c.split(":")) for c in args.cells.split(",") if c):
        c = equal_orders(n, count, args.reps)
        result["equal_orders"].append(c)
        print("n=%4d count=%4d   %14.4f %12.4f %+12.4f %16.4f   %s" % (
            n, count, c["ragged_large_ms"], c["uniform_ms"], c["ragged_large_minus_uniform_ms"], c["uniform_spread_ms"],
            "yes" if c["within_twice_the_uniform_spread"] else "NO"), flush=True)
        save()
    if not args.skip_ramp:
        mix, mats, orders = ramp(args.count, args.reps)
        result["ramp"] = mix
        print("ramp, %d matrices, orders in a seeded ramp 4..1024, tiers (wave, 64, 128, mid, large) %r, %d group(s), "
              "%d launches, %d panel and %d sweep workgroups; split by hand: ragged-mid tiers %r + %d matrices padded "
              "to 1024 (device forms, HIP events, ms)"
              % (args.count, mix["tier_count"], mix["groups"], mix["launches"], mix["panel_workgroups"],
                 mix["sweep_workgroups"], mix["split_by_hand"]["ragged_mid_tier_count"],
                 mix["split_by_hand"]["padded_to_1024"]), flush=True)
        for name in ("ragged_large", "padded_1024", "split_by_hand"):
            print("  %-14s %9.4f  (min %9.4f, max %9.4f)" % (name, mix[name + "_ms"], mix[name + "_min_ms"],
                                                            mix[name + "_max_ms"]), flush=True)
        print("  padded_1024 / ragged_large = %.2f (%s); split_by_hand / ragged_large = %.2f (%s)" % (
            mix["padded_1024_over_ragged_large"],
            "ranges apart" if mix["ragged_large_beats_padded_1024"] else "RANGES OVERLAP",
            mix["split_by_hand_over_ragged_large"],
            "ranges apart" if mix["ragged_large_beats_split_by_hand"] else "RANGES OVERLAP"), flush=True)
        save()
        if not args.skip_host:
            hp = host_pair(mats, orders, args.reps)
            result["host_pair"] = hp
            print("host forms, the same ramp (host clock, ms): fwx_solve_ragged_large_f64 %.3f (min %.3f, max %.3f), "
                  "fwx_solve_batch_large_f64 padded to 1024 %.3f (min %.3f, max %.3f), ratio %.2f" % (
                      hp["host_ragged_large_ms"], hp["host_ragged_large_min_ms"], hp["host_ragged_large_max_ms"],
                      hp["host_padded_1024_ms"], hp["host_padded_1024_min_ms"], hp["host_padded_1024_max_ms"],
                      hp["host_padded_1024_over_ragged_large"]), flush=True)
    save()


if __name__ == "__main__":
    main()
