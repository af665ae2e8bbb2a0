#!/usr/bin/env python3
"""Ragged batched small solves against what a caller with mixed orders could do before (f64 + next + hops).

History mix, device forms, HIP events on one stream over device-resident data: `count` matrices whose orders follow a
seeded ramp from 4 to 128 (a price history whose vertex set grows), solved by
  (r) one fwx_dev_solve_ragged call on the packed batch (one launch per tier, the 128-wide tier first)
  (p) the same matrices padded to 128 -- NaN rates, next -1, hops 0 -- in ONE fwx_dev_solve_batch launch
  (t) three fwx_dev_solve_batch launches over the matrices sorted into tiers and padded by hand to 16, 64 and 128,
      issued in the order of (r): the 128-wide tier first
Host-form pair, host clock around blocking calls: fwx_solve_ragged_f64 on the packed batch against
fwx_solve_batch_f64 on the batch padded to 128.
Equal orders, device forms: a ragged batch whose orders are all n against fwx_dev_solve_batch on the same input, per
cell (n, count) -- what the per-matrix indirection costs.  Both are called through ctypes with arguments built once.

Every timed launch runs on unsolved data: the device arrays are re-uploaded before every repetition; where a copy of
the batch is small, `inner` pristine copies (as many as fit 1 GiB, at most 32) are solved between the two events and
the time per copy is reported.  One warm-up repetition per variant, then REPS repetitions in which the variants
alternate; median, minimum and maximum of each.

No torch in the process.  usage: measure_ragged.py [--out FILE.json] [--reps 5] [--count 4096] [--cells n:count,...]"""
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

KINDS = ("d1", "d2", "t1", "t3")
PAD = (np.nan, -1, 0)                 # what the kernels pad their tiles with: inert in every pivot step


def ramp_orders(count, seed=11):
    """Orders rising from 4 to 128 over the batch with a seeded jitter of +-3."""
    rnd = np.random.default_rng(seed)
    base = 4 + 124 * np.arange(count) / max(count - 1, 1)
    return np.clip(np.round(base + rnd.integers(-3, 4, count)), 4, 128).astype(np.int32)


def matrices_of(orders):
    """One matrix per entry of `orders`: (rate, next, hops) of synth.make, one seeded matrix per distinct order."""
    made = {}
    for n in sorted(set(int(n) for n in orders)):
        made[n] = synth.make(KINDS[n % 4], n, np.float64, seed=synth.BASE_SEED + 2000 + n)
    return [made[int(n)] for n in orders]


def packed(mats):
    return [np.concatenate([m[f].reshape(-1) for m in mats]) for f in range(3)]


def padded(mats, tile):
    out = [np.full((len(mats), tile, tile), PAD[f], dtype=mats[0][f].dtype) for f in range(3)]
    for b, m in enumerate(mats):
        n = m[0].shape[0]
        for f in range(3):
            out[f][b, :n, :n] = m[f]
    return [a.reshape(-1) for a in out]


def alternate(variants, reps):
    """variants: {name: (prepare, run)}.  One warm-up each, then reps rounds in which the variants take turns.
    {name: (median, min, max)} in ms."""
    for prepare, run in variants.values():
        prepare()
        run()
    times = {name: [] for name in variants}
    for _ in range(reps):
        for name, (prepare, run) in variants.items():
            prepare()
            times[name].append(run())
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


class DeviceBatch:
    """`inner` pristine copies of three flat host arrays on the device, re-uploaded by prepare()."""

    def __init__(self, flat, inner=1):
        self.inner, self.cells = inner, len(flat[0])
        self.host = [np.ascontiguousarray(np.tile(a, (inner, 1))) for a in flat]       # one copy per row
        self.dev = [hip.DeviceArray(a.shape, a.dtype) for a in self.host]

    def prepare(self):
        for da, a in zip(self.dev, self.host):
            da.copy_from_host(a)

    def copy(self, i):
        return [da.rows(i, i + 1) for da in self.dev]

    def free(self):
        for da in self.dev:
            da.free()


def timed(s, e0, e1, launches, per=1):
    e0.record(s)
    launches()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) / per


def put(a):
    return hip.DeviceArray.from_numpy(np.ascontiguousarray(a))


def history_mix(count, reps):
    orders = ramp_orders(count)
    mats = matrices_of(orders)
    offset, order, tiers = engine.ragged_plan(orders)
    d_n, d_off, d_order = put(orders), put(offset[:-1]), put(order)
    ragged = DeviceBatch(packed(mats))
    pad128 = DeviceBatch(padded(mats, 128))
    groups = [[m for m, n in zip(mats, orders) if lo < n <= hi] for lo, hi in ((0, 16), (16, 64), (64, 128))]
    assert [len(g) for g in groups] == [int(t) for t in tiers]
    by_hand = [(DeviceBatch(padded(g, tile)), len(g), tile) for g, tile in zip(groups, (16, 64, 128)) if g]
    s = hip.Stream()
    e0, e1 = hip.Event(), hip.Event()

    def run_ragged():
        r, x, h = ragged.dev
        return timed(s, e0, e1, lambda: engine.dev_solve_ragged(r, d_n, d_off, d_order, tiers, next_t=x, hops_t=h,
                                                                 stream=s))

    def run_pad128():
        r, x, h = pad128.dev
        return timed(s, e0, e1, lambda: engine.dev_solve_batch(r, count, 128, next_t=x, hops_t=h, stream=s))

    def launch_by_hand():
        for batch, c, tile in reversed(by_hand):
            r, x, h = batch.dev
            engine.dev_solve_batch(r, c, tile, next_t=x, hops_t=h, stream=s)

    def prepare_by_hand():
        for batch, _, _ in by_hand:
            batch.prepare()
        hip.synchronize()

    def sync_after(prepare):
        def go():
            prepare()
            hip.synchronize()
        return go

    os.environ.pop("FWX_BATCH_WAVE_MAX_N", None)
    got = alternate({"ragged": (sync_after(ragged.prepare), run_ragged),
                     "padded_128": (sync_after(pad128.prepare), run_pad128),
                     "three_by_hand": (prepare_by_hand, lambda: timed(s, e0, e1, launch_by_hand))}, reps)
    cell = {"count": count, "orders": "seeded ramp 4..128", "tier_count": [int(t) for t in tiers],
            "cells_packed": int(offset[-1]), "cells_padded_128": count * 128 * 128}
    for name, (med, lo, hi) in got.items():
        cell[name + "_ms"], cell[name + "_min_ms"], cell[name + "_max_ms"] = med, lo, hi
    cell["padded_128_over_ragged"] = cell["padded_128_ms"] / cell["ragged_ms"]
    cell["ragged_minus_three_by_hand_ms"] = cell["ragged_ms"] - cell["three_by_hand_ms"]
    cell["three_by_hand_spread_ms"] = cell["three_by_hand_max_ms"] - cell["three_by_hand_min_ms"]
    cell["ragged_beats_padded_128"] = cell["ragged_ms"] < cell["padded_128_ms"]
    cell["ragged_within_spread_of_three_by_hand"] = \
        cell["ragged_minus_three_by_hand_ms"] <= cell["three_by_hand_spread_ms"]
    for b in [ragged, pad128] + [b for b, _, _ in by_hand]:
        b.free()
    s.close()
    return cell, mats, orders


def host_pair(mats, orders, reps):
    count = len(mats)
    pristine_r, pristine_p = packed(mats), padded(mats, 128)
    work_r, work_p = [a.copy() for a in pristine_r], [a.copy() for a in pristine_p]
    rates_p = [a.reshape(count, 128, 128) for a in work_p]
    n_each = np.ascontiguousarray(orders, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def restore(work, pristine):
        def go():
            for w, q in zip(work, pristine):
                np.copyto(w, q)
        return go

    def run_ragged():
        t0 = time.perf_counter()
        _lib.check(_lib.lib().fwx_solve_ragged_f64(count, p(n_each), p(work_r[0]), p(work_r[1]), p(work_r[2]), None,
                                                   None), "fwx_solve_ragged_f64")
        return 1e3 * (time.perf_counter() - t0)

    def run_padded():
        t0 = time.perf_counter()
        engine.solve_batch(*rates_p)
        return 1e3 * (time.perf_counter() - t0)

    got = alternate({"host_ragged": (restore(work_r, pristine_r), run_ragged),
                     "host_padded_128": (restore(work_p, pristine_p), run_padded)}, reps)
    cell = {"count": count, "bytes_packed": sum(a.nbytes for a in pristine_r),
            "bytes_padded_128": sum(a.nbytes for a in pristine_p)}
    for name, (med, lo, hi) in got.items():
        cell[name + "_ms"], cell[name + "_min_ms"], cell[name + "_max_ms"] = med, lo, hi
    cell["host_padded_128_over_ragged"] = cell["host_padded_128_ms"] / cell["host_ragged_ms"]
    return cell


def equal_orders(n, count, reps):
    mats = [synth.make(KINDS[b % 4], n, np.float64, seed=synth.BASE_SEED + 1000 + b) for b in range(8)]
    mats = [mats[b % 8] for b in range(count)]
    flat = packed(mats)
    inner = max(1, min(32, (1 << 30) // sum(a.nbytes for a in flat)))
    batch = DeviceBatch(flat, inner)
    orders = np.full(count, n, dtype=np.int32)
    offset, order, tiers = engine.ragged_plan(orders)
    d_n, d_off, d_order = put(orders), put(offset[:-1]), put(order)
    s = hip.Stream()
    e0, e1 = hip.Event(), hip.Event()

    def prepare():
        batch.prepare()
        hip.synchronize()

    # both entry points through ctypes with arguments built once: a launch of 25 us is shorter than either Python
    # wrapper, and the wrappers differ, so a window over engine.dev_solve_* would time them and not the library
    vp = ctypes.c_void_p
    L = _lib.lib()
    tiers_p = vp(tiers.ctypes.data)
    ptrs = [[vp(a.data_ptr()) for a in batch.copy(i)] for i in range(inner)]
    index = [vp(a.data_ptr()) for a in (d_n, d_off, d_order)]

    def ragged():
        for r, x, h in ptrs:
            L.fwx_dev_solve_ragged(count, _lib.FWX_F64, r, x, h, index[0], index[1], index[2], tiers_p, None, None,
                                   s.ptr)

    def uniform():
        for r, x, h in ptrs:
            L.fwx_dev_solve_batch(count, n, _lib.FWX_F64, r, x, h, n * n, 0, 0, None, s.ptr)

    for r, x, h in ptrs[:1]:                 # statuses once, outside the windows
        _lib.check(L.fwx_dev_solve_ragged(count, _lib.FWX_F64, r, x, h, index[0], index[1], index[2], tiers_p, None,
                                          None, s.ptr), "fwx_dev_solve_ragged")
        _lib.check(L.fwx_dev_solve_batch(count, n, _lib.FWX_F64, r, x, h, n * n, 0, 0, None, s.ptr),
                   "fwx_dev_solve_batch")

    os.environ.pop("FWX_BATCH_WAVE_MAX_N", None)
    got = alternate({"ragged": (prepare, lambda: timed(s, e0, e1, ragged, inner)),
                     "uniform": (prepare, lambda: timed(s, e0, e1, uniform, inner))}, reps)
    cell = {"n": n, "count": count, "launches_per_window": inner}
    for name, (med, lo, hi) in got.items():
        cell[name + "_ms"], cell[name + "_min_ms"], cell[name + "_max_ms"] = med, lo, hi
    cell["uniform_spread_ms"] = cell["uniform_max_ms"] - cell["uniform_min_ms"]
    cell["ragged_minus_uniform_ms"] = cell["ragged_ms"] - cell["uniform_ms"]
    cell["within_twice_the_uniform_spread"] = cell["ragged_minus_uniform_ms"] <= 2 * cell["uniform_spread_ms"]
    batch.free()
    s.close()
    return cell


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--count", type=int, default=4096)
    ap.add_argument("--cells", default=",".join("%d:%d" % (n, c) for n in (4, 16, 64, 128) for c in (256, 4096)))
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if engine.device_count() < 1:
        sys.exit("measure_ragged.py: no HIP device (nothing is measured without one)")
    result = {"what": "f64 + next + hops; ms; median (min, max) of %d repetitions after one warm-up, the variants "
                      "taking turns; every timed launch on unsolved data" % args.reps}
    mix, mats, orders = history_mix(args.count, args.reps)
    result["history_mix"] = mix
    print("history mix, %d matrices, orders in a seeded ramp 4..128, tiers %r (device forms, HIP events, ms)"
          % (args.count, mix["tier_count"]), flush=True)
    for name in ("ragged", "padded_128", "three_by_hand"):
        print("  %-14s %9.4f  (min %9.4f, max %9.4f)" % (name, mix[name + "_ms"], mix[name + "_min_ms"],
                                                        mix[name + "_max_ms"]), flush=True)
    print("  padded_128 / ragged = %.2f; ragged - three_by_hand = %+.4f ms against a spread of %.4f ms of "
          "three_by_hand: %s" % (mix["padded_128_over_ragged"], mix["ragged_minus_three_by_hand_ms"],
                                 mix["three_by_hand_spread_ms"],
                                 "within" if mix["ragged_within_spread_of_three_by_hand"] else "OUTSIDE"), flush=True)
    if not args.skip_host:
        hp = host_pair(mats, orders, args.reps)
        result["host_pair"] = hp
        print("host forms, the same ramp (host clock, ms): fwx_solve_ragged_f64 %.3f (min %.3f, max %.3f), "
              "fwx_solve_batch_f64 padded to 128 %.3f (min %.3f, max %.3f), ratio %.2f" % (
                  hp["host_ragged_ms"], hp["host_ragged_min_ms"], hp["host_ragged_max_ms"], hp["host_padded_128_ms"],
                  hp["host_padded_128_min_ms"], hp["host_padded_128_max_ms"], hp["host_padded_128_over_ragged"]),
              flush=True)
    del mats
    result["equal_orders"] = []
    print("equal orders (device forms, ms)   ragged      uniform   difference   uniform spread   within twice it",
          flush=True)
    for n, count in (tuple(int(v) for v in c.split(":")) for c in args.cells.split(",")):
        c = equal_orders(n, count, args.reps)
        result["equal_orders"].append(c)
        print("n=%3d count=%4d   %14.4f %12.4f %+12.4f %16.4f   %s" % (
            n, count, c["ragged_ms"], c["uniform_ms"], c["ragged_minus_uniform_ms"], c["uniform_spread_ms"],
            "yes" if c["within_twice_the_uniform_spread"] else "NO"), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
