#!/usr/bin/env python3
"""Ragged batches up to order 256 against what a caller with such a history could do before (f64 + next + hops).

History mix, device forms, HIP events on one stream over device-resident data: `count` matrices whose orders follow a
seeded ramp from 4 to 256 (a price history whose vertex set grows past 128), solved by
  (r) one fwx_dev_solve_ragged_mid call on the packed batch (one launch per tier, the mid tier first)
  (a) the same matrices padded to 256 -- NaN rates, next -1, hops 0 -- in ONE fwx_dev_solve_batch_mid launch
  (b) the split by hand: fwx_dev_solve_ragged over the matrices of order <= 128 (packed) plus ONE
      fwx_dev_solve_batch_mid launch over the others padded to 256, the mid launch first
Equal orders (c): a ragged batch whose orders are all n against fwx_dev_solve_batch_mid on the same input, per cell
(n, count) -- what the per-workgroup indirection costs.  Both through ctypes with arguments built once.
Host forms, host clock around blocking calls: fwx_solve_ragged_mid_f64 on the packed batch against
fwx_solve_batch_mid_f64 on the batch padded to 256.
Lists: the traced fwx_dev_solve_ragged_mid plus one fwx_dev_exact_paths_ragged_mid walk of `--lists` seeded items
against the untraced call.

Method as tools/measure_ragged.py, whose helpers this tool uses: every timed launch on unsolved data (re-uploaded
before every repetition), one warm-up per variant, then REPS repetitions in which the variants alternate; median,
minimum and maximum of each.

No torch in the process.
usage: measure_ragged_mid.py [--out FILE.json] [--reps 5] [--count 4096] [--cells n:count,...] [--lists 65536]"""
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


def ramp_orders(count, seed=22):
    """Orders rising from 4 to 256 over the batch with a seeded jitter of +-3."""
    rnd = np.random.default_rng(seed)
    base = 4 + 252 * np.arange(count) / max(count - 1, 1)
    return np.clip(np.round(base + rnd.integers(-3, 4, count)), 4, 256).astype(np.int32)


def synced(prepare):
    def go():
        prepare()
        hip.synchronize()
    return go


def report(cell, got):
    for name, (med, lo, hi) in got.items():
        cell[name + "_ms"], cell[name + "_min_ms"], cell[name + "_max_ms"] = med, lo, hi


def history_mix(count, reps, items):
    orders = ramp_orders(count)
    mats = matrices_of(orders)
    offset, order, tiers = engine.ragged_mid_plan(orders)
    d_n, d_off, d_order = put(orders), put(offset[:-1]), put(order)
    ragged = DeviceBatch(packed(mats))
    pad256 = DeviceBatch(padded(mats, 256))
    small = [m for m, n in zip(mats, orders) if n <= 128]
    large = [m for m, n in zip(mats, orders) if n > 128]
    small_orders = np.array([m[0].shape[0] for m in small], dtype=np.int32)
    s_offset, s_order, s_tiers = engine.ragged_plan(small_orders)
    s_n, s_off, s_ord = put(small_orders), put(s_offset[:-1]), put(s_order)
    hand_small, hand_large = DeviceBatch(packed(small)), DeviceBatch(padded(large, 256))
    s = hip.Stream()
    e0, e1 = hip.Event(), hip.Event()

    def run_ragged():
        r, x, h = ragged.dev
        return timed(s, e0, e1, lambda: engine.dev_solve_ragged_mid(r, d_n, d_off, d_order, tiers, next_t=x, hops_t=h,
                                                                     stream=s))

    def run_pad256():
        r, x, h = pad256.dev
        return timed(s, e0, e1, lambda: engine.dev_solve_batch_mid(r, count, 256, next_t=x, hops_t=h, stream=s))

    def launch_by_hand():
        r, x, h = hand_large.dev
        engine.dev_solve_batch_mid(r, len(large), 256, next_t=x, hops_t=h, stream=s)
        r, x, h = hand_small.dev
        engine.dev_solve_ragged(r, s_n, s_off, s_ord, s_tiers, next_t=x, hops_t=h, stream=s)

    def prepare_by_hand():
        hand_small.prepare()
        hand_large.prepare()
        hip.synchronize()

    os.environ.pop("FWX_BATCH_WAVE_MAX_N", None)
    os.environ.pop("FWX_BATCH_MID_MIN_N", None)
    got = alternate({"ragged_mid": (synced(ragged.prepare), run_ragged),
                     "padded_256": (synced(pad256.prepare), run_pad256),
                     "split_by_hand": (prepare_by_hand, lambda: timed(s, e0, e1, launch_by_hand))}, reps)
    cell = {"count": count, "orders": "seeded ramp 4..256", "tier_count": [int(t) for t in tiers],
            "split_by_hand": {"ragged_tier_count": [int(t) for t in s_tiers], "padded_to_256": len(large)},
            "cells_packed": int(offset[-1]), "cells_padded_256": count * 256 * 256}
    report(cell, got)
    cell["padded_256_over_ragged_mid"] = cell["padded_256_ms"] / cell["ragged_mid_ms"]
    cell["split_by_hand_over_ragged_mid"] = cell["split_by_hand_ms"] / cell["ragged_mid_ms"]
    cell["ragged_mid_beats_padded_256"] = cell["ragged_mid_max_ms"] < cell["padded_256_min_ms"]
    cell["ragged_mid_beats_split_by_hand"] = cell["ragged_mid_max_ms"] < cell["split_by_hand_min_ms"]
    pad256.free()
    hand_small.free()
    hand_large.free()

    # the traced solve plus one walk against the untraced call, on the same packed batch
    lists = None
    if items > 0:
        cells = int(offset[-1])
        trace_arrays = [hip.DeviceArray((cells,), np.int32) for _ in range(3)]
        trace = engine.Trace(0, 0, _views=tuple(trace_arrays))
        next0 = put(ragged.host[1].reshape(-1))
        rnd = np.random.default_rng(2222)
        mat = rnd.integers(0, count, items).astype(np.int32)
        src = (rnd.random(items) * orders[mat]).astype(np.int32)
        dst = (rnd.random(items) * orders[mat]).astype(np.int32)
        d_mat, d_src, d_dst = put(mat), put(src), put(dst)
        cap = 64
        out = {}

        def solve_and_walk():
            r, x, h = ragged.dev
            engine.dev_solve_ragged_mid(r, d_n, d_off, d_order, tiers, next_t=x, hops_t=h, trace=trace, stream=s)
            out["len"], out["path"] = engine.dev_exact_paths_ragged_mid(next0, d_n, d_off, 256, trace, d_mat, d_src,
                                                                        d_dst, cap, stream=s)

        got = alternate({"untraced": (synced(ragged.prepare), run_ragged),
                         "traced_and_walk": (synced(ragged.prepare), lambda: timed(s, e0, e1, solve_and_walk))}, reps)
        lens = out["len"].numpy()
        lists = {"items": items, "cap": cap, "items_over_cap": int((lens == _lib.FWX_ERR_CAPACITY).sum()),
                 "items_failed": int(((lens < 0) & (lens != _lib.FWX_ERR_CAPACITY)).sum())}
        report(lists, got)
        lists["traced_and_walk_over_untraced"] = lists["traced_and_walk_ms"] / lists["untraced_ms"]
    ragged.free()
    s.close()
    return cell, lists, mats, orders


def host_pair(mats, orders, reps):
    count = len(mats)
    pristine_r, pristine_p = packed(mats), padded(mats, 256)
    work_r, work_p = [a.copy() for a in pristine_r], [a.copy() for a in pristine_p]
    rates_p = [a.reshape(count, 256, 256) for a in work_p]
    n_each = np.ascontiguousarray(orders, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def restore(work, pristine):
        def go():
            for w, q in zip(work, pristine):
                np.copyto(w, q)
        return go

    def run_ragged():
        t0 = time.perf_counter()
        _lib.check(_lib.lib().fwx_solve_ragged_mid_f64(count, p(n_each), p(work_r[0]), p(work_r[1]), p(work_r[2]),
                                                       None, None), "fwx_solve_ragged_mid_f64")
        return 1e3 * (time.perf_counter() - t0)

    def run_padded():
        t0 = time.perf_counter()
        engine.solve_batch_mid(*rates_p)
        return 1e3 * (time.perf_counter() - t0)

    got = alternate({"host_ragged_mid": (restore(work_r, pristine_r), run_ragged),
                     "host_padded_256": (restore(work_p, pristine_p), run_padded)}, reps)
    cell = {"count": count, "bytes_packed": sum(a.nbytes for a in pristine_r),
            "bytes_padded_256": sum(a.nbytes for a in pristine_p)}
    report(cell, got)
    cell["host_padded_256_over_ragged_mid"] = cell["host_padded_256_ms"] / cell["host_ragged_mid_ms"]
    return cell


def equal_orders(n, count, reps):
    mats = [synth.make(KINDS[b % 4], n, np.float64, seed=synth.BASE_SEED + 1000 + b) for b in range(8)]
    mats = [mats[b % 8] for b in range(count)]
    flat = packed(mats)
    inner = max(1, min(8, (1 << 30) // sum(a.nbytes for a in flat)))
    batch = DeviceBatch(flat, inner)
    orders = np.full(count, n, dtype=np.int32)
    offset, order, tiers = engine.ragged_mid_plan(orders)
    assert list(tiers) == [0, 0, 0, count]
    d_n, d_off, d_order = put(orders), put(offset[:-1]), put(order)
    s = hip.Stream()
    e0, e1 = hip.Event(), hip.Event()
    vp = ctypes.c_void_p
    L = _lib.lib()
    tiers_p = vp(tiers.ctypes.data)
    ptrs = [[vp(a.data_ptr()) for a in batch.copy(i)] for i in range(inner)]
    index = [vp(a.data_ptr()) for a in (d_n, d_off, d_order)]

    def ragged():
        for r, x, h in ptrs:
            L.fwx_dev_solve_ragged_mid(count, _lib.FWX_F64, r, x, h, index[0], index[1], index[2], tiers_p, None, None,
                                       s.ptr)

    def uniform():
        for r, x, h in ptrs:
            L.fwx_dev_solve_batch_mid(count, n, _lib.FWX_F64, r, x, h, n * n, 0, 0, None, s.ptr)

    batch.prepare()
    r, x, h = ptrs[0]                        # statuses once, outside the windows
    _lib.check(L.fwx_dev_solve_ragged_mid(count, _lib.FWX_F64, r, x, h, index[0], index[1], index[2], tiers_p, None,
                                          None, s.ptr), "fwx_dev_solve_ragged_mid")
    _lib.check(L.fwx_dev_solve_batch_mid(count, n, _lib.FWX_F64, r, x, h, n * n, 0, 0, None, s.ptr),
               "fwx_dev_solve_batch_mid")
    s.synchronize()
    os.environ.pop("FWX_BATCH_MID_MIN_N", None)
    got = alternate({"ragged_mid": (synced(batch.prepare), lambda: timed(s, e0, e1, ragged, inner)),
                     "uniform": (synced(batch.prepare), lambda: timed(s, e0, e1, uniform, inner))}, reps)
    cell = {"n": n, "count": count, "launches_per_window": inner}
    report(cell, got)
    cell["uniform_spread_ms"] = cell["uniform_max_ms"] - cell["uniform_min_ms"]
    cell["ragged_mid_minus_uniform_ms"] = cell["ragged_mid_ms"] - cell["uniform_ms"]
    cell["ragged_mid_over_uniform"] = cell["ragged_mid_ms"] / cell["uniform_ms"]
    cell["within_twice_the_uniform_spread"] = cell["ragged_mid_minus_uniform_ms"] <= 2 * cell["uniform_spread_ms"]
    batch.free()
    s.close()
    return cell


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--count", type=int, default=4096)
    ap.add_argument("--cells", default=",".join("%d:%d" % (n, c) for n in (129, 192, 256) for c in (256, 4096)))
    ap.add_argument("--lists", type=int, default=65536)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if engine.device_count() < 1:
        sys.exit("measure_ragged_mid.py: no HIP device (nothing is measured without one)")
    result = {"what": "f64 + next + hops; ms; median (min, max) of %d repetitions after one warm-up, the variants "
                      "taking turns; every timed launch on unsolved data" % args.reps}
    mix, lists, mats, orders = history_mix(args.count, args.reps, args.lists)
    result["history_mix"] = mix
    print("history mix, %d matrices, orders in a seeded ramp 4..256, tiers (wave, 64, 128, mid) %r; split by hand: "
          "ragged tiers %r + %d matrices padded to 256 (device forms, HIP events, ms)"
          % (args.count, mix["tier_count"], mix["split_by_hand"]["ragged_tier_count"],
             mix["split_by_hand"]["padded_to_256"]), flush=True)
    for name in ("ragged_mid", "padded_256", "split_by_hand"):
        print("  %-14s %9.4f  (min %9.4f, max %9.4f)" % (name, mix[name + "_ms"], mix[name + "_min_ms"],
                                                        mix[name + "_max_ms"]), flush=True)
    print("  padded_256 / ragged_mid = %.2f (%s); split_by_hand / ragged_mid = %.2f (%s)" % (
        mix["padded_256_over_ragged_mid"], "ranges apart" if mix["ragged_mid_beats_padded_256"] else "RANGES OVERLAP",
        mix["split_by_hand_over_ragged_mid"],
        "ranges apart" if mix["ragged_mid_beats_split_by_hand"] else "RANGES OVERLAP"), flush=True)
    if lists:
        result["lists"] = lists
        print("lists, the same batch: untraced %.4f (min %.4f, max %.4f); traced + a walk of %d lists %.4f (min %.4f, "
              "max %.4f), ratio %.2f; %d items over cap %d, %d failed" % (
                  lists["untraced_ms"], lists["untraced_min_ms"], lists["untraced_max_ms"], lists["items"],
                  lists["traced_and_walk_ms"], lists["traced_and_walk_min_ms"], lists["traced_and_walk_max_ms"],
                  lists["traced_and_walk_over_untraced"], lists["items_over_cap"], lists["cap"],
                  lists["items_failed"]), flush=True)
    if not args.skip_host:
        hp = host_pair(mats, orders, args.reps)
        result["host_pair"] = hp
        print("host forms, the same ramp (host clock, ms): fwx_solve_ragged_mid_f64 %.3f (min %.3f, max %.3f), "
              "fwx_solve_batch_mid_f64 padded to 256 %.3f (min %.3f, max %.3f), ratio %.2f" % (
                  hp["host_ragged_mid_ms"], hp["host_ragged_mid_min_ms"], hp["host_ragged_mid_max_ms"],
                  hp["host_padded_256_ms"], hp["host_padded_256_min_ms"], hp["host_padded_256_max_ms"],
                  hp["host_padded_256_over_ragged_mid"]), flush=True)
    del mats
    result["equal_orders"] = []
    print("equal orders (device forms, ms)   ragged_mid    uniform   difference   uniform spread   within twice it",
          flush=True)
    for n, count in (tuple(int(v) for v in c.split(":")) for c in args.cells.split(",")):
        c = equal_orders(n, count, args.reps)
        result["equal_orders"].append(c)
        print("n=%3d count=%4d   %14.4f %12.4f %+12.4f %16.4f   %s" % (
            n, count, c["ragged_mid_ms"], c["uniform_ms"], c["ragged_mid_minus_uniform_ms"], c["uniform_spread_ms"],
            "yes" if c["within_twice_the_uniform_spread"] else "NO"), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
