#!/usr/bin/env python3
"""Where a relax_tile workgroup spends its cycles (a -DFWX_CLOCK_PROBE variant build:
python -m floydwarshall_amd.build --variant clock -DFWX_CLOCK_PROBE=1; FWX_LIB_PATH=build/variants/libfwx_clock.so).
One benchmark-shaped solve -- uncounted f32 D1, n = 16384, sixteen fwx_dev_relax calls of 1024 pivots -- per value of
FWX_PERK_GROUP_MAX: the s_memtime cycles of every workgroup of every relax_tile launch (main and cross launches alike),
summed per phase, their shares, the shader clock held inside the kernel and the mean per workgroup and per stage.
usage: measure_tile_phases.py [n] [group max ...]     (default: 16384, group max 2 and 8)"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from floydwarshall_amd import _lib, engine, hip, synth  # noqa: E402

lib = ctypes.CDLL(_lib.LIB_PATH)
lib.fwx_debug_tile_clock.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]


def clock():
    out = (ctypes.c_ulonglong * 8)()
    assert lib.fwx_debug_tile_clock(out, 1) == 0
    return [int(v) for v in out]


args = [a for a in sys.argv[1:] if a.isdigit()]
n = int(args[0]) if args else 16384
hip.set_device(0)
st = hip.Stream()
rate0, _ = synth.GENERATORS["d1"](n, np.float32, synth.BASE_SEED + 1)
pristine = hip.DeviceArray.from_numpy(rate0)
rate = hip.DeviceArray(pristine.shape, np.float32)
for gmax in args[1:] or ["2", "8"]:
    os.environ["FWX_PERK_GROUP_MAX"] = gmax
    for rep in range(2):                             # the first solve warms up
        rate.copy_(pristine, st)
        st.synchronize()
        clock()
        e0, e1 = hip.Event(), hip.Event()
        e0.record(st)
        for k0 in range(0, n, 1024):
            engine.dev_relax(rate, n, 0, k0, min(n, k0 + 1024), stream=st)
        e1.record(st)
        st.synchronize()
        first, loop, ends, store, whole, ticks, wgs, stages = clock()
    print(json.dumps({
        "n": n, "group_max": int(gmax), "solve_ms": round(e0.elapsed_time(e1), 2), "workgroups": wgs, "stages": stages,
        "shader_clock_GHz": round(whole / ticks * 0.1, 3),
        "share_load_to_first_barrier": round(first / whole, 4), "share_stage_loop": round(loop / whole, 4),
        "share_stage_end_commit_and_barrier": round(ends / whole, 4), "share_store_to_exit": round(store / whole, 4),
        "cycles_per_workgroup": {"load_to_first_barrier": round(first / wgs), "stage_loop": round(loop / wgs),
                                 "of_it_stage_ends": round(ends / wgs), "store_to_exit": round(store / wgs),
                                 "whole": round(whole / wgs)},
        "cycles_per_stage": {"stage_loop": round(loop / stages, 1), "of_it_stage_end": round(ends / stages, 1)},
        "us_per_workgroup": round(ticks / wgs / 100.0, 1)}), flush=True)
