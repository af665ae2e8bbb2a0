#!/usr/bin/env python3
"""The crossover of the per-k engine's pair schedule (FWX_PERK_PAIR_MIN_N): whole
uncounted f32 D1 solves through fwx_dev_relax, the serial schedule (FWX_PERK_PAIR_MIN_N=0) against the pair schedule
forced on (=128) and the shipped default (the variable unset), alternated in one process on one stream; the variable is
read on every call.  Per order: ms per solve of every repetition, the medians and the ratio pair / serial.  The results
of the schedules are compared bit for bit.
usage: measure_perk_pair.py [reps] [n ...]     (default: 5 repetitions of 4096 6144 8192 12288 16384)"""
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from floydwarshall_amd import engine, hip, synth  # noqa: E402

args = [int(a) for a in sys.argv[1:]]
reps = args[0] if args else 5
orders = args[1:] or [4096, 6144, 8192, 12288, 16384]
hip.set_device(0)
st = hip.Stream()
for n in orders:
    rate0, _ = synth.GENERATORS["d1"](n, np.float32, synth.BASE_SEED + 1)
    pristine = hip.DeviceArray.from_numpy(rate0)
    rate = hip.DeviceArray(pristine.shape, np.float32)
    ms = {"0": [], "128": [], None: []}
    out = {}
    for rep in range(reps + 1):                      # the first repetition warms both schedules up
        for min_n in ("0", "128", None):
            os.environ.pop("FWX_PERK_PAIR_MIN_N", None)
            if min_n is not None:
                os.environ["FWX_PERK_PAIR_MIN_N"] = min_n
            rate.copy_(pristine, st)
            e0, e1 = hip.Event(), hip.Event()
            e0.record(st)
            engine.dev_relax(rate, n, 0, 0, n, stream=st)
            e1.record(st)
            st.synchronize()
            if rep:
                ms[min_n].append(round(e0.elapsed_time(e1), 3))
            else:
                out[min_n] = rate.numpy(st)
    same = all(bool(np.array_equal(out["0"].view(np.uint32), out[k].view(np.uint32))) for k in ("128", None))
    serial, pair = statistics.median(ms["0"]), statistics.median(ms["128"])
    print(json.dumps({"n": n, "serial_ms": ms["0"], "pair_ms": ms["128"], "default_ms": ms[None], "serial_median": serial,
                      "pair_median": pair, "default_median": statistics.median(ms[None]),
                      "pair_over_serial": round(pair / serial, 4), "same_bits": same}), flush=True)
    del pristine, rate, out
