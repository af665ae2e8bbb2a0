#!/usr/bin/env python3
"""The crossover of the per-k engine's group schedule (FWX_PERK_GROUP_MAX): whole
uncounted f32 D1 solves through fwx_dev_relax in ONE call, the serial schedule (FWX_PERK_PAIR_MIN_N=0) against the
schedule forced on (FWX_PERK_PAIR_MIN_N=128) at FWX_PERK_GROUP_MAX = 2, 4 and 8 and the shipped default (both variables
unset), alternated in one process on one stream; the variables are read on every call.  Per order: ms per solve of every
repetition, the medians, and whether the results of all schedules are the same bits.
usage: measure_perk_group.py [reps] [n ...]     (default: 5 repetitions of 5120 6144 8192 12288 16384)"""
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from floydwarshall_amd import engine, hip, synth  # noqa: E402

VARS = ("FWX_PERK_PAIR_MIN_N", "FWX_PERK_GROUP_MAX")
FORMS = {"serial": ("0", None), "2": ("128", "2"), "4": ("128", "4"), "8": ("128", "8"), "default": (None, None)}

args = [int(a) for a in sys.argv[1:]]
reps = args[0] if args else 5
orders = args[1:] or [5120, 6144, 8192, 12288, 16384]
hip.set_device(0)
st = hip.Stream()
for n in orders:
    rate0, _ = synth.GENERATORS["d1"](n, np.float32, synth.BASE_SEED + 1)
    pristine = hip.DeviceArray.from_numpy(rate0)
    rate = hip.DeviceArray(pristine.shape, np.float32)
    ms = {form: [] for form in FORMS}
    out = {}
    for rep in range(reps + 1):                      # the first repetition warms every schedule up
        for form, values in FORMS.items():
            for var, value in zip(VARS, values):
                os.environ.pop(var, None)
                if value is not None:
                    os.environ[var] = value
            rate.copy_(pristine, st)
            e0, e1 = hip.Event(), hip.Event()
            e0.record(st)
            engine.dev_relax(rate, n, 0, 0, n, stream=st)
            e1.record(st)
            st.synchronize()
            if rep:
                ms[form].append(round(e0.elapsed_time(e1), 3))
            else:
                out[form] = rate.numpy(st)
    same = all(bool(np.array_equal(out["serial"].view(np.uint32), out[form].view(np.uint32))) for form in FORMS)
    row = {"n": n, "same_bits": same}
    for form in FORMS:
        row[form + "_ms"] = ms[form]
        row[form + "_median"] = statistics.median(ms[form])
    print(json.dumps(row), flush=True)
    del pristine, rate, out
