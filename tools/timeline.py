#!/usr/bin/env python3
"""Timeline of one solve from a rocprofv3 --kernel-trace CSV: per kernel family the launches' durations, and for
the main launches the gaps between one's end and the next one's start (what the side chain costs the sweep).
usage: timeline.py <kernel_trace.csv> [--after NAME] [--dump]   (analyses the LAST solve: the launches after the last
launch whose name contains NAME, by default nonneg_check, the fused engine's domain check; the whole trace if there is
none.  bench.py's per-k run: --after relax_kt, the counting sweep of the solve before the timed one.)  With a side
chain beside the main launches (the fused engine's double pass, the per-k engine's pair schedule) it also prints the
chain: the other launches that start between two main launches, their span and each step's duration."""
import csv
import sys
from collections import defaultdict


def family(name):
    for key in ("fused_main_arg_f64", "fused_main_arg", "fused_main_max_f64", "fused_main_max", "fused_main",
                "fused_panels_next_f32", "fused_panels", "fused_rowpanel", "fused_colpanel", "nonneg_check", "relax_tile",
                "relax_walk", "relax_kt", "relax_k"):
        if key in name:
            return key
    return name[:40]


def main():
    rows = []
    with open(sys.argv[1]) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"],
                         int(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0), int(r.get("Grid_Size_Y", 1) or 1)))
    rows.sort()
    # last solve = launches after the last domain check
    after = sys.argv[sys.argv.index("--after") + 1] if "--after" in sys.argv else "nonneg_check"
    last = max([i for i, r in enumerate(rows) if after in r[2]] or [-1])
    rows = rows[last + 1:]
    t0 = rows[0][0]
    fam = defaultdict(list)
    for s, e, name, gx, gy in rows:
        fam[(family(name), gx * gy)].append((s - t0, e - t0))
    print("solve span: %.1f us, %d launches" % ((max(r[1] for r in rows) - t0) / 1e3, len(rows)))
    for (k, g), v in sorted(fam.items(), key=lambda kv: -sum(e - s for s, e in kv[1])):
        d = [e - s for s, e in v]
        print("  %-26s grid %9d  x%4d  avg %8.1f us  min %8.1f  max %8.1f  total %9.1f us" %
              (k, g, len(v), sum(d) / len(d) / 1e3, min(d) / 1e3, max(d) / 1e3, sum(d) / 1e3))
    # the big main launches: biggest grid of a main family
    mains = [(k, g) for (k, g) in fam if k.startswith("fused_main") or k == "relax_tile"]
    if mains:
        big = max(mains, key=lambda kg: kg[1])
        # ... and the launches of that family that leave a cross out (the pair schedule: a grid one tile shorter each way)
        same = [kg for kg in mains if kg[0] == big[0] and 2 * kg[1] >= big[1]]
        big = max(same, key=lambda kg: len(fam[kg]))
        v = sorted(x for kg in same for x in fam[kg])
        gaps = [v[i + 1][0] - v[i][1] for i in range(len(v) - 1)]
        dur = [e - s for s, e in v]
        print("main launches (%s grid %d): %d, avg %.1f us; gap between them avg %.1f us, max %.1f us; sum of durations %.1f us = %.3f of the span"
              % (big[0], big[1], len(v), sum(dur) / len(dur) / 1e3, sum(gaps) / max(len(gaps), 1) / 1e3,
                 max(gaps or [0]) / 1e3, sum(dur) / 1e3, sum(dur) / (max(r[1] for r in rows) - t0)))
        # the side chain: what starts between one main launch's start and the next one's
        chains = []
        for i in range(len(v) - 1):
            c = sorted((s, e, family(name), gx * gy) for s, e, name, gx, gy in rows
                       if v[i][0] + t0 <= s < v[i + 1][0] + t0 and (family(name), gx * gy) not in same)
            if c:
                chains.append((c, v[i], v[i + 1]))
        if chains:
            lens = [len(c) for c, _, _ in chains]
            # every kind of chain by its number of launches, the usual one first (the per-k engine's group schedule has
            # one kind per group size; those at a call's edge differ as well)
            for steps in sorted(set(lens), key=lambda n: -lens.count(n)):
                full = [x for x in chains if len(x[0]) == steps]
                span = [max(e for _, e, _, _ in c) - c[0][0] for c, _, _ in full]
                late = [max(e for _, e, _, _ in c) - (m[1] + t0) for c, m, _ in full]
                mdur = [m[1] - m[0] for _, m, _ in full]
                print("side chain: %d chains of %d launches beside main launches of avg %.1f us; span avg %.1f us, max %.1f "
                      "us; its end against the end of the main launch beside it: avg %+.1f us, max %+.1f us" %
                      (len(full), steps, sum(mdur) / len(mdur) / 1e3, sum(span) / len(span) / 1e3, max(span) / 1e3,
                       sum(late) / len(late) / 1e3, max(late) / 1e3))
                for j in range(steps):
                    d = [c[j][1] - c[j][0] for c, _, _ in full]
                    w = [c[j][0] - (c[j - 1][1] if j else m[0] + t0) for c, m, _ in full]
                    print("  step %d  %-16s grid %8d  avg %7.1f us  max %7.1f us   starts %7.1f us after %s" %
                          (j, full[0][0][j][2], full[0][0][j][3], sum(d) / len(d) / 1e3, max(d) / 1e3,
                           sum(w) / len(w) / 1e3, "the step before ends" if j else "the main launch starts"))
        if "--dump" in sys.argv:
            for s, e, name, gx, gy in rows[:60]:
                print("    %9.1f %9.1f  %-24s %d" % ((s - t0) / 1e3, (e - t0) / 1e3, family(name), gx * gy))


if __name__ == "__main__":
    try:
        main()
    except BrokenPipeError:          # piped into `head`
        pass
