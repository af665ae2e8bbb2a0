"""Writes tests/golden/handle_kinds_lists_n258_f32.json: exact `_path` lists of the t1 input of order 258 in f32
(synth.make("t1", 258, np.float32, seed=358)), as the list-faithful restatement (oracle/list_faithful.py) builds
them.  The pure-Python triple loop takes over a minute at this order, which is why tests/test_gpu_handle_kinds.py
reads the lists from the fixture; tests/test_oracle_golden.py ties the fixture to the input and to the C oracle.

    python tests/golden/make_handle_kinds_lists.py

Kept: the longest list, the pairs the GPU test names (one per slab of two and of three partitions, the last real
row and column) and 40 seeded random pairs."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from floydwarshall_amd import synth  # noqa: E402
from oracle import list_faithful as lf  # noqa: E402

N, SEED = 258, 358


def main():
    rate, nxt, _ = synth.make("t1", N, np.float32, seed=SEED)
    vertices = [("X", "C%03d" % i) for i in range(N)]
    paths = lf.path_indices(lf.run_algo(lf.from_dense(vertices, rate, nxt), np.float32))
    longest = max(((s, d) for s in range(N) for d in range(N)), key=lambda sd: len(paths[sd[0]][sd[1]]))
    pairs = [longest, (0, N - 1), (N - 1, 0), (N // 2, N // 2 + 1), (N - 1, N - 2), (5, 200), (100, 3), (200, 90)]
    rnd = np.random.default_rng(SEED)
    pairs += [(int(s), int(d)) for s, d in zip(rnd.integers(0, N, 40), rnd.integers(0, N, 40))]
    out = {"kind": "t1", "n": N, "dtype": "float32", "seed": SEED, "longest": list(longest),
           "max_len": len(paths[longest[0]][longest[1]]),
           "lists": [{"src": s, "dst": d, "path": list(paths[s][d])} for s, d in dict.fromkeys(pairs)]}
    with open(os.path.join(ROOT, "tests", "golden", "handle_kinds_lists_n258_f32.json"), "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
