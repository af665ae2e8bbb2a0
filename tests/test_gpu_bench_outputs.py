"""A plain `bench.py` run on the GPU: the line carries the headline keys and none of what `--full` adds, `--steps`
is the number of timed steps, and `--dump-outputs` writes what the timed path computed -- the oracle's solve of
the benchmark's own seeded input, bit for bit, on the per-k and the fused engine."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import assert_bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _bench(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("engine,dtype,with_next", [("perk", "f32", False), ("perk", "f32", True),
                                                    ("perk", "f64", False), ("fused", "f32", True)])
def test_plain_line_and_dumped_outputs(engine, dtype, with_next, tmp_path):
    import bench
    import oracle
    n = 320
    d = _bench(["--size", str(n), "--steps", "3", "--warmup", "1", "--engine", engine, "--dtype", dtype,
                "--dump-outputs", str(tmp_path)] + (["--with-next"] if with_next else []))
    assert d["steps"] == 3 and d["n_gpus"] == 1 and d["dtype"] == dtype
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
    assert d["unit"] == "edge-relaxations/s" and d["metric"].startswith("edge-relaxations/sec")
    for key in ("cpu_baseline", "check", "fused_engine", "fused_engine_next", "per_k_with_next", "f64",
                "reference_regime"):
        assert key not in d, key

    rate64, nxt = bench.make_input(argparse.Namespace(config=0, dist="d1"), n)
    rate = rate64 if dtype == "f64" else rate64.astype(np.float32)
    oracle.relax(rate, nxt)
    got = np.load(os.path.join(tmp_path, "rate.npy"))
    assert_bits_equal(got, rate, "dumped rates")
    if with_next:
        got_next = np.load(os.path.join(tmp_path, "next.npy"))
        assert got_next.dtype == np.float32
        assert_bits_equal(got_next, nxt.astype(np.float32), "dumped next-hops")
    else:
        assert not os.path.exists(os.path.join(tmp_path, "next.npy"))
