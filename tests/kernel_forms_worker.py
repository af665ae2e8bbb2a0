"""Child process of tests/test_gpu_kernel_forms.py (no test functions here).

The tile and schedule thresholds of the fused engine are read once per process, so every setting of
them needs a fresh interpreter: the parent starts this module with the knobs in its environment and a
JSON list of cases as argv[1], one child at a time.  Each case solves one input on the GPU and on the
oracle and compares every field bit for bit; it also records the launch forms it reached
(fwx_test_kernel_forms).  The child prints one JSON line: per case an error message or null and the
forms seen.  It imports numpy, the oracle and floydwarshall_amd only -- never torch.  A traced case (nt) of
order <= 452 also has the exact `_path` lists of 800 sampled pairs compared with the rope oracle
(oracle/list_ropes.py), hostile inputs included; "lists" keeps one case on the list-faithful restatement.

A case: {"kind": t1 | t2 | t3 | t4 | hostile, "n", "dtype": f32 | f64, "fields", "seed",
"engine": fused | perk | auto, "lists": bool}.  fields: r (rates), ru (rates, counting U),
n (+ next), nh (+ next + hops), nhu (+ next + hops, counting U), nt (+ next + path trace)."""
import json
import os
import sys
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import oracle  # noqa: E402
from floydwarshall_amd import engine, synth  # noqa: E402

from helpers import assert_bits_equal  # noqa: E402
from hostile_inputs import hostile_matrix  # noqa: E402

THREADS = min(16, len(os.sched_getaffinity(0)))
ROPES_MAX_N = 452             # traced cases up to this order also have 800 sampled lists read (oracle/list_ropes.py)
ENGINES = {"fused": engine.FWX_ENGINE_FUSED, "perk": engine.FWX_ENGINE_PERK, "auto": engine.FWX_ENGINE_AUTO}


def make_input(kind, n, dtype, seed):
    if kind == "hostile":
        return hostile_matrix(np.random.default_rng(seed), n, dtype)
    return synth.make(kind, n, dtype, seed=seed)


def run_case(c):
    dtype = np.float32 if c["dtype"] == "f32" else np.float64
    n, fields = c["n"], c["fields"]
    rate, nxt, hops = make_input(c["kind"], n, dtype, c["seed"])
    with_next = fields != "r" and fields != "ru"
    with_hops = fields in ("nh", "nhu")
    count = fields in ("ru", "nhu")
    nxt = nxt if with_next else None
    hops = hops if with_hops else None
    er = rate.copy()
    en = None if nxt is None else nxt.copy()
    eh = None if hops is None else hops.copy()
    eu = oracle.relax_mt(er, en, hops=eh, threads=THREADS)
    eng = ENGINES[c.get("engine", "fused")]
    if fields == "nt":
        with engine.DeviceMatrix(n, dtype, with_next=True) as dm:
            dm.enable_path_log()
            dm.upload(rate, nxt)
            dm.solve(engine=eng)
            gr, gn, _ = dm.download()
            lists = ropes = None
            if c.get("lists") or n <= ROPES_MAX_N:
                rnd = np.random.default_rng(c["seed"] + 1)
                src = rnd.integers(0, n, 800).astype(np.int32)
                dst = rnd.integers(0, n, 800).astype(np.int32)
                cap = None
                if not c.get("lists"):
                    # every other traced case: the sampled lists against the rope oracle, hostile inputs included
                    # (there a list can be far longer than the default cap of 4 n: cap comes from the oracle)
                    from oracle import list_ropes
                    ropes = list_ropes.solve(rate, nxt)
                    longest = int(ropes.lengths[src, dst].max())
                    assert longest <= 1 << 16, "sampled list of %d entries" % longest
                    cap = max(longest, 1) + 2
                lists = (src, dst, dm.query_exact_batch(src, dst, cap=cap))
        assert_bits_equal(gr, er, "rate")
        assert_bits_equal(gn, en, "next")
        if ropes is not None:
            assert_bits_equal(ropes.rate, er, "rope oracle vs dense oracle: rate")
            assert_bits_equal(ropes.next, en, "rope oracle vs dense oracle: next")
            assert ropes.updates == eu, "rope oracle U %d vs dense oracle %d" % (ropes.updates, eu)
            src, dst, got = lists
            want = ropes.paths(src, dst)
            assert sum(len(w) for w in want) > 0
            for q in range(len(src)):
                assert tuple(got[q]) == want[q], "exact list (%d, %d): %r vs %r" % (src[q], dst[q], got[q], want[q])
        elif lists is not None:
            from oracle import list_faithful as lf
            m = lf.run_algo(lf.from_dense([("X", "C%04d" % i) for i in range(n)], rate, nxt), dtype)
            paths = lf.path_indices(m)
            src, dst, got = lists
            for q in range(len(src)):
                want = paths[src[q]][dst[q]]
                assert tuple(got[q]) == want, "exact list (%d, %d): %r vs %r" % (src[q], dst[q], got[q], want)
        return
    gr = rate.copy()
    gn = None if nxt is None else nxt.copy()
    gh = None if hops is None else hops.copy()
    u = engine.solve(gr, gn, gh, device=0, engine=eng, count_updates=count)
    assert_bits_equal(gr, er, "rate")
    if gn is not None:
        assert_bits_equal(gn, en, "next")
    if gh is not None:
        assert_bits_equal(gh, eh, "hops")
    if count:
        assert u == eu, "U %d vs oracle %d" % (u, eu)


def main():
    cases = json.loads(sys.argv[1])
    out = []
    engine.kernel_forms_seen(reset=True)
    for c in cases:
        err = None
        try:
            run_case(c)
        except AssertionError as e:
            err = "mismatch: %s" % e
        except Exception:
            err = traceback.format_exc(limit=3)
        out.append({"case": c, "error": err, "forms": sorted(engine.kernel_forms_seen(reset=True))})
    print("KERNEL_FORMS_RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
