"""The threading contract of the C ABI (include/fwx.h "Threading / streams"): calls "may come from any OS thread", the
only global mutable state is mutex-protected pools, and "solves on different host threads overlap on the device".
Every other GPU test makes one library call at a time; here several are inside the library together, every result is
compared with the oracle bit for bit (rates, next, hops, U; lists against the rope oracle), and the process-wide pools
are driven through the paths only concurrency reaches: more callers than a pool keeps, a context that returns to a
caller with another shape, an eviction beside running solves, the process's first calls arriving together.

Each scenario runs in a fresh child (tests/threads_worker.py SCENARIO), so its pools start cold and the counts of the
hook fwx_test_pools are exact; the scenarios themselves are described there.  Every test asserts FROM THE HOOK that
the case it is about occurred -- the peak number of entries leased at one time, the entries destroyed or evicted: a run
in which the calls happened not to overlap fails with "the case did not occur", it does not pass.  Thread counts come
from the capacities the hook reports (capacity + 4), so a later change of a constant cannot quietly turn an overflow
test into one that fits the pool.

A child that overruns its limit, ends on a signal or reports a thread that did not come back fails the test and ends
the session (pytest.exit): nothing else starts on the GPU after a hang or a crash.  There are no retries.
Environment variables are set in the child's environment only."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# what a scenario may set; everything else of the per-k and fused engines' switches is removed from the child's environment
KNOBS = ("FWX_PERK_PIVOTS", "FWX_PERK_WIDE", "FWX_PERK_DEEP", "FWX_PERK_WALK", "FWX_PERK_FOLD", "FWX_PERK_TILE_MIN_N",
         "FWX_PERK_PAIR_MIN_N", "FWX_PERK_GROUP_MAX", "FWX_PERK_TEMPORAL_MIB", "FWX_PANELS_TIGHT",
         "FWX_BATCH_WAVE_MAX_N", "FWX_BATCH_MID_MIN_N", "FWX_BATCH_LARGE_MIN_N", "FWX_BATCH_LISTS_CHUNK",
         "FWX_THREADS_OVERFLOW_N")
GROUPS = {"FWX_PERK_TILE_MIN_N": "1", "FWX_PERK_PAIR_MIN_N": "1", "FWX_PERK_GROUP_MAX": "4"}
# seconds per child: the threads' own limit in the worker (JOIN_TIMEOUT, 30 s; they need one or two) after the oracle's
# share in front of them (on 16 CPUs: cold and inject under 1 s, oneshot, handles and batches about 2 s, the streams
# scenarios about 3 s with the gate's order-2048 solves) and the interpreter's start, with as much again to spare
LIMIT = {"cold": 40, "inject": 40, "oneshot": 50, "handles": 50, "batches": 50, "streams": 50, "streams_overflow": 60}


def stop(why):
    """The test fails and the session ends: nothing else starts on the GPU after a hang or a crash."""
    pytest.exit("%s: stopping the GPU tests" % why, returncode=3)


def run(scenario, env_over=None):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(env_over or {})
    limit = LIMIT[scenario]
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "threads_worker.py"), scenario], env=env,
                           capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        stop("threads_worker %s overran %d s with %r" % (scenario, limit, env_over))
    if r.returncode < 0 or r.returncode in (134, 139):
        stop("threads_worker %s ended with status %d (%r)\n%s" % (scenario, r.returncode, env_over, r.stderr[-3000:]))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("THREADS_RESULT ")]
    assert line, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    res = json.loads(line[-1][len("THREADS_RESULT "):])
    if res["hung"]:
        stop("threads_worker %s: threads %r did not come back" % (scenario, res["hung"]))
    assert not res["errors"], "%s: %d errors, the first:\n%s" % (scenario, len(res["errors"]), res["errors"][0])
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return res


def occurred(cond, what, pools):
    assert cond, "the case did not occur: %s (pools: %r)" % (what, pools)


def test_oneshot_more_callers_than_contexts():
    res = run("oneshot")
    ctx = res["pools"]["ctx"]
    assert res["threads"] == ctx["capacity"] + 4
    occurred(ctx["peak"] >= ctx["capacity"] + 1, "more contexts leased at once than the pool keeps", res["pools"])
    occurred(ctx["destroyed"] >= 1, "a context destroyed on release", res["pools"])


def test_injected_failure_stays_on_its_thread():
    res = run("inject")
    assert res["threads"] == 4


def test_handles_one_per_thread_and_same_key_oneshots():
    res = run("handles")
    multi = res["pools"]["multi"]
    assert res["threads"] == 6 <= multi["capacity"] + 4
    occurred(multi["peak"] >= 2, "two same-key one-shot calls at once", res["pools"])
    occurred(multi["created"] >= 3, "same-key takes that share no handle, and a third key", res["pools"])
    occurred(multi["destroyed"] >= 1, "a park past the pool's capacity", res["pools"])


def test_batched_families_side_by_side():
    res = run("batches")
    assert res["threads"] == 6
    occurred(res["pools"]["ctx"]["peak"] >= 6, "six batched calls at once", res["pools"])


def test_streams_that_fit_the_pool():
    res = run("streams", GROUPS)
    perk = res["pools"]["perk"]
    assert res["threads"] == 8 <= perk["capacity"]
    occurred(perk["peak"] == 8, "eight streams' entries in use at once", res["pools"])
    assert perk["destroyed"] == 0 and perk["created"] == 8, res["pools"]
    occurred(res["pair_launches"] > 0, "the group schedule and its look-ahead streams", res["pools"])


@pytest.mark.parametrize("n,env", [(256, {}), (640, GROUPS)], ids=["ladder-n256", "groups-n640"])
def test_streams_overflow_the_pool(n, env):
    res = run("streams_overflow", dict(env, FWX_THREADS_OVERFLOW_N=str(n)))
    perk = res["pools"]["perk"]
    assert res["threads"] == perk["capacity"] + 4 and res["n"] == n
    occurred(perk["peak"] >= perk["capacity"] + 1, "more streams' entries in use at once than the pool keeps",
             res["pools"])
    # (a stream whose idle entry another stream's first call evicted makes a new one: created may exceed the streams)
    assert perk["created"] >= res["threads"] + 1 and res["streams_alive"] == res["threads"], res
    assert res["kept_after"] <= perk["capacity"], "a later call did not trim the pool: %r" % res
    assert perk["destroyed"] >= perk["created"] - perk["capacity"] >= 1, res["pools"]


def test_first_calls_of_the_process_arrive_together():
    res = run("cold", {"FWX_PANELS_TIGHT": "0"})
    assert res["threads"] == 8
