"""Child process of tests/test_gpu_threads.py (no test functions here): concurrent C-ABI calls against the oracle.

    python tests/threads_worker.py SCENARIO [--gate N]

One scenario per process, so the process-wide pools behind the library's threading promise (include/fwx.h "Threading /
streams") start cold and the counts of the test hook fwx_test_pools are exact.  The worker imports numpy, the oracle
and floydwarshall_amd only -- never torch.  Every expected result is computed with the C oracle (lists: the rope oracle,
oracle/list_ropes.py) BEFORE any thread starts; the threads are released together by one threading.Barrier (ctypes.CDLL
drops the GIL for the length of a call) and compare what they get bit for bit: rates, next, hops and U.  Exceptions and
mismatches are collected per thread.  Threads are joined with a timeout: one that does not come back is reported and
the process ends with os._exit, nothing more is started.  The last line printed is

    THREADS_RESULT {"scenario", "threads", "gate_n", "errors": [...], "hung": [...], "pools": {...}, ...}

pools: per pool (ctx, perk, multi) capacity, created, destroyed, peak -- the parent asserts from them that the case the
scenario is about occurred.  Thread counts come from the reported capacities (capacity + 4), never from a literal.

The gate.  The first call of every thread after the barrier is one long call, so that all threads are inside the
library together: a one-shot per-k solve with next and hops (one launch per pivot) where the pool under test is the
contexts' or the handles', a counted whole-matrix fwx_dev_relax (one launch per 8 pivots, no look-ahead) where it is the
per-stream panels, whose lease lasts only while the host queues launches.  GATE_N holds the order per scenario: the
smaller of the two orders tried on an MI355X (one run each; both reached the peak the scenario needs -- the figures
are in the scenarios' docstrings; no smaller order was tried, so nothing is claimed about a margin); --gate overrides
it for such a measurement.  The peak is the condition, not the results of the code under test."""
import ctypes
import json
import os
import sys
import threading
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import oracle  # noqa: E402
from oracle import list_ropes  # noqa: E402
from floydwarshall_amd import _lib, engine, hip, synth  # noqa: E402
from floydwarshall_amd._lib import FWX_ERR_OOM, FWX_XCHG_PEER  # noqa: E402

from helpers import assert_bits_equal  # noqa: E402
from hostile_inputs import hostile_matrix  # noqa: E402

THREADS = min(16, len(os.sched_getaffinity(0)))
F32, F64 = np.float32, np.float64
PERK, FUSED, AUTO = engine.FWX_ENGINE_PERK, engine.FWX_ENGINE_FUSED, engine.FWX_ENGINE_AUTO
JOIN_TIMEOUT = 30.0            # seconds for all threads of a scenario together (they need one or two); the parent's
                               # limit per child adds the oracle's share in front of it
LIST_MAX = 4096                # lists longer than this (hostile inputs grow them without bound) are not asked for

# order of the gate call per scenario (see the module docstring and each scenario's docstring)
GATE_N = {"oneshot": 512, "inject": 512, "handles": 512, "batches": 256, "streams": 1024, "streams_overflow": 2048}


# ---- the hook --------------------------------------------------------------------------------------------------------
def pools(reset=False):
    out = (ctypes.c_uint64 * 12)()
    assert _lib.lib().fwx_test_pools(out, 1 if reset else 0) == 3
    names = ("capacity", "created", "destroyed", "peak")
    return {pool: dict(zip(names, (int(v) for v in out[4 * i:4 * i + 4])))
            for i, pool in enumerate(("ctx", "perk", "multi"))}


# ---- inputs and expected results -----------------------------------------------------------------------------------
def make_input(kind, n, dtype, seed):
    if kind == "hostile":
        return hostile_matrix(np.random.default_rng(seed), n, dtype)
    if kind == "neg":                  # D1 with ONE negative rate: outside the domain, so AUTO leaves the fused engine
        rate, nxt, hops = synth.make("d1", n, dtype, seed=seed)
        rate[n // 3, n // 2] = -0.5
        return rate, nxt, hops
    return synth.make(kind, n, dtype, seed=seed)


def cp(a):
    return None if a is None else a.copy()


def solved(rate, nxt=None, hops=None, kb=0, ke=None, fast=False):
    """(rate, next, hops, U) of the oracle over pivots [kb, ke); the inputs are left alone."""
    er, en, eh = rate.copy(), cp(nxt), cp(hops)
    if rate.shape[0] == 0:
        return er, en, eh, 0
    u = oracle.relax_mt(er, en, kb, ke, threads=THREADS, hops=eh, fast=fast)
    return er, en, eh, u


def check(got, want, what):
    """got / want: (rate, next, hops[, U]); fields the caller did not ask for are None on both sides."""
    for g, w, field in zip(got[:3], want[:3], ("rate", "next", "hops")):
        assert (g is None) == (w is None), "%s: %s" % (what, field)
        if g is not None:
            assert_bits_equal(g, w, "%s: %s" % (what, field))
    if len(got) > 3 and got[3] is not None:
        assert int(got[3]) == int(want[3]), "%s: U %d vs oracle %d" % (what, int(got[3]), int(want[3]))


def solve_on_stream(rate, nxt, hops, stream, eng=AUTO):
    """fwx_solve_* with fwx_opts.stream: the (still blocking) call runs on the caller's stream."""
    o, _ = engine._opts(-1, eng, stream=stream)
    fn = _lib.lib().fwx_solve_f64 if rate.dtype == F64 else _lib.lib().fwx_solve_f32
    _lib.check(fn(rate.shape[0], engine._np_ptr(rate), engine._np_ptr(nxt), engine._np_ptr(hops), ctypes.byref(o)),
               "fwx_solve (caller's stream)")


def upload(d, a):
    d.copy_from_host(a)                # hipMemcpy: returns when the copy is done


def download(d, stream):
    return d.numpy(stream=stream)      # waits for `stream`, then hipMemcpy


def sampled_lists(ropes, n, seed, count):
    """(src, dst, [lists], cap): `count` seeded pairs of the matrix whose oracle list has at most LIST_MAX entries."""
    rnd = np.random.default_rng(seed)
    src, dst = rnd.integers(0, n, 4 * count), rnd.integers(0, n, 4 * count)
    keep = np.flatnonzero(ropes.lengths[src, dst] <= LIST_MAX)[:count]
    assert len(keep) >= count // 2, "only %d of the sampled lists have at most %d entries" % (len(keep), LIST_MAX)
    src, dst = src[keep].astype(np.int32), dst[keep].astype(np.int32)
    want = ropes.paths(src, dst)
    return src, dst, want, max([len(w) for w in want] + [1]) + 2


# ---- threads -----------------------------------------------------------------------------------------------------------
class Run:
    """Thread bodies released together.  A body is fn(t, note): it raises on the first thing that is wrong, or calls
    note(text) and goes on."""

    def __init__(self, scenario, gate_n):
        self.out = {"scenario": scenario, "gate_n": gate_n, "errors": [], "hung": []}
        self.lock = threading.Lock()

    def note(self, text):
        with self.lock:
            self.out["errors"].append(text)

    def go(self, bodies):
        self.out["threads"] = len(bodies)
        barrier = threading.Barrier(len(bodies))

        def body(t, fn):
            try:
                barrier.wait(timeout=JOIN_TIMEOUT)
                fn(t, self.note)
            except AssertionError as e:
                self.note("thread %d: mismatch: %s" % (t, e))
            except BaseException:
                self.note("thread %d: %s" % (t, traceback.format_exc(limit=4)))

        ths = [threading.Thread(target=body, args=(t, fn), daemon=True) for t, fn in enumerate(bodies)]
        for th in ths:
            th.start()
        import time
        end = time.monotonic() + JOIN_TIMEOUT
        for th in ths:
            th.join(max(0.0, end - time.monotonic()))
        self.out["hung"] = [t for t, th in enumerate(ths) if th.is_alive()]
        if self.out["hung"]:
            self.finish(code=4)        # a thread is still inside the library: nothing more is started

    def finish(self, code=None):
        self.out["pools"] = pools()
        print("THREADS_RESULT " + json.dumps(self.out), flush=True)
        if code is None:
            code = 1 if self.out["errors"] else 0
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(code)


GATE_KINDS = ("d2", "d1", "t1", "t2")


class SolveGate:
    """The gate of the scenarios on contexts and handles: fwx_solve_f32, per-k engine, next and hops, order n -- one
    launch per pivot.  Four inputs in turn; the oracle solves each once."""

    def __init__(self, n):
        self.n = n
        self.inputs = [make_input(k, n, F32, 9000 + i) for i, k in enumerate(GATE_KINDS)]
        self.want = [solved(*inp) for inp in self.inputs]

    def __call__(self, t):
        i = t % len(self.inputs)
        r, nx, h = (a.copy() for a in self.inputs[i])
        u = engine.solve(r, nx, h, engine=PERK, count_updates=True)
        check((r, nx, h, u), self.want[i], "gate (thread %d, n = %d)" % (t, self.n))


# ---- oneshot ------------------------------------------------------------------------------------------------------
def oneshot(gate_n):
    """kMaxFree + 4 threads, six rounds each through fwx_solve_f32 / _f64 and fwx_dev_solve; in round r thread t takes
    row (t + r) % len of ROWS, so a context comes back to a caller with another order, dtype and field set, and the
    contexts of the callers beyond the pool's capacity are destroyed beside running solves.
    Gate: n = 512; peak of leased contexts observed on an MI355X: 12 of 12 threads, 5 contexts destroyed (n = 1024:
    12 of 12, 4 destroyed)."""
    rows = [  # what, kind, n, dtype, fields, engine
        ("n=4 single launch", "d2", 4, F64, "nh", AUTO),
        ("n=64 single launch", "t1", 64, F32, "n", AUTO),
        ("n=128 outside the domain: the 128-wide launch", "neg", 128, F32, "n", AUTO),
        ("n=130 padded pitch, fused", "d2", 130, F32, "n", FUSED),
        ("n=257 f64 + next + hops", "t1", 257, F64, "nh", AUTO),
        ("n=300 rates only, per-k: the multi-pivot schedule on the context's workspace", "d1", 300, F32, "r", PERK),
        ("n=512 f32 + next + hops, counted", "d2", 512, F32, "nhu", AUTO),
        ("n=512 f64 + next: no pinned staging", "d1", 512, F64, "n", AUTO),
        ("n=130 on the caller's stream", "t2", 130, F32, "n", "stream"),
        ("n=300 fwx_dev_solve", "d2", 300, F32, "nh", "dev"),
    ]
    cases = []
    for i, (what, kind, n, dtype, fields, eng) in enumerate(rows):
        rate, nxt, hops = make_input(kind, n, dtype, 100 + i)
        nxt = nxt if "n" in fields else None
        hops = hops if "h" in fields else None
        cases.append((what, (rate, nxt, hops), solved(rate, nxt, hops), "u" in fields, eng))
    gate = SolveGate(gate_n)
    cap = pools()["ctx"]["capacity"]
    nthreads = cap + 4
    hip.default_stream()
    streams = [hip.Stream() for _ in range(nthreads)]
    n_dev = rows[9][2]
    dev = [[hip.DeviceArray((n_dev, n_dev), d) for d in (F32, np.int32, np.int32)] for _ in range(nthreads)]

    def one(t, i, tag):
        what, inp, want, count, eng = cases[i]
        r, nx, h = (cp(a) for a in inp)
        u = None
        if eng == "stream":
            solve_on_stream(r, nx, h, streams[t])
        elif eng == "dev":
            for d, a in zip(dev[t], (r, nx, h)):
                upload(d, a)
            engine.dev_solve(dev[t][0], next_t=dev[t][1], hops_t=dev[t][2], stream=streams[t])
            r, nx, h = (download(d, streams[t]) for d in dev[t])
        else:
            u = engine.solve(r, nx, h, engine=eng, count_updates=count)
        check((r, nx, h, u), want, "%s: %s" % (tag, what))

    def body(t, note):
        gate(t)
        for r in range(6):
            one(t, (t + r) % len(cases), "thread %d round %d" % (t, r))

    run = Run("oneshot", gate_n)
    run.go([body] * nthreads)
    for i in range(len(cases)):                    # afterwards, one caller at a time: every row is still exact
        try:
            one(0, i, "serial, after the threads")
        except AssertionError as e:
            run.note("mismatch: %s" % e)
    run.finish()


# ---- inject ---------------------------------------------------------------------------------------------------------
def inject(gate_n):
    """Four threads, eight rounds, f32 + next at n = 130 and 512.  Thread 0 arms fwx_test_fail_after(1) before each call
    and must get FWX_ERR_OOM every time, its arrays untouched; the hook is per thread, so the others never get it, their
    results are exact and fwx_last_hip_error() reads 0 on their threads.  Then thread 0 disarms and its next calls are
    exact.  The hook throws on the host: no GPU fault is involved.  fwx_solve_f32 itself has no allocation point of the
    hook, so thread 0 calls the batched one-shot forms with one matrix (fwx_solve_batch_mid_f32 at 130,
    fwx_solve_batch_large_f32 at 512: a pooled context like fwx_solve_f32, the first allocation point in front of any
    device work, the context back in the pool on the error return); the other threads call fwx_solve_f32.
    Gate: n = 512 (no peak is asserted here)."""
    L = _lib.lib()
    cases = []
    for i, n in enumerate((130, 512)):
        rate, nxt, _ = make_input("d2", n, F32, 300 + i)
        cases.append((n, (rate, nxt), solved(rate, nxt)))
    gate = SolveGate(gate_n)

    def exact(t, r, tag):
        n, inp, want = cases[(t + r) % 2]
        rate, nxt = inp[0].copy(), inp[1].copy()
        engine.solve(rate, nxt)
        check((rate, nxt, None), want, "%s n = %d" % (tag, n))

    def batched(i, rate, nxt):
        fn = engine.solve_batch_mid if cases[i][0] <= 256 else engine.solve_batch_large
        return fn(rate, nxt, count_updates=True)

    def victim(t, note):
        gate(t)
        for r in range(8):
            n, inp, _ = cases[r % 2]
            rate, nxt = inp[0].copy()[None], inp[1].copy()[None]
            assert L.fwx_test_fail_after(1) == 0
            try:
                batched(r % 2, rate, nxt)
                note("thread 0 round %d: the armed call returned FWX_OK" % r)
            except engine.FwxError as e:
                if e.status != FWX_ERR_OOM:
                    note("thread 0 round %d: status %d, not FWX_ERR_OOM" % (r, e.status))
                check((rate[0], nxt[0], None), (inp[0], inp[1], None), "thread 0 round %d: arrays after the failure" % r)
        assert L.fwx_test_fail_after(0) == 0
        for i in range(2):
            n, inp, want = cases[i]
            rate, nxt = inp[0].copy()[None], inp[1].copy()[None]
            us = batched(i, rate, nxt)
            check((rate[0], nxt[0], None, us[0]), want, "thread 0, disarmed, n = %d" % n)

    def other(t, note):
        gate(t)
        for r in range(8):
            exact(t, r, "thread %d round %d" % (t, r))
            err = L.fwx_last_hip_error()
            assert err == 0, "thread %d round %d: fwx_last_hip_error() = %d" % (t, r, err)

    run = Run("inject", gate_n)
    run.go([victim, other, other, other])
    run.finish()


# ---- handles ----------------------------------------------------------------------------------------------------------
def handles(gate_n):
    """Six threads at once, one handle (or one-shot partitioned solve) each, exchange FWX_XCHG_PEER throughout:
    0  single-device traced handle, n = 258 on t1 ties: query_exact_batch borrows a context's scratch; rope oracle
    1  single-device handle with keep_input, enable_resume(3) and four resolve calls, two of them just before and just
       after the checkpoint at pivot 256
    2  a [0, 0] handle, f64 + next + hops
    3  a [0, 0, 0] handle on the per-k engine with hops
    4, 5  fwx_solve_multi_f32 with the SAME key at once (the gate of these two: order gate_n, per-k, next and hops): the
       pool is empty, so each creates a handle and none is shared; then 4 calls again with that key (takes a parked
       handle) while 5 calls with another key (creates a third): the parks go past kMaxIdle and evict beside running
       solves.
    Gate: n = 512; MultiPool observed on an MI355X: peak 2 of the 2 same-key callers, created 3, evicted 1 (the same
    at n = 1024)."""
    gate = SolveGate(gate_n)
    # 0: traced
    n0 = 258
    r0, nx0, _ = make_input("t1", n0, F32, 400)
    ropes0 = list_ropes.solve(r0, nx0)
    want0 = solved(r0, nx0)
    assert_bits_equal(ropes0.rate, want0[0], "rope oracle vs dense oracle")
    src0, dst0, lists0, cap0 = sampled_lists(ropes0, n0, 401, 800)
    # 1: resumed
    n1 = 512
    r1, nx1, _ = make_input("d2", n1, F32, 402)
    want1 = [solved(r1, nx1)]
    plan1, cur_r, cur_n = [], r1.copy(), nx1.copy()
    for step, (u, v) in enumerate([(400, 500), (254, 255), (256, 257), (40, 90)]):
        idx = np.array([u * n1 + v, v * n1 + u], dtype=np.int64)
        vals = (cur_r.reshape(-1)[idx] * F32(0.93 + 0.01 * step)).astype(F32)
        nv = np.array([v, u], dtype=np.int32)
        cur_r.reshape(-1)[idx] = vals
        cur_n.reshape(-1)[idx] = nv
        start = max(p for p in (0, 128, 256, 384) if p <= min(u, v))
        plan1.append((idx, vals, nv, start, solved(cur_r, cur_n)))
    assert [p[3] for p in plan1] == [384, 128, 256, 0]
    # 2, 3: partitioned handles
    n2 = 320
    in2 = make_input("t1", n2, F64, 403)
    want2 = solved(*in2)
    n3 = 300
    in3 = make_input("d2", n3, F32, 404)
    want3 = solved(*in3)
    # 4, 5: one-shot partitioned solves
    in4 = [make_input(k, gate_n, F32, 405 + i) for i, k in enumerate(("d2", "t1"))]
    want4 = [solved(*inp) for inp in in4]
    n5 = 200
    in5 = make_input("t2", n5, F32, 407)[:2]
    want5 = solved(*in5)

    def traced(t, note):
        gate(t)
        with engine.DeviceMatrix(n0, F32, with_next=True) as dm:
            dm.enable_path_log()
            dm.upload(r0, nx0)
            dm.solve()
            gr, gn, _ = dm.download()
            got = dm.query_exact_batch(src0, dst0, cap=cap0)
        check((gr, gn, None), want0, "traced handle")
        bad = [q for q in range(len(src0)) if tuple(got[q]) != lists0[q]]
        assert not bad, "traced handle: %d lists differ, first (%d, %d)" % (len(bad), src0[bad[0]], dst0[bad[0]])

    def resumed(t, note):
        gate(t)
        with engine.DeviceMatrix(n1, F32, with_next=True) as dm:
            dm.keep_input()
            assert dm.enable_resume(3) == 3
            dm.upload(r1, nx1)
            dm.solve()
            gr, gn, _ = dm.download()
            check((gr, gn, None), want1[0], "resumable handle, first solve")
            for step, (idx, vals, nv, start, want) in enumerate(plan1):
                started = dm.resolve(idx, vals, nv)
                assert started == start, "resolve %d started at %d, not %d" % (step, started, start)
                gr, gn, _ = dm.download()
                check((gr, gn, None), want, "resolve %d (from pivot %d)" % (step, start))

    def part(n, dtype, inp, want, devices, eng, what):
        def body(t, note):
            gate(t)
            with engine.DeviceMatrix(n, dtype, with_next=True, with_hops=True, devices=devices,
                                     exchange=FWX_XCHG_PEER) as dm:
                dm.upload(*inp)
                u = dm.solve(engine=eng, count_updates=True)
                check(dm.download() + (u,), want, what)
        return body

    def multi(rate_next_hops, want, what):
        r, nx, h = (cp(a) for a in rate_next_hops)
        u = engine.solve_multi(r, nx, h, devices=[0, 0], exchange=FWX_XCHG_PEER,
                               engine=PERK if h is not None else AUTO, count_updates=True)
        check((r, nx, h, u), want, what)

    def same_key(t, note):
        multi(in4[t - 4], want4[t - 4], "same-key one-shot (thread %d)" % t)
        if t == 4:
            multi(in4[1], want4[1], "same key again (thread 4)")
        else:
            multi(in5 + (None,), want5, "another key (thread 5)")

    run = Run("handles", gate_n)
    run.go([traced, resumed, part(n2, F64, in2, want2, [0, 0], AUTO, "[0, 0] handle"),
            part(n3, F32, in3, want3, [0, 0, 0], PERK, "[0, 0, 0] per-k handle"), same_key, same_key])
    run.finish()


# ---- batches ----------------------------------------------------------------------------------------------------------
def batches(gate_n):
    """Six threads, each on another family of the batched solves, two rounds, next + hops and U per matrix against the
    oracle; the `_lists` forms on hostile inputs against the rope oracle.  No pool overflows here: six callers fit the
    contexts' pool; the peak asserted is that all six held a context at once.
    Gate: n = 256; peak observed on an MI355X: 6 of 6 (the same at n = 512)."""
    gate = SolveGate(gate_n)

    def uniform(fn, kinds, n, count, seed):
        mats = [make_input(kinds[b % len(kinds)], n, F64 if seed % 2 else F32, seed + b) for b in range(count)]
        inp = tuple(np.stack([m[f] for m in mats]) for f in range(3))
        want = [solved(*m) for m in mats]

        def call(tag):
            r, nx, h = (a.copy() for a in inp)
            us = fn(r, nx, h, count_updates=True)
            for b in range(count):
                check((r[b], nx[b], h[b], us[b]), want[b], "%s n = %d matrix %d" % (tag, n, b))
        return call

    def ragged(fn, orders, seed):
        kinds = ("d2", "t1", "hostile", "t2", "d1")
        mats = [make_input(kinds[b % 5], n, F32, seed + b) if n else
                (np.zeros((0, 0), F32), np.zeros((0, 0), np.int32), np.zeros((0, 0), np.int32))
                for b, n in enumerate(orders)]
        want = [solved(*m) for m in mats]

        def call(tag):
            rs, ns, hs = ([m[f].copy() for m in mats] for f in range(3))
            us = fn(rs, ns, hs, count_updates=True)
            for b, n in enumerate(orders):
                if n:
                    check((rs[b], ns[b], hs[b], us[b]), want[b], "%s matrix %d (n = %d)" % (tag, b, n))
        return call

    def lists(fn, orders, seed, is_ragged):
        mats = [make_input("hostile", n, F64 if is_ragged else F32, seed + b) for b, n in enumerate(orders)]
        want = [solved(*m) for m in mats]
        items, want_lists = [[], [], []], []
        for b, (m, n) in enumerate(zip(mats, orders)):
            ropes = list_ropes.solve(m[0], m[1])
            assert_bits_equal(ropes.rate, want[b][0], "rope oracle vs dense oracle, matrix %d" % b)
            src, dst, ws, _ = sampled_lists(ropes, n, seed + 50 + b, 200)
            items[0] += [b] * len(src)
            items[1] += list(src)
            items[2] += list(dst)
            want_lists += ws
        cap = max([len(w) for w in want_lists] + [1]) + 2

        def call(tag):
            if is_ragged:
                rs, ns, hs = ([m[f].copy() for m in mats] for f in range(3))
            else:
                rs, ns, hs = (np.stack([m[f] for m in mats]) for f in range(3))
            got, us = fn(rs, ns, hs, items=tuple(items), cap=cap, count_updates=True)
            for b in range(len(orders)):
                check((rs[b], ns[b], hs[b], us[b]), want[b], "%s matrix %d" % (tag, b))
            bad = [q for q in range(len(got)) if tuple(got[q]) != want_lists[q]]
            assert not bad, "%s: %d lists differ, first item %d" % (tag, len(bad), bad[0])
        return call

    work = [
        [uniform(engine.solve_batch, ("d2", "t1", "hostile"), 8, 64, 500),
         uniform(engine.solve_batch, ("t1", "hostile", "d1"), 100, 8, 601)],
        [uniform(engine.solve_batch_mid, ("d2", "hostile", "t1"), 130, 8, 700)],
        [uniform(engine.solve_batch_large, ("t1", "d2", "hostile"), 260, 3, 801)],
        [ragged(engine.solve_ragged_large, [0, 1, 5, 17, 64, 129, 257, 300], 900)],
        [lists(engine.solve_batch_lists, [64] * 4, 1000, False)],
        [lists(engine.solve_ragged_mid_lists, [3, 16, 17, 129, 200], 1100, True)],
    ]

    def body(t, note):
        gate(t)
        for r in range(2):
            for call in work[t]:
                call("thread %d round %d" % (t, r))

    run = Run("batches", gate_n)
    run.go([body] * len(work))
    run.finish()


# ---- streams, streams_overflow -------------------------------------------------------------------------------------
def relax_gate_inputs(n):
    inputs = [make_input(k, n, F32, 9100 + i)[0] for i, k in enumerate(("d1", "d2"))]
    return inputs, [solved(r, fast=True) for r in inputs]


def streams_body(n, nthreads, gate_n):
    """Thread bodies for the two scenarios on the per-stream panels: per thread a stream, a gate matrix and a matrix of
    order n from its own seed (cross-talk between two streams' panels changes bits).  The gate: counted whole-matrix
    fwx_dev_relax at order gate_n; then fwx_dev_relax, rates-only f32, over [0, n / 2) and [n / 2, n)."""
    kinds = ("d1", "t1", "t2", "hostile", "d2")
    g_in, g_want = relax_gate_inputs(gate_n)
    rates = [make_input(kinds[t % 5], n, F32, 1200 + t)[0] for t in range(nthreads)]
    want = [solved(r) for r in rates]
    hip.default_stream()
    st = [hip.Stream() for _ in range(nthreads)]
    g_dev = [hip.DeviceArray.from_numpy(g_in[t % 2]) for t in range(nthreads)]
    g_upd = [hip.DeviceArray((engine.FWX_UPDATE_SHARDS,), np.int64).zero_(hip.default_stream()) for _ in range(nthreads)]
    m_dev = [hip.DeviceArray.from_numpy(r) for r in rates]
    hip.synchronize()

    def body(t, note):
        engine.dev_relax(g_dev[t], gate_n, 0, 0, gate_n, updates_t=g_upd[t], stream=st[t])
        engine.dev_relax(m_dev[t], n, 0, 0, n // 2, stream=st[t])
        engine.dev_relax(m_dev[t], n, 0, n // 2, n, stream=st[t])
        got_g, got_u = download(g_dev[t], st[t]), download(g_upd[t], st[t])
        check((got_g, None, None, int(got_u.sum())), g_want[t % 2], "gate (thread %d, n = %d)" % (t, gate_n))
        check((download(m_dev[t], st[t]), None, None), want[t], "thread %d (%s, n = %d)" % (t, kinds[t % 5], n))

    # the streams stay alive to the end of the process: a destroyed stream's handle comes back with the next
    # hipStreamCreate, and a "new" stream would then find the entry of an old one
    return [body] * nthreads, (st, g_dev, g_upd, m_dev)


def streams(gate_n):
    """Eight threads -- they fit the pool of 16 -- each on its own stream with its own matrix, n = 640 under
    FWX_PERK_TILE_MIN_N=1, FWX_PERK_PAIR_MIN_N=1 and FWX_PERK_GROUP_MAX=4 (set by the parent in this process's
    environment): ten full blocks, the group schedule, every entry with a look-ahead stream of its own; two calls of
    half the range each.  The buffer each stream's gate call made is regrown for the group schedule's panel sets.
    Gate: n = 1024; PerkScratch observed on an MI355X: peak 8 of 8, evicted 0, 32 main launches of the group schedule
    (the same at n = 2048)."""
    for name in ("FWX_PERK_TILE_MIN_N", "FWX_PERK_PAIR_MIN_N"):
        assert os.environ.get(name) == "1", name
    assert os.environ.get("FWX_PERK_GROUP_MAX") == "4"
    run = Run("streams", gate_n)
    bodies, keep = streams_body(640, 8, gate_n)
    run.go(bodies)
    pair = (ctypes.c_uint64 * 1)()
    _lib.lib().fwx_test_perk_pair(pair, 0)
    run.out["pair_launches"] = int(pair[0])
    run.finish()


def streams_overflow(gate_n):
    """The same with kMax + 4 streams: more callers inside fwx_dev_relax at once than the pool keeps.  No entry that a
    call still holds is evicted: the pool grows past kMax for the moment, and after all threads have returned one
    further call on a new stream trims it back to kMax.  n and the environment come from the parent: n = 256 with
    the environment unset (the ladder: entries without a look-ahead stream) or n = 640 as in `streams` (entries that
    own a look-ahead stream and events).
    Gate: n = 2048, the only order tried; PerkScratch peak observed on an MI355X: 20 of 20 streams at n = 256 and at
    n = 640, nothing evicted while the threads ran."""
    n = int(os.environ["FWX_THREADS_OVERFLOW_N"])
    cap = pools()["perk"]["capacity"]
    run = Run("streams_overflow", gate_n)
    run.out["n"] = n
    bodies, keep = streams_body(n, cap + 4, gate_n)
    run.go(bodies)
    before = pools()["perk"]
    run.out["kept_before"] = before["created"] - before["destroyed"]
    rate = make_input("d1", 256, F32, 1300)[0]
    want = solved(rate)
    s = hip.Stream()
    d = hip.DeviceArray.from_numpy(rate)
    try:
        engine.dev_relax(d, 256, 0, 0, 256, stream=s)
        check((download(d, s), None, None), want, "the call on a new stream, after the threads")
    except AssertionError as e:
        run.note("mismatch: %s" % e)
    after = pools()["perk"]
    run.out["kept_after"] = after["created"] - after["destroyed"]
    run.out["streams_alive"] = len(keep[0])
    run.finish()


# ---- cold ---------------------------------------------------------------------------------------------------------------
def cold(gate_n):
    """The library is mapped, but no solve, stream or allocation has been made: eight threads make the process's first
    calls together, each through another door -- the HIP module load, the leaked pool singletons, the retire barrier's
    pad and the once-per-process switches of the fused engine (the parent sets FWX_PANELS_TIGHT=0, so a function-local
    static is first evaluated by racing threads).  No gate: the first calls ARE the case."""
    assert os.environ.get("FWX_PANELS_TIGHT") == "0"
    a = make_input("d2", 4, F32, 1400)
    b = make_input("t1", 300, F64, 1401)[:2]
    c = [make_input(("d2", "hostile")[i % 2], 8, F64, 1402 + i) for i in range(16)]
    d = make_input("t1", 200, F64, 1420)[:2]
    e = make_input("d1", 256, F32, 1421)[0]
    f = make_input("d2", 132, F32, 1422)[:2]
    g = make_input("d2", 300, F64, 1423)[:2]
    h = make_input("t1", 100, F32, 1424)[:2]
    wa, wb, wd, we, wf, wh = solved(*a), solved(*b), solved(*d), solved(e), solved(*f), solved(*h)
    wc = [solved(*m) for m in c]
    g_next = solved(*g)[1]
    pairs = [(0, 299), (17, 3), (150, 151), (299, 0), (5, 5)]
    walks = [oracle.follow_path(g_next, s, t) for s, t in pairs]
    assert all(w is not None for w in walks)
    ropes = list_ropes.solve(*h)
    assert_bits_equal(ropes.rate, wh[0], "rope oracle vs dense oracle")
    assert pools()["ctx"]["created"] == 0 and pools()["perk"]["created"] == 0

    def door_solve_f32(t, note):
        r, nx, hp = (x.copy() for x in a)
        u = engine.solve(r, nx, hp, count_updates=True)
        check((r, nx, hp, u), wa, "fwx_solve_f32 n = 4")

    def door_solve_f64(t, note):
        r, nx = b[0].copy(), b[1].copy()
        engine.solve(r, nx, engine=FUSED)
        check((r, nx, None), wb, "fwx_solve_f64 fused n = 300")

    def door_batch(t, note):
        r, nx, hp = (np.stack([m[i] for m in c]) for i in range(3))
        us = engine.solve_batch(r, nx, hp, count_updates=True)
        for i in range(len(c)):
            check((r[i], nx[i], hp[i], us[i]), wc[i], "fwx_solve_batch_f64 matrix %d" % i)

    def door_handle(t, note):
        with engine.DeviceMatrix(200, F64, with_next=True, devices=[0, 0], exchange=FWX_XCHG_PEER) as dm:
            dm.upload(*d)
            dm.solve()
            check(dm.download(), wd, "[0, 0] handle")

    def door_relax(t, note):
        s = hip.Stream()
        m = hip.DeviceArray.from_numpy(e)
        engine.dev_relax(m, 256, 0, 0, 256, stream=s)
        check((download(m, s), None, None), we, "fwx_dev_relax on a stream")

    def door_dev_solve(t, note):
        s = hip.Stream()
        r, nx = hip.DeviceArray.from_numpy(f[0]), hip.DeviceArray.from_numpy(f[1])
        engine.dev_solve(r, next_t=nx, stream=s)
        check((download(r, s), download(nx, s), None), wf, "fwx_dev_solve")

    def door_follow(t, note):
        for (src, dst), w in zip(pairs, walks):
            assert engine.follow_path(g_next, src, dst) == w, "fwx_follow_path (%d, %d)" % (src, dst)

    def door_traced(t, note):
        with engine.DeviceMatrix(100, F32, with_next=True) as dm:
            dm.enable_path_log()
            dm.upload(*h)
            dm.solve()
            gr, gn, _ = dm.download()
            check((gr, gn, None), wh, "traced handle")
            for src, dst in ((0, 99), (42, 7), (99, 98)):
                _, got = dm.query_exact(src, dst, cap=LIST_MAX)
                assert tuple(got) == ropes.path(src, dst), "query_exact (%d, %d)" % (src, dst)

    run = Run("cold", 0)
    run.go([door_solve_f32, door_solve_f64, door_batch, door_handle, door_relax, door_dev_solve, door_follow,
            door_traced])
    run.finish()


SCENARIOS = {"oneshot": oneshot, "inject": inject, "handles": handles, "batches": batches, "streams": streams,
             "streams_overflow": streams_overflow, "cold": cold}


def main():
    name = sys.argv[1]
    gate_n = GATE_N.get(name, 0)
    if "--gate" in sys.argv:
        gate_n = int(sys.argv[sys.argv.index("--gate") + 1])
    try:
        SCENARIOS[name](gate_n)
    except BaseException:
        print("THREADS_RESULT " + json.dumps({"scenario": name, "gate_n": gate_n, "hung": [], "pools": pools(),
                                              "errors": ["setup: " + traceback.format_exc(limit=6)]}), flush=True)
        os._exit(2)


if __name__ == "__main__":
    main()
