"""Shared helpers for the parity tests (the oracle is the checker, never the thing tested)."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


def golden_rates_dict(g):
    return {(tuple(r["src"]), tuple(r["dst"])): r["rate"] for r in g["rates"]}


def golden_dense(entries, dtype=np.float64):
    """[[ [rate,[path idx]] ]] -> rate, next (= head of path or -1), hops (= len path), paths."""
    n = len(entries)
    rate = np.zeros((n, n), dtype=dtype)
    nxt = np.full((n, n), -1, dtype=np.int32)
    hops = np.zeros((n, n), dtype=np.int32)
    paths = [[tuple(e[1]) for e in row] for row in entries]
    for i in range(n):
        for j in range(n):
            rate[i, j] = entries[i][j][0]
            p = entries[i][j][1]
            hops[i, j] = len(p)
            if p:
                nxt[i, j] = p[0]
    return rate, nxt, hops, paths


def bits_equal(a, b):
    """Bit-exact comparison that treats NaNs by payload, and -0.0 != +0.0."""
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "f":
        it = np.uint64 if a.dtype.itemsize == 8 else np.uint32
        return bool(np.array_equal(a.view(it), b.view(it)))
    return bool(np.array_equal(a, b))


def assert_bits_equal(a, b, what=""):
    if not bits_equal(a, b):
        a = np.ascontiguousarray(a)
        b = np.ascontiguousarray(b)
        if a.dtype.kind == "f":
            it = np.uint64 if a.dtype.itemsize == 8 else np.uint32
            diff = a.view(it) != b.view(it)
        else:
            diff = a != b
        idx = np.argwhere(diff)
        first = tuple(idx[0]) if len(idx) else None
        raise AssertionError("%s: %d entries differ; first at %s: %r vs %r" % (
            what, int(diff.sum()), first, a[first] if first else None, b[first] if first else None))


# ---- device memory for the tests: the HIP runtime through ctypes, no torch in the process ----------
def dev(a):
    """numpy array -> device array (floydwarshall_amd.hip.DeviceArray)."""
    from floydwarshall_amd import hip
    return hip.DeviceArray.from_numpy(np.ascontiguousarray(a))


def dev_empty(shape, dtype):
    from floydwarshall_amd import hip
    return hip.DeviceArray(shape, dtype)


def dev_zeros(shape, dtype):
    from floydwarshall_amd import hip
    return hip.DeviceArray(shape, dtype).zero_(hip.default_stream())


def host(d):
    """device array -> numpy (waits for the default stream first)."""
    return d.numpy()


def host_cat(ds):
    return np.concatenate([d.numpy() for d in ds])


def dev_sync():
    from floydwarshall_amd import hip
    hip.synchronize()


def digest(a):
    """xxh64 of an array's bytes, in 64 MiB chunks ("xxh64:<hex>": the form the committed fixtures use)."""
    import xxhash
    buf = memoryview(np.ascontiguousarray(a)).cast("B")
    h = xxhash.xxh64()
    for off in range(0, len(buf), 1 << 26):
        h.update(buf[off:off + (1 << 26)])
    return "xxh64:" + h.hexdigest()


def spawn_ranks(fn, args, nprocs, timeout=600):
    """Start `nprocs` fresh interpreters ("spawn": nothing of this process's GPU state is inherited)
    running fn(rank, *args); every rank must exit with 0.  The stdlib twin of
    torch.multiprocessing.spawn -- the pytest process itself never imports torch, so libfwx stays on
    the HIP runtime it was built against here while the ranks are free to import torch first."""
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=fn, args=(rank,) + tuple(args)) for rank in range(nprocs)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout)
    bad = [(i, p.exitcode) for i, p in enumerate(procs) if p.exitcode != 0]
    for p in procs:
        if p.is_alive():
            p.kill()
    assert not bad, "ranks failed (rank, exit code): %s" % bad


def path_from_trace(last, at_col, at_row, next0, a, b):
    """Host restatement of exact_path_kernel: path(a,b) = path_q(a,q) ++ path_q(q,b), q = newest
    pivot of (a,b) -- `last` for the query, at_col / at_row for the two halves."""
    out = []
    stack = [(a, b, 0)]
    while stack:
        x, y, kind = stack.pop()
        q = (last, at_col, at_row)[kind][x, y]
        if q < 0:
            if next0[x, y] >= 0:
                out.append(y)
        else:
            stack.append((int(q), y, 2))
            stack.append((x, int(q), 1))
    return out


def pass_reference(rate, nxt, hops, k0, k1):
    """Everything ONE pass over the pivots [k0, k1) produces, from the whole-matrix state (rate, nxt, hops; nxt /
    hops may be None) at time k0: the oracle stepped one pivot at a time (oracle.relax).  The inputs are left alone.

    Returns a namespace with
      rate, next, hops   the state at time k1
      W, WH, WN          the snapshot panels: row t is row k0 + t of rate / hops / next at the start of step k0 + t
      mask               (k1 - k0) x n x n bool: the entries step k0 + t updated.  An update is a strict x < cand,
                         so an entry was updated exactly when its rate bits changed
      u_rows             U per row: the updates of the pass in each row (int64, n entries)
      last, at_col, at_row   the path trace of this one pass, from all -1: last[i][j] = the last pivot of the pass
                         that updated (i, j) or -1; at_col[i][k] = last[i][k] at the start of step k; at_row[k][j] =
                         last[k][j] at the start of step k (cells of other columns / rows stay -1)."""
    import types
    import oracle
    n, bt = rate.shape[0], k1 - k0
    assert 0 <= k0 <= k1 <= n
    r = rate.copy()
    nx = None if nxt is None else nxt.copy()
    hp = None if hops is None else hops.copy()
    it = np.uint64 if r.dtype.itemsize == 8 else np.uint32
    out = types.SimpleNamespace(
        W=np.empty((bt, n), dtype=r.dtype),
        WH=None if hp is None else np.empty((bt, n), dtype=np.int32),
        WN=None if nx is None else np.empty((bt, n), dtype=np.int32),
        mask=np.zeros((bt, n, n), dtype=bool),
        last=np.full((n, n), -1, dtype=np.int32), at_col=np.full((n, n), -1, dtype=np.int32),
        at_row=np.full((n, n), -1, dtype=np.int32))
    for t, k in enumerate(range(k0, k1)):
        out.W[t] = r[k]
        if hp is not None:
            out.WH[t] = hp[k]
        if nx is not None:
            out.WN[t] = nx[k]
        out.at_col[:, k] = out.last[:, k]
        out.at_row[k, :] = out.last[k, :]
        before = r.view(it).copy()
        oracle.relax(r, nx, hp, k, k + 1)
        out.mask[t] = r.view(it) != before
        out.last[out.mask[t]] = k
    out.rate, out.next, out.hops = r, nx, hp
    out.u_rows = out.mask.sum(axis=(0, 2)).astype(np.int64)
    return out


# ---- BASELINE config 5 (N = 32768 f32, rate + next + hops): oracle slices around launch boundaries -----
CONFIG5_SLICES = ((0, 256), (16256, 16512), (32512, 32768))


def config5_solve_with_oracle_slices(dm, n, threads=None):
    """Solves the matrix uploaded into the handle `dm` (rate + next + hops) over all n pivots, and pins
    three 256-pivot stretches to the oracle: the first pivots (from the input itself), a stretch across the
    middle of the matrix (pivot 16384 = a partition boundary at P = 8; the stretch starts 128 before it, so
    a 128-pivot launch ends exactly there) and the last 256 pivots (ending at the solved matrix).  See
    solve_with_oracle_stretches.  Two tests (the plain handle, P = 8 partitions) walk the same input through
    the same stretches: the second only has to reach the states the first verified (their digests)."""
    return solve_with_oracle_stretches(dm, n, CONFIG5_SLICES, threads, cache=_CONFIG5_ORACLE)


def solve_with_oracle_stretches(dm, n, stretches, threads=None, cache=None):
    """Solves the matrix uploaded into the handle `dm` over all n pivots and pins the pivot `stretches`
    ((a, b) pairs, ascending, the last ending at n) to the oracle.  Every stretch is a pivot range of its own
    on the GPU and is continued on the oracle (the fields the handle carries: rate, + next, + hops; the loop
    tiled over 16 pivots, oracle.relax_mt_tiled, which tests/test_oracle_golden.py pins to the plain loop)
    from the state the GPU held before it.  Returns the solved (rate, next, hops), None for a field the
    handle does not carry.

    cache: a dict shared by tests that walk the same input through the same stretches.  The first to run
    records the digests of the oracle's state after each stretch; a later one only has to reach THOSE states:
    equal digests after a stretch mean its matrix equals one the oracle produced from a verified predecessor
    -- no second oracle run, no download before the stretch.  The oracle runs on a thread of its own (ctypes
    releases the GIL) while the GPU solves the stretch and the result comes back over PCIe."""
    import threading
    import oracle
    pos = 0
    for a, b in stretches:
        if a > pos:
            dm.solve(k_begin=pos, k_end=a)
        cached = cache.get((n, a, b)) if cache is not None else None
        if cached is None:
            er, en, eh = dm.download()
            t = threading.Thread(target=oracle.relax_mt_tiled, args=(er, en, a, b),
                                 kwargs={"threads": threads, "hops": eh, "tile": 16})
            t.start()                                # the oracle continues from the GPU state, beside the GPU
        dm.solve(k_begin=a, k_end=b)
        got = dm.download()
        if cached is None:
            t.join()
            for g, e, what in zip(got, (er, en, eh), ("rate", "next", "hops")):
                if e is not None:
                    assert_bits_equal(g, e, "%s after pivots [%d, %d)" % (what, a, b))
            if cache is not None:
                cache[(n, a, b)] = tuple(digest(e) for e in (er, en, eh) if e is not None)
            del er, en, eh
        else:
            assert tuple(digest(g) for g in got if g is not None) == cached, \
                "state after pivots [%d, %d) differs from the oracle's continuation" % (a, b)
        pos = b
    assert pos == n
    return got


_CONFIG5_ORACLE = {}     # (n, a, b) -> digests (rate, next, hops) of the oracle's state after the stretch


def check_walks_and_exact_lists(rate0, rate, nxt, hops, src, dst, walk_len, walk_prod, exact_lists_of):
    """What path reconstruction must satisfy at config 5's size, stated exactly:
    (1) every walk of the FINAL next-hops from src ends at dst (length >= 1 iff src != dst: D1 is dense);
    (2) its product of INPUT edge rates is the solved rate up to the fp32 roundings of the two routes
        involved: |walk product - rate| <= (len + hops) * 2^-24 * rate  (each of the multiplications that
        formed the stored rate, and each the walk's own route would take, rounds by at most 2^-24);
    (3) `hops` is the length of the list the reference concatenated when the entry last improved
        (Algorithms.hs:55).  The walk may be a different route of equal rank (sub-routes re-routed later),
        so len(walk) == hops is NOT a property -- but for EVERY sampled pair where they differ (and a
        sample of those where they agree) the exact list rebuilt from the path trace has length `hops`,
        ends at dst, starts with the stored next-hop, and the f64 product of the input edges along it
        equals the stored rate up to its own hops - 1 fp32 multiplications: <= (hops - 1) * 2^-24 * 1.001."""
    u = 2.0 ** -24
    same = src == dst
    assert bool((walk_len[same] == 0).all()) and bool((walk_len[~same] >= 1).all())
    solved = rate[src, dst].astype(np.float64)
    h = hops[src, dst].astype(np.int64)
    rel = np.abs(walk_prod - solved) / np.maximum(solved, 1e-300)
    bound = (walk_len.astype(np.int64) + h) * u
    worst = int(np.argmax((rel - bound)[~same]))
    assert bool((rel[~same] <= bound[~same]).all()), (float(rel[~same][worst]), float(bound[~same][worst]))
    differ = np.flatnonzero((walk_len != h) & ~same)
    agree = np.flatnonzero((walk_len == h) & ~same)[:2000]
    pick = np.concatenate([differ, agree])
    lists = exact_lists_of(src[pick], dst[pick])
    for q, i in enumerate(pick):
        s_, d_, path = int(src[i]), int(dst[i]), lists[q]
        assert len(path) == hops[s_, d_], (s_, d_, len(path), int(hops[s_, d_]), int(walk_len[i]))
        assert path[-1] == d_ and path[0] == nxt[s_, d_]
        p, cur = 1.0, s_
        for v in path:
            p *= float(rate0[cur, v])
            cur = v
        r = float(rate[s_, d_])
        assert abs(p - r) <= (len(path) - 1) * u * 1.001 * r, (s_, d_, p, r, len(path))
    return len(differ)


# ---- the per-k engine's multi-pivot schedule (tests/test_gpu_perk_pivots*.py) --------------------------------------
MIB = float(1 << 20)
PERK_PIVOTS = [1, 2, 4, 8]


def perk_launches(reset=True):
    """(single-pivot, 2-, 4-, 8-pivot sweeps, panel launches) of the multi-pivot schedule since the last reset."""
    import ctypes
    from floydwarshall_amd import _lib
    c = (ctypes.c_uint64 * 5)()
    _lib.lib().fwx_test_perk_pivots(c, 1 if reset else 0)
    return [int(v) for v in c]


def perk_expected_launches(kb, ke, np_):
    """What relax_range_kt (csrc/fwx_perk.hip) issues for pivots [kb, ke): per block of <= 64 pivots from kb one panel launch, the
    block's pivots np_ at a time, a ragged end down the powers of two, a last single pivot on relax_k."""
    want = [0, 0, 0, 0, 0]
    if np_ == 1 or ke - kb < 2:
        return want
    for k0 in range(kb, ke, 64):
        bt = min(64, ke - k0)
        if bt >= 2:
            want[4] += 1
            g = np_
            while g >= 2:
                want[{2: 1, 4: 2, 8: 3}[g]] += bt // g
                bt %= g
                g //= 2
        want[0] += bt
    return want


def perk_oracle(rate, kb, ke):
    """(rates, U) of the C oracle over pivots [kb, ke); the input is left alone."""
    import oracle
    er = rate.copy()
    u = oracle.relax_mt(er, None, kb, ke, threads=16, fast=True)
    return er, u


def perk_relax(rate, kb, ke, serp=True, stream=None):
    """fwx_dev_relax on the whole matrix in place, counting: (rates, U)."""
    from floydwarshall_amd import engine
    n = rate.shape[0]
    r_t = dev(rate)
    upd = dev_zeros((engine.FWX_UPDATE_SHARDS,), np.int64)
    engine.dev_relax(r_t, n, 0, kb, ke, serpentine=serp, updates_t=upd, stream=stream)
    return host(r_t), int(host(upd).sum())


def perk_check(rate, kb, ke, monkeypatch, what, budgets=None, serps=(True, False), pivots=PERK_PIVOTS, want=None):
    """Rates, U and the launch counters of fwx_dev_relax over pivots [kb, ke) for every width in `pivots`, every
    temporal budget (default: one that splits the matrix, one that does not) and sweep order.  want: the oracle's
    (rates, U) where the caller shares them between cases."""
    want_r, want_u = want if want is not None else perk_oracle(rate, kb, ke)
    for np_ in pivots:
        monkeypatch.setenv("FWX_PERK_PIVOTS", str(np_))
        for budget in budgets or [repr(rate.nbytes / 2 / MIB), "1e12"]:
            monkeypatch.setenv("FWX_PERK_TEMPORAL_MIB", budget)
            for serp in serps:
                perk_launches()
                got_r, got_u = perk_relax(rate, kb, ke, serp)
                tag = "%s NP=%d budget=%s serp=%s pivots [%d, %d)" % (what, np_, budget, serp, kb, ke)
                assert_bits_equal(got_r, want_r, tag)
                assert got_u == want_u, tag
                assert perk_launches() == perk_expected_launches(kb, ke, np_), tag
