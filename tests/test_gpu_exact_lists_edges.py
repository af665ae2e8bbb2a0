"""Exact `_path` lists of ALL pairs after one traced solve, at the orders where the kernels that keep the path trace
change shape and on inputs outside the reference's domain, against the rope oracle (oracle/list_ropes.py, pinned to
the list-faithful restatement and to the dense C loop by tests/test_oracle_ropes.py).

Why these inputs.  On the reference's domain every winning product has a non-empty ikPath and every leaf of a
list's concatenation tree is a vertex.  Outside it -- NaN, negative or -0.0 rates, positive rates whose path is
empty (hostile_inputs.hostile_matrix_mix) -- an update can concatenate an EMPTY ikPath, an entry can hold a positive
rate and an empty list, and a leaf with next0 < 0 contributes nothing.  Every hostile case asserts, from the oracle
alone and before any GPU call, that all three occur and that some list is not the walk of the final next-hops.
(t3 leaves the domain through NaN and negative rates only: each of its off-diagonal entries starts with a one-vertex
path, so no list of it is ever empty; it asserts the differing walk alone.)

Why these orders (n is the caller's order; the device pitch nd pads rows to 16 bytes, and the single-launch kernel is
given nd):
  single launch, 64 x 64 register tile   n <= 64: 61 (f32 pitch 64, f64 62), 63, 64
  single launch, 128-wide tile, LDS      65, 125 (f32 pitch 128), 127, 128 -- AUTO takes it there for inputs outside the
                                         domain; an input inside it goes to the fused engine above 64 (fwx.h,
                                         fwx_engine), so t2 and the market run the fused kernels with the trace at
                                         one and two ragged blocks
  relax_k with the trace (PERK)          63, 65, 129, 130 (pitches 132 / 130)
  AUTO outside the domain above 128      129, 136: per-k
  fused with the trace, padded pitch     129, 130, 193: t1, t2
Each case: one traced solve counting U; rate bits, next, hops (where the route carries them: the fused engine with the
trace does not) and U against the C oracle; the route through engine.kernel_forms_seen; all n^2 lists in one
query_exact_batch with cap = longest list + 2 (the capacity rule has its own tests below) against the ropes.

The capacity rule (fwx.h, fwx_matrix_query_exact): cap >= L returns the list, cap < L FWX_ERR_CAPACITY, nothing
else -- also where pending halves of the concatenation yield nothing, which is where a walk stack sized by cap
ran out before the list did."""
import ctypes
import functools

import numpy as np
import pytest

import oracle
from floydwarshall_amd import engine, synth
from floydwarshall_amd._lib import FWX_ERR_CAPACITY, lib
from oracle import list_faithful as lf
from oracle import list_ropes

from helpers import assert_bits_equal
from hostile_inputs import hostile_matrix_mix, market_rates

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
MAX_LIST = 4096
NOT_FUSED = {"SMALL_SOLVE", "RELAX_K"}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _off_domain_facts(ropes):
    """(lists that are not the walk of the final next-hops, updates with an empty ikPath, off-diagonal entries with
    a positive rate and an empty list) -- from the oracle alone."""
    n = ropes.n
    en = ropes.next
    differ = 0
    for s in range(n):
        for d in range(n):
            walk = oracle.follow_path(en, s, d)
            differ += walk is None or tuple(walk) != ropes.path(s, d)
    off = ~np.eye(n, dtype=bool)
    with np.errstate(invalid="ignore"):
        positive_empty = int(((ropes.rate > 0) & (ropes.lengths == 0) & off).sum())
    return differ, ropes.updates_empty_left, positive_empty


@functools.lru_cache(maxsize=None)
def _input(kind, n, dtype):
    """(rate, next, hops, ropes) of one named input: computed once, never modified.  Seeds are derived from n; where
    an input has to have a property (see the module docstring) the first draw or seed that has it is taken, decided
    by the oracle alone."""
    if kind in ("hostile_light", "hostile_heavy"):
        rnd = np.random.default_rng(7000 + n)
        for _ in range(32):
            rate, nxt, hops, heavy = hostile_matrix_mix(rnd, n, dtype)
            if heavy != (kind == "hostile_heavy"):
                continue
            ropes = list_ropes.solve(rate, nxt)
            if int(ropes.lengths.max()) <= MAX_LIST and all(_off_domain_facts(ropes)):
                return _frozen(rate, nxt, hops) + (ropes,)
        raise AssertionError("no %s draw of order %d with the properties the case is about" % (kind, n))
    if kind == "market":
        n_ccy = 8
        n_exch = -(-n // n_ccy) + 1
        m0 = lf.build_matrix(market_rates(n_exch, n_ccy, seed=23 + n), dtype)
        assert len(m0) >= n
        _, rate, nxt, hops = lf.to_dense(m0, dtype)      # the leading n vertices: a market on fewer vertices
        rate, nxt, hops = _frozen(*(np.ascontiguousarray(a[:n, :n]) for a in (rate, nxt, hops)))
    elif kind == "t3":                                   # arbitrage: lists grow; a seed whose lists stay in bounds
        for seed in range(500 + n, 532 + n):
            rate, nxt, hops = _frozen(*synth.make("t3", n, dtype, seed=seed))
            ropes = list_ropes.solve(rate, nxt)
            if int(ropes.lengths.max()) <= MAX_LIST:
                return rate, nxt, hops, ropes
        raise AssertionError("no t3 seed of order %d whose lists stay within %d entries" % (n, MAX_LIST))
    else:
        rate, nxt, hops = _frozen(*synth.make(kind, n, dtype, seed=500 + n))
    return rate, nxt, hops, list_ropes.solve(rate, nxt)


@functools.lru_cache(maxsize=None)
def _ref(kind, n, dtype):
    """The input, the C oracle's solution, the ropes and all n^2 lists: computed once, shared, never modified."""
    rate, nxt, hops, ropes = _input(kind, n, dtype)
    er, en, eh = rate.copy(), nxt.copy(), hops.copy()
    eu = oracle.relax(er, en, eh)
    off = ~np.eye(n, dtype=bool)
    assert_bits_equal(ropes.rate, er, "ropes vs dense loop: rate")       # the two oracles agree on this input
    assert_bits_equal(ropes.next, en, "ropes vs dense loop: next")
    assert np.array_equal(ropes.hops[off], eh[off]) and ropes.updates == eu
    _frozen(er, en, eh)
    lists = ropes.all_paths()
    longest = max(len(p) for row in lists for p in row)
    assert longest == int(ropes.lengths.max()) <= MAX_LIST
    facts = _off_domain_facts(ropes) if kind.startswith("hostile") or kind == "t3" else None
    return {"rate": rate, "next": nxt, "hops": hops, "er": er, "en": en, "eh": eh, "eu": eu, "ropes": ropes,
            "lists": lists, "longest": longest, "facts": facts}


def _in_domain(rate, nxt):
    with np.errstate(invalid="ignore"):
        d1 = bool((~np.signbit(rate) & ~np.isnan(rate)).all())
    return d1 and bool(((rate == 0) | (nxt >= 0)).all())


def _expected_route(n, dtype, in_domain, eng):
    """The route fwx.h documents for a handle (fwx_engine, "Domain"): small | perk | fused."""
    if eng == engine.FWX_ENGINE_PERK:
        return "perk"
    if n <= 64:
        return "small"
    if in_domain:
        return "fused"
    nd = -(-n // (16 // np.dtype(dtype).itemsize)) * (16 // np.dtype(dtype).itemsize)
    return "small" if nd <= 128 else "perk"


def _case(kind, n, dtype, eng, route):
    ref = _ref(kind, n, dtype)
    rate, nxt, hops, ropes, lists = ref["rate"], ref["next"], ref["hops"], ref["ropes"], ref["lists"]
    # ---- preconditions, from the oracle alone ------------------------------------------------------------
    in_domain = _in_domain(rate, nxt)
    assert in_domain == (kind in ("t1", "t2", "market"))
    assert _expected_route(n, dtype, in_domain, eng) == route
    assert ref["eu"] > 0
    if kind.startswith("hostile"):
        assert all(f > 0 for f in ref["facts"]), ref["facts"]
    elif kind == "t3":
        assert ref["facts"][0] > 0, ref["facts"]
    # ---- the GPU -----------------------------------------------------------------------------------------
    with_hops = route != "fused"
    cap = max(ref["longest"], 1) + 2
    src = np.repeat(np.arange(n, dtype=np.int32), n)
    dst = np.tile(np.arange(n, dtype=np.int32), n)
    with engine.DeviceMatrix(n, dtype, with_next=True, with_hops=with_hops) as dm:
        dm.enable_path_log()
        dm.upload(rate, nxt, hops if with_hops else None)
        engine.kernel_forms_seen(reset=True)
        u = dm.solve(count_updates=True, engine=eng)
        forms = engine.kernel_forms_seen(reset=True)
        logged = dm.path_log_count()
        gr, gn, gh = dm.download()
        got = dm.query_exact_batch(src, dst, cap=cap)
    print("%s n=%d %s: route %s, forms %s, U %d (oracle %d), longest list %d, empty-ikPath updates %d"
          % (kind, n, np.dtype(dtype).name, route, sorted(forms), u, ref["eu"], ref["longest"],
             ropes.updates_empty_left))
    if route == "small":
        assert forms == {"SMALL_SOLVE"}
    elif route == "perk":
        assert forms == {"RELAX_K"}
    else:
        assert forms and not forms & NOT_FUSED
    assert_bits_equal(gr, ref["er"], "rate")
    assert_bits_equal(gn, ref["en"], "next")
    if with_hops:
        assert_bits_equal(gh, ref["eh"], "hops")
    assert u == ref["eu"] and logged == ref["eu"]
    assert len(got) == n * n
    bad = [(int(src[q]), int(dst[q])) for q in range(n * n) if tuple(got[q]) != lists[src[q]][dst[q]]]
    assert not bad, "%d lists differ, first (%d, %d): %r vs %r" % (
        len(bad), bad[0][0], bad[0][1], got[bad[0][0] * n + bad[0][1]], lists[bad[0][0]][bad[0][1]])


DTYPES = [F32, F64]
HOSTILE = ("hostile_light", "hostile_heavy")
AUTO, PERK = engine.FWX_ENGINE_AUTO, engine.FWX_ENGINE_PERK


def _ids(v):
    return np.dtype(v).name if isinstance(v, type) else None


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("kind", HOSTILE + ("t2", "market"))
@pytest.mark.parametrize("n", [61, 63, 64])
def test_single_launch_64_wide_tile(n, kind, dtype):
    _case(kind, n, dtype, AUTO, "small")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("kind", HOSTILE + ("t2", "market"))
@pytest.mark.parametrize("n", [65, 125, 127, 128])
def test_single_launch_128_wide_tile(n, kind, dtype):
    """Outside the domain AUTO keeps the single launch up to a pitch of 128; t2 and the market are inside it, and
    AUTO gives them to the fused engine above n = 64 (module docstring)."""
    _case(kind, n, dtype, AUTO, "small" if kind in HOSTILE else "fused")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("kind", HOSTILE + ("t1",))
@pytest.mark.parametrize("n", [63, 65, 129, 130])
def test_relax_k_with_the_trace(n, kind, dtype):
    _case(kind, n, dtype, PERK, "perk")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("kind", ["hostile_light", "hostile_heavy", "t3"])
@pytest.mark.parametrize("n", [129, 136])
def test_auto_outside_the_domain_above_128(n, kind, dtype):
    _case(kind, n, dtype, AUTO, "perk")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("kind", ["t1", "t2"])
@pytest.mark.parametrize("n", [129, 130, 193])
def test_fused_with_the_trace_padded_pitch(n, kind, dtype):
    _case(kind, n, dtype, AUTO, "fused")


# ---- the capacity rule ---------------------------------------------------------------------------------------------
def _query_raw(dm, s, d, cap):
    """fwx_matrix_query_exact as the C caller sees it: (status or length, list)."""
    out = np.full(max(cap, 1), -7, dtype=np.int32)
    r = ctypes.c_double(-1.0)
    st = lib().fwx_matrix_query_exact(dm._h, int(s), int(d), ctypes.byref(r), out.ctypes.data_as(ctypes.c_void_p),
                                      int(cap))
    return st, tuple(int(x) for x in out[:max(st, 0)])


def _batch_raw(dm, src, dst, cap):
    src = np.ascontiguousarray(src, dtype=np.int32)
    dst = np.ascontiguousarray(dst, dtype=np.int32)
    lens = np.full(len(src), -99, dtype=np.int32)
    paths = np.full((len(src), cap), -7, dtype=np.int32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    st = lib().fwx_matrix_query_exact_batch(dm._h, len(src), ptr(src), ptr(dst), ptr(lens), ptr(paths), cap)
    assert st == 0
    return [(int(lens[q]), tuple(int(v) for v in paths[q, :max(int(lens[q]), 0)])) for q in range(len(src))]


def _peak_pending(ropes, s, d):
    """Most halves pending at once when the concatenation tree of list (s, d) is flattened depth-first with no
    knowledge of which halves are empty: what a stack has to hold.  From the oracle's tree alone."""
    n, left, right = ropes.n, ropes._left, ropes._right
    stack, peak = [int(ropes.node[s, d])], 1
    while stack:
        x = stack.pop()
        if x > n:
            stack.append(int(right[x]))
            stack.append(int(left[x]))
            peak = max(peak, len(stack))
    return peak


def _probes(ref, n, hostile):
    """The longest list and three more, chosen from the oracle: lists of length 1 and 2 that an update made (any
    updated entry of length 1 is one whose other half is empty; in-domain no update yields length 1 and an input
    edge stands in), and the list whose tree has the most pending halves beyond its own length -- outside the
    domain more than the list has entries, which a stack of `cap` triples cannot hold at cap = L."""
    lists, ropes = ref["lists"], ref["ropes"]
    pairs = [(s, d) for s in range(n) for d in range(n) if s != d]
    length = lambda sd: len(lists[sd[0]][sd[1]])  # noqa: E731
    updated = ropes.node > n
    longest = max(pairs, key=length)
    one = next(sd for sd in pairs if length(sd) == 1 and (updated[sd] or not hostile))
    two = next(sd for sd in pairs if length(sd) == 2 and updated[sd])
    excess = lambda sd: _peak_pending(ropes, *sd) - length(sd)  # noqa: E731
    deep = max((sd for sd in pairs if sd not in (longest, one, two) and length(sd) >= 3), key=excess)
    if hostile:
        assert updated[one] and excess(deep) > 0, (one, deep, excess(deep))
    else:
        assert max(excess(sd) for sd in pairs) <= 0          # module docstring of test_gpu_query_kinds.py
    return [longest, one, two, deep]


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("kind", ["t1", "hostile_heavy"])
def test_capacity_rule(kind, dtype):
    """cap >= L returns the list, cap < L is FWX_ERR_CAPACITY, nothing else: one query at a time and in a batch
    that mixes fitting and non-fitting items, in-domain and outside."""
    n = 65
    ref = _ref(kind, n, dtype)
    lists = ref["lists"]
    probes = _probes(ref, n, kind != "t1")
    assert len(lists[probes[0][0]][probes[0][1]]) >= 3
    with engine.DeviceMatrix(n, dtype, with_next=True) as dm:
        dm.enable_path_log()
        dm.upload(ref["rate"], ref["next"])
        dm.solve()
        bad = []
        for s, d in probes:
            want = lists[s][d]
            L = len(want)
            caps = sorted({c for c in (L - 1, L, L + 1, 1, 2) if c >= 1 and (c >= L - 1 or L <= 2)})
            for cap in caps:
                expect = (L, want) if cap >= L else (FWX_ERR_CAPACITY, ())
                got = _query_raw(dm, s, d, cap)
                print("(%d, %d) L=%d cap=%d: single %r" % (s, d, L, cap, got[0]))
                if got != expect:
                    bad.append(("single", s, d, L, cap, got[0]))
        # batches: every probe beside the others at each probe's own L - 1, L, L + 1 (and 1, 2)
        for cap in sorted({c for s, d in probes for c in (len(lists[s][d]) - 1, len(lists[s][d]),
                                                           len(lists[s][d]) + 1, 1, 2) if c >= 1}):
            items = probes + [(0, 0)] + probes[::-1]
            got = _batch_raw(dm, [s for s, _ in items], [d for _, d in items], cap)
            fits = [len(lists[s][d]) <= cap for s, d in items]
            for (s, d), g in zip(items, got):
                want = lists[s][d]
                expect = (len(want), want) if cap >= len(want) else (FWX_ERR_CAPACITY, ())
                if g[0] < 0:
                    g = (g[0], ())
                if g != expect:
                    bad.append(("batch", s, d, len(want), cap, g[0]))
            if 1 < cap < ref["longest"]:
                assert any(fits) and not all(fits)
        assert not bad, "(form, src, dst, L, cap, status): %r" % bad
