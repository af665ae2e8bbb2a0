"""Every launch form of the fused engine, pinned to the oracle where kernels go wrong: ragged orders
(n mod 128 in {4, 12, 68}, ragged pivot tails), ties, overflow, NaN / negative / -0.0 inputs, f32 and f64,
every field set.  The form a launch takes is picked by tile-count thresholds (csrc/fwx_fused.hip) and by
the schedule crossovers (csrc/fwx_api.hip), so each case also asserts, through the test hook
fwx_test_kernel_forms, that the form it is about actually launched, and the last test asserts that the
file as a whole reached every form but a listed few.

(a) Thresholds forced to 0 in child processes (tests/kernel_forms_worker.py; the knobs are read once
    per process): the large-tile forms at orders the oracle solves in a moment.
(b) Natural orders just past each default crossover, in this process: the whole fused solve against the
    whole per-k solve, and three 256-pivot stretches continued on the oracle from the GPU's state.
(c) Partitioned handles on one GPU at n = 6212, in the [5120, 8192) range of the f32 + next schedule."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from floydwarshall_amd import engine, synth

from helpers import assert_bits_equal, solve_with_oracle_stretches

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
THREADS = min(16, len(os.sched_getaffinity(0)))
SEEN = set()                  # union of the forms every case of this file reached (checked last)

LARGE = {"FWX_SMALL_TILES_BELOW": "0", "FWX_MID_TILES_BELOW": "0", "FWX_ARG_SMALL_TILES_BELOW": "0"}
DOUBLE = {"FWX_DOUBLE_PASS_MIN_N": "0", "FWX_DOUBLE_PASS_NEXT_MIN_N": "0"}
KNOBS = tuple(LARGE) + tuple(DOUBLE) + (
    "FWX_LOOKAHEAD_MIN_N", "FWX_ARG_GENERAL_STAGING", "FWX_ARG_F64_SHORT_TILES", "FWX_PANELS_TIGHT",
    "FWX_PANELS_32_ROWS", "FWX_SPLIT_MAIN", "FWX_SYMMETRIC_MIN_N")


def _run_child(env_over, cases, timeout):
    """One worker process; nothing more starts on the card if it dies by a signal or overruns."""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(env_over)
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "kernel_forms_worker.py"), json.dumps(cases)],
                           env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        pytest.exit("kernel_forms_worker overran %d s with %r: stopping the GPU tests" % (timeout, env_over),
                    returncode=3)
    if r.returncode < 0 or r.returncode in (134, 139):
        pytest.exit("kernel_forms_worker ended with status %d (%r): stopping the GPU tests\n%s"
                    % (r.returncode, env_over, r.stderr[-3000:]), returncode=3)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("KERNEL_FORMS_RESULT ")]
    assert r.returncode == 0 and line, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    return json.loads(line[-1][len("KERNEL_FORMS_RESULT "):])


def _check_results(results, expect):
    bad = []
    for res in results:
        c, forms = res["case"], set(res["forms"])
        SEEN.update(forms)
        want = expect(c)
        if res["error"]:
            bad.append("%r: %s" % (c, res["error"]))
        elif not want <= forms:
            bad.append("%r: forms %s not reached (saw %s)" % (c, sorted(want - forms), sorted(forms)))
    assert not bad, "\n".join(bad)


IN_DOMAIN = ("t1", "t2", "t4")
OUT_OF_DOMAIN = ("t3", "hostile")
ORDERS = (260, 324, 452, 1036)


def _cases(kinds, fields, orders=ORDERS, dtypes=("f32", "f64"), **extra):
    out = []
    for n in orders:
        for kind in kinds:
            for dt in dtypes:
                for f in fields:
                    out.append(dict(kind=kind, n=n, dtype=dt, fields=f, seed=1000 * n + len(out), **extra))
    return out


def _sfx(c):
    return "F32" if c["dtype"] == "f32" else "F64"


def _large_forms(c, two_pass):
    """The main form a fused launch of this case takes with every tile threshold at 0."""
    if c["kind"] in OUT_OF_DOMAIN and c["fields"] not in ("r", "ru"):
        return {"RELAX_K"}        # next-hops outside the domain: the per-k engine solves it (route_solve)
    if c["kind"] in OUT_OF_DOMAIN or c["fields"] in ("ru", "nhu"):
        return {"MAIN_LARGE_" + _sfx(c)}            # compare form: outside the domain, or counting
    if c["fields"] == "r":
        return {"MAX_LARGE_" + _sfx(c)}
    np_ = "NP2" if two_pass else "NP1"
    return {"ARG_RI8_%s_F32" % np_} if c["dtype"] == "f32" else {"ARG_F64_RI4_" + np_}


def test_forced_large_tiles_single_pass():
    """Large-tile forms (128-row arg kernel, 128 x 128 max form, fused_main_max_f64, generic 128-row
    fused_main) at ragged orders, single pass: all kinds, both dtypes, every field set."""
    cases = _cases(IN_DOMAIN, ("r", "ru", "n", "nh", "nhu", "nt")) + _cases(OUT_OF_DOMAIN, ("r", "ru", "nh"))
    _check_results(_run_child(LARGE, cases, 600), lambda c: _large_forms(c, False))


def test_forced_large_tiles_double_pass():
    """The same with the double pass forced: two-pass (NP = 2) instantiations of the arg kernels and the
    max forms on large tiles, split main launches, and the pivot tail (n mod 64 = 4 or 12) that follows
    in the serial schedule.  The exact `_path` lists of one f64 case against the list-faithful oracle."""
    cases = _cases(IN_DOMAIN, ("r", "n", "nh", "nt"))
    cases.append(dict(kind="t1", n=260, dtype="f64", fields="nt", seed=11, lists=True))
    _check_results(_run_child(dict(LARGE, **DOUBLE), cases, 600), lambda c: _large_forms(c, True))


def test_forced_look_ahead_on_large_tiles():
    """The look-ahead schedule (row panel, column panel, main launches restricted to rows or columns)
    with large tiles, at every order."""
    env = dict(LARGE, FWX_LOOKAHEAD_MIN_N="0")
    cases = _cases(("t1", "hostile"), ("r", "n", "nt"), orders=(260, 452))

    def expect(c):
        if c["kind"] == "hostile" and c["fields"] != "r":
            return {"RELAX_K"}
        return {"ROWPANEL_" + _sfx(c), "COLPANEL_" + _sfx(c)}
    _check_results(_run_child(env, cases, 300), expect)


# A/B-only forms the library ships beside the defaults: one child each, a tie-heavy kind at two orders,
# double pass forced (the schedule these switches act on), default tile thresholds
AB_SWITCHES = [
    ({"FWX_ARG_GENERAL_STAGING": "1"}, ("f32", "f64"), lambda c: {"ARG_RI4_NP2_F32"} if c["dtype"] == "f32"
     else {"ARG_F64_RI4_NP2"}),
    ({"FWX_ARG_F64_SHORT_TILES": "1"}, ("f64",), lambda c: {"ARG_F64_RI2_NP2", "ARG_F64_RI2_NP1"}),
    ({"FWX_PANELS_TIGHT": "0"}, ("f32",), lambda c: {"PANELS_F32"}),
    ({"FWX_PANELS_32_ROWS": "0"}, ("f32",), lambda c: {"PANELS_NEXT_F32"} if c["fields"] == "n"
     else {"PANELS_NEXT_TRACE_F32"}),
    ({"FWX_SPLIT_MAIN": "0"}, ("f32",), lambda c: {"ARG_RI4_NP2_F32", "ARG_RI4_NP1_F32"}),
]


@pytest.mark.parametrize("switch", range(len(AB_SWITCHES)), ids=[next(iter(s[0])) for s in AB_SWITCHES])
def test_ab_switch_forms(switch):
    env, dtypes, expect = AB_SWITCHES[switch]
    cases = _cases(("t1",), ("n", "nt"), orders=(260, 708), dtypes=dtypes)
    results = _run_child(dict(DOUBLE, **env), cases, 300)
    _check_results(results, expect)
    if "FWX_PANELS_32_ROWS" in env or "FWX_PANELS_TIGHT" in env:
        for res in results:                           # the switched-off form must not launch
            assert "PANELS_NEXT_F32_R32" not in res["forms"], res["case"]


def test_default_small_forms():
    """At default thresholds small orders take the 64 x 64 forms, n <= 128 the one-workgroup solve and
    the per-k engine relax_k: the rest of the record, same checks."""
    cases = _cases(("t1", "hostile"), ("r", "n", "nt"), orders=(60, 100, 260), engine="auto")
    cases += _cases(("t4",), ("r", "nh"), orders=(324,), engine="perk")
    cases += _cases(("t2",), ("n",), orders=(708,), dtypes=("f32",))

    def expect(c):
        if c["n"] <= 64 or (c["kind"] == "hostile" and c["fields"] != "r" and c["n"] <= 128):
            return {"SMALL_SOLVE"}     # AUTO: the one-workgroup solve, or its fallback outside the domain
        if c.get("engine") == "perk" or (c["kind"] == "hostile" and c["fields"] != "r"):
            return {"RELAX_K"}
        if c["kind"] == "hostile":
            return {"MAIN_SMALL_" + _sfx(c)}
        if c["fields"] == "r":
            return {"MAX_SMALL_" + _sfx(c)}
        return {"ARG_RI4_NP1_F32"} if c["dtype"] == "f32" else {"ARG_F64_RI4_NP1"}
    _check_results(_run_child({}, cases, 300), expect)


# ---- (b) natural orders at default thresholds, in this process -----------------------------------------
def _fields(rate, nxt, hops, fields):
    return rate, (nxt if fields != "r" else None), (hops if "h" in fields else None)


def _stretches(n):
    """First 256 pivots, 256 across the middle (starting at a multiple of 128), the last 256 with the tail."""
    mid = n // 2 // 128 * 128
    last = (n - 256) // 128 * 128
    return ((0, 256), (mid, mid + 256), (last, n))


def _natural(n, dtype, kind, fields, want, seed):
    rate, nxt, hops = _fields(*synth.make(kind, n, dtype, seed=seed), fields)
    with_next, with_hops, trace = nxt is not None, hops is not None, fields == "nt"
    engine.kernel_forms_seen(reset=True)
    out = {}
    for name, eng in (("auto", engine.FWX_ENGINE_AUTO), ("perk", engine.FWX_ENGINE_PERK)):
        with engine.DeviceMatrix(n, dtype, with_next=with_next, with_hops=with_hops) as dm:
            if trace:
                dm.enable_path_log()
            dm.upload(rate, nxt, hops)
            dm.solve(engine=eng)
            got = dm.download()
            if trace:
                rnd = np.random.default_rng(seed)
                src = rnd.integers(0, n, 20000).astype(np.int32)
                dst = rnd.integers(0, n, 20000).astype(np.int32)
                got = got + (dm.query_exact_batch(src, dst),)
        out[name] = got
        if name == "auto":
            forms = engine.kernel_forms_seen(reset=True)
            SEEN.update(forms)
            assert want <= forms, (sorted(want - forms), sorted(forms))
    for i, what in enumerate(("rate", "next", "hops")):
        if out["auto"][i] is not None:
            assert_bits_equal(out["auto"][i], out["perk"][i], what + " fused vs per-k")
    if trace:
        assert out["auto"][3] == out["perk"][3], "exact lists fused vs per-k"
        return                                            # a traced solve covers the whole range only
    with engine.DeviceMatrix(n, dtype, with_next=with_next, with_hops=with_hops) as dm:
        dm.upload(rate, nxt, hops)
        gr, gn, gh = solve_with_oracle_stretches(dm, n, _stretches(n), threads=THREADS)
    SEEN.update(engine.kernel_forms_seen(reset=True))
    for a, b, what in ((gr, out["auto"][0], "rate"), (gn, out["auto"][1], "next"), (gh, out["auto"][2], "hops")):
        if a is not None:
            assert_bits_equal(a, b, what + ": stretched solve vs whole solve")


@pytest.mark.parametrize("kind,fields", [("t1", "n"), ("t1", "nh"), ("t1", "nt"), ("t4", "n")])
def test_natural_10436_arg_128_rows(kind, fields):
    """f32 + next past the arg kernel's tile threshold: 128-row arg kernel, two passes and the 4-pivot tail."""
    want = {"ARG_RI8_NP2_F32", "ARG_RI8_NP1_F32"}
    _natural(10436, np.float32, kind, fields, want, seed=104)


@pytest.mark.parametrize("kind", ["t1", "t4"])
def test_natural_7684_max_128(kind):
    _natural(7684, np.float32, kind, "r", {"MAX_LARGE_F32"}, seed=768)


def test_natural_6212_max_f64():
    """97 blocks (an odd count) and a 4-pivot tail on fused_main_max_f64."""
    _natural(6212, np.float64, "t4", "r", {"MAX_LARGE_F64"}, seed=621)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind,fields,count", [("t3", "r", False), ("hostile", "r", True), ("t1", "r", False),
                                               ("t1", "nh", True)])
def test_natural_2948_whole_oracle(kind, fields, count, dtype):
    """Past the 512-tile threshold: large generic forms (out of the domain, counting), the max forms."""
    from hostile_inputs import hostile_matrix
    n = 2948
    if kind == "hostile":
        src = hostile_matrix(np.random.default_rng(29), n, dtype)
    else:
        src = synth.make(kind, n, dtype, seed=29)
    rate, nxt, hops = _fields(*src, fields)
    er, en, eh = rate.copy(), None if nxt is None else nxt.copy(), None if hops is None else hops.copy()
    eu = oracle.relax_mt(er, en, hops=eh, threads=THREADS, fast=True)
    gr, gn, gh = rate.copy(), None if nxt is None else nxt.copy(), None if hops is None else hops.copy()
    engine.kernel_forms_seen(reset=True)
    u = engine.solve(gr, gn, gh, device=0, engine=engine.FWX_ENGINE_FUSED, count_updates=count)
    forms = engine.kernel_forms_seen(reset=True)
    SEEN.update(forms)
    sfx = "F32" if dtype == np.float32 else "F64"
    want = {"MAIN_LARGE_" + sfx} if (count or kind != "t1") else {"MAX_MID_F32" if sfx == "F32" else "MAX_LARGE_F64"}
    assert want <= forms, (sorted(want - forms), sorted(forms))
    assert_bits_equal(gr, er, "rate")
    if gn is not None:
        assert_bits_equal(gn, en, "next")
        assert_bits_equal(gh, eh, "hops")
    if count:
        assert u == eu


# ---- (c) partitioned handles at default thresholds ------------------------------------------------------
def test_partitioned_6212_next_trace():
    """f32 + next + trace, t1, on two and three logical partitions of one GPU (the last slab ragged):
    the single-device handle's result and exact lists bit for bit, and oracle stretches (+ next)."""
    n = 6212
    rate, nxt, _ = synth.make("t1", n, np.float32, seed=62)
    rnd = np.random.default_rng(62)
    src = rnd.integers(0, n, 20000).astype(np.int32)
    dst = rnd.integers(0, n, 20000).astype(np.int32)
    outs = []
    for devices in (None, [0, 0], [0, 0, 0]):
        engine.kernel_forms_seen(reset=True)
        with engine.DeviceMatrix(n, np.float32, with_next=True, devices=devices) as dm:
            dm.enable_path_log()
            dm.upload(rate, nxt)
            dm.solve()
            gr, gn, _ = dm.download()
            outs.append((gr, gn, dm.query_exact_batch(src, dst)))
        SEEN.update(engine.kernel_forms_seen(reset=True))
    for o, d in zip(outs[1:], ("2 partitions", "3 partitions")):
        assert_bits_equal(o[0], outs[0][0], "rate " + d)
        assert_bits_equal(o[1], outs[0][1], "next " + d)
        assert o[2] == outs[0][2], "exact lists " + d
    cache = {}                                       # the second handle reaches the states the first verified
    for devices in ([0, 0], [0, 0, 0]):
        with engine.DeviceMatrix(n, np.float32, with_next=True, devices=devices) as dm:
            dm.upload(rate, nxt)
            gr, gn, _ = solve_with_oracle_stretches(dm, n, _stretches(n), threads=THREADS, cache=cache)
        SEEN.update(engine.kernel_forms_seen(reset=True))
        assert_bits_equal(gr, outs[0][0], "rate, stretched partitioned solve")
        assert_bits_equal(gn, outs[0][1], "next, stretched partitioned solve")


# ---- (d) coverage: runs last ------------------------------------------------------------------------------
# Forms no case above is expected to reach, name -> reason.  Empty: every form the library ships launches
# in this file.  A form added later, or one a threshold change leaves unreached, fails the test below until
# a case reaches it or it is listed here with its reason.
EXCLUDED = {}


def test_zz_every_form_was_reached():
    missing = set(engine.KERNEL_FORMS) - SEEN - set(EXCLUDED)
    assert not missing, "forms no test of this file reached: %s (seen: %s)" % (sorted(missing), sorted(SEEN))
