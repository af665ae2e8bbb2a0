"""The data operations of a handle (upload, download, keep_input, patch_input, enable_path_log, enable_resume,
resolve) are written once, as loops over the handle's slabs (csrc/fwx_handle.h): a single-device handle is one
slab of all rows, a row-partitioned handle one slab per partition.  These tests pin what both kinds did before
that: every download equals the CPU oracle bit for bit, exact `_path` lists equal the list-faithful restatement,
and the state machine (what can be resumed, and from where) answers the recorded values.

Orders.  n = 258 f32: the device pitch is 260, two partitions are cut at rows 0 / 128 (258 >= 2 * 128: aligned),
three at 0 / 86 / 172 (unaligned), and one checkpoint lands at pivot 128 -- the smallest order at which padding,
aligned partitions and a resumable checkpoint occur together.  n = 131 f64 (pitch 132; partitions at 0 / 65 and
0 / 43 / 87) where no checkpoint is involved.  The list-faithful restatement is a pure-Python triple loop: 1.6 s
at n = 131 f64, where it runs here, and over a minute at n = 258 in f32, where its lists come from the fixture
tests/golden/handle_kinds_lists_n258_f32.json (written by tests/golden/make_handle_kinds_lists.py, tied to the
input and to the C oracle by tests/test_oracle_golden.py)."""
import functools

import numpy as np
import pytest

import oracle
from floydwarshall_amd import engine, synth
from floydwarshall_amd._lib import FWX_ERR_OOM, lib
from oracle import list_faithful as lf

from helpers import assert_bits_equal, load_golden

pytestmark = pytest.mark.gpu

KINDS = {"single": None, "parts2": [0, 0], "parts3": [0, 0, 0]}
ORDERS = [(258, np.float32), (131, np.float64)]


@functools.lru_cache(maxsize=None)
def _input(kind, n, dtype, seed):
    """An input and its oracle solution: computed once, never modified."""
    rate, nxt, hops = synth.make(kind, n, dtype, seed=seed)
    er, en, eh = rate.copy(), nxt.copy(), hops.copy()
    oracle.relax(er, en, eh)
    for a in (rate, nxt, hops, er, en, eh):
        a.setflags(write=False)
    return rate, nxt, hops, er, en, eh


@functools.lru_cache(maxsize=None)
def _lists(n, dtype, seed):
    """{(src, dst): list-faithful `_path`} with the longest list first: every pair at n = 131, the fixture's at
    n = 258 (module docstring)."""
    if n == 258:
        g = load_golden("handle_kinds_lists_n258_f32.json")
        assert (g["kind"], g["n"], g["dtype"], g["seed"]) == ("t1", n, np.dtype(dtype).name, seed)
        assert [g["lists"][0]["src"], g["lists"][0]["dst"]] == g["longest"] and len(g["lists"][0]["path"]) == g["max_len"]
        return {(e["src"], e["dst"]): tuple(e["path"]) for e in g["lists"]}
    rate, nxt = _input("t1", n, dtype, seed)[:2]
    vertices = [("X", "C%03d" % i) for i in range(n)]
    paths = lf.path_indices(lf.run_algo(lf.from_dense(vertices, rate, nxt), dtype))
    s, d = max(((s, d) for s in range(n) for d in range(n)), key=lambda sd: len(paths[sd[0]][sd[1]]))
    pairs = [(s, d), (0, n - 1), (n - 1, 0), (n // 2, n // 2 + 1), (n - 1, n - 2)]       # one per slab and more
    return {sd: paths[sd[0]][sd[1]] for sd in pairs}


def _handle(n, dtype, kind, **kw):
    return engine.DeviceMatrix(n, dtype, with_next=True, devices=KINDS[kind], **kw)


def _equals_oracle(dm, rate, nxt, hops=None, what=""):
    er, en = rate.copy(), nxt.copy()
    eh = None if hops is None else hops.copy()
    oracle.relax(er, en, eh)
    gr, gn, gh = dm.download()
    assert_bits_equal(gr, er, "rate " + what)
    assert_bits_equal(gn, en, "next " + what)
    if hops is not None:
        assert_bits_equal(gh, eh, "hops " + what)


# resumed_from after each step of test_what_invalidates_a_recording's sequence (tests/test_gpu_resume.py), as
# the library answered before the operations were merged; the two kinds agree at every step:
#   resolve | solved twice over, resolve | resolve | patch_input + solve, resolve | counted resolve |
#   per-k resolve | resolve (the per-k solve recorded nothing) | resolve | new upload, resolve
STATE_MACHINE = {"single": [128, 0, 128, 128, 0, 0, 0, 128, 0],
                 "parts2": [128, 0, 128, 128, 0, 0, 0, 128, 0]}


@pytest.mark.parametrize("kind", ["single", "parts2"])
def test_the_state_machine_is_the_same_on_both_kinds(kind):
    n = 258
    rate, nxt = (a.copy() for a in _input("d1", n, np.float32, 9)[:2])
    idx = np.array([200 * n + 201], dtype=np.int64)
    nv = np.array([201], dtype=np.int32)
    started = []

    def change(dm, val, **kw):
        v = np.array([val], dtype=np.float32)
        rate.reshape(-1)[idx] = v
        started.append(dm.resolve(idx, v, nv, **kw))
        _equals_oracle(dm, rate, nxt, what="after step %d (resumed at %d)" % (len(started), started[-1]))

    with _handle(n, np.float32, kind) as dm:
        if kind != "single":
            assert [dm.part_rows(p) for p in range(2)] == [(0, 128), (128, 130)]
        dm.keep_input()
        assert dm.enable_resume(1) == 1                        # one checkpoint, at pivot 128
        dm.upload(rate, nxt)
        dm.solve()
        change(dm, 0.41)
        dm.solve()                                             # solved twice over: not the input's solve
        change(dm, 0.42)
        change(dm, 0.43)
        dm.patch_input(idx, np.array([0.44], dtype=np.float32), nv)
        rate.reshape(-1)[idx] = np.float32(0.44)
        dm.solve()
        _equals_oracle(dm, rate, nxt, what="after patch_input + solve")
        change(dm, 0.45)
        change(dm, 0.46, count_updates=True)
        change(dm, 0.47, engine=engine.FWX_ENGINE_PERK)
        change(dm, 0.48)
        change(dm, 0.49)
        dm.upload(rate, nxt)
        change(dm, 0.50)
    print("resumed_from", kind, started)
    assert started == STATE_MACHINE[kind]


@pytest.mark.parametrize("kind", ["single", "parts3"])
@pytest.mark.parametrize("n,dtype", ORDERS)
def test_a_second_upload_replaces_the_first(n, dtype, kind):
    """A padded partitioned handle writes its padding again on every upload, a single-device handle wrote it
    once at create: either way the second solve sees the second input and inert padding."""
    a = _input("d2", n, dtype, 31)
    b = _input("d1", n, dtype, 32)
    with _handle(n, dtype, kind, with_hops=True) as dm:
        for rate, nxt, hops, er, en, eh in (a, b):
            dm.upload(rate, nxt, hops)
            dm.solve()
            gr, gn, gh = dm.download()
            assert_bits_equal(gr, er, "rate")
            assert_bits_equal(gn, en, "next")
            assert_bits_equal(gh, eh, "hops")


@pytest.mark.parametrize("keep_first", [True, False], ids=["keep-then-upload", "upload-then-keep"])
@pytest.mark.parametrize("kind", ["single", "parts2", "parts3"])
@pytest.mark.parametrize("n,dtype", ORDERS)
def test_keep_input_patch_input_solve(n, dtype, kind, keep_first):
    """Patched entries in the first slab, in the last real row (the slab that also holds the padding rows) and,
    on three partitions, in the middle slab; (1, 0) and the last column besides."""
    rate, nxt, hops = (a.copy() for a in _input("d2", n, dtype, 33)[:3])
    index = np.array([5 * n + (n - 1), (n - 1) * n + 3, (n // 2) * n + (n // 2 + 1), 1 * n + 0], dtype=np.int64)
    vals = (rate.reshape(-1)[index] * dtype(0.93)).astype(dtype)
    vals[3] = 0.0                                              # a pair that stops trading
    pn = (index % n).astype(np.int32)
    ph = np.ones(4, dtype=np.int32)
    pn[3], ph[3] = -1, 0
    with _handle(n, dtype, kind, with_hops=True) as dm:
        if keep_first:
            dm.keep_input()
        dm.upload(rate, nxt, hops)
        if not keep_first:
            dm.keep_input()
        dm.solve()
        dm.patch_input(index, vals, pn, ph)
        dm.solve()
        rate.reshape(-1)[index], nxt.reshape(-1)[index], hops.reshape(-1)[index] = vals, pn, ph
        _equals_oracle(dm, rate, nxt, hops, "after patch_input")


@pytest.mark.parametrize("kind", ["single", "parts2", "parts3"])
@pytest.mark.parametrize("n,dtype", ORDERS)
def test_a_trace_enabled_on_a_fresh_upload_keeps_that_upload(n, dtype, kind):
    rate, nxt, _, er, en, _ = _input("t1", n, dtype, 100 + n)
    with _handle(n, dtype, kind) as dm:
        dm.upload(rate, nxt)
        dm.enable_path_log()
        dm.solve()
        gr, gn, _ = dm.download()
        assert_bits_equal(gr, er, "rate")
        assert_bits_equal(gn, en, "next")
        paths = _lists(n, dtype, 100 + n)
        (s, d), longest = next(iter(paths.items()))
        assert len(longest) >= 2
        r, p = dm.query_exact(s, d)
        assert tuple(p) == longest
        assert_bits_equal(np.array([r]), np.array([er[s, d]]).astype(np.float64), "rate of the longest list")
        for (s, d), want in paths.items():
            assert tuple(dm.query_exact(s, d)[1]) == want, (s, d)


@pytest.mark.parametrize("countdown", [1, 2, 3])
@pytest.mark.parametrize("kind", ["single", "parts2"])
def test_a_failed_enable_resume_leaves_a_usable_handle(kind, countdown):
    """The injected bad_alloc (fwx_test_fail_after: host side, no GPU fault) at the countdown-th allocation point
    from enable_resume on: 1 = before anything is allocated, 2 = before the first slab's store, 3 = before the
    second slab's, when the first slab's store exists and has to be released again (one device: no third point,
    the call succeeds and the hook is disarmed unused; a library with the one point at the start succeeds at 2
    and 3 on both kinds).  Whether it failed or not, the handle then enables, solves, resolves from the checkpoint
    and matches the oracle."""
    n = 258
    rate, nxt = (a.copy() for a in _input("d2", n, np.float32, 23)[:2])
    with _handle(n, np.float32, kind) as dm:
        dm.keep_input()
        enabled = None
        try:
            lib().fwx_test_fail_after(countdown)
            try:
                enabled = dm.enable_resume(1)
            except engine.FwxError as e:
                assert e.status == FWX_ERR_OOM
        finally:
            lib().fwx_test_fail_after(0)
        assert enabled in (None, 1) and (countdown > 1 or enabled is None)
        dm.upload(rate, nxt)
        dm.solve()
        _equals_oracle(dm, rate, nxt, what="after the failed enable_resume")
        idx = np.array([200 * n + 201], dtype=np.int64)
        v = (rate.reshape(-1)[idx] * np.float32(0.95)).astype(np.float32)
        rate.reshape(-1)[idx] = v
        assert dm.resolve(idx, v, np.array([201], dtype=np.int32)) == (0 if enabled is None else 128)
        _equals_oracle(dm, rate, nxt, what="after the first resolve")
        if enabled is None:
            assert dm.enable_resume(1) == 1
            dm.upload(rate, nxt)
            dm.solve()
        idx = np.array([257 * n + 130], dtype=np.int64)            # the last real row
        v = (rate.reshape(-1)[idx] * np.float32(0.96)).astype(np.float32)
        rate.reshape(-1)[idx] = v
        assert dm.resolve(idx, v, np.array([130], dtype=np.int32)) == 128
        _equals_oracle(dm, rate, nxt, what="after the resumed resolve")
