"""The per-k engine's multi-pivot schedule (relax_kt from the snapshots of one fused_panels launch per 64-pivot
block) at the shapes and states tests/test_gpu_perk_pivots.py does not reach.  Everything is compared bit for bit
with the C oracle, U too wherever the call counts, and the launch counters of the test hook with
helpers.perk_expected_launches:

  1. f64 orders n = 2 (mod 4): multiples of 16 bytes but not of 4 elements, the only case in which the column
     panel's leading dimension ct_ld = (n + 3) & ~3 is not n;
  2. small orders through fwx_dev_relax (which never routes to small_solve): n from 2 (f64) / 4 up, around 64 and
     128 where a second block of 2 or 4 pivots begins, blocks shorter than FWX_PERK_PIVOTS, one ragged row tile of
     the panel launch, r_cnt < RPB in every workgroup;
  3. padded rates-only handles (device pitch nd > n) through fwx_matrix_solve: the fold runs over the pad row and
     column, the rates and U are those of the unpadded matrix;
  4. the scratch pool: eviction past its 16 buffers with launches queued, growth and shrink on one stream, the null
     stream, two host threads, and that no call depends on what an earlier one left in the scratch;
  5. the calls that must NOT take the multi-pivot schedule, each beside a positive control.
"""
import threading

import numpy as np
import pytest

import oracle
from floydwarshall_amd import engine, hip, synth

from helpers import (MIB, PERK_PIVOTS, assert_bits_equal, dev, dev_empty, dev_sync, dev_zeros, host, perk_check,
                     perk_expected_launches, perk_launches, perk_oracle, perk_relax)
from hostile_inputs import hostile_matrix, hostile_matrix_mix

pytestmark = pytest.mark.gpu

STORE_BYTES = ["16", "32", "64", "128"]
_ORACLE = {}     # (what, n, dtype, kb, ke) -> the oracle's (rates, U): computed once, shared, never modified


def _input(kind, n, dtype, seed):
    """d1 / d2 / t1 / t2 from synth, `hostile` from a generator seeded with `seed`."""
    if kind == "hostile":
        return hostile_matrix(np.random.default_rng(seed), n, dtype)[0]
    return synth.make(kind, n, dtype, seed=seed)[0]


def _want(key, rate, kb, ke):
    k = key + (kb, ke)
    if k not in _ORACLE:
        _ORACLE[k] = perk_oracle(rate, kb, ke)
    return _ORACLE[k]


def _sum(lists):
    return [sum(v) for v in zip(*lists)]


# ---- 1. multiples of 16 bytes that are no multiples of 4 elements ---------------------------------------------------
def _check_16_byte_order(n, kind, monkeypatch):
    """Pivots [5, 160): three blocks from an odd start, the last one 27 = 8 + 8 + 8 + 2 + 1 pivots, so that groups
    start at every t (mod 8) of a block and the group's panel rows are ct + t * ct_ld with ct_ld = n + 2; and the
    last 77 pivots of the matrix."""
    rate = _input(kind, n, np.float64, n + 11)
    for kb, ke in ((5, 160), (n - 77, n)):
        perk_check(rate, kb, ke, monkeypatch, "%s n=%d" % (kind, n), want=_want((kind, n), rate, kb, ke))


@pytest.mark.parametrize("kind", ["d1", "hostile"])
@pytest.mark.parametrize("n", [262, 326, 454])
def test_f64_orders_2_mod_4(n, kind, monkeypatch):
    monkeypatch.delenv("FWX_PERK_STORE_BYTES", raising=False)
    _check_16_byte_order(n, kind, monkeypatch)


@pytest.mark.parametrize("kind", ["d1", "hostile"])
@pytest.mark.parametrize("store", STORE_BYTES)
def test_f64_order_1038_every_store_width(store, kind, monkeypatch):
    """n = 1038: three column strips, the last with 7 vectors and 249 clamped lanes."""
    monkeypatch.setenv("FWX_PERK_STORE_BYTES", store)
    _check_16_byte_order(1038, kind, monkeypatch)


# ---- 2. small orders ------------------------------------------------------------------------------------------------
SMALL_F32 = [4, 8, 12, 60, 64, 68, 124, 128, 132, 196]
SMALL_F64 = sorted(SMALL_F32 + [2, 6, 10, 62, 66, 130])
SMALL = [(n, np.float32) for n in SMALL_F32] + [(n, np.float64) for n in SMALL_F64]


def _small_ranges(n):
    r = [(0, n)]
    if n >= 12:
        r += [(1, n), (n // 2 - 1, n // 2 + 2)]
    return r


def _small_hostile(n, dtype):
    """Hostile draws of order n from one seeded generator: at least two, and on until both of hostile_matrix's
    mixes (mostly ordinary rates / every awkward value equally likely) have come up.  No draw is left out."""
    rnd = np.random.default_rng(7000 + n)
    out, seen = [], set()
    while len(out) < 2 or len(seen) < 2:
        assert len(out) < 24, "the seeded draws of order %d never produced both mixes" % n
        rate, _, _, heavy = hostile_matrix_mix(rnd, n, dtype)
        out.append(rate)
        seen.add(heavy)
    return out, seen


@pytest.mark.parametrize("n,dtype", SMALL)
def test_small_orders_through_dev_relax(n, dtype, monkeypatch):
    """Blocks of bt = n < 64 pivots (one ragged row tile in the panel launch), bt < FWX_PERK_PIVOTS, a second block
    of 2 or 4 pivots just past 64 and 128, r_cnt < RPB and nstrips = 1 with almost every lane clamped.  t1: exact
    ties everywhere, the earliest pivot must win."""
    hostile, seen = _small_hostile(n, dtype)
    assert seen == {False, True}                 # both mixes, at every order of either dtype
    inputs = [("d1", _input("d1", n, dtype, n + 1)), ("t1", _input("t1", n, dtype, n + 2))]
    inputs += [("hostile draw %d" % i, r) for i, r in enumerate(hostile)]
    for what, rate in inputs:
        for kb, ke in _small_ranges(n):
            perk_check(rate, kb, ke, monkeypatch, "%s n=%d" % (what, n), budgets=[repr(rate.nbytes / 2 / MIB)])
            if n < 8:
                # FWX_PERK_PIVOTS = 8 on fewer than 8 pivots: the counters themselves show a 4- or 2-wide sweep, one
                # panel launch and nothing 8 wide
                monkeypatch.setenv("FWX_PERK_PIVOTS", "8")
                perk_launches()
                got_r, got_u = perk_relax(rate, kb, ke)
                got = perk_launches()
                want_r, want_u = perk_oracle(rate, kb, ke)
                assert_bits_equal(got_r, want_r, "%s n=%d NP=8" % (what, n))
                assert got_u == want_u, (what, n)
                assert got[3] == 0 and got[4] == 1 and got[1] + got[2] >= 1, (what, n, got)
                assert got == {2: [0, 1, 0, 0, 1], 4: [0, 0, 1, 0, 1], 6: [0, 1, 1, 0, 1]}[n]


# ---- 3. padded handles ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["d1", "t1", "hostile"])
@pytest.mark.parametrize("n,dtype,nd", [(261, np.float32, 264), (263, np.float32, 264), (261, np.float64, 262),
                                        (325, np.float64, 326)])
def test_padded_rates_only_handles(n, dtype, nd, kind, monkeypatch):
    """fwx_matrix_solve with the per-k engine on a rates-only handle whose pitch nd exceeds n: relax_range without a
    workspace (the pool), the fold running over the pad row and column too.  A whole solve, and one cut into
    slices that are no multiples of 64.  The counters are those of the schedule at the handle's pitch: nd is a
    multiple of the vector width whatever n is (at f64 also nd = 2 (mod 4): ct_ld != nd)."""
    w = 16 // np.dtype(dtype).itemsize
    assert nd == (n + w - 1) // w * w and nd % w == 0 and n % w != 0
    rate = _input(kind, n, dtype, 3 * n + 1)
    want_r, want_u = _want((kind, n, np.dtype(dtype).name, "whole"), rate, 0, n)
    cuts = [0, 37, 101, 102, 230, n]
    with engine.DeviceMatrix(n, dtype, with_next=False) as dm:
        for np_ in PERK_PIVOTS:
            monkeypatch.setenv("FWX_PERK_PIVOTS", str(np_))
            half = repr(nd * nd * rate.itemsize / 2 / MIB)
            for what, slices, budget in (("whole", [(0, n)], "1e12"),
                                         ("sliced", list(zip(cuts[:-1], cuts[1:])), half)):
                monkeypatch.setenv("FWX_PERK_TEMPORAL_MIB", budget)
                dm.upload(rate)
                perk_launches()
                u = sum(dm.solve(engine=engine.FWX_ENGINE_PERK, k_begin=lo, k_end=hi, count_updates=True)
                        for lo, hi in slices)
                tag = "%s n=%d nd=%d NP=%d %s" % (kind, n, nd, np_, what)
                assert_bits_equal(dm.download()[0], want_r, tag)
                assert u == want_u, tag
                want_l = _sum(perk_expected_launches(lo, hi, np_) for lo, hi in slices)
                assert perk_launches() == want_l, tag
                assert np_ == 1 or want_l[4] >= len(slices) - 1, tag       # (the one-pivot slice has no panel)


# ---- 4. the scratch pool --------------------------------------------------------------------------------------------
def _slices(cuts):
    return list(zip(cuts[:-1], cuts[1:]))


@pytest.mark.parametrize("np_", [2, 8])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pool_eviction_with_launches_queued(dtype, np_, monkeypatch):
    """20 streams on a pool of 16 buffers, each with its own matrix, the slices issued round-robin without any
    synchronisation: from the 17th stream on every first call of a round evicts the least recently used buffer,
    whose stream still has launches queued that read it (hipFree waits for them).  Five kinds of input, so that
    a panel taken from another stream's buffer, or a stale one, changes bits."""
    n, nstreams = 260, 20
    kinds = ["d1", "t1", "t2", "hostile", "d2"]
    rates = [_input(kinds[i % 5], n, dtype, 100 + i) for i in range(nstreams)]
    want = [_want(("evict", i, np.dtype(dtype).name), rates[i], 0, n) for i in range(nstreams)]
    monkeypatch.setenv("FWX_PERK_PIVOTS", str(np_))
    streams = [hip.Stream() for _ in range(nstreams)]
    try:
        mats = [dev(r) for r in rates]
        upds = [dev_zeros((engine.FWX_UPDATE_SHARDS,), np.int64) for _ in rates]
        dev_sync()
        perk_launches()
        sl = _slices([0, 37, 101, 165, 230, n])
        for lo, hi in sl:
            for i in range(nstreams):
                engine.dev_relax(mats[i], n, 0, lo, hi, updates_t=upds[i], stream=streams[i])
        for s in streams:
            s.synchronize()
        for i in range(nstreams):
            tag = "stream %d (%s) NP=%d" % (i, kinds[i % 5], np_)
            assert_bits_equal(host(mats[i]), want[i][0], tag)
            assert int(host(upds[i]).sum()) == want[i][1], tag
        assert perk_launches() == [nstreams * v for v in _sum(perk_expected_launches(lo, hi, np_) for lo, hi in sl)]
    finally:
        dev_sync()
        for s in streams:
            s.close()


@pytest.mark.parametrize("null_stream", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pool_growth_and_shrink_on_one_stream(dtype, null_stream, monkeypatch):
    """n = 260 in slices, then n = 1036 over pivots [0, 200) on another buffer (the stream's scratch is freed and
    allocated again while the first solve's launches may still be queued), then another n = 260 matrix in the
    grown scratch -- nothing synchronised in between.  Again on the null stream (raw handle 0)."""
    a, c = _input("d1", 260, dtype, 21), _input("t2", 260, dtype, 22)
    b = _input("d2", 1036, dtype, 23)
    name = np.dtype(dtype).name
    want_a, want_c = _want(("grow a", name), a, 0, 260), _want(("grow c", name), c, 0, 260)
    want_b = _want(("grow b", name), b, 0, 200)
    monkeypatch.setenv("FWX_PERK_PIVOTS", "8")
    own = None if null_stream else hip.Stream()
    s = 0 if null_stream else own
    try:
        a_t, b_t, c_t = dev(a), dev(b), dev(c)
        upds = [dev_zeros((engine.FWX_UPDATE_SHARDS,), np.int64) for _ in range(3)]
        dev_sync()
        perk_launches()
        sl = _slices([0, 37, 101, 230, 260])
        for lo, hi in sl:
            engine.dev_relax(a_t, 260, 0, lo, hi, updates_t=upds[0], stream=s)
        engine.dev_relax(b_t, 1036, 0, 0, 200, updates_t=upds[1], stream=s)
        for lo, hi in sl:
            engine.dev_relax(c_t, 260, 0, lo, hi, updates_t=upds[2], stream=s)
        dev_sync()
        for t, u, want, what in ((a_t, upds[0], want_a, "first 260"), (b_t, upds[1], want_b, "1036"),
                                 (c_t, upds[2], want_c, "second 260")):
            assert_bits_equal(host(t), want[0], what)
            assert int(host(u).sum()) == want[1], what
        small = _sum(perk_expected_launches(lo, hi, 8) for lo, hi in sl)
        assert perk_launches() == _sum([small, small, perk_expected_launches(0, 200, 8)])
    finally:
        dev_sync()
        if own is not None:
            own.close()


@pytest.mark.parametrize("np_", [2, 8])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pool_two_host_threads(dtype, np_, monkeypatch):
    """Two host threads, each with a new stream and its own matrix, released together by a barrier: their first
    calls may allocate under the pool mutex at the same time (a new stream can also find the buffer an earlier
    stream with the same handle left in the pool), and each issues its slices from its own thread."""
    n = 452
    rates = [_input("d1", n, dtype, 31), _input("t2", n, dtype, 32)]
    want = [_want(("threads", i, np.dtype(dtype).name), rates[i], 0, n) for i in range(2)]
    monkeypatch.setenv("FWX_PERK_PIVOTS", str(np_))
    barrier = threading.Barrier(2)
    got, errors = [None, None], []
    sl = _slices([0, 37, 101, 230, 231, 400, n])

    def work(i):
        s = None
        try:
            s = hip.Stream()
            r_t = dev(rates[i])
            upd = dev_empty((engine.FWX_UPDATE_SHARDS,), np.int64).zero_(s)
            s.synchronize()
            barrier.wait(30)
            for lo, hi in sl:
                engine.dev_relax(r_t, n, 0, lo, hi, updates_t=upd, stream=s)
            got[i] = (r_t.numpy(s), int(upd.numpy(s).sum()))
        except BaseException as e:           # noqa: B902 -- reported by the test below, never lost
            errors.append((i, repr(e)))
            barrier.abort()
        finally:
            if s is not None:
                s.close()

    perk_launches()
    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not any(t.is_alive() for t in threads), "a thread did not return"
    assert not errors, errors
    for i in range(2):
        assert_bits_equal(got[i][0], want[i][0], "thread %d NP=%d" % (i, np_))
        assert got[i][1] == want[i][1], i
    assert perk_launches() == [2 * v for v in _sum(perk_expected_launches(lo, hi, np_) for lo, hi in sl)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_scratch_is_not_state(dtype, monkeypatch):
    """A over [0, 100), then B of the same order over [0, n), then A over [100, n), all on one stream: the second
    call on A finds B's last panels in the scratch and must retake its own."""
    n = 324
    a, b = _input("d1", n, dtype, 41), _input("hostile", n, dtype, 42)
    (want_a, ua), (want_b, ub) = perk_oracle(a, 0, n), perk_oracle(b, 0, n)
    for np_ in (2, 4, 8):
        monkeypatch.setenv("FWX_PERK_PIVOTS", str(np_))
        s = hip.Stream()
        try:
            a_t, b_t = dev(a), dev(b)
            upa, upb = (dev_zeros((engine.FWX_UPDATE_SHARDS,), np.int64) for _ in range(2))
            dev_sync()
            engine.dev_relax(a_t, n, 0, 0, 100, updates_t=upa, stream=s)
            engine.dev_relax(b_t, n, 0, 0, n, updates_t=upb, stream=s)
            engine.dev_relax(a_t, n, 0, 100, n, updates_t=upa, stream=s)
            s.synchronize()
            assert_bits_equal(host(a_t), want_a, "A NP=%d" % np_)
            assert_bits_equal(host(b_t), want_b, "B NP=%d" % np_)
            assert (int(host(upa).sum()), int(host(upb).sum())) == (ua, ub), np_
        finally:
            dev_sync()
            s.close()


# ---- 5. calls that must not take the multi-pivot schedule -----------------------------------------------------------
ZERO = [0, 0, 0, 0, 0]
KB, KE = 70, 135          # 65 pivots across a block boundary; one 64-row panel covers [KB, KE - 1)


def _counted(call):
    """Runs call(updates) with FWX_PERK_PIVOTS = 8 set by the caller: (U, launch counters)."""
    upd = dev_zeros((engine.FWX_UPDATE_SHARDS,), np.int64)
    perk_launches()
    call(upd)
    return int(host(upd).sum()), perk_launches()


def _updates_in_rows(rate, kb, ke, lo, hi):
    """The oracle's updates in rows [lo, hi) over pivots [kb, ke) (strict improvements: an update changes bits)."""
    rate, u = rate.copy(), 0
    for k in range(kb, ke):
        before = rate[lo:hi].copy()
        oracle.relax(rate, None, None, k, k + 1)
        u += int(np.count_nonzero(rate[lo:hi] != before))
    return u


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_positive_control_takes_the_schedule(dtype, monkeypatch):
    """The call every case below restricts: n = 260, whole matrix in place, aligned, rates only, pivots [KB, KE)."""
    monkeypatch.setenv("FWX_PERK_PIVOTS", "8")
    n = 260
    rate = _input("d2", n, dtype, 51)
    want_r, want_u = _want(("control", np.dtype(dtype).name), rate, KB, KE)
    r_t = dev(rate)
    u, launches = _counted(lambda upd: engine.dev_relax(r_t, n, 0, KB, KE, updates_t=upd))
    assert_bits_equal(host(r_t), want_r, "control")
    assert u == want_u
    assert launches == perk_expected_launches(KB, KE, 8) == [1, 0, 0, 8, 1]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_order_that_is_no_multiple_of_16_bytes(dtype, monkeypatch):
    monkeypatch.setenv("FWX_PERK_PIVOTS", "8")
    n = 261
    rate = _input("d2", n, dtype, 52)
    want_r, want_u = perk_oracle(rate, KB, KE)
    r_t = dev(rate)
    u, launches = _counted(lambda upd: engine.dev_relax(r_t, n, 0, KB, KE, updates_t=upd))
    assert_bits_equal(host(r_t), want_r, "n=261")
    assert (u, launches) == (want_u, ZERO)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_misaligned_rate_pointer(dtype, monkeypatch):
    """The matrix one element into a larger allocation: 4 (f32) / 8 (f64) bytes off 16-byte alignment.  The same
    matrix at the start of the allocation is the control."""
    monkeypatch.setenv("FWX_PERK_PIVOTS", "8")
    n = 260
    rate = _input("d2", n, dtype, 51)
    want_r, want_u = _want(("control", np.dtype(dtype).name), rate, KB, KE)
    es = rate.itemsize
    buf = dev_empty((n * n + 16 // es,), dtype)
    for off, want_l in ((1, ZERO), (0, perk_expected_launches(KB, KE, 8))):
        view = hip.DeviceArray((n, n), dtype, _ptr=buf.data_ptr() + off * es, _base=buf)
        assert view.data_ptr() % 16 == off * es
        view.copy_from_host(rate)
        u, launches = _counted(lambda upd: engine.dev_relax(view, n, 0, KB, KE, updates_t=upd))
        assert_bits_equal(host(view), want_r, "offset %d" % off)
        assert (u, launches) == (want_u, want_l), off


@pytest.mark.parametrize("row0,rows", [(0, 200), (64, 136), (0, 260)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_row_slabs(dtype, row0, rows, monkeypatch):
    """A slab of rows [row0, row0 + rows) that holds the pivot rows itself, as a view into the whole matrix on the
    device: its rows equal the oracle's, U counts its rows only, the rows outside it keep their bits.  rows = n
    is the control."""
    monkeypatch.setenv("FWX_PERK_PIVOTS", "8")
    n = 260
    rate = _input("d2", n, dtype, 51)
    want_r = _want(("control", np.dtype(dtype).name), rate, KB, KE)[0]
    full_t = dev(rate)
    slab = full_t[row0:row0 + rows]
    u, launches = _counted(lambda upd: engine.dev_relax(slab, n, row0, KB, KE, updates_t=upd))
    got = host(full_t)
    inside = np.zeros(n, dtype=bool)
    inside[row0:row0 + rows] = True
    assert_bits_equal(got[inside], want_r[inside], "slab rows")
    assert_bits_equal(got[~inside], rate[~inside], "rows outside the slab")
    assert u == _updates_in_rows(rate, KB, KE, row0, row0 + rows)
    assert launches == (perk_expected_launches(KB, KE, 8) if rows == n else ZERO)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pivots_from_an_external_panel(dtype, monkeypatch):
    """The pivot rows come from a panel of time-k snapshots (fwx_dev_panel_snap), not from the matrix: what
    tests/test_gpu_perk_store_path.py expects of such a call, every row equal to the oracle's."""
    monkeypatch.setenv("FWX_PERK_PIVOTS", "8")
    n, ke = 260, KE - 1
    rate = _input("d2", n, dtype, 51)
    want_r, want_u = perk_oracle(rate, KB, ke)
    r_t = dev(rate)
    w = dev_empty((ke - KB, n), dtype)
    engine.dev_panel_snap(r_t[KB:ke], n, KB, w)
    u, launches = _counted(lambda upd: engine.dev_relax(r_t, n, 0, KB, ke, pivots_t=w, updates_t=upd))
    assert_bits_equal(host(r_t), want_r, "external panel")
    assert (u, launches) == (want_u, ZERO)
    r_t = dev(rate)
    u, launches = _counted(lambda upd: engine.dev_relax(r_t, n, 0, KB, ke, updates_t=upd))
    assert_bits_equal(host(r_t), want_r, "in place")
    assert (u, launches) == (want_u, perk_expected_launches(KB, ke, 8))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_skip_range(dtype, monkeypatch):
    """Rows [200, 232) are skipped (no pivot row among them): they keep their bits, every other row equals the
    oracle's -- what test_per_k_relax_with_a_skipped_row_range expects.  An empty range is no restriction."""
    monkeypatch.setenv("FWX_PERK_PIVOTS", "8")
    n, lo, hi = 260, 200, 232
    rate = _input("d2", n, dtype, 51)
    want_r = _want(("control", np.dtype(dtype).name), rate, KB, KE)[0]
    keep = np.ones(n, dtype=bool)
    keep[lo:hi] = False
    r_t = dev(rate)
    u, launches = _counted(lambda upd: engine.dev_relax(r_t, n, 0, KB, KE, updates_t=upd, skip=(lo, hi)))
    got = host(r_t)
    assert_bits_equal(got[keep], want_r[keep], "rows outside the skipped range")
    assert_bits_equal(got[~keep], rate[~keep], "skipped rows")
    assert u == _updates_in_rows(rate, KB, KE, 0, lo) + _updates_in_rows(rate, KB, KE, hi, n)
    assert launches == ZERO
    r_t = dev(rate)
    u, launches = _counted(lambda upd: engine.dev_relax(r_t, n, 0, KB, KE, updates_t=upd, skip=(lo, lo)))
    assert_bits_equal(host(r_t), want_r, "empty skip range")
    assert launches == perk_expected_launches(KB, KE, 8)


@pytest.mark.parametrize("with_hops", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_next_hops_and_hops_present(dtype, with_hops, monkeypatch):
    monkeypatch.setenv("FWX_PERK_PIVOTS", "8")
    n = 260
    rate, nxt, hops = synth.make("d2", n, dtype, seed=51)
    want_r, want_n, want_h = rate.copy(), nxt.copy(), hops.copy() if with_hops else None
    want_u = oracle.relax(want_r, want_n, want_h, KB, KE)
    r_t, n_t, h_t = dev(rate), dev(nxt), dev(hops) if with_hops else None
    u, launches = _counted(lambda upd: engine.dev_relax(r_t, n, 0, KB, KE, next_t=n_t, hops_t=h_t, updates_t=upd))
    assert_bits_equal(host(r_t), want_r, "rate")
    assert np.array_equal(host(n_t), want_n)
    if with_hops:
        assert np.array_equal(host(h_t), want_h)
    assert (u, launches) == (want_u, ZERO)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_single_pivot(dtype, monkeypatch):
    monkeypatch.setenv("FWX_PERK_PIVOTS", "8")
    n = 260
    rate = _input("d2", n, dtype, 51)
    want_r, want_u = perk_oracle(rate, KB, KB + 1)
    r_t = dev(rate)
    u, launches = _counted(lambda upd: engine.dev_relax(r_t, n, 0, KB, KB + 1, updates_t=upd))
    assert_bits_equal(host(r_t), want_r, "one pivot")
    assert (u, launches) == (want_u, ZERO)
    r_t = dev(rate)
    u, launches = _counted(lambda upd: engine.dev_relax(r_t, n, 0, KB, KB + 2, updates_t=upd))
    assert_bits_equal(host(r_t), perk_oracle(rate, KB, KB + 2)[0], "two pivots")
    assert launches == [0, 1, 0, 0, 1]
