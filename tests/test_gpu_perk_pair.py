"""The pair schedule of the per-k engine (round 29, FWX_PERK_PAIR_MIN_N): a call that takes the tile sweep, starts on a
multiple of 64 and has at least four full blocks from its first pivot that is a multiple of 128 applies those blocks two
at a time -- ONE 128-pivot relax_tile launch per pair on every tile but the tile row and tile column of the next pair,
while a chain on a look-ahead stream takes that cross through the pair, makes the panels of the next pair's first block
from it, applies that block to it and makes the panels of the second.  The next main launch then folds that first block
into the cross a second time, which must move nothing.  It must end at the bits of the sequential fold for every input.

Every case sets FWX_PERK_PAIR_MIN_N=128 and FWX_PERK_TILE_MIN_N=64 itself (nothing depends on the shipped defaults),
compares the rates bit for bit with the C oracle and reads all five hooks: a 128-pivot launch counts as sixteen 8-pivot
groups in fwx_test_perk_pivots, as eight in fwx_test_perk_wide, as four in fwx_test_perk_deep, as two in
fwx_test_perk_tile and as one in fwx_test_perk_pair; the cross launches count nowhere.

Orders.  512: 4 x 4 whole tiles, four pairs, crosses at tile 1, 2 and 3.  520: an 8-wide ragged edge beside them.
576: nine blocks -- the odd last block, whose cross is the half tile row and column.  644: ten blocks and four ragged
pivots, n % 128 = 4.
"""
import ctypes

import numpy as np
import pytest

from floydwarshall_amd import _lib, engine, hip, synth

from helpers import assert_bits_equal, dev, host, perk_expected_launches, perk_launches, perk_oracle
from test_gpu_perk_deep import _deep, _expected_deep
from test_gpu_perk_tile import _expected_tile, _tile
from test_gpu_perk_wide import _expected_wide, _matrix, _reset, _want, _wide

pytestmark = pytest.mark.gpu

F32 = np.float32
KNOBS = ("FWX_PERK_PIVOTS", "FWX_PERK_WIDE", "FWX_PERK_WALK", "FWX_PERK_DEEP", "FWX_PERK_FOLD", "FWX_PERK_STORE_BYTES",
         "FWX_PERK_TEMPORAL_MIB", "FWX_PERK_TILE_MIN_N", "FWX_PERK_PAIR_MIN_N")
ORDERS = [512, 520, 576, 644]


def _pair(reset=True):
    """(what FWX_PERK_PAIR_MIN_N parses to, 128-pivot main launches since the last reset)."""
    c = ctypes.c_uint64(0)
    min_n = _lib.lib().fwx_test_perk_pair(ctypes.byref(c), 1 if reset else 0)
    return min_n, int(c.value)


def _expected_pair(kb, ke):
    """128-pivot main launches of the schedule over pivots [kb, ke)."""
    if kb % 64:
        return 0
    ka = (kb + 127) // 128 * 128
    return (ke - ka) // 64 // 2 if ke - ka >= 256 else 0


def _ranges(n):
    """(0, n) and (64, n): whole solves, the second behind a single leading block.  (128, 384): exactly four blocks.
    (0, 192): three blocks, and (4, 324): an unaligned start -- neither takes the pair schedule."""
    return [(0, n), (64, n), (128, 384), (0, 192), (4, 324)]


def _defaults(monkeypatch, pair="128", tile="64"):
    for v in KNOBS:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("FWX_PERK_TILE_MIN_N", tile)
    monkeypatch.setenv("FWX_PERK_PAIR_MIN_N", pair)


def _reset_all():
    _reset()
    _deep()
    _tile()
    _pair()


def _hooks():
    """The five hooks since the last reset: (the five launch counters, wide, deep, tile, pair)."""
    return perk_launches(), _wide()[1], _deep()[1], _tile()[1], _pair()[1]


def _expected_hooks(kb, ke, pair_on=True, times=1):
    return ([times * v for v in perk_expected_launches(kb, ke, 8)], times * _expected_wide(kb, ke),
            times * _expected_deep(kb, ke), times * _expected_tile(kb, ke),
            times * _expected_pair(kb, ke) if pair_on else 0)


def _run_pair(rate, kb, ke, stream=None, sync=None):
    """(rates, the five hooks) of one uncounted fwx_dev_relax."""
    n = rate.shape[0]
    _reset_all()
    r_t = dev(rate)
    engine.dev_relax(r_t, n, 0, kb, ke, stream=stream)
    if sync:
        sync()
    return host(r_t), _hooks()


def _check(rate, kb, ke, want, tag, pair_on=True):
    got, hooks = _run_pair(rate, kb, ke)
    what = "%s pivots [%d, %d)" % (tag, kb, ke)
    assert_bits_equal(got, want[0], what)
    assert hooks == _expected_hooks(kb, ke, pair_on), what
    return got


def test_the_orders_and_ranges_cover_the_schedule():
    assert [(n + 127) // 128 for n in ORDERS] == [4, 5, 5, 6] and all(n % 4 == 0 for n in ORDERS)
    assert [n // 64 for n in ORDERS] == [8, 8, 9, 10] and [n % 64 for n in ORDERS] == [0, 8, 0, 4]
    assert 576 % 128 == 64 and 644 % 128 == 4
    assert [_expected_pair(0, n) for n in ORDERS] == [4, 4, 4, 5]
    assert [_expected_pair(64, n) for n in ORDERS] == [3, 3, 3, 4]          # one leading block, then pairs from 128
    assert _expected_pair(128, 384) == 2 and _expected_pair(0, 192) == 0 and _expected_pair(4, 324) == 0
    assert _expected_pair(64, 384) == 2 and _expected_pair(64, 383) == 0    # four full blocks from 128, or not
    assert _expected_tile(0, 576) == 9 and _expected_tile(64, 644) == 9     # the odd last block is one tile launch more
    assert perk_expected_launches(0, 644, 8) == [0, 0, 1, 80, 11]           # ten blocks, then 4 ragged pivots


# ---- every order, every range, every kind of input ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hostile", "d1", "d1_diag"])
@pytest.mark.parametrize("n", ORDERS)
def test_uncounted_relax_orders(n, kind, monkeypatch):
    _defaults(monkeypatch)
    assert _pair(reset=False)[0] == 128 and _tile(reset=False)[0] == 64
    rate = _matrix(kind, n)
    for kb, ke in _ranges(n):
        want = _want((kind, n), rate, kb, ke)
        if (kb, ke) == (0, n):
            assert_bits_equal(np.diagonal(want[0]).copy(), np.diagonal(rate).copy(), "oracle: the diagonal")
        _check(rate, kb, ke, want, "%s n=%d" % (kind, n))


@pytest.mark.parametrize("kind", ["hostile", "d1", "d1_diag"])
@pytest.mark.parametrize("n", ORDERS)
def test_compare_fold(n, kind, monkeypatch):
    """FWX_PERK_FOLD=compare: every tile folds in the compare form from its first stage, the second application of a
    block on the cross included."""
    _defaults(monkeypatch)
    monkeypatch.setenv("FWX_PERK_FOLD", "compare")
    rate = _matrix(kind, n)
    for kb, ke in ((0, n), (64, n)):
        _check(rate, kb, ke, _want((kind, n), rate, kb, ke), "%s n=%d compare" % (kind, n))


# ---- the only sign-set operand sits in the second block of a pair ----------------------------------------------------
SB_N, SB_K, SB_COL = 512, 128 + 64 + 37, 450


def _second_block_case():
    """D1 (every entry positive) with one -0.0: the W operand of pivot SB_K = 229 -- stage 6 of the pair [128, 256), in
    its second block -- at column SB_COL.  Row SB_K is NaN left of its diagonal, so no earlier pivot moves it (its Ct
    operands are NaN) and the -0.0 is still there at its time: the tiles of column tile 3 whose entries are clean fold
    six stages in the max form and the rest of the pair in the compare form."""
    rate = synth.make("d1", SB_N, F32, seed=SB_N + 37)[0]
    rate[SB_K, :SB_K] = F32(np.nan)
    rate[SB_K, SB_COL] = F32(-0.0)
    return rate


def test_sign_set_operand_in_the_second_block(monkeypatch):
    _defaults(monkeypatch)
    rate = _second_block_case()
    kb, ke = 0, 256
    want = _want(("pair second block",), rate, kb, ke)
    # the case itself, replayed on the oracle pivot by pivot: at its own time no pivot's row or column carries a sign bit
    # (r[k][k] apart, which the NaN patch hides) except the planted zero
    state, found = rate.copy(), set()
    for k in range(kb, ke):
        for side, line in (("row", state[k, :]), ("col", state[:, k])):
            for at in np.flatnonzero(np.signbit(line)):
                if at != k:
                    found.add((k, side, int(at)))
        state = perk_oracle(state, k, k + 1)[0]
    assert found == {(SB_K, "row", SB_COL)}, found
    assert_bits_equal(state, want[0], "the replay")
    for fold in (None, "compare"):
        if fold:
            monkeypatch.setenv("FWX_PERK_FOLD", fold)
        _check(rate, kb, ke, want, "second block fold=%s" % fold)
    monkeypatch.delenv("FWX_PERK_FOLD")
    _check(rate, 0, SB_N, _want(("pair second block",), rate, 0, SB_N), "second block, whole solve")


# ---- the switches ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hostile", "d1"])
@pytest.mark.parametrize("n", [576, 644])
def test_pair_off_is_the_same_solve(n, kind, monkeypatch):
    """FWX_PERK_PAIR_MIN_N=0, an order below the threshold and every older switch at `off` give the serial schedule:
    the same bits, the four older hooks the same, no 128-pivot launch."""
    _defaults(monkeypatch)
    rate = _matrix(kind, n)
    want = _want((kind, n), rate, 0, n)
    on = _check(rate, 0, n, want, "pair on")
    for min_n, parsed in (("0", 0), (str(n + 1), n + 1)):
        monkeypatch.setenv("FWX_PERK_PAIR_MIN_N", min_n)
        assert _pair(reset=False)[0] == parsed
        off = _check(rate, 0, n, want, "pair min n " + min_n, pair_on=False)
        assert_bits_equal(on, off, "on against off")
    monkeypatch.setenv("FWX_PERK_PAIR_MIN_N", str(n))
    _check(rate, 0, n, want, "pair min n = n")
    monkeypatch.setenv("FWX_PERK_PAIR_MIN_N", "128")
    monkeypatch.setenv("FWX_PERK_TILE_MIN_N", "0")
    got, hooks = _run_pair(rate, 0, n)
    assert_bits_equal(got, want[0], "tile off")
    assert hooks[3:] == (0, 0) and hooks[:3] == _expected_hooks(0, n)[:3]
    monkeypatch.setenv("FWX_PERK_TILE_MIN_N", "64")
    for var in ("FWX_PERK_DEEP", "FWX_PERK_WALK", "FWX_PERK_WIDE"):
        monkeypatch.setenv(var, "0")
        got, hooks = _run_pair(rate, 0, n)
        assert_bits_equal(got, want[0], var + "=0")
        assert hooks[2:] == (0, 0, 0) and hooks[0] == perk_expected_launches(0, n, 8), var
        monkeypatch.delenv(var)


def test_a_counted_call_and_f64_keep_their_schedule(monkeypatch):
    _defaults(monkeypatch)
    n = 512
    rate = _matrix("d1", n)
    want = _want(("d1", n), rate, 0, n)
    _reset_all()
    r_t = dev(rate)
    upd = hip.DeviceArray((engine.FWX_UPDATE_SHARDS,), np.int64).zero_(hip.default_stream())
    engine.dev_relax(r_t, n, 0, 0, n, updates_t=upd)
    assert_bits_equal(host(r_t), want[0], "counted")
    assert int(host(upd).sum()) == want[1]
    assert _hooks() == (perk_expected_launches(0, n, 8), 0, 0, 0, 0)
    rate64 = rate.astype(np.float64)
    _reset_all()
    r_t = dev(rate64)
    engine.dev_relax(r_t, n, 0, 0, n)
    assert_bits_equal(host(r_t), perk_oracle(rate64, 0, n)[0], "f64")
    assert _hooks() == (perk_expected_launches(0, n, 8), 0, 0, 0, 0)


# ---- streams -----------------------------------------------------------------------------------------------------------
def test_two_streams_at_once(monkeypatch):
    """Two different matrices, each on a stream of its own, the calls interleaved without any synchronisation in
    between: the panels, the look-ahead stream and the events of a call are its stream's own."""
    _defaults(monkeypatch)
    n = 644
    a = synth.make("d1", n, F32, seed=1)[0]
    b = synth.make("t2", n, F32, seed=2)[0]
    want_a, want_b = _want(("pair streams a",), a, 0, n)[0], _want(("pair streams b",), b, 0, n)[0]
    slices = [(0, 256), (256, 320), (320, n)]      # pairs; one block; a leading block, pairs from 384, four pivots
    assert [_expected_pair(lo, hi) for lo, hi in slices] == [2, 0, 2]
    sa, sb = hip.Stream(), hip.Stream()
    hip.default_stream().synchronize()
    a_t, b_t = dev(a), dev(b)
    hip.default_stream().synchronize()
    _reset_all()
    for lo, hi in slices:
        engine.dev_relax(a_t, n, 0, lo, hi, stream=sa)
        engine.dev_relax(b_t, n, 0, lo, hi, stream=sb)
    sa.synchronize()
    sb.synchronize()
    assert_bits_equal(host(a_t), want_a, "stream a")
    assert_bits_equal(host(b_t), want_b, "stream b")
    want_h = [_expected_hooks(lo, hi, times=2) for lo, hi in slices]
    assert _hooks() == ([sum(h[0][i] for h in want_h) for i in range(5)],) + tuple(
        sum(h[j] for h in want_h) for j in range(1, 5))


def test_the_null_stream(monkeypatch):
    """The caller's stream is the legacy null stream: the look-ahead stream is non-blocking, so only the events order
    the two."""
    _defaults(monkeypatch)
    for n in (512, 644):
        rate = _matrix("d1", n)
        want = _want(("d1", n), rate, 0, n)
        got, hooks = _run_pair(rate, 0, n, stream=ctypes.c_void_p(0), sync=hip.synchronize)
        assert_bits_equal(got, want[0], "null stream n=%d" % n)
        assert hooks == _expected_hooks(0, n)


def test_back_to_back_calls_regrow_the_buffer(monkeypatch):
    """Two calls on one stream with nothing between them, the second at a larger order: its panel sets do not fit the
    stream's buffer, which is released only behind the first call's launches, the look-ahead stream's included."""
    _defaults(monkeypatch)
    s = hip.Stream()
    n1, n2 = 512, 644
    r1, r2 = _matrix("d1", n1), _matrix("hostile", n2)
    want1, want2 = _want(("d1", n1), r1, 0, n1)[0], _want(("hostile", n2), r2, 0, n2)[0]
    hip.default_stream().synchronize()
    t1, t2 = dev(r1), dev(r2)
    hip.default_stream().synchronize()
    _reset_all()
    engine.dev_relax(t1, n1, 0, 0, n1, stream=s)
    engine.dev_relax(t2, n2, 0, 0, n2, stream=s)
    s.synchronize()
    assert_bits_equal(host(t1), want1, "the first call")
    assert_bits_equal(host(t2), want2, "the second call")
    h1, h2 = _expected_hooks(0, n1), _expected_hooks(0, n2)
    assert _hooks() == ([x + y for x, y in zip(h1[0], h2[0])],) + tuple(h1[j] + h2[j] for j in range(1, 5))


def test_a_capturing_stream_keeps_the_serial_schedule(monkeypatch):
    """A captured graph gets no parallel branches: under capture the call issues the serial schedule, launch for launch.
    Capture only -- ended and destroyed, never replayed; the stream's buffer exists before the capture begins."""
    _defaults(monkeypatch)
    n = 512
    rate = _matrix("d1", n)
    want = _want(("d1", n), rate, 0, n)
    s = hip.Stream()
    hip.default_stream().synchronize()
    r_t = dev(rate)
    hip.default_stream().synchronize()
    _reset_all()
    engine.dev_relax(r_t, n, 0, 0, n, stream=s)              # not capturing: the pair schedule, and the buffer
    s.synchronize()
    assert_bits_equal(host(r_t), want[0], "before the capture")
    assert _hooks() == _expected_hooks(0, n)
    h = hip.rt()
    vp = ctypes.c_void_p
    h.hipStreamBeginCapture.restype = h.hipStreamEndCapture.restype = h.hipGraphDestroy.restype = ctypes.c_int
    h.hipStreamBeginCapture.argtypes = [vp, ctypes.c_int]
    h.hipStreamEndCapture.argtypes = [vp, ctypes.POINTER(vp)]
    h.hipGraphDestroy.argtypes = [vp]
    graph = vp()
    assert h.hipStreamBeginCapture(s.ptr, 2) == 0            # hipStreamCaptureModeRelaxed
    try:
        engine.dev_relax(r_t, n, 0, 0, n, stream=s)
    finally:
        rc = h.hipStreamEndCapture(s.ptr, ctypes.byref(graph))
    assert rc == 0 and graph.value
    assert h.hipGraphDestroy(graph) == 0
    assert _hooks() == _expected_hooks(0, n, pair_on=False)
    s.synchronize()
    assert_bits_equal(host(r_t), want[0], "the capture ran nothing")
