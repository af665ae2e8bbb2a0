"""helpers.pass_reference -- the one-pass reference of tests/test_gpu_step_api.py -- pinned to the oracle's own
pivot ranges on the CPU: the state it ends in, U, and what its panels and its trace must be by definition."""
import functools

import numpy as np
import pytest

import oracle
from floydwarshall_amd import synth

from helpers import assert_bits_equal, pass_reference
from hostile_inputs import hostile_matrix

ORDERS = (68, 132)
KINDS = ("d2", "t1", "t3", "hostile")


def _passes(n):
    return ((0, 64), (37, 64), (64, n))


@functools.lru_cache(maxsize=None)
def _input(kind, n, dtype_name):
    dtype = np.dtype(dtype_name).type
    if kind == "hostile":
        out = hostile_matrix(np.random.default_rng(700 + n), n, dtype)
    else:
        out = synth.make(kind, n, dtype, seed=700 + n)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("n", ORDERS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pass_reference_equals_the_oracle_range(dtype, kind, n):
    rate0, nxt0, hops0 = _input(kind, n, np.dtype(dtype).name)
    updated = traced = 0
    for k0, k1 in _passes(n):
        rate, nxt, hops = rate0.copy(), nxt0.copy(), hops0.copy()
        oracle.relax(rate, nxt, hops, 0, k0)                   # the state at time k0
        kept = rate.copy(), nxt.copy(), hops.copy()
        ref = pass_reference(rate, nxt, hops, k0, k1)
        for a, b in zip((rate, nxt, hops), kept):
            assert_bits_equal(a, b, "pass_reference changed its input")
        er, en, eh = (a.copy() for a in kept)
        eu = oracle.relax(er, en, eh, k0, k1)
        tag = "%s n=%d pass [%d, %d)" % (kind, n, k0, k1)
        assert_bits_equal(ref.rate, er, tag + " rate")
        assert_bits_equal(ref.next, en, tag + " next")
        assert_bits_equal(ref.hops, eh, tag + " hops")
        assert int(ref.u_rows.sum()) == eu, tag
        assert ref.u_rows.shape == (n,) and int(ref.mask.sum()) == eu
        assert [int(u) for u in ref.u_rows] == [int(ref.mask[:, i, :].sum()) for i in range(n)], tag + " U per row"
        assert not ref.mask[:, np.arange(n), np.arange(n)].any(), tag + " the diagonal is never updated"
        for t, k in enumerate(range(k0, k1)):                  # step k leaves row k and column k alone
            assert not ref.mask[t, k, :].any() and not ref.mask[t, :, k].any(), tag
        updated += eu
        # the panels: row k is not written by step k, so W[t] is also row k0 + t right after that step
        assert ref.W.shape == ref.WH.shape == ref.WN.shape == (k1 - k0, n)
        # rates only: same rates, same U
        ro = pass_reference(kept[0], None, None, k0, k1)
        assert_bits_equal(ro.rate, er, tag + " rates only")
        assert_bits_equal(ro.W, ref.W, tag + " rates-only panel")
        assert bool((ro.mask == ref.mask).all()) and ro.WH is None and ro.WN is None
        # the trace, from its definition: last = the newest step whose mask holds the entry
        steps = np.arange(k0, k1, dtype=np.int32)[:, None, None]
        want_last = np.where(ref.mask, steps, -1).max(axis=0).astype(np.int32)
        assert_bits_equal(ref.last, want_last, tag + " last")
        for t, k in enumerate(range(k0, k1)):
            upto = np.where(ref.mask[:t], steps[:t], -1).max(axis=0, initial=-1).astype(np.int32)
            upto = np.broadcast_to(upto, (n, n))
            assert_bits_equal(ref.at_col[:, k], np.ascontiguousarray(upto[:, k]), tag + " at_col")
            assert_bits_equal(ref.at_row[k], np.ascontiguousarray(upto[k]), tag + " at_row")
        outside = np.ones(n, dtype=bool)
        outside[k0:k1] = False
        assert bool((ref.at_col[:, outside] == -1).all()) and bool((ref.at_row[outside] == -1).all())
        traced += int((ref.at_col >= 0).sum()) + int((ref.at_row >= 0).sum())
    assert updated > 0, "no pass of this input updates anything"
    assert traced > 0 or kind == "t1", "at_col / at_row never differ from -1: the start-of-step rule is not exercised"


def test_snapshot_rows_are_taken_at_their_own_time():
    """W[t] is row k0 + t AFTER the pivots before it and BEFORE its own step, which leaves it alone: it differs from
    the row at time k0 for some t, and equals the row at time k0 + t + 1."""
    n, k0, k1 = 68, 5, 40
    rate, nxt, hops = (a.copy() for a in _input("d2", n, "float64"))
    oracle.relax(rate, nxt, hops, 0, k0)
    ref = pass_reference(rate, nxt, hops, k0, k1)
    assert any(not np.array_equal(ref.W[t], rate[k0 + t]) for t in range(k1 - k0))
    r, nx, hp = rate.copy(), nxt.copy(), hops.copy()
    for t, k in enumerate(range(k0, k1)):
        oracle.relax(r, nx, hp, k, k + 1)
        assert_bits_equal(ref.W[t], r[k], "W[%d]" % t)
        assert_bits_equal(ref.WN[t], nx[k], "WN[%d]" % t)
        assert_bits_equal(ref.WH[t], hp[k], "WH[%d]" % t)
