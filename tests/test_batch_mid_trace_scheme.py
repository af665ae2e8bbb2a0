"""The path trace of the mid batch tier (floydwarshall_amd/csrc/fwx_mid.hip, HAS_LAST), restated in numpy and pinned
to a direct definition before any GPU time is spent.  The restatement extends tests/test_batch_mid_scheme.py's with
the three arrays of the trace, maintained exactly as the kernel maintains them:

  0. `last` is filled with -1 by the kernel itself before the first block (the caller initialises nothing).
  1. panel load of block [k0, k0 + bt): at_row[k][:] = last[k][:] and at_col[:][k] = last[:][k] for the block's
     pivots k, as `last` stands at BLOCK START -- the only time those cells are written "from nothing"; then every
     panel-phase win of pivot k0 + t on the W panel's row u > t overwrites at_row[k0 + u][j] = k0 + t, and on the C
     panel's row u overwrites at_col[i][k0 + u] = k0 + t.  When row u is frozen the cells hold `last` of the entry
     at the start of step k0 + u.  A cross entry (k0 + a, k0 + b) lives in both panels: its at_row follows the W
     panel (wins at t < a), its at_col the C panel (wins at t < b).
  2. sweep: a win keeps the LAST winning t of the block, last[i][j] = k0 + t.

The direct definition: the plain k-i-j loop with the reference's three skips, `last` recorded on every win, column k
and row k of it copied at the start of step k.  A walk over the three arrays (the recursion of
fwx_dev_exact_paths_batch) must give the lists of oracle.list_ropes.  CPU only."""
import numpy as np
import pytest

import oracle
from floydwarshall_amd import synth
from oracle import list_ropes

from helpers import assert_bits_equal
from hostile_inputs import hostile_matrix_mix

ORDERS = list(range(1, 14)) + [20]
WIDTHS = [2, 3, 4]
KINDS = ("d1", "d2", "t1", "t3")
UNWRITTEN = 0x5A5A5A5A


def direct(rate, nxt, hops):
    """The definition.  Solves in place; returns (last, at_col, at_row, U)."""
    n = rate.shape[0]
    last = np.full((n, n), -1, dtype=np.int32)
    at_col, at_row = last.copy(), last.copy()
    idx = np.arange(n)
    u = 0
    with np.errstate(all="ignore"):
        for k in range(n):
            at_col[:, k] = last[:, k]
            at_row[k, :] = last[k, :]
            col, row = rate[:, k].copy(), rate[k, :].copy()
            cn, rn = nxt[:, k].copy(), nxt[k, :].copy()
            ch, rh = hops[:, k].copy(), hops[k, :].copy()
            cand = col[:, None] * row[None, :]
            win = (rate < cand) & (idx[:, None] != idx[None, :]) & (idx[:, None] != k) & (idx[None, :] != k)
            rate[win] = cand[win]
            nxt[win] = np.where(cn[:, None] >= 0, cn[:, None], rn[None, :])[win]
            hops[win] = (ch[:, None] + rh[None, :])[win]
            last[win] = k
            u += int(win.sum())
    return last, at_col, at_row, u


def scheme(rate, nxt, hops, B, panel_wins=True, keep="last"):
    """The kernel's bookkeeping.  Solves in place; returns (last, at_col, at_row, U, cells of at_row / at_col that a
    panel win overwrote).  panel_wins=False and keep="first" are the two mutants the tests must tell apart."""
    n = rate.shape[0]
    last = np.full((n, n), UNWRITTEN, dtype=np.int32)
    at_col, at_row = last.copy(), last.copy()
    last[:, :] = -1                                  # 0. the kernel's own fill
    off_diag = ~np.eye(n, dtype=bool)
    u = overwritten = 0
    with np.errstate(all="ignore"):
        for k0 in range(0, n, B):
            bt = min(B, n - k0)
            ks = np.arange(k0, k0 + bt)
            # ---- 1. panel: load
            W, C = rate[ks, :].copy(), rate[:, ks].T.copy()
            WN, CN = nxt[ks, :].copy(), nxt[:, ks].T.copy()
            WH, CH = hops[ks, :].copy(), hops[:, ks].T.copy()
            assert (at_row[ks, :] == UNWRITTEN).all() and (at_col[:, ks] == UNWRITTEN).all()    # written once
            at_row[ks, :] = last[ks, :]
            at_col[:, ks] = last[:, ks]
            for t in range(bt):
                W[t, k0 + t] = np.nan
                C[t, k0 + t] = np.nan
            # ---- 1. panel: pivots on the rows not yet frozen
            for t in range(bt):
                for v in range(t + 1, bt):
                    kv = k0 + v
                    cand = C[t, kv] * W[t, :]
                    win = W[v, :] < cand
                    W[v, win] = cand[win]
                    WN[v, win] = CN[t, kv] if CN[t, kv] >= 0 else WN[t, win]
                    WH[v, win] = CH[t, kv] + WH[t, win]
                    if panel_wins:
                        at_row[kv, win] = k0 + t
                        overwritten += int(win.sum())
                    cand = C[t, :] * W[t, kv]
                    win = C[v, :] < cand
                    C[v, win] = cand[win]
                    CN[v, win] = np.where(CN[t, win] >= 0, CN[t, win], WN[t, kv])
                    CH[v, win] = CH[t, win] + WH[t, kv]
                    if panel_wins:
                        at_col[win, kv] = k0 + t
                        overwritten += int(win.sum())
            # ---- 2. sweep: the fold keeps x, one t and a count
            x = rate.copy()
            tb = np.full((n, n), -1, dtype=np.int32)
            for t in range(bt):
                cand = C[t][:, None] * W[t][None, :]
                win = (x < cand) & off_diag
                x[win] = cand[win]
                if keep == "last":
                    tb[win] = t
                else:
                    tb[win & (tb < 0)] = t
                u += int(win.sum())
            won = tb >= 0
            tw = np.where(won, tb, 0)
            rate[won] = x[won]
            head = np.take_along_axis(CN.T, tw, axis=1)              # CN[tb][i]
            nxt[won] = np.where(head >= 0, head, np.take_along_axis(WN, tw, axis=0))[won]
            hops[won] = (np.take_along_axis(CH.T, tw, axis=1) + np.take_along_axis(WH, tw, axis=0))[won]
            last[won] = (k0 + tb)[won]
    return last, at_col, at_row, u, overwritten


def walk(last, at_col, at_row, next0, src, dst):
    """The recursion of the device walk: (a, b, kind) with kind 0 = final, 1 = as pivot column, 2 = as pivot row."""
    tabs = (last, at_col, at_row)
    out, stack = [], [(src, dst, 0)]
    while stack:
        a, b, kind = stack.pop()
        q = int(tabs[kind][a, b])
        if q < 0:
            if next0[a, b] >= 0:
                out.append(b)
        else:
            assert len(stack) + 2 <= last.shape[0] + 2           # exact_stack_triples
            stack.append((q, b, 2))
            stack.append((a, q, 1))
    return tuple(out)


def _inputs(n, dtype):
    for s, kind in enumerate(KINDS):
        yield kind, synth.make(kind, n, dtype, seed=synth.BASE_SEED + 4000 + s)
    rnd = np.random.default_rng(7700 + n)
    for d in range(4):
        r, x, h, heavy = hostile_matrix_mix(rnd, n, dtype)
        yield "hostile%d" % d, (r, x, h)


def _both(r0, x0, h0, B, **mutant):
    want = r0.copy(), x0.copy(), h0.copy()
    d = direct(*want)
    got = r0.copy(), x0.copy(), h0.copy()
    s = scheme(*got, B, **mutant)
    return want, d, got, s


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("B", WIDTHS)
def test_scheme_equals_the_definition(B, dtype):
    """Orders 1..13 and 20, ordinary and hostile inputs: the three arrays cell for cell, diagonals included; the
    solution is the oracle's.  Precondition of the group: panel wins overwrote block-start values, and some at_row /
    at_col cell differs from `last` as it stood at the start of its block."""
    overwritten = moved = 0
    for n in ORDERS:
        for name, (r0, x0, h0) in _inputs(n, dtype):
            what = "%s n=%d B=%d" % (name, n, B)
            want, d, got, s = _both(r0, x0, h0, B)
            er, ex, eh = r0.copy(), x0.copy(), h0.copy()
            eu = oracle.relax(er, ex, eh)
            for a, b, e, field in zip(got, want, (er, ex, eh), ("rate", "next", "hops")):
                assert_bits_equal(b, e, "%s definition %s" % (what, field))
                assert_bits_equal(a, e, "%s scheme %s" % (what, field))
            assert d[3] == eu and s[3] == eu, what
            for a, b, field in zip(s[:3], d[:3], ("last", "at_col", "at_row")):
                assert (a != UNWRITTEN).all(), "%s: a cell of %s was never written" % (what, field)
                assert np.array_equal(a, b), "%s %s" % (what, field)
            assert (np.diagonal(s[0]) == -1).all() and (np.diagonal(s[1]) == -1).all() and (np.diagonal(s[2]) == -1).all()
            overwritten += s[4]
            blind = scheme(r0.copy(), x0.copy(), h0.copy(), B, panel_wins=False)     # block-start `last` as exported
            moved += int((blind[1] != s[1]).sum() + (blind[2] != s[2]).sum())
    assert overwritten > 0 and moved > 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("B", WIDTHS)
@pytest.mark.parametrize("mutant", [{"panel_wins": False}, {"keep": "first"}], ids=["no-panel-wins", "first-win"])
def test_the_inputs_tell_the_mutants_apart(mutant, B, dtype):
    """at_row / at_col exported as block-start `last`, and the sweep keeping the first winning t: each is caught by
    the arrays and by the lists."""
    arrays = lists = 0
    for n in (5, 9, 13, 20):
        for name, (r0, x0, h0) in _inputs(n, dtype):
            _, d, _, s = _both(r0, x0, h0, B, **mutant)
            arrays += any(not np.array_equal(a, b) for a, b in zip(s[:3], d[:3]))
            if n <= 9:
                lists += any(walk(*s[:3], x0, i, j) != walk(*d[:3], x0, i, j) for i in range(n) for j in range(n))
    assert arrays > 0 and lists > 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("B", WIDTHS)
def test_a_walk_over_the_scheme_s_arrays_gives_the_ropes_lists(B, dtype):
    differ = 0
    for n in ORDERS:
        for name, (r0, x0, h0) in _inputs(n, dtype):
            if name == "t3" and n > 9:
                continue                                   # arbitrage: lists double per pivot
            ropes = list_ropes.solve(np.ascontiguousarray(r0), np.ascontiguousarray(x0))
            got = r0.copy(), x0.copy(), h0.copy()
            s = scheme(*got, B)
            assert_bits_equal(got[1], ropes.next, "%s n=%d next" % (name, n))
            for i in range(n):
                for j in range(n):
                    lst = walk(*s[:3], x0, i, j)
                    assert lst == ropes.path(i, j), "%s n=%d B=%d (%d, %d)" % (name, n, B, i, j)
                    hop = oracle.follow_path(got[1], i, j)
                    differ += hop is None or tuple(hop) != lst
    assert differ > 0            # some list is not the walk of the final next-hops
