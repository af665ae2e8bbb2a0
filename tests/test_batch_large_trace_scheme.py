"""The path trace of the large batch tier (floydwarshall_amd/csrc/fwx_large.hip, HAS_LAST), restated in numpy and
pinned to a direct definition before any GPU time is spent.  The restatement extends the strip scheme of
tests/test_batch_large_scheme.py with the three arrays of the trace, maintained exactly as the two launches maintain
them:

  0. `last` is filled with -1 by a launch of its own before the first block (the caller initialises nothing).
  1. panel, once per strip [s0, s0 + S): two more int32 panels AR / AC [bt][B + S] beside W / C, loaded with
     AR[t][p] = last[k0+t][index(p)] and AC[t][p] = last[index(p)][k0+t] -- `last` as it stands at BLOCK START.  A
     panel-phase win of pivot k0+t on W[u][c] sets AR[u][c] = k0+t, one on C[u][c] sets AC[u][c] = k0+t.  After the
     pivot loop ONLY the strip positions (p >= B, the positions the rate panels store) go to the caller's trace:
     at_row[k0+t][x] = AR[t][p], at_col[x][k0+t] = AC[t][p].  Every cell of at_row / at_col is therefore written by
     exactly one strip of exactly one block; the strips' copies of the cross cells (p < B) are dropped.
  2. sweep, per tile: a win keeps the LAST winning t of the block, last[i][j] = k0 + t.

Pinned to direct() of tests/test_batch_mid_trace_scheme.py (the k-i-j loop that records `last` on every win and copies
column k / row k of it at the start of step k) and to that file's mid scheme, cell for cell; a walk over the arrays
(the recursion of fwx_dev_exact_paths_batch) must give the lists of oracle.list_ropes.  CPU only."""
import numpy as np
import pytest

import oracle
from floydwarshall_amd import synth
from oracle import list_ropes

import test_batch_large_scheme as large
import test_batch_mid_trace_scheme as mid
from helpers import assert_bits_equal
from hostile_inputs import hostile_matrix_mix

ORDERS = list(range(1, 14)) + [20]
WIDTHS = [2, 3, 4]
STRIPS = [2, 3, 5]
TILES = {2: (2, 5), 3: (4, 4), 5: (5, 3)}          # (rows, columns) of a sweep tile, one shape per strip width
KINDS = mid.KINDS
UNWRITTEN = mid.UNWRITTEN


def _strip_trace(rate, nxt, hops, last, k0, bt, B, s0, S, panel_wins):
    """Phase 1 of ONE strip with the trace: the strip's columns of (W, WN, WH, C, CN, CH) and the whole AR / AC panels
    [bt][B + S], cross positions included.  Reads the matrix and `last` only."""
    n = rate.shape[0]
    index = [k0 + p if p < bt else -1 for p in range(B)] + [s0 + y if s0 + y < n else -1 for y in range(S)]
    P = B + S
    W, C = np.full((bt, P), np.nan, dtype=rate.dtype), np.full((bt, P), np.nan, dtype=rate.dtype)
    WN, CN = np.full((bt, P), -1, dtype=np.int32), np.full((bt, P), -1, dtype=np.int32)
    WH, CH = np.zeros((bt, P), dtype=np.int32), np.zeros((bt, P), dtype=np.int32)
    AR, AC = np.full((bt, P), -1, dtype=np.int32), np.full((bt, P), -1, dtype=np.int32)
    for t in range(bt):
        k = k0 + t
        for p, x in enumerate(index):
            if x < 0:
                continue
            if x != k:
                W[t, p], C[t, p] = rate[k, x], rate[x, k]
            WN[t, p], CN[t, p] = nxt[k, x], nxt[x, k]
            WH[t, p], CH[t, p] = hops[k, x], hops[x, k]
            AR[t, p], AC[t, p] = last[k, x], last[x, k]
    with np.errstate(all="ignore"):
        for t in range(bt - 1):
            for u in range(t + 1, bt):
                cand = C[t, u] * W[t, :]
                win = W[u, :] < cand
                W[u, win] = cand[win]
                WN[u, win] = CN[t, u] if CN[t, u] >= 0 else WN[t, win]
                WH[u, win] = CH[t, u] + WH[t, win]
                if panel_wins:
                    AR[u, win] = k0 + t
                cand = C[t, :] * W[t, u]
                win = C[u, :] < cand
                C[u, win] = cand[win]
                CN[u, win] = np.where(CN[t, win] >= 0, CN[t, win], WN[t, u])
                CH[u, win] = CH[t, win] + WH[t, u]
                if panel_wins:
                    AC[u, win] = k0 + t
    w = min(S, n - s0)
    return tuple(a[:, B:B + w] for a in (W, WN, WH, C, CN, CH)), AR, AC


def scheme(rate, nxt, hops, B, S, tile, panel_wins=True, keep="last"):
    """The two launches' bookkeeping over the whole pivot range.  Solves in place; returns (last, at_col, at_row, U,
    stores per cell of at_col, stores per cell of at_row).  panel_wins=False and keep="first" are the two mutants the
    tests must tell apart."""
    n = rate.shape[0]
    tr, tc = tile
    last = np.full((n, n), UNWRITTEN, dtype=np.int32)
    at_col, at_row = last.copy(), last.copy()
    col_stores, row_stores = np.zeros((n, n), dtype=np.int64), np.zeros((n, n), dtype=np.int64)
    last[:, :] = -1                                  # 0. the fill launch
    u = 0
    for k0 in range(0, n, B):
        bt = min(B, n - k0)
        # ---- 1. the panel launch: strips that read the matrix and `last` and never each other
        frozen = rate.copy(), nxt.copy(), hops.copy(), last.copy()
        panels = (np.empty((bt, n), rate.dtype), np.empty((bt, n), np.int32), np.empty((bt, n), np.int32),
                  np.empty((bt, n), rate.dtype), np.empty((bt, n), np.int32), np.empty((bt, n), np.int32))
        for s0 in range(0, n, S):
            parts, AR, AC = _strip_trace(*frozen, k0, bt, B, s0, S, panel_wins)
            for got, want in zip(parts, large._strip_panels(*frozen[:3], k0, bt, B, s0, S)):
                assert_bits_equal(got, want, "the trace changed the strip's rate panels")
            w = parts[0].shape[1]
            for whole, part in zip(panels, parts):
                whole[:, s0:s0 + w] = part
            for t in range(bt):                      # only the strip positions are stored
                at_row[k0 + t, s0:s0 + w] = AR[t, B:B + w]
                at_col[s0:s0 + w, k0 + t] = AC[t, B:B + w]
                row_stores[k0 + t, s0:s0 + w] += 1
                col_stores[s0:s0 + w, k0 + t] += 1
        for a, b in zip((rate, nxt, hops, last), frozen):
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), "the panel launch modified the matrix or `last`"
        # ---- 2. the sweep launch, tile by tile
        W, WN, WH, C, CN, CH = panels
        for i0 in range(0, n, tr):
            for j0 in range(0, n, tc):
                i1, j1 = min(i0 + tr, n), min(j0 + tc, n)
                v = rate[i0:i1, j0:j1].copy()
                tb = np.full(v.shape, -1)
                off_diag = np.arange(i0, i1)[:, None] != np.arange(j0, j1)[None, :]
                with np.errstate(all="ignore"):
                    for t in range(bt):
                        cand = C[t, i0:i1][:, None] * W[t, j0:j1][None, :]
                        win = (v < cand) & off_diag
                        v[win] = cand[win]
                        if keep == "last":
                            tb[win] = t
                        else:
                            tb[win & (tb < 0)] = t
                        u += int(win.sum())
                for a, b in zip(*np.nonzero(tb >= 0)):
                    t, i, j = tb[a, b], i0 + a, j0 + b
                    rate[i, j] = v[a, b]
                    nxt[i, j] = CN[t, i] if CN[t, i] >= 0 else WN[t, j]
                    hops[i, j] = CH[t, i] + WH[t, j]
                    last[i, j] = k0 + t
    return last, at_col, at_row, u, col_stores, row_stores


def _inputs(n, dtype):
    for s, kind in enumerate(KINDS):
        yield kind, synth.make(kind, n, dtype, seed=synth.BASE_SEED + 4000 + s)
    rnd = np.random.default_rng(7700 + n)
    for d in range(4):
        r, x, h, heavy = hostile_matrix_mix(rnd, n, dtype)
        yield "hostile%d" % d, (r, x, h)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("S", STRIPS)
@pytest.mark.parametrize("B", WIDTHS)
def test_scheme_equals_the_definition_and_the_mid_scheme(B, S, dtype):
    """Orders 1..13 and 20, ordinary and hostile inputs: the three arrays cell for cell against the direct definition
    and against the mid scheme at the same B, diagonals included; the solution is the oracle's; every cell of at_row
    and at_col is stored exactly once.  Precondition of the group: panel wins moved some at_row / at_col cell away
    from `last` as it stood at the start of its block."""
    moved = 0
    for n in ORDERS:
        for name, (r0, x0, h0) in _inputs(n, dtype):
            what = "%s n=%d B=%d S=%d" % (name, n, B, S)
            er, ex, eh = r0.copy(), x0.copy(), h0.copy()
            eu = oracle.relax(er, ex, eh)
            want = r0.copy(), x0.copy(), h0.copy()
            d = mid.direct(*want)
            m = mid.scheme(r0.copy(), x0.copy(), h0.copy(), B)
            got = r0.copy(), x0.copy(), h0.copy()
            s = scheme(*got, B, S, TILES[S])
            for a, e, field in zip(got, (er, ex, eh), ("rate", "next", "hops")):
                assert_bits_equal(a, e, "%s scheme %s" % (what, field))
            assert s[3] == eu == d[3], what
            for a, b, c, field in zip(s[:3], d[:3], m[:3], ("last", "at_col", "at_row")):
                assert (a != UNWRITTEN).all(), "%s: a cell of %s was never written" % (what, field)
                assert np.array_equal(a, b), "%s %s against the definition" % (what, field)
                assert np.array_equal(a, c), "%s %s against the mid scheme" % (what, field)
            assert (s[4] == 1).all(), "%s: a cell of at_col is not stored exactly once" % what
            assert (s[5] == 1).all(), "%s: a cell of at_row is not stored exactly once" % what
            assert all((np.diagonal(a) == -1).all() for a in s[:3]), what
            blind = scheme(r0.copy(), x0.copy(), h0.copy(), B, S, TILES[S], panel_wins=False)
            moved += int((blind[1] != s[1]).sum() + (blind[2] != s[2]).sum())
    assert moved > 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("S", STRIPS)
@pytest.mark.parametrize("B", WIDTHS)
@pytest.mark.parametrize("mutant", [{"panel_wins": False}, {"keep": "first"}], ids=["no-panel-wins", "first-win"])
def test_the_inputs_tell_the_mutants_apart(mutant, B, S, dtype):
    """at_row / at_col exported as block-start `last`, and the sweep keeping the first winning t: each is caught by
    the arrays and by the lists."""
    arrays = lists = 0
    for n in (5, 9, 13, 20):
        for name, (r0, x0, h0) in _inputs(n, dtype):
            d = mid.direct(r0.copy(), x0.copy(), h0.copy())
            s = scheme(r0.copy(), x0.copy(), h0.copy(), B, S, TILES[S], **mutant)
            arrays += any(not np.array_equal(a, b) for a, b in zip(s[:3], d[:3]))
            if n <= 9:
                lists += any(mid.walk(*s[:3], x0, i, j) != mid.walk(*d[:3], x0, i, j)
                             for i in range(n) for j in range(n))
    assert arrays > 0 and lists > 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("B,S", [(2, 5), (3, 2), (4, 3)])
def test_a_walk_over_the_scheme_s_arrays_gives_the_ropes_lists(B, S, dtype):
    differ = 0
    for n in ORDERS:
        for name, (r0, x0, h0) in _inputs(n, dtype):
            if name == "t3" and n > 9:
                continue                                   # arbitrage: lists double per pivot
            ropes = list_ropes.solve(np.ascontiguousarray(r0), np.ascontiguousarray(x0))
            got = r0.copy(), x0.copy(), h0.copy()
            s = scheme(*got, B, S, TILES[S])
            assert_bits_equal(got[1], ropes.next, "%s n=%d next" % (name, n))
            for i in range(n):
                for j in range(n):
                    lst = mid.walk(*s[:3], x0, i, j)
                    assert lst == ropes.path(i, j), "%s n=%d B=%d S=%d (%d, %d)" % (name, n, B, S, i, j)
                    hop = oracle.follow_path(got[1], i, j)
                    differ += hop is None or tuple(hop) != lst
    assert differ > 0            # some list is not the walk of the final next-hops


def test_a_strip_reads_only_its_own_index_set_of_last():
    """Poison `last` outside (cross U strip) x cross and cross x (cross U strip): the strip's AR / AC do not change."""
    n, B, S, k0, bt = 13, 4, 3, 4, 4
    r, x, h = synth.make("d2", n, np.float64, seed=synth.BASE_SEED + 4100)
    last = mid.direct(r.copy(), x.copy(), h.copy())[0]      # any array of pivots will do
    for s0 in range(0, n, S):
        want = _strip_trace(r, x, h, last, k0, bt, B, s0, S, True)
        mine = np.zeros(n, dtype=bool)
        mine[k0:k0 + bt] = True
        mine[s0:s0 + S] = True
        cross = np.zeros(n, dtype=bool)
        cross[k0:k0 + bt] = True
        read = (cross[:, None] & mine[None, :]) | (mine[:, None] & cross[None, :])
        got = _strip_trace(r, x, h, np.where(read, last, 12345).astype(np.int32), k0, bt, B, s0, S, True)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), s0
