"""The scheme of the large batch tier (floydwarshall_amd/csrc/fwx_large.hip), restated in numpy and pinned to the
oracle before any GPU time is spent.  It is the mid tier's scheme (test_batch_mid_scheme.py) with the panel phase cut
into column strips that never talk to each other, and the sweep cut into tiles:

  1. panel, once per strip [s0, s0 + S) n [0, n): the index set is cross U strip, cross = [k0, k0 + bt).  Position
     p < B stands for the cross index k0 + p, position B + y for the strip index s0 + y.  W / WN / WH [t][p] = entry
     (k0+t, index(p)), C / CN / CH [t][p] = entry (index(p), k0+t), NaN at (k, k) and where a position has no index.
     For t = 0 .. bt-2 row t is frozen and pivot k0+t applied to the rows u > t, the operands from outside the strip
     being the strip's OWN copy of the cross entries C[t][u], W[t][u].  The strip positions are the strip's part of
     the [bt][n] panels.  The matrix is only read.
  2. sweep, once per tile of the matrix, from the assembled panels: every entry (i, j), i != j, folds the candidates
     C[t][i] * W[t][j] in ascending t with the strict <, keeping the value, the LAST winning t and a count; only the
     entries that moved are written, next = CN[t*][i] if >= 0 else WN[t*][j], hops = CH[t*][i] + WH[t*][j].

It must equal oracle.relax bit for bit (rate, next, hops, U) at block widths, strip widths, tile shapes and pivot
ranges off every boundary, on ordinary and hostile inputs, and the assembled panels must be the whole-width panels of
the mid scheme.  CPU only."""
import numpy as np
import pytest

import oracle
from floydwarshall_amd import synth

from helpers import assert_bits_equal
from hostile_inputs import hostile_matrix_mix

ORDERS = list(range(1, 14)) + [20]
WIDTHS = [2, 3, 4]
STRIPS = [3, 4, 8]
TILES = {3: (2, 5), 4: (4, 4), 8: (5, 3)}          # (rows, columns) of a sweep tile, one shape per strip width
KINDS = ("d1", "d2", "t1", "t3")


def _whole_width_panels(rate, nxt, hops, k0, bt):
    """The mid scheme's phase 1 (a copy of test_batch_mid_scheme._panels): (W, WN, WH, C, CN, CH), each bt x n."""
    ks = np.arange(k0, k0 + bt)
    W, C = rate[ks, :].copy(), rate[:, ks].T.copy()
    WN, CN = nxt[ks, :].copy(), nxt[:, ks].T.copy()
    WH, CH = hops[ks, :].copy(), hops[:, ks].T.copy()
    for t in range(bt):
        W[t, k0 + t] = np.nan
        C[t, k0 + t] = np.nan
    with np.errstate(all="ignore"):
        for t in range(bt):
            for u in range(t + 1, bt):
                ku = k0 + u
                cand = C[t, ku] * W[t, :]
                win = W[u, :] < cand
                W[u, win] = cand[win]
                WN[u, win] = CN[t, ku] if CN[t, ku] >= 0 else WN[t, win]
                WH[u, win] = CH[t, ku] + WH[t, win]
                cand = C[t, :] * W[t, ku]
                win = C[u, :] < cand
                C[u, win] = cand[win]
                CN[u, win] = np.where(CN[t, win] >= 0, CN[t, win], WN[t, ku])
                CH[u, win] = CH[t, win] + WH[t, ku]
    return W, WN, WH, C, CN, CH


def _strip_panels(rate, nxt, hops, k0, bt, B, s0, S):
    """Phase 1 of ONE strip, from the matrix alone.  Returns the strip's columns of (W, WN, WH, C, CN, CH)."""
    n = rate.shape[0]
    index = [k0 + p if p < bt else -1 for p in range(B)] + [s0 + y if s0 + y < n else -1 for y in range(S)]
    P = B + S
    W, C = np.full((bt, P), np.nan, dtype=rate.dtype), np.full((bt, P), np.nan, dtype=rate.dtype)
    WN, CN = np.full((bt, P), -1, dtype=np.int32), np.full((bt, P), -1, dtype=np.int32)
    WH, CH = np.zeros((bt, P), dtype=np.int32), np.zeros((bt, P), dtype=np.int32)
    for t in range(bt):
        k = k0 + t
        for p, x in enumerate(index):
            if x < 0:
                continue
            if x != k:                               # the diagonal's rate is not read
                W[t, p], C[t, p] = rate[k, x], rate[x, k]
            WN[t, p], CN[t, p] = nxt[k, x], nxt[x, k]
            WH[t, p], CH[t, p] = hops[k, x], hops[x, k]
    with np.errstate(all="ignore"):
        for t in range(bt - 1):                      # row t of both panels is frozen from here on
            for u in range(t + 1, bt):               # position u IS the cross index k0 + u
                cand = C[t, u] * W[t, :]
                win = W[u, :] < cand
                W[u, win] = cand[win]
                WN[u, win] = CN[t, u] if CN[t, u] >= 0 else WN[t, win]
                WH[u, win] = CH[t, u] + WH[t, win]
                cand = C[t, :] * W[t, u]
                win = C[u, :] < cand
                C[u, win] = cand[win]
                CN[u, win] = np.where(CN[t, win] >= 0, CN[t, win], WN[t, u])
                CH[u, win] = CH[t, win] + WH[t, u]
    w = min(S, n - s0)
    return tuple(a[:, B:B + w] for a in (W, WN, WH, C, CN, CH))


def _panels(rate, nxt, hops, k0, bt, B, S):
    """The [bt][n] panels assembled from the strips."""
    n = rate.shape[0]
    out = (np.empty((bt, n), rate.dtype), np.empty((bt, n), np.int32), np.empty((bt, n), np.int32),
           np.empty((bt, n), rate.dtype), np.empty((bt, n), np.int32), np.empty((bt, n), np.int32))
    for s0 in range(0, n, S):
        for whole, part in zip(out, _strip_panels(rate, nxt, hops, k0, bt, B, s0, S)):
            whole[:, s0:s0 + part.shape[1]] = part
    return out


def _sweep_tile(rate, nxt, hops, panels, bt, i0, i1, j0, j1):
    """Phase 2 on the tile [i0, i1) x [j0, j1), in place: value, last winning t and count per entry, then one
    write-back of the entries that moved.  Returns the tile's number of successful compares."""
    W, WN, WH, C, CN, CH = panels
    v = rate[i0:i1, j0:j1].copy()
    tb = np.full(v.shape, -1)
    off_diag = np.arange(i0, i1)[:, None] != np.arange(j0, j1)[None, :]
    u = 0
    with np.errstate(all="ignore"):
        for t in range(bt):
            cand = C[t, i0:i1][:, None] * W[t, j0:j1][None, :]
            win = (v < cand) & off_diag
            v[win] = cand[win]
            tb[win] = t
            u += int(win.sum())
    for a, b in zip(*np.nonzero(tb >= 0)):
        t, i, j = tb[a, b], i0 + a, j0 + b
        rate[i, j] = v[a, b]
        nxt[i, j] = CN[t, i] if CN[t, i] >= 0 else WN[t, j]
        hops[i, j] = CH[t, i] + WH[t, j]
    return u


def scheme(rate, nxt, hops, kb, ke, B, S, tile, check_panels=False):
    n = rate.shape[0]
    tr, tc = tile
    u = 0
    for k0 in range(kb, ke, B):
        bt = min(B, ke - k0)
        before = rate.copy(), nxt.copy(), hops.copy()
        panels = _panels(rate, nxt, hops, k0, bt, B, S)
        for a, b in zip((rate, nxt, hops), before):
            assert_bits_equal(a, b, "the panel phase modified the matrix")
        if check_panels:
            for got, want, name in zip(panels, _whole_width_panels(rate, nxt, hops, k0, bt),
                                       ("W", "WN", "WH", "C", "CN", "CH")):
                assert_bits_equal(got, want, "%s of pivots [%d, %d)" % (name, k0, k0 + bt))
        for i0 in range(0, n, tr):
            for j0 in range(0, n, tc):
                u += _sweep_tile(rate, nxt, hops, panels, bt, i0, min(i0 + tr, n), j0, min(j0 + tc, n))
    return u


def _ranges(n, B):
    """The whole range and ranges that start and end off block boundaries."""
    out = {(0, n), (0, min(1, n)), (n - 1, n), (1, n), (1, max(1, n - 1)), (min(B + 1, n), n), (n // 2, n // 2)}
    return sorted((a, b) for a, b in out if 0 <= a <= b <= n)


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
@pytest.mark.parametrize("n", ORDERS)
def test_scheme_equals_the_oracle(n, B, S, dtype):
    for name, (r0, x0, h0) in _inputs(n, dtype):
        for kb, ke in _ranges(n, B):
            want = r0.copy(), x0.copy(), h0.copy()
            wu = oracle.relax(*want, kb, ke)
            got = r0.copy(), x0.copy(), h0.copy()
            gu = scheme(*got, kb, ke, B, S, TILES[S], check_panels=True)
            what = "%s n=%d B=%d S=%d [%d, %d)" % (name, n, B, S, kb, ke)
            for g, w, field in zip(got, want, ("rate", "next", "hops")):
                assert_bits_equal(g, w, "%s %s" % (what, field))
            assert gu == wu, what


def test_a_strip_reads_only_its_own_index_set():
    """Poison every entry outside (cross U strip) x cross and cross x (cross U strip): the strip's panels do not
    change -- strips need nothing from each other."""
    n, B, S, k0, bt = 13, 4, 4, 3, 4
    r, x, h = synth.make("d2", n, np.float64, seed=synth.BASE_SEED + 4100)
    for s0 in range(0, n, S):
        want = _strip_panels(r, x, h, k0, bt, B, s0, S)
        mine = np.zeros(n, dtype=bool)
        mine[k0:k0 + bt] = True
        mine[s0:s0 + S] = True
        cross = np.zeros(n, dtype=bool)
        cross[k0:k0 + bt] = True
        read = (cross[:, None] & mine[None, :]) | (mine[:, None] & cross[None, :])
        r2, x2, h2 = np.where(read, r, 1e300), np.where(read, x, 77).astype(np.int32), \
            np.where(read, h, 99).astype(np.int32)
        for got, w, name in zip(_strip_panels(r2, x2, h2, k0, bt, B, s0, S), want, ("W", "WN", "WH", "C", "CN", "CH")):
            assert_bits_equal(got, w, "strip at %d: %s" % (s0, name))
