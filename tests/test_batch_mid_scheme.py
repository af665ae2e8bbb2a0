"""The scheme of the mid batch tier (floydwarshall_amd/csrc/fwx_mid.hip), restated in numpy and pinned to the oracle
before any GPU time is spent: the matrix stays where it is, pivots are taken B at a time, and every block is

  1. panel: copies of the pivot rows (W / WN / WH, bt x n) and pivot columns (C / CN / CH, kept transposed, bt x n),
     NaN in place of the diagonal entries (k, k); for t = 0 .. bt-1 row t of both panels is frozen as the time-k
     snapshot and pivot k is applied to the rows below it in both panels.  The matrix is not modified.
  2. sweep: every entry (i, j), i != j, folds the candidates C[t][i] * W[t][j] in ascending t with the strict <;
     next = CN[t][i] if that is >= 0 else WN[t][j], hops = CH[t][i] + WH[t][j]; every win counts towards U.

It must equal oracle.relax bit for bit (rate, next, hops, U) at block widths and pivot ranges off every boundary, on
ordinary and hostile inputs, and its panels must be helpers.pass_reference's snapshots.  CPU only."""
import numpy as np
import pytest

import oracle
from floydwarshall_amd import synth

from helpers import assert_bits_equal, pass_reference
from hostile_inputs import hostile_matrix_mix

ORDERS = list(range(1, 14)) + [20]
WIDTHS = [2, 3, 4]
KINDS = ("d1", "d2", "t1", "t3")


def _panels(rate, nxt, hops, k0, bt):
    """Phase 1.  Returns (W, WN, WH, C, CN, CH), each bt x n; the matrix is only read."""
    n = rate.shape[0]
    ks = np.arange(k0, k0 + bt)
    W, C = rate[ks, :].copy(), rate[:, ks].T.copy()
    WN, CN = nxt[ks, :].copy(), nxt[:, ks].T.copy()
    WH, CH = hops[ks, :].copy(), hops[:, ks].T.copy()
    for t in range(bt):
        W[t, k0 + t] = np.nan                    # the diagonal entry is not read: these ARE the skips
        C[t, k0 + t] = np.nan
    with np.errstate(all="ignore"):
        for t in range(bt):                      # row t of both panels is frozen from here on
            for u in range(t + 1, bt):
                ku = k0 + u
                cand = C[t, ku] * W[t, :]        # row ku of the matrix
                win = W[u, :] < cand
                W[u, win] = cand[win]
                WN[u, win] = CN[t, ku] if CN[t, ku] >= 0 else WN[t, win]
                WH[u, win] = CH[t, ku] + WH[t, win]
                cand = C[t, :] * W[t, ku]        # column ku of the matrix
                win = C[u, :] < cand
                C[u, win] = cand[win]
                CN[u, win] = np.where(CN[t, win] >= 0, CN[t, win], WN[t, ku])
                CH[u, win] = CH[t, win] + WH[t, ku]
    return W, WN, WH, C, CN, CH


def _sweep(rate, nxt, hops, panels, bt):
    """Phase 2, in place.  Returns the number of successful compares."""
    W, WN, WH, C, CN, CH = panels
    n = rate.shape[0]
    off_diag = ~np.eye(n, dtype=bool)
    u = 0
    with np.errstate(all="ignore"):
        for t in range(bt):
            cand = C[t][:, None] * W[t][None, :]
            win = (rate < cand) & off_diag
            rate[win] = cand[win]
            nxt[win] = np.where(CN[t][:, None] >= 0, CN[t][:, None], WN[t][None, :])[win]
            hops[win] = (CH[t][:, None] + WH[t][None, :])[win]
            u += int(win.sum())
    return u


def scheme(rate, nxt, hops, kb, ke, B, check_panels=False):
    u = 0
    for k0 in range(kb, ke, B):
        bt = min(B, ke - k0)
        before = rate.copy(), nxt.copy(), hops.copy()
        panels = _panels(rate, nxt, hops, k0, bt)
        for a, b in zip((rate, nxt, hops), before):
            assert_bits_equal(a, b, "the panel phase modified the matrix")
        if check_panels:
            ref = pass_reference(rate, nxt, hops, k0, k0 + bt)
            skip = np.zeros_like(ref.W, dtype=bool)
            skip[np.arange(bt), k0 + np.arange(bt)] = True      # (k, k): NaN in the scheme, never an operand
            assert_bits_equal(np.where(skip, 0, panels[0]), np.where(skip, 0, ref.W), "W")
            assert_bits_equal(panels[1], ref.WN, "WN")
            assert_bits_equal(panels[2], ref.WH, "WH")
        u += _sweep(rate, nxt, hops, panels, bt)
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
@pytest.mark.parametrize("B", WIDTHS)
@pytest.mark.parametrize("n", ORDERS)
def test_scheme_equals_the_oracle(n, B, dtype):
    for name, (r0, x0, h0) in _inputs(n, dtype):
        for kb, ke in _ranges(n, B):
            want = r0.copy(), x0.copy(), h0.copy()
            wu = oracle.relax(*want, kb, ke)
            got = r0.copy(), x0.copy(), h0.copy()
            gu = scheme(*got, kb, ke, B, check_panels=(kb, ke) == (0, n))
            what = "%s n=%d B=%d [%d, %d)" % (name, n, B, kb, ke)
            for g, w, field in zip(got, want, ("rate", "next", "hops")):
                assert_bits_equal(g, w, "%s %s" % (what, field))
            assert gu == wu, what


def test_the_hostile_draws_hit_the_fallback_to_the_head_of_kjpath():
    """Some winning product has an empty ikPath (a positive rate whose next is -1): the WN / next[k][j] fallback is
    exercised, not just written down."""
    hit = 0
    for n in (5, 9, 13, 20):
        rnd = np.random.default_rng(7700 + n)
        for _ in range(4):
            r, x, h, _heavy = hostile_matrix_mix(rnd, n, np.float64)
            assert ((r > 0) & (x < 0)).any()
            for k in range(n):
                before = r.copy()
                col_empty = x[:, k] < 0
                oracle.relax(r, x, h, k, k + 1)
                changed = r.view(np.uint64) != before.view(np.uint64)
                hit += int((changed & col_empty[:, None]).sum())
    assert hit > 0
