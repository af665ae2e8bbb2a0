"""Vectorised list oracle: runAlgo's whole `_path` lists with O(1) concatenation (ORACLE -- test infrastructure).

Only tests/ may import this module; the product (floydwarshall_amd/) never does.

list_faithful.py restates runAlgo (Algorithms.hs:42-61) with Python tuples: every successful compare of :55 copies
`ikPath ++ kjPath`, O(n^3) interpreter steps with list copies on top -- a minute at n = 258.  This module keeps
the same lists as ROPES.  A list is a node id:

    0            the empty list
    1 + v        the one-vertex list [v]                      (v in 0 .. n-1)
    > n          a concatenation, left[id] ++ right[id]       (both ids are older than id)

so `ikPath ++ kjPath` allocates one node, and step k is a handful of numpy operations on n x n arrays:

    cand = r[:, k, None] * r[None, k, :]      one IEEE multiply in the working dtype, nothing fused      (:61)
    p    = r < cand                           strict; false for NaN on either side                       (:55)
           with row k (:50), column k and the diagonal (:54) masked off
    for the entries in p:  node = (id[i, k], id[k, j]), both read before anything of this step is written (a new
           matrix per k, :44), the rate becomes cand.

Per node the module keeps what a list has whatever its representation: its length (saturating at 2^62; as int32
modulo 2^32 too, which is what a dense int32 `hops` array holds) and its first vertex (-1 for an empty list).  Whole
lists are flattened on demand, iteratively.  Nothing here knows how the engine stores or rebuilds a list.

0.1 s at n = 260; pinned to list_faithful.run_algo list for list and to the dense C loop (rate bits, next, hops, U)
by tests/test_oracle_ropes.py.
"""
import numpy as np

_SAT = np.int64(1) << 62


class RopeSolve:
    """State of runAlgo over some pivots: rate[n, n], node[n, n] (list ids) and the node table."""

    def __init__(self, rate, nxt=None):
        assert rate.ndim == 2 and rate.shape[0] == rate.shape[1]
        assert rate.dtype in (np.float32, np.float64)
        n = rate.shape[0]
        self.n = n
        self.rate = rate.copy()
        if nxt is None:                          # buildMatrix on a dense graph: [j] off the diagonal, [] on it
            first = np.where(np.eye(n, dtype=bool), -1, np.arange(n)[None, :])
        else:
            assert nxt.shape == rate.shape
            first = np.where(nxt >= 0, nxt, -1).astype(np.int64)
            assert int(first.max(initial=-1)) < n
        self.node = (first + 1).astype(np.int64)
        self._cap = max(4 * (n + 1), 1024)
        self._count = n + 1                      # ids 0 .. n are the empty list and the n one-vertex lists
        self._left = np.zeros(self._cap, dtype=np.int64)
        self._right = np.zeros(self._cap, dtype=np.int64)
        self._len = np.zeros(self._cap, dtype=np.int64)
        self._len32 = np.zeros(self._cap, dtype=np.int32)
        self._head = np.full(self._cap, -1, dtype=np.int64)
        self._len[1:n + 1] = 1
        self._len32[1:n + 1] = 1
        self._head[1:n + 1] = np.arange(n)
        self.updates = 0                         # U: successful compares of :55
        self.updates_empty_left = 0              # ... of which ikPath was the empty list
        self.updates_both_empty = 0              # ... of which both halves were

    def _reserve(self, more):
        need = self._count + more
        if need <= self._cap:
            return
        cap = max(need, 2 * self._cap)
        for name in ("_left", "_right", "_len", "_len32", "_head"):
            old = getattr(self, name)
            new = np.full(cap, -1, dtype=old.dtype) if name == "_head" else np.zeros(cap, dtype=old.dtype)
            new[:self._count] = old[:self._count]
            setattr(self, name, new)
        self._cap = cap

    def step(self, k):
        """Pivot k (one `runAlgo k` level, Algorithms.hs:44-61)."""
        n, r, node = self.n, self.rate, self.node
        with np.errstate(all="ignore"):
            cand = r[:, k, None] * r[None, k, :]
            p = r < cand
        assert cand.dtype == r.dtype
        p[k, :] = False
        p[:, k] = False
        p[np.arange(n), np.arange(n)] = False
        ii, jj = np.nonzero(p)
        m = len(ii)
        if m == 0:
            return
        lft = node[ii, k]                        # fancy indexing copies: both taken before this step writes
        rgt = node[k, jj]
        self._reserve(m)
        new = np.arange(self._count, self._count + m, dtype=np.int64)
        self._left[new] = lft
        self._right[new] = rgt
        self._len[new] = np.minimum(self._len[lft] + self._len[rgt], _SAT)
        with np.errstate(over="ignore"):
            self._len32[new] = self._len32[lft] + self._len32[rgt]
        self._head[new] = np.where(self._len[lft] > 0, self._head[lft], self._head[rgt])
        self._count += m
        r[ii, jj] = cand[ii, jj]
        node[ii, jj] = new
        self.updates += m
        self.updates_empty_left += int((self._len[lft] == 0).sum())
        self.updates_both_empty += int(((self._len[lft] == 0) & (self._len[rgt] == 0)).sum())

    # ---- what the lists are, per entry ------------------------------------------------------------------------
    @property
    def next(self):
        """First vertex of every list, -1 for an empty one (int32)."""
        return self._head[self.node].astype(np.int32)

    @property
    def hops(self):
        """Length of every list as a dense int32 array holds it (modulo 2^32)."""
        return self._len32[self.node].copy()

    @property
    def lengths(self):
        """Length of every list (int64, saturating at 2^62)."""
        return self._len[self.node].copy()

    def path(self, i, j, limit=1 << 22):
        """The list of entry (i, j) as a tuple of vertex indices."""
        n, left, right, ln = self.n, self._left, self._right, self._len
        root = int(self.node[i, j])
        assert int(ln[root]) <= limit, "list of %d entries" % int(ln[root])
        out, stack = [], [root]
        while stack:
            x = stack.pop()
            if x <= n:
                if x:
                    out.append(x - 1)
            elif ln[x]:
                stack.append(int(right[x]))
                stack.append(int(left[x]))
        return tuple(out)

    def paths(self, src, dst):
        return [self.path(int(s), int(d)) for s, d in zip(src, dst)]

    def all_paths(self):
        """[[path(i, j) for j] for i]."""
        return [[self.path(i, j) for j in range(self.n)] for i in range(self.n)]


def solve(rate, nxt=None, k_begin=0, k_end=None):
    """runAlgo over pivots [k_begin, k_end) from dense (rate, next) as the engine takes them: a RopeSolve.
    The inputs are left alone."""
    s = RopeSolve(rate, nxt)
    for k in range(k_begin, s.n if k_end is None else k_end):
        s.step(k)
    return s


__all__ = ["RopeSolve", "solve"]
