"""oracle/list_ropes.py (whole `_path` lists with O(1) concatenation) pinned to the two restatements it has to agree
with: list for list to oracle/list_faithful.py's run_algo where pure Python is affordable, and in rate bits,
next (= head of the list), hops (= its length) and U to the dense C loop at the orders where the GPU tests use it
(tests/test_gpu_exact_lists_edges.py).  Hostile inputs (NaN, negatives, -0.0, positive rates whose path is empty)
are the point: there an update can concatenate an empty ikPath, and the list is not the walk of the final next-hops.
No GPU here."""
import numpy as np
import pytest

import oracle
from floydwarshall_amd import synth
from oracle import list_faithful as lf
from oracle import list_ropes

from helpers import assert_bits_equal, golden_dense, load_golden
from hostile_inputs import hostile_matrix, market_rates

DTYPES = [np.float32, np.float64]


def _vertices(n):
    return [("X", "C%04d" % i) for i in range(n)]


def _same_lists(rate, nxt, dtype, kb=0, ke=None):
    """Every entry of the rope solve against lf.run_algo over the same pivots: rate bits and the whole list; the
    head and the length the ropes report are those of the flattened list.  Returns the rope solve."""
    n = rate.shape[0]
    m = lf.run_algo(lf.from_dense(_vertices(n), rate, nxt), dtype, kb, ke)
    _, er, en, eh = lf.to_dense(m, dtype)
    want = lf.path_indices(m)
    got = list_ropes.solve(rate, nxt, kb, ke)
    assert_bits_equal(got.rate, er, "rate")
    assert got.all_paths() == want
    assert_bits_equal(got.next, en, "next")
    assert_bits_equal(got.hops, eh, "hops")
    assert np.array_equal(got.lengths, eh)
    src, dst = [0, n - 1, n // 2], [n - 1, 0, n // 2]
    assert got.paths(src, dst) == [want[s][d] for s, d in zip(src, dst)]
    return got


@pytest.mark.parametrize("dtype", DTYPES)
def test_golden_4x4(dtype):
    g = load_golden("algorithms_4x4.json")
    rate, nxt, _, _ = golden_dense(g["initial"], dtype)
    got = _same_lists(rate, nxt, dtype)
    assert got.all_paths() == golden_dense(g["solved"], dtype)[3]       # the reference's own lists
    assert got.updates > 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [3, 5, 8, 13, 21])
def test_hostile_lists_equal_list_faithful(n, dtype):
    empty_left = 0
    for seed in range(4):
        rate, nxt, _ = hostile_matrix(np.random.default_rng(4100 + 10 * n + seed), n, dtype)
        full = _same_lists(rate, nxt, dtype)
        empty_left += full.updates_empty_left
        for kb, ke in ((0, n // 2), (n // 2, n), (1, n - 1)):
            _same_lists(rate, nxt, dtype, kb, ke)
        # a range continued from the state the first half left: the two halves compose to the whole
        half = list_ropes.solve(rate, nxt, 0, n // 2)
        rest = list_ropes.solve(half.rate, half.next, n // 2, n)
        assert_bits_equal(rest.rate, full.rate, "rate of the composed halves")
        assert half.updates + rest.updates == full.updates
    if n >= 5:
        assert empty_left > 0               # the case the dense head rule has a second branch for did occur


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["t1", "t2", "t3"])
def test_synth_kinds_equal_list_faithful(kind, dtype):
    n = 20
    rate, nxt, _ = synth.make(kind, n, dtype, seed=77)
    got = _same_lists(rate, nxt, dtype)
    assert got.updates > 0
    _same_lists(rate, nxt, dtype, 3, 17)


def test_market_equals_list_faithful():
    m0 = lf.build_matrix(market_rates(8, 6, seed=23))
    assert 32 < len(m0) <= 48
    _, rate, nxt, _ = lf.to_dense(m0)
    want = lf.path_indices(lf.run_algo(m0))
    got = list_ropes.solve(rate, nxt)
    assert got.all_paths() == want
    walks = [[oracle.follow_path(got.next, s, d) for d in range(len(m0))] for s in range(len(m0))]
    assert any(list(want[s][d]) != walks[s][d] for s in range(len(m0)) for d in range(len(m0)))


def _inputs(n, dtype):
    yield "hostile", hostile_matrix(np.random.default_rng(5200 + n), n, dtype)
    for kind in sorted(synth.GENERATORS):
        yield kind, synth.make(kind, n, dtype, seed=300 + n)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [63, 64, 65, 127, 128, 129, 136, 260])
def test_equals_the_dense_loop(n, dtype):
    off = ~np.eye(n, dtype=bool)
    for what, (rate, nxt, hops) in _inputs(n, dtype):
        assert np.array_equal(hops[off], (nxt >= 0).astype(np.int32)[off])      # one-vertex lists where there is one
        er, en, eh = rate.copy(), nxt.copy(), hops.copy()
        eu = oracle.relax(er, en, eh)
        got = list_ropes.solve(rate, nxt)
        assert_bits_equal(got.rate, er, what + " rate")
        assert_bits_equal(got.next, en, what + " next")
        assert np.array_equal(got.hops[off], eh[off]), what + " hops"
        assert np.array_equal(np.diag(eh), np.diag(hops)), what + " hops on the diagonal"
        assert got.updates == eu, what
        assert eu > 0, what


def test_equals_the_committed_lists_of_order_258():
    g = load_golden("handle_kinds_lists_n258_f32.json")
    rate, nxt, _ = synth.make(g["kind"], g["n"], np.float32, seed=g["seed"])
    got = list_ropes.solve(rate, nxt)
    assert len(g["lists"]) >= 40
    for e in g["lists"]:
        assert got.path(e["src"], e["dst"]) == tuple(e["path"]), (e["src"], e["dst"])
    assert int(got.lengths.max()) == g["max_len"]
    assert int(got.lengths[g["longest"][0], g["longest"][1]]) == g["max_len"]


def test_the_product_does_not_import_it():
    import os
    import re
    from helpers import ROOT
    pkg = os.path.join(ROOT, "floydwarshall_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                with open(os.path.join(d, f)) as fh:
                    assert not re.search(r"list_ropes|import oracle|from oracle", fh.read()), f
