"""Batched what-if sweeps on the GPU (fwx_dev_solve_sweep, fwx_solve_sweep_*): `count` variants of ONE base matrix of
order n <= 128 in one call, variant b = the base with its patches applied in list order.  Every output -- the queried
entries, the full matrices where asked for (diagonals included) and U -- is bit for bit what the oracle's loop
(oracle.relax) leaves of M_b, which is built here on the CPU with numpy: a copy of the base, the patches in order.

The device form runs with guard bands of a sentinel around every output and around the base: what the call may write
is written, nothing else is, and the base comes back as it went in.  FWX_BATCH_WAVE_MAX_N = 16 / 0 puts the orders up
to 16 through both tiers."""
import functools

import numpy as np
import pytest

import oracle
from floydwarshall_amd import engine, hip, synth

from helpers import assert_bits_equal, dev
from hostile_inputs import hostile_matrix_mix

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
WAVE_ORDERS = [1, 2, 3, 4, 5, 15, 16]
WORKGROUP_ORDERS = [17, 63, 64, 65, 127, 128]
ORDER_TIERS = [(n, w) for n in WAVE_ORDERS for w in ("16", "0")] + [(n, "16") for n in WORKGROUP_ORDERS]
GUARD = 64                          # elements of sentinel on either side of every device array
RATE_SENTINEL, INT_SENTINEL = -1234.5, -99999
FIELD_NAMES = ("rate", "next", "hops")


# ---- inputs ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _base(kind, n, dtype_name, seed=synth.BASE_SEED + 3000):
    b = synth.make(kind, n, np.dtype(dtype_name).type, seed=seed)
    for a in b:
        a.setflags(write=False)
    return b


def _six_variants(base, n, rnd):
    """The patch lists of the six variants of the issue: per variant a list of (cell, rate, next, hops)."""
    r = base[0]

    def patch(i, j, factor=4.0, nxt=None, hops=1):
        return (i * n + j, r.dtype.type(r[i, j] * factor), j if nxt is None else nxt, hops)

    i = int(rnd.integers(n))
    j = (i + 1 + int(rnd.integers(n - 1))) % n if n > 1 else 0
    corners = [patch(0, n - 1), patch(n - 1, 0), patch(n - 1, max(n - 2, 0), 8.0), patch(n - 1, n - 1, 0.5)]
    odd = [patch(i, j, 4.0, (j + 1) % n, 3), patch(j, i, 2.0, -1, 0), patch(0, 0, 3.0, n - 1, 7)]
    return [[], [patch(i, j)], [patch(i, j, 2.0), patch(i, j, 16.0, (j + 1) % n, 2)], corners, odd, list(odd)]


def _items_for(n, count, rnd, skip=(0,)):
    """Per variant (0, n-1), (n-1, 0), one diagonal cell and 8 seeded pairs; the variants in `skip` ask nothing."""
    out = []
    for b in range(count):
        if b in skip:
            out.append([])
            continue
        d = int(rnd.integers(n))
        pairs = [(0, n - 1), (n - 1, 0), (d, d)] + [(int(rnd.integers(n)), int(rnd.integers(n))) for _ in range(8)]
        out.append(pairs)
    return out


def _materialise(base, fields, plist, patch_fields):
    """M_b: the first fields + 1 arrays of the base, copied, with the patches applied in order; next / hops of a patch
    only where the call passes those arrays (patch_fields >= 1 / >= 2)."""
    m = [base[f].copy() if f <= fields else None for f in range(3)]
    for cell, v, pn, ph in plist:
        m[0].flat[cell] = v
        if patch_fields >= 1:
            m[1].flat[cell] = pn
        if patch_fields >= 2:
            m[2].flat[cell] = ph
    return m


def _oracle(base, fields, plists, patch_fields):
    """(rate, next, hops) stacked over the variants, solved by oracle.relax one at a time, and [U_b]."""
    solved, us = [], []
    for plist in plists:
        m = _materialise(base, fields, plist, patch_fields)
        us.append(int(oracle.relax(m[0], m[1], m[2])))
        solved.append(m)
    return [np.stack([m[f] for m in solved]) if f <= fields else None for f in range(3)], us


def _csr(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(v) for v in lists])
    return ptr


# ---- the device form under guard bands -------------------------------------------------------------------------------
class Guarded:
    """A device array with GUARD sentinel elements on either side; `view` is what the call sees."""

    def __init__(self, a, fill):
        a = np.ascontiguousarray(a)
        self.fill = np.full(GUARD, fill, dtype=a.dtype)
        self.whole = dev(np.concatenate([self.fill, a.reshape(-1), self.fill]))
        self.view = hip.DeviceArray((a.size,), a.dtype, _ptr=self.whole.data_ptr() + GUARD * a.dtype.itemsize,
                                    _base=self.whole)
        self.shape = a.shape

    def read(self, what):
        got = self.whole.numpy()
        assert_bits_equal(got[:GUARD], self.fill, "%s: the guard band in front" % what)
        assert_bits_equal(got[len(got) - GUARD:], self.fill, "%s: the guard band behind" % what)
        return got[GUARD:len(got) - GUARD].reshape(self.shape)


def _sentinel(shape, dtype):
    return np.full(shape, RATE_SENTINEL if np.dtype(dtype).kind == "f" else INT_SENTINEL, dtype=dtype)


def run_dev(base, fields, plists, ilists, *, patch_fields=0, full=True, stride=None, upd_start=None, mutate=None,
            item_fields=None):
    """fwx_dev_solve_sweep on the first fields + 1 arrays of `base`.  Returns (full arrays stacked (count, n, n) or
    None, item outputs flat over all items, updates); every guard band and the base are checked on the way."""
    n = base[0].shape[0]
    count = len(plists)
    dtype = base[0].dtype
    item_fields = fields if item_fields is None else item_fields
    t = {"pptr": _csr(plists), "iptr": _csr(ilists),
         "pindex": np.array([p[0] for v in plists for p in v], dtype=np.int64),
         "prate": np.array([p[1] for v in plists for p in v], dtype=dtype),
         "pnext": np.array([p[2] for v in plists for p in v], dtype=np.int32),
         "phops": np.array([p[3] for v in plists for p in v], dtype=np.int32),
         "src": np.array([q[0] for v in ilists for q in v], dtype=np.int32),
         "dst": np.array([q[1] for v in ilists for q in v], dtype=np.int32)}
    if mutate:
        mutate(t)
    g = {k: Guarded(v, INT_SENTINEL if v.dtype.kind == "i" else RATE_SENTINEL) for k, v in t.items()}
    gbase = [Guarded(base[f], _sentinel((), base[f].dtype)[()]) if f <= fields else None for f in range(3)]
    total_items = len(t["src"])
    outs = [Guarded(_sentinel(total_items, dtype if f == 0 else np.int32), 55) if f <= item_fields else None
            for f in range(3)]
    stride = n * n if stride is None else stride
    fulls = [None, None, None]
    if full:
        fulls = [Guarded(_sentinel(count * stride, dtype if f == 0 else np.int32), 66) if f <= fields else None
                 for f in range(3)]
    start = np.zeros(count, dtype=np.uint64) if upd_start is None else np.asarray(upd_start, dtype=np.uint64)
    upd = Guarded(start, 77)
    v = lambda x: None if x is None else x.view
    patches = (g["pptr"].view, g["pindex"].view, g["prate"].view, v(g["pnext"]) if patch_fields >= 1 else None,
               v(g["phops"]) if patch_fields >= 2 else None)
    items = (g["iptr"].view, g["src"].view, g["dst"].view, v(outs[0]), v(outs[1]), v(outs[2]))
    engine.dev_solve_sweep(gbase[0].view, count, n, base_next_t=v(gbase[1]), base_hops_t=v(gbase[2]),
                           patches=patches if len(t["pindex"]) else None, items=items if total_items else None,
                           full=(v(fulls[0]), v(fulls[1]), v(fulls[2]), stride) if full else None, updates_t=upd.view)
    hip.synchronize()
    for k, arr in g.items():
        assert_bits_equal(arr.read(k), t[k], "the table %s" % k)
    for f in range(3):
        if gbase[f] is not None:
            assert_bits_equal(gbase[f].read("base " + FIELD_NAMES[f]), base[f], "the base's %s" % FIELD_NAMES[f])
    got_items = [None if o is None else o.read("item " + FIELD_NAMES[f]) for f, o in enumerate(outs)]
    got_full = [None if o is None else o.read("full " + FIELD_NAMES[f]).reshape(count, stride)
                for f, o in enumerate(fulls)]
    return got_full, got_items, [int(u) for u in upd.read("updates")]


def _check(got, want, us, n, ilists, what, start=None, skip_items=()):
    """got = run_dev's result against the oracle's stacked matrices: the full outputs whole (and their gaps still the
    sentinel), every item's outputs, U on top of `start`."""
    got_full, got_items, got_u = got
    count = len(us)
    for f in range(3):
        if got_full[f] is not None:
            assert_bits_equal(got_full[f][:, :n * n].reshape(count, n, n), want[f], "%s: full %s" % (what, FIELD_NAMES[f]))
            gap = got_full[f][:, n * n:]
            assert_bits_equal(gap, _sentinel(gap.shape, gap.dtype), "%s: the gap of full %s" % (what, FIELD_NAMES[f]))
    q = 0
    for b, pairs in enumerate(ilists):
        for s, d in pairs:
            for f in range(3):
                if got_items[f] is None:
                    continue
                if q in skip_items:
                    w = _sentinel((), got_items[f].dtype)
                else:
                    w = want[f][b, s, d]
                assert_bits_equal(got_items[f][q:q + 1], np.array([w], dtype=got_items[f].dtype),
                                  "%s: item %d = (%d, %d) of variant %d, %s" % (what, q, s, d, b, FIELD_NAMES[f]))
            q += 1
    start = [0] * count if start is None else [int(x) for x in start]
    assert got_u == [a + b for a, b in zip(start, us)], "%s: U per variant %s, the oracle's %s on top of %s" % (
        what, got_u, us, start)


# ---- orders, tiers, fields ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["d2", "t1"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n,wave", ORDER_TIERS)
def test_six_variants_full_outputs_and_items(n, wave, dtype, kind, monkeypatch):
    monkeypatch.setenv("FWX_BATCH_WAVE_MAX_N", wave)
    base = _base(kind, n, np.dtype(dtype).name)
    rnd = np.random.default_rng(100 * n + len(kind))
    plists = _six_variants(base, n, rnd)
    ilists = _items_for(n, 6, rnd)
    plain, plain_u = _oracle(base, 2, [[]], 0)
    # (fields, patch_fields): rates only; + next with the patches' next given / NULL; + hops likewise
    for fields, patch_fields in ((0, 0), (1, 1), (1, 0), (2, 2), (2, 1), (2, 0)):
        what = "n=%d wave<=%s %s %s fields=%d patch_fields=%d" % (n, wave, np.dtype(dtype).name, kind, fields, patch_fields)
        want, us = _oracle(base, fields, plists, patch_fields)
        for f in range(fields + 1):         # variant 0 has no patches: the plain solve of the base
            assert_bits_equal(want[f][0], plain[f][0], what + ": the oracle itself")
        assert us[0] == plain_u[0]
        if n >= 4:
            assert min(us) > 0, "%s: the oracle relaxes nothing in variant %d" % (what, int(np.argmin(us)))
        _check(run_dev(base, fields, plists, ilists, patch_fields=patch_fields), want, us, n, ilists, what)


def test_a_later_patch_of_a_cell_wins_and_null_fields_keep_the_base():
    """The oracle side of variants (2), (4) and (5), stated on its own so that the cases above cannot agree by
    accident: the two patches of (2) differ, and (5) differs from (4) exactly in next / hops of the patched cells."""
    n = 16
    base = _base("d2", n, "float64")
    v = _six_variants(base, n, np.random.default_rng(5))
    assert v[2][0][0] == v[2][1][0] and v[2][0][1] != v[2][1][1]
    given, null = _materialise(base, 2, v[4], 2), _materialise(base, 2, v[5], 0)
    assert np.array_equal(given[0], null[0])
    assert not np.array_equal(given[1], null[1]) and not np.array_equal(given[2], null[2])


# ---- counts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,count,wave", [(4, c, w) for c in (1, 3, 4, 5, 257) for w in ("16", "0")] +
                         [(64, 1, "16"), (64, 2, "16"), (64, 130, "16"), (128, 3, "16")])
def test_counts(n, count, wave, monkeypatch):
    """A last wave-tier workgroup with 1 or 3 waves in use, and more workgroups than the chip has CUs."""
    monkeypatch.setenv("FWX_BATCH_WAVE_MAX_N", wave)
    base = _base("d2", n, "float64")
    rnd = np.random.default_rng(7 * n + count)
    r = base[0]
    plists = []
    for b in range(count):
        i = int(rnd.integers(n))
        j = (i + 1 + int(rnd.integers(n - 1))) % n
        plists.append([(i * n + j, r[i, j] * (2.0 + b % 5), j, 1), (j * n + i, r[j, i] * 0.5, i, 1)])
    ilists = _items_for(n, count, rnd, skip=())
    ilists = [v[:4] for v in ilists]
    want, us = _oracle(base, 2, plists, 2)
    assert min(us) > 0
    what = "n=%d count=%d wave<=%s" % (n, count, wave)
    _check(run_dev(base, 2, plists, ilists, patch_fields=2), want, us, n, ilists, what)


# ---- hostile values ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", [5, 16, 17, 64, 65, 128])
def test_hostile_base_and_patch_values(n, dtype):
    rnd = np.random.default_rng(9100 + n)
    base = hostile_matrix_mix(rnd, n, dtype)[:3]
    fi = np.finfo(dtype)
    values = [np.nan, np.inf, -np.inf, -0.0, -2.5, fi.tiny / 4]
    plists = [[]]
    for v in values:                          # one variant per value, the cell and a second one drawn
        cells = rnd.choice(n * n, size=2, replace=False)
        plists.append([(int(cells[0]), dtype(v), int(cells[0]) % n, 1), (int(cells[1]), dtype(1.5), int(cells[1]) % n, 1)])
    cells = rnd.choice(n * n, size=3, replace=False)
    plists.append([(int(c), dtype(3.0), -1, 0) for c in cells])         # positive rates without a path
    plists.append([(int(c), dtype(v), -1 if k % 2 else int(c) % n, k % 3) for k, (c, v) in
                   enumerate(zip(rnd.choice(n * n, size=len(values)), values))])
    ilists = _items_for(n, len(plists), rnd, skip=())
    for fields, patch_fields in ((0, 0), (1, 1), (2, 2), (2, 0)):
        want, us = _oracle(base, fields, plists, patch_fields)
        what = "hostile n=%d %s fields=%d patch_fields=%d" % (n, np.dtype(dtype).name, fields, patch_fields)
        _check(run_dev(base, fields, plists, ilists, patch_fields=patch_fields), want, us, n, ilists, what)


# ---- items only, strides, U ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,wave", [(5, "16"), (5, "0"), (64, "16"), (100, "16")])
def test_items_only_writes_the_item_outputs_and_nothing_else(n, wave, monkeypatch):
    """full NULL: the answers equal the oracle's cells; run_dev checks the guard bands around every output, every table
    and the base, and that the base is bit-identical afterwards."""
    monkeypatch.setenv("FWX_BATCH_WAVE_MAX_N", wave)
    base = _base("d2", n, "float64")
    rnd = np.random.default_rng(31 * n)
    plists = _six_variants(base, n, rnd)
    ilists = _items_for(n, 6, rnd)
    want, us = _oracle(base, 2, plists, 2)
    _check(run_dev(base, 2, plists, ilists, patch_fields=2, full=False), want, us, n, ilists, "items only n=%d" % n)
    # rates only out of a base with next and hops: the optional item outputs left out
    _check(run_dev(base, 2, plists, ilists, patch_fields=2, full=False, item_fields=0), want, us, n, ilists,
           "items only, rate_out alone, n=%d" % n)


@pytest.mark.parametrize("n,wave", [(7, "16"), (7, "0"), (70, "16")])
def test_full_outputs_with_a_gap_and_counters_on_a_nonzero_start(n, wave, monkeypatch):
    monkeypatch.setenv("FWX_BATCH_WAVE_MAX_N", wave)
    base = _base("t1", n, "float32")
    rnd = np.random.default_rng(17 * n)
    plists = _six_variants(base, n, rnd)
    ilists = _items_for(n, 6, rnd)
    want, us = _oracle(base, 2, plists, 2)
    assert min(us) > 0
    start = [5, 0, 1 << 40, 7, 9, 11]
    got = run_dev(base, 2, plists, ilists, patch_fields=2, stride=n * n + 13, upd_start=start)
    _check(got, want, us, n, ilists, "stride n*n+13, n=%d" % n, start=start)
    # no patches at all, no items at all: every variant is the base
    plain, plain_u = _oracle(base, 2, [[], [], []], 0)
    _check(run_dev(base, 2, [[], [], []], [[], [], []]), plain, plain_u, n, [[], [], []], "patches NULL, items NULL")


# ---- tables that do not belong ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,wave", [(6, "16"), (6, "0"), (64, "16"), (90, "16")])
def test_tables_that_do_not_belong_are_passed_over(n, wave, monkeypatch):
    """What the device form cannot check is defended against in the kernel: each case states the lists a correct kernel
    acts on, and the arrays keep their true extents, so nothing here reaches a bad address."""
    monkeypatch.setenv("FWX_BATCH_WAVE_MAX_N", wave)
    base = _base("d2", n, "float64")
    rnd = np.random.default_rng(13 * n)
    r = base[0]
    flat = []                                      # 8 patches, two a variant; 3 items a variant
    for _ in range(8):
        i = int(rnd.integers(n))
        j = (i + 1 + int(rnd.integers(n - 1))) % n
        flat.append((i * n + j, r[i, j] * 4.0, j, 1))
    plists = [flat[2 * b:2 * b + 2] for b in range(4)]
    ilists = [v[:3] for v in _items_for(n, 4, rnd, skip=())]

    def run(plists_seen, mutate, what, skip_items=()):
        want, us = _oracle(base, 2, plists_seen, 2)
        _check(run_dev(base, 2, plists, ilists, patch_fields=2, mutate=mutate), want, us, n, ilists, what,
               skip_items=skip_items)

    # a descending pair: variant 1 = [2, 1) is empty, variant 2 = [1, 6)
    run([flat[0:2], [], flat[1:6], flat[6:8]], lambda t: t["pptr"].__setitem__(2, 1), "a descending patch ptr pair")
    # ptr past total: clamped to the 8 entries there are; a negative start: clamped to 0
    run(plists, lambda t: t["pptr"].__setitem__(4, 8 + 5), "a patch ptr past total")
    # variant 0 = [0, -3) is empty, variant 1 = [-3, 4) is [0, 4)
    run([[], flat[0:4], flat[4:6], flat[6:8]], lambda t: t["pptr"].__setitem__(1, -3), "a negative patch ptr")
    # variant 2 = [4, 99) is [4, 8); variant 3 starts past total and is empty
    run([flat[0:2], flat[2:4], flat[4:8], []], lambda t: t["pptr"].__setitem__(3, 99), "a patch ptr start past total")
    # indices that name no cell are ignored
    run([flat[0:1], flat[2:4], flat[4:5], flat[6:8]],
        lambda t: (t["pindex"].__setitem__(1, -1), t["pindex"].__setitem__(5, n * n)), "patch indices -1 and n*n")
    # items: src = n, dst = -1 keep their sentinels; a ptr past total is clamped; a descending pair asks nothing
    run(plists, lambda t: (t["src"].__setitem__(4, n), t["dst"].__setitem__(7, -1)), "an item with src = n, one with dst = -1",
        skip_items=(4, 7))
    run(plists, lambda t: t["iptr"].__setitem__(4, 12 + 9), "an item ptr past total")

    def descending_items(t):
        t["iptr"][2] = 2                           # variant 1 = [3, 2): nothing; variant 2 = [2, 9): items 2 .. 8
    want, us = _oracle(base, 2, plists, 2)
    got = run_dev(base, 2, plists, ilists, patch_fields=2, mutate=descending_items)
    flat_items = [q for v in ilists for q in v]
    for q, (s, d) in enumerate(flat_items):
        owner = 0 if q < 3 else 2 if 2 <= q < 9 else 3          # item 2 is asked by variants 0 and 2; 3 .. 5 by 2 only
        if q == 2:
            continue                               # two variants write it: either answer is one of the two
        for f in range(3):
            assert_bits_equal(got[1][f][q:q + 1], np.array([want[f][owner, s, d]], dtype=got[1][f].dtype),
                              "a descending item ptr pair: item %d, %s" % (q, FIELD_NAMES[f]))
    assert got[2] == us


# ---- host form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 16, 64, 120])
def test_host_form_matches_the_device_form_on_the_market_case(n):
    """64 variants of a market matrix, each multiplying one quote by 4 (the quote and its inverse: two entries); four
    items a variant, the patched pair among them."""
    count = 64
    base = _base("d2", n, "float64")
    rnd = np.random.default_rng(41 * n)
    r = base[0]
    plists, ilists = [], []
    for b in range(count):
        i = int(rnd.integers(n))
        j = (i + 1 + int(rnd.integers(n - 1))) % n
        plists.append([(i * n + j, r[i, j] * 4.0, j, 1), (j * n + i, r[j, i] / 4.0, i, 1)])
        ilists.append([(i, j), (j, i)] + [(int(rnd.integers(n)), int(rnd.integers(n))) for _ in range(2)])
    want, us = _oracle(base, 2, plists, 2)
    plain, _ = _oracle(base, 2, [[]], 0)
    # not vacuous, stated on the ORACLE's results
    assert min(us) > 0, "the oracle relaxes nothing in variant %d" % int(np.argmin(us))
    moved = sum(any(want[0][b, s, d].tobytes() != plain[0][0, s, d].tobytes() for s, d in ilists[b]) for b in range(count))
    assert 2 * moved >= count, "only %d of %d variants move an answer" % (moved, count)

    what = "market n=%d" % n
    dev_got = run_dev(base, 2, plists, ilists, patch_fields=2, full=False)
    _check(dev_got, want, us, n, ilists, what + " device form")
    res, each = engine.solve_sweep(
        base[0], base[1], base[2],
        patches=[tuple(np.array([p[k] for p in v]) for k in range(4)) for v in plists],
        items=[(np.array([q[0] for q in v]), np.array([q[1] for q in v])) for v in ilists], count_updates=True)
    q = 0
    for b in range(count):
        assert len(res[b]) == 3
        for f in range(3):
            assert_bits_equal(res[b][f], dev_got[1][f][q:q + 4], "%s: host form against device form, variant %d %s" % (
                what, b, FIELD_NAMES[f]))
            assert_bits_equal(res[b][f], np.array([want[f][b, s, d] for s, d in ilists[b]], dtype=res[b][f].dtype),
                              "%s: host form against the oracle, variant %d %s" % (what, b, FIELD_NAMES[f]))
        q += 4
    assert [int(u) for u in each] == us


def test_host_form_updates_out_is_the_sum_and_f32_rates_only():
    import ctypes
    from floydwarshall_amd import _lib
    n, count = 16, 5
    base = _base("t1", n, "float32")
    rnd = np.random.default_rng(77)
    plists = _six_variants(base, n, rnd)[1:]
    ilists = _items_for(n, count, rnd, skip=())
    want, us = _oracle(base, 0, plists, 0)
    res, each = engine.solve_sweep(base[0], patches=[(np.array([p[0] for p in v]), np.array([p[1] for p in v]))
                                                     for v in plists],
                                   items=[(np.array([q[0] for q in v]), np.array([q[1] for q in v])) for v in ilists],
                                   count_updates=True)
    for b in range(count):
        assert len(res[b]) == 1
        assert_bits_equal(res[b][0], np.array([want[0][b, s, d] for s, d in ilists[b]], dtype=np.float32), "variant %d" % b)
    assert [int(u) for u in each] == us
    # opts->updates_out: the sum, with and without updates_each
    pptr = _csr(plists)
    pindex = np.array([p[0] for v in plists for p in v], dtype=np.int64)
    prate = np.array([p[1] for v in plists for p in v], dtype=np.float32)
    p = _lib.FwxSweepPatches(pptr.ctypes.data, int(pptr[-1]), pindex.ctypes.data, prate.ctypes.data, None, None)
    total = ctypes.c_uint64(123)
    o = _lib.FwxOpts()
    o.struct_size, o.device, o.updates_out = ctypes.sizeof(_lib.FwxOpts), -1, ctypes.pointer(total)
    rc = _lib.lib().fwx_solve_sweep_f32(count, n, base[0].ctypes.data, None, None, ctypes.byref(p), None, None,
                                        ctypes.byref(o))
    assert rc == _lib.FWX_OK and total.value == sum(us)
