"""What-if sweeps up to order 256 on the GPU (fwx_dev_solve_sweep_mid, fwx_solve_sweep_mid_*): `count` variants of ONE
base matrix, built and solved in workspace slots -- a fixed grid of workgroups, each walking its share of the variants
through one slot of scratch.  Every output -- the queried entries, the full matrices where asked for (diagonals
included) and U -- is bit for bit what the oracle's loop (oracle.relax) leaves of M_b, which is built here on the CPU
with numpy: a copy of the base, the patches in order.

The device form runs with guard bands of a sentinel around every output, every table, the base and the scratch: what
the call may write is written, nothing else is, the base comes back as it went in, and of the scratch -- handed over
larger than needed -- everything past slots x FWX_SWEEP_MID_SCRATCH_BYTES(n) still holds the sentinel.

The input builders and the guard bands are those of test_gpu_sweep.py.  Orders 129 ... 256 cover the 64-column
geometry of the mid tier (cw 192 -> 256, rgs 5 -> 4, the idle wave at 192); FWX_BATCH_MID_MIN_N = 1 puts orders 1 ...
128 through the same kernel for the edges of the 16-pivot blocks."""
import numpy as np
import pytest

from floydwarshall_amd import _lib, engine, hip

from helpers import assert_bits_equal
from hostile_inputs import hostile_matrix_mix
from test_gpu_sweep import (FIELD_NAMES, INT_SENTINEL, RATE_SENTINEL, Guarded, _base, _check, _csr, _items_for,
                            _oracle, _sentinel, _six_variants)
from test_gpu_sweep import run_dev as run_dev_small

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
MID_ORDERS = [129, 130, 191, 192, 193, 255, 256]          # the 64-column geometry edges
BLOCK_ORDERS = [1, 2, 15, 16, 17, 33, 64, 65, 128]        # the 16-pivot block edges, under FWX_BATCH_MID_MIN_N=1
SCRATCH_SENTINEL = 0xA5
SPARE = 1000                                               # bytes of scratch past the last whole slot handed over


# ---- the device form under guard bands -------------------------------------------------------------------------------
def run_dev(base, fields, plists, ilists, *, patch_fields=0, full=True, stride=None, upd_start=None, mutate=None,
            item_fields=None, scratch_slots=None, null_scratch=False):
    """fwx_dev_solve_sweep_mid on the first fields + 1 arrays of `base`, with a scratch of scratch_slots slots
    (default: two more than there are variants) plus SPARE bytes.  Returns (full arrays stacked or None, item outputs
    flat over all items, updates, slots) -- slots = the grid the hook reports for this call; every guard band, the
    base, the tables and the unused part of the scratch are checked on the way."""
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
    per_slot = _lib.sweep_mid_scratch_bytes(n)
    scratch_slots = count + 2 if scratch_slots is None else scratch_slots
    scratch = Guarded(np.full(scratch_slots * per_slot + SPARE, SCRATCH_SENTINEL, dtype=np.uint8), 0x5A)
    assert scratch.view.data_ptr() % 16 == 0
    routed = n >= _lib.lib().fwx_test_batch_mid_min_n()
    slots = _lib.lib().fwx_test_sweep_mid_slots(count, n, scratch.view.numel()) if routed else 0
    v = lambda x: None if x is None else x.view
    patches = (g["pptr"].view, g["pindex"].view, g["prate"].view, v(g["pnext"]) if patch_fields >= 1 else None,
               v(g["phops"]) if patch_fields >= 2 else None)
    items = (g["iptr"].view, g["src"].view, g["dst"].view, v(outs[0]), v(outs[1]), v(outs[2]))
    kw = dict(base_next_t=v(gbase[1]), base_hops_t=v(gbase[2]), patches=patches if len(t["pindex"]) else None,
              items=items if total_items else None,
              full=(v(fulls[0]), v(fulls[1]), v(fulls[2]), stride) if full else None, updates_t=upd.view)
    if null_scratch and not routed:           # a forwarded order: the binding allocates nothing and passes NULL, 0
        assert engine.dev_solve_sweep_mid(gbase[0].view, count, n, scratch_t=None, **kw) is None
    elif null_scratch:                        # the binding's own scratch: the slots the hook reports, no more
        own = engine.dev_solve_sweep_mid(gbase[0].view, count, n, scratch_t=None, **kw)
        want_slots = _lib.lib().fwx_test_sweep_mid_slots(count, n, count * per_slot)
        assert own.numel() * own.element_size() == want_slots * per_slot
        slots = 0                             # the guarded scratch was not handed over: all of it stays the sentinel
    else:
        engine.dev_solve_sweep_mid(gbase[0].view, count, n, scratch_t=scratch.view, **kw)
    hip.synchronize()
    for k, arr in g.items():
        assert_bits_equal(arr.read(k), t[k], "the table %s" % k)
    for f in range(3):
        if gbase[f] is not None:
            assert_bits_equal(gbase[f].read("base " + FIELD_NAMES[f]), base[f], "the base's %s" % FIELD_NAMES[f])
    rest = scratch.read("scratch")[slots * per_slot:]
    assert_bits_equal(rest, np.full(rest.shape, SCRATCH_SENTINEL, dtype=np.uint8),
                      "the scratch past %d slots of %d bytes" % (slots, per_slot))
    got_items = [None if o is None else o.read("item " + FIELD_NAMES[f]) for f, o in enumerate(outs)]
    got_full = [None if o is None else o.read("full " + FIELD_NAMES[f]).reshape(count, stride)
                for f, o in enumerate(fulls)]
    return got_full, got_items, [int(u) for u in upd.read("updates")], slots


def _oracle_fields(base, plists):
    """The oracle's results for the six (fields, patch_fields) combinations from three solves of each variant: rate
    and next do not depend on hops, rate on neither, so (2, 2) / (2, 1) / (2, 0) hold the others as their first
    arrays.  {(fields, patch_fields): (want, us)}."""
    out = {}
    for pf in (2, 1, 0):
        out[(2, pf)] = _oracle(base, 2, plists, pf)
    for fields, pf in ((1, 1), (1, 0), (0, 0)):
        want, us = out[(2, pf)]
        out[(fields, pf)] = ([want[f] if f <= fields else None for f in range(3)], us)
    return out


def _six_variant_case(n, dtype, kind, what):
    base = _base(kind, n, np.dtype(dtype).name)
    rnd = np.random.default_rng(100 * n + len(kind))
    plists = _six_variants(base, n, rnd)
    ilists = _items_for(n, 6, rnd)
    plain, plain_u = _oracle(base, 2, [[]], 0)
    wants = _oracle_fields(base, plists)
    for (fields, patch_fields), (want, us) in sorted(wants.items()):
        w = "%s fields=%d patch_fields=%d" % (what, fields, patch_fields)
        for f in range(fields + 1):         # variant 0 has no patches: the plain solve of the base
            assert_bits_equal(want[f][0], plain[f][0], w + ": the oracle itself")
        assert us[0] == plain_u[0]
        if n >= 4:
            assert min(us) > 0, "%s: the oracle relaxes nothing in variant %d" % (w, int(np.argmin(us)))
        if n >= 129:                        # at least two patched variants solve to other rates than variant 0
            moved = sum(want[0][b].tobytes() != want[0][0].tobytes() for b in range(1, 6))
            assert moved >= 2, "%s: only %d patched variants differ from the base's solve" % (w, moved)
        got = run_dev(base, fields, plists, ilists, patch_fields=patch_fields)
        _check(got[:3], want, us, n, ilists, w)
        assert got[3] == 6, "%s: %d slots for six variants and eight slots of scratch" % (w, got[3])


# ---- orders, fields ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["d2", "t1"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", MID_ORDERS)
def test_six_variants_full_outputs_and_items(n, dtype, kind):
    _six_variant_case(n, dtype, kind, "n=%d %s %s" % (n, np.dtype(dtype).name, kind))


@pytest.mark.parametrize("kind", ["d2", "t1"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", BLOCK_ORDERS)
def test_six_variants_at_the_pivot_block_edges(n, dtype, kind, monkeypatch):
    monkeypatch.setenv("FWX_BATCH_MID_MIN_N", "1")
    _six_variant_case(n, dtype, kind, "mid from 1, n=%d %s %s" % (n, np.dtype(dtype).name, kind))


# ---- slot reuse --------------------------------------------------------------------------------------------------------
def _seven_variants(n):
    base = _base("d2", n, "float64")
    rnd = np.random.default_rng(100 * n + 7)
    plists = _six_variants(base, n, rnd)
    r = base[0]
    plists.append([(1 * n + 2, r[1, 2] * 32.0, 2, 1), (2 * n + 1, r[2, 1] / 32.0, 1, 1)])
    ilists = _items_for(n, 7, rnd, skip=())
    return base, plists, ilists


_SEVEN = {}


def _seven_oracle(n):
    if n not in _SEVEN:
        base, plists, ilists = _seven_variants(n)
        _SEVEN[n] = (base, plists, ilists) + _oracle(base, 2, plists, 2)
    return _SEVEN[n]


@pytest.mark.parametrize("how", ["scratch", "env"])
@pytest.mark.parametrize("count,slots", [(1, 1), (7, 1), (7, 2), (7, 3), (5, 8)])
def test_a_slot_is_rebuilt_for_every_variant_it_serves(count, slots, how, monkeypatch):
    """(count, slots) by sizing the scratch, or by FWX_SWEEP_MID_SLOTS over a scratch of 9 slots.  A slot that kept
    the previous variant's solved matrix would relax almost nothing: U per variant tells, and so does every cell."""
    n = 130
    base, plists, ilists, want, us = _seven_oracle(n)
    assert min(us) > 0
    if how == "env":
        monkeypatch.setenv("FWX_SWEEP_MID_SLOTS", str(slots))
    want_c = [w[:count] for w in want]
    got = run_dev(base, 2, plists[:count], ilists[:count], patch_fields=2,
                  scratch_slots=slots if how == "scratch" else 9)
    assert got[3] == min(count, slots), "the hook reports %d slots" % got[3]
    _check(got[:3], want_c, us[:count], n, ilists[:count], "count=%d slots=%d by %s" % (count, slots, how))


def test_no_result_bit_depends_on_the_slot_count(monkeypatch):
    n = 130
    base, plists, ilists, want, us = _seven_oracle(n)
    runs = []
    for slots in ("1", "3", "7", "garbage"):
        monkeypatch.setenv("FWX_SWEEP_MID_SLOTS", slots)
        runs.append(run_dev(base, 2, plists, ilists, patch_fields=2, scratch_slots=9))
    assert [r[3] for r in runs] == [1, 3, 7, 7]
    for r in runs[1:]:
        for f in range(3):
            assert_bits_equal(r[0][f], runs[0][0][f], "full %s" % FIELD_NAMES[f])
            assert_bits_equal(r[1][f], runs[0][1][f], "item %s" % FIELD_NAMES[f])
        assert r[2] == runs[0][2] == us


@pytest.mark.parametrize("cap", [None, "3"])
def test_the_binding_allocates_the_slots_the_call_will_use(cap, monkeypatch):
    """dev_solve_sweep_mid(scratch_t=None) at a routed order: min(count, FWX_SWEEP_MID_SLOTS) slots, the same results."""
    n = 130
    base, plists, ilists, want, us = _seven_oracle(n)
    if cap:
        monkeypatch.setenv("FWX_SWEEP_MID_SLOTS", cap)
    else:
        monkeypatch.delenv("FWX_SWEEP_MID_SLOTS", raising=False)
    got = run_dev(base, 2, plists, ilists, patch_fields=2, null_scratch=True)
    _check(got[:3], want, us, n, ilists, "the binding's own scratch, FWX_SWEEP_MID_SLOTS=%s" % cap)


def test_more_variants_than_the_default_slot_count(monkeypatch):
    """600 variants of n = 20 on the mid kernel: 512 slots, 88 of them serve a second variant."""
    monkeypatch.setenv("FWX_BATCH_MID_MIN_N", "1")
    monkeypatch.delenv("FWX_SWEEP_MID_SLOTS", raising=False)
    n, count = 20, 600
    base = _base("d2", n, "float64")
    rnd = np.random.default_rng(2000 + n)
    r = base[0]
    plists = []
    for b in range(count):
        i = int(rnd.integers(n))
        j = (i + 1 + int(rnd.integers(n - 1))) % n
        plists.append([(i * n + j, r[i, j] * (2.0 + b % 5), j, 1), (j * n + i, r[j, i] * 0.5, i, 1)])
    ilists = [v[:4] for v in _items_for(n, count, rnd, skip=())]
    want, us = _oracle(base, 2, plists, 2)
    assert min(us) > 0
    got = run_dev(base, 2, plists, ilists, patch_fields=2)
    assert got[3] == 512
    _check(got[:3], want, us, n, ilists, "600 variants of n=20")


# ---- hostile values ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", [129, 256])
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
        # three slots for nine variants: the hostile cells of one variant must not survive into the next
        got = run_dev(base, fields, plists, ilists, patch_fields=patch_fields, scratch_slots=3)
        _check(got[:3], want, us, n, ilists, what)


# ---- items only, strides, U ------------------------------------------------------------------------------------------
def test_items_only_writes_the_item_outputs_and_nothing_else():
    n = 200
    base = _base("d2", n, "float64")
    rnd = np.random.default_rng(31 * n)
    plists = _six_variants(base, n, rnd)
    ilists = _items_for(n, 6, rnd)
    want, us = _oracle(base, 2, plists, 2)
    _check(run_dev(base, 2, plists, ilists, patch_fields=2, full=False)[:3], want, us, n, ilists, "items only n=%d" % n)
    _check(run_dev(base, 2, plists, ilists, patch_fields=2, full=False, item_fields=0, scratch_slots=4)[:3], want, us,
           n, ilists, "items only, rate_out alone, n=%d" % n)


def test_full_outputs_with_a_gap_and_counters_on_a_nonzero_start():
    n = 131
    base = _base("t1", n, "float32")
    rnd = np.random.default_rng(17 * n)
    plists = _six_variants(base, n, rnd)
    ilists = _items_for(n, 6, rnd)
    want, us = _oracle(base, 2, plists, 2)
    assert min(us) > 0
    start = [5, 0, 1 << 40, 7, 9, 11]
    got = run_dev(base, 2, plists, ilists, patch_fields=2, stride=n * n + 13, upd_start=start, scratch_slots=4)
    _check(got[:3], want, us, n, ilists, "stride n*n+13, n=%d" % n, start=start)
    # no patches at all, no items at all: every variant is the base
    plain, plain_u = _oracle(base, 2, [[], [], []], 0)
    _check(run_dev(base, 2, [[], [], []], [[], [], []], scratch_slots=2)[:3], plain, plain_u, n, [[], [], []],
           "patches NULL, items NULL")


# ---- tables that do not belong ---------------------------------------------------------------------------------------
def test_tables_that_do_not_belong_are_passed_over():
    """The clamp cases of the small sweep at n = 130, two slots for four variants: each case states the lists a
    correct kernel acts on, and the arrays keep their true extents, so nothing here reaches a bad address."""
    n = 130
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
        _check(run_dev(base, 2, plists, ilists, patch_fields=2, mutate=mutate, scratch_slots=2)[:3], want, us, n, ilists,
               what, skip_items=skip_items)

    run([flat[0:2], [], flat[1:6], flat[6:8]], lambda t: t["pptr"].__setitem__(2, 1), "a descending patch ptr pair")
    run(plists, lambda t: t["pptr"].__setitem__(4, 8 + 5), "a patch ptr past total")
    run([[], flat[0:4], flat[4:6], flat[6:8]], lambda t: t["pptr"].__setitem__(1, -3), "a negative patch ptr")
    run([flat[0:2], flat[2:4], flat[4:8], []], lambda t: t["pptr"].__setitem__(3, 99), "a patch ptr start past total")
    run([flat[0:1], flat[2:4], flat[4:5], flat[6:8]],
        lambda t: (t["pindex"].__setitem__(1, -1), t["pindex"].__setitem__(5, n * n)), "patch indices -1 and n*n")
    run(plists, lambda t: (t["src"].__setitem__(4, n), t["dst"].__setitem__(7, -1)),
        "an item with src = n, one with dst = -1", skip_items=(4, 7))
    run(plists, lambda t: t["iptr"].__setitem__(4, 12 + 9), "an item ptr past total")

    def descending_items(t):
        t["iptr"][2] = 2                           # variant 1 = [3, 2): nothing; variant 2 = [2, 9): items 2 .. 8
    want, us = _oracle(base, 2, plists, 2)
    got = run_dev(base, 2, plists, ilists, patch_fields=2, mutate=descending_items, scratch_slots=2)
    flat_items = [q for v in ilists for q in v]
    for q, (s, d) in enumerate(flat_items):
        owner = 0 if q < 3 else 2 if 2 <= q < 9 else 3          # item 2 is asked by variants 0 and 2; 3 .. 5 by 2 only
        if q == 2:
            continue                               # two variants write it: either answer is one of the two
        for f in range(3):
            assert_bits_equal(got[1][f][q:q + 1], np.array([want[f][owner, s, d]], dtype=got[1][f].dtype),
                              "a descending item ptr pair: item %d, %s" % (q, FIELD_NAMES[f]))
    assert got[2] == us


# ---- default routing ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 128])
def test_orders_below_the_mid_tier_are_forwarded_and_need_no_scratch(n, monkeypatch):
    monkeypatch.delenv("FWX_BATCH_MID_MIN_N", raising=False)
    base = _base("d2", n, "float64")
    rnd = np.random.default_rng(53 * n)
    plists = _six_variants(base, n, rnd)
    ilists = _items_for(n, 6, rnd)
    want, us = _oracle(base, 2, plists, 2)
    small = run_dev_small(base, 2, plists, ilists, patch_fields=2)
    _check(small, want, us, n, ilists, "fwx_dev_solve_sweep n=%d" % n)
    for null in (True, False):              # NULL, and a scratch that must stay the sentinel from its first byte
        got = run_dev(base, 2, plists, ilists, patch_fields=2, null_scratch=null)
        assert got[3] == 0
        for f in range(3):
            assert_bits_equal(got[0][f], small[0][f], "full %s against fwx_dev_solve_sweep" % FIELD_NAMES[f])
            assert_bits_equal(got[1][f], small[1][f], "item %s against fwx_dev_solve_sweep" % FIELD_NAMES[f])
        assert got[2] == small[2]


# ---- host form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [144, 256])
def test_host_form_matches_the_device_form_on_the_market_case(n):
    """64 variants of a market matrix, each multiplying one quote by 4 (the quote and its inverse: two entries); four
    items a variant, the patched pair among them."""
    import ctypes
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
    dev_got = run_dev(base, 2, plists, ilists, patch_fields=2, full=False, scratch_slots=24)
    _check(dev_got[:3], want, us, n, ilists, what + " device form")
    p_arg = [tuple(np.array([p[k] for p in v]) for k in range(4)) for v in plists]
    i_arg = [(np.array([q[0] for q in v]), np.array([q[1] for q in v])) for v in ilists]
    res, each = engine.solve_sweep_mid(base[0], base[1], base[2], patches=p_arg, items=i_arg, count_updates=True)
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
    # opts->updates_out: the sum, without updates_each
    pptr = _csr(plists)
    pindex = np.array([p[0] for v in plists for p in v], dtype=np.int64)
    prate = np.array([p[1] for v in plists for p in v], dtype=np.float64)
    p = _lib.FwxSweepPatches(pptr.ctypes.data, int(pptr[-1]), pindex.ctypes.data, prate.ctypes.data, None, None)
    total = ctypes.c_uint64(123)
    o = _lib.FwxOpts()
    o.struct_size, o.device, o.updates_out = ctypes.sizeof(_lib.FwxOpts), -1, ctypes.pointer(total)
    rc = _lib.lib().fwx_solve_sweep_mid_f64(count, n, base[0].ctypes.data, None, None, ctypes.byref(p), None, None,
                                            ctypes.byref(o))
    assert rc == _lib.FWX_OK and total.value == sum(us)       # U is decided by the rates alone
