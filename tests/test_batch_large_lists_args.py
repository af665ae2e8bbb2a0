"""Batched large solves with the exact `_path` lists (fwx_dev_solve_batch_large_traced, fwx_dev_exact_paths_batch_large,
fwx_solve_batch_large_lists_f64 / _f32): the symbols exist, and every status rule of include/fwx.h is decided before any
device call -- the rules of the mid family (tests/test_batch_mid_lists_args.py) with the limit at
FWX_BATCH_LARGE_MAX_N = 1024, plus the scratch of the traced device solve, which is judged only where the order is
routed to the large tier (tests/test_batch_large_args.py).  CPU only: no launch is made here."""
import ctypes

import numpy as np
import pytest

from floydwarshall_amd import _lib, engine

OK, INVALID, UNSUPPORTED, NO_DEVICE = (_lib.FWX_OK, _lib.FWX_ERR_INVALID, _lib.FWX_ERR_UNSUPPORTED,
                                      _lib.FWX_ERR_NO_DEVICE)
HOST = {np.float64: "fwx_solve_batch_large_lists_f64", np.float32: "fwx_solve_batch_large_lists_f32"}
DTYPES = [np.float64, np.float32]
FAKE = ctypes.c_void_p(4096)        # a device pointer that is never dereferenced; 16-byte aligned
PLENTY = 1 << 30
BUDGET = 64 << 20                   # bytes of lists + stacks + item arrays per launch, as include/fwx.h states it
MAX_N = 1024
NO_GPU = pytest.mark.skipif(engine.device_count() > 0, reason="only meaningful without a GPU")


def _batch(count, n, dtype):
    rate = np.full((count, n, n), 0.5, dtype=dtype)
    nxt = np.tile(np.arange(n, dtype=np.int32), (count, n, 1))
    hops = np.ones((count, n, n), dtype=np.int32)
    return rate, nxt, hops


def _items(k, cap):
    z = np.zeros(k, dtype=np.int32)
    return {"mat": z.copy(), "src": z.copy(), "dst": z.copy() + 1, "len": np.full(k, -99, dtype=np.int32),
            "path": np.full((max(k, 1), max(cap, 1)), -7, dtype=np.int32)}


def _opts(**kw):
    o = _lib.FwxOpts()
    o.struct_size = ctypes.sizeof(_lib.FwxOpts)
    o.device = -1
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _host(dtype, count, n, rate, nxt, hops, items=0, it=None, cap=4, each=None, opts=None, **null):
    """The host form; it: the dict of _items, a key named in `null` is passed as NULL."""
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    arr = {k: (None if it is None or null.get(k) else it[k]) for k in ("mat", "src", "dst", "len", "path")}
    return getattr(_lib.lib(), HOST[dtype])(count, n, p(rate), p(nxt), p(hops), p(each), items, p(arr["mat"]),
                                            p(arr["src"]), p(arr["dst"]), p(arr["len"]), p(arr["path"]), cap,
                                            None if opts is None else ctypes.byref(opts))


def _trace(last=FAKE, at_col=FAKE, at_row=FAKE):
    t = _lib.FwxTrace()
    t.last, t.at_col, t.at_row = last, at_col, at_row
    return t


def _traced(count, n, code, rate=FAKE, nxt=FAKE, hops=FAKE, stride=None, trace="fake", scratch=FAKE,
            scratch_bytes=PLENTY):
    tr = _trace() if trace == "fake" else trace
    return _lib.lib().fwx_dev_solve_batch_large_traced(count, n, code, rate, nxt, hops,
                                                       n * n if stride is None else stride,
                                                       None if tr is None else ctypes.byref(tr), None, scratch,
                                                       scratch_bytes, None)


def _walk(count, n, items, stride=None, next0=FAKE, trace="fake", mat=FAKE, src=FAKE, dst=FAKE, lens=FAKE,
          paths=FAKE, cap=4, scratch=FAKE):
    tr = _trace() if trace == "fake" else trace
    return _lib.lib().fwx_dev_exact_paths_batch_large(count, n, n * n if stride is None else stride, next0,
                                                      None if tr is None else ctypes.byref(tr), items, mat, src, dst,
                                                      lens, paths, cap, scratch, None)


def test_the_symbols_are_exported_and_bound():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("fwx_dev_solve_batch_large_traced", "fwx_dev_exact_paths_batch_large",
                 "fwx_solve_batch_large_lists_f64", "fwx_solve_batch_large_lists_f32"):
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.lib().fwx_abi_version() == 3           # symbols are only added
    assert _lib.FWX_BATCH_LARGE_MAX_N == MAX_N
    for name in ("solve_batch_large_lists", "dev_solve_batch_large_traced", "dev_exact_paths_batch_large"):
        assert name in engine.__all__ and callable(getattr(engine, name))


@pytest.mark.parametrize("n", [4, 300])
@pytest.mark.parametrize("dtype", DTYPES)
def test_host_form_rejects_bad_arguments_before_any_device_call(dtype, n):
    rate, nxt, hops = _batch(2, n, dtype)
    before = rate.copy(), nxt.copy(), hops.copy()
    it = _items(3, 4)
    assert _host(dtype, -1, n, rate, nxt, hops, 3, it) == INVALID                   # count < 0
    assert _host(dtype, 2, -1, rate, nxt, hops, 3, it) == INVALID                   # n < 0
    assert _host(dtype, 2, n, rate, nxt, hops, -1, it) == INVALID                   # items < 0
    assert _host(dtype, 0, n, rate, nxt, hops, -1, it) == INVALID                   # negative beats zero
    assert _host(dtype, -1, 0, rate, nxt, hops, 3, it) == INVALID
    assert _host(dtype, 2, n, None, nxt, hops, 3, it) == INVALID                    # no rates
    assert _host(dtype, 2, n, rate, None, None, 3, it) == INVALID                   # the lists need next
    assert _host(dtype, 2, n, rate, None, None, 0, None) == INVALID                 # ... also without items
    assert _host(dtype, 2, n, rate, None, hops, 3, it) == INVALID                   # hops without next
    for cap in (0, -1):
        assert _host(dtype, 2, n, rate, nxt, hops, 3, it, cap=cap) == INVALID       # cap < 1 with items
    for key in ("mat", "src", "dst", "len", "path"):
        assert _host(dtype, 2, n, rate, nxt, hops, 3, it, **{key: True}) == INVALID, key   # a NULL item array
    assert _host(dtype, 2, n, rate, nxt, hops, 3, it, opts=_opts(struct_size=4)) == INVALID
    for kb, ke in ((3, 2), (-1, n), (0, n + 1), (n + 1, 0), (1, 0), (1, n), (0, n - 1), (2, 3)):   # only [0, n) is traced
        assert _host(dtype, 2, n, rate, nxt, hops, 3, it, opts=_opts(k_begin=kb, k_end=ke)) == INVALID, (kb, ke)
    assert _host(dtype, 2, n, rate, nxt, hops, 3, it, opts=_opts(engine=99)) == INVALID
    for eng in (_lib.FWX_ENGINE_PERK, _lib.FWX_ENGINE_FUSED):
        assert _host(dtype, 2, n, rate, nxt, hops, 3, it, opts=_opts(engine=eng)) == UNSUPPORTED, eng
    for got, want in zip((rate, nxt, hops), before):
        assert np.array_equal(got, want)
    assert (it["len"] == -99).all() and (it["path"] == -7).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_form_at_the_limit(dtype):
    """1025 is refused; a pivot range at a large order is INVALID, and comes before the order (as batch_range orders
    them for the untraced calls)."""
    it = _items(3, 4)
    big = np.zeros((1, MAX_N + 1, MAX_N + 1), dtype=dtype)
    bign = np.zeros((1, MAX_N + 1, MAX_N + 1), dtype=np.int32)
    assert _host(dtype, 1, MAX_N + 1, big, bign, None, 3, it) == UNSUPPORTED
    assert _host(dtype, 1, MAX_N + 1, big, bign, None, 0, None) == UNSUPPORTED
    assert _host(dtype, 1, MAX_N + 1, big, bign, None, 3, it, opts=_opts(k_begin=1, k_end=MAX_N + 1)) == INVALID
    for n in (257, MAX_N):
        rate, nxt, hops = big[:, :n, :n].copy(), bign[:, :n, :n].copy(), bign[:, :n, :n].copy()
        for kb, ke in ((1, n), (0, n - 1), (0, 256), (16, 32)):
            assert _host(dtype, 1, n, rate, nxt, hops, 3, it, opts=_opts(k_begin=kb, k_end=ke)) == INVALID, (n, kb, ke)
        for eng in (_lib.FWX_ENGINE_PERK, _lib.FWX_ENGINE_FUSED):
            assert _host(dtype, 1, n, rate, nxt, hops, 3, it, opts=_opts(engine=eng)) == UNSUPPORTED
    assert (it["len"] == -99).all() and (it["path"] == -7).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_batches_are_success_and_touch_nothing(dtype):
    rate, nxt, hops = _batch(2, 4, dtype)
    before = rate.copy(), nxt.copy(), hops.copy()
    it = _items(3, 4)
    each = np.full(2, 77, dtype=np.uint64)
    total = ctypes.c_uint64(55)
    o = _opts(updates_out=ctypes.pointer(total))
    assert _host(dtype, 0, 4, rate, nxt, hops, 3, it, each=each, opts=o) == OK
    assert _host(dtype, 0, 600, rate, nxt, hops, 3, it, each=each, opts=o) == OK
    assert _host(dtype, 2, 0, rate, nxt, hops, 3, it, each=each, opts=o) == OK
    assert _host(dtype, 0, 0, None, None, None) == OK
    assert _host(dtype, 0, 4096, None, None, None) == OK                            # nothing to solve, whatever n
    for got, want in zip((rate, nxt, hops), before):
        assert np.array_equal(got, want)
    assert list(each) == [77, 77] and total.value == 55
    assert (it["len"] == -99).all() and (it["path"] == -7).all()


def test_traced_device_solve_rejects_bad_arguments_before_any_device_call():
    for code in (_lib.FWX_F32, _lib.FWX_F64):
        for n in (4, 129, 256, 257, 600, MAX_N):
            assert _traced(-1, n, code) == INVALID
            assert _traced(2, n, code, rate=None) == INVALID
            assert _traced(2, n, code, nxt=None, hops=None) == INVALID                  # the trace needs next
            assert _traced(2, n, code, nxt=None) == INVALID                             # hops without next
            assert _traced(2, n, code, trace=None) == INVALID
            for hole in ("last", "at_col", "at_row"):
                assert _traced(2, n, code, trace=_trace(**{hole: None})) == INVALID, hole
            assert _traced(2, n, code, stride=n * n - 1) == INVALID                     # stride < n*n
            assert _traced(2, n, code, stride=-n * n) == INVALID
        assert _traced(2, -1, code) == INVALID
        assert _traced(1, MAX_N + 1, code) == UNSUPPORTED
        assert _traced(1, MAX_N + 1, code, scratch=None, scratch_bytes=0) == UNSUPPORTED   # the order is judged first
        assert _traced(1, MAX_N + 1, code, stride=4) == INVALID                         # INVALID comes first
        assert _traced(0, 4, code, rate=None, nxt=None, hops=None, trace=None, scratch=None, scratch_bytes=0) == OK
        assert _traced(2, 0, code, rate=None, nxt=None, hops=None, trace=None, scratch=None, scratch_bytes=0) == OK
        assert _traced(0, 600, code, rate=None, nxt=None, hops=None, trace=None, scratch=None, scratch_bytes=0) == OK
    assert _traced(2, 4, 7) == INVALID                                                  # no such dtype
    assert _traced(2, 600, 7) == INVALID
    assert _traced(2, 600, 7, scratch=None) == INVALID


@pytest.mark.parametrize("n", [257, 600, MAX_N])
def test_bad_scratch_is_invalid_when_the_traced_solve_is_routed_to_the_large_tier(n, monkeypatch):
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    per = _lib.batch_large_scratch_bytes(n)
    for code in (_lib.FWX_F32, _lib.FWX_F64):
        assert _traced(2, n, code, scratch=None) == INVALID                                        # NULL
        assert _traced(2, n, code, scratch=None, scratch_bytes=0) == INVALID
        for misaligned in (4097, 4100, 4104, 4111):
            assert _traced(2, n, code, scratch=ctypes.c_void_p(misaligned)) == INVALID, misaligned
        assert _traced(2, n, code, scratch_bytes=per - 1) == INVALID                               # less than one
        assert _traced(2, n, code, scratch_bytes=0) == INVALID
        assert _traced(2, n, code, hops=None, scratch_bytes=per - 1) == INVALID                    # the value is fixed


@NO_GPU
def test_scratch_of_the_traced_solve_is_judged_only_where_it_is_used(monkeypatch):
    """Past every check the call reports FWX_ERR_NO_DEVICE: bad scratch passes where the order is forwarded to the mid
    traced entry point, and only there; FWX_BATCH_LARGE_SCRATCH_BYTES(n) for one matrix is enough."""
    bad = dict(scratch=None, scratch_bytes=0)
    monkeypatch.delenv("FWX_BATCH_LARGE_MIN_N", raising=False)
    for code in (_lib.FWX_F32, _lib.FWX_F64):
        for n in (1, 5, 128, 129, 256):                                          # below the default threshold
            assert _traced(2, n, code, **bad) == NO_DEVICE, n
            assert _traced(2, n, code, scratch=ctypes.c_void_p(4097), scratch_bytes=3) == NO_DEVICE
        for n in (257, 600, MAX_N):
            assert _traced(2, n, code, **bad) == INVALID
            assert _traced(2, n, code, scratch_bytes=_lib.batch_large_scratch_bytes(n)) == NO_DEVICE, n
            assert _traced(2, n, code, stride=n * n + 7, hops=None) == NO_DEVICE, n
    monkeypatch.setenv("FWX_BATCH_LARGE_MIN_N", "1")                             # now everything is routed there
    for n in (1, 5, 256):
        assert _traced(2, n, _lib.FWX_F64, **bad) == INVALID, n
        assert _traced(2, n, _lib.FWX_F64, scratch_bytes=_lib.batch_large_scratch_bytes(n) - 1) == INVALID, n
        assert _traced(2, n, _lib.FWX_F64, scratch_bytes=_lib.batch_large_scratch_bytes(n)) == NO_DEVICE, n
    monkeypatch.setenv("FWX_BATCH_LARGE_MIN_N", "6")
    assert _traced(2, 5, _lib.FWX_F64, **bad) == NO_DEVICE
    assert _traced(2, 6, _lib.FWX_F64, **bad) == INVALID


def test_device_walk_rejects_bad_arguments_before_any_device_call():
    for n in (4, 129, 257, 600, MAX_N):
        assert _walk(-1, n, 3) == INVALID
        assert _walk(2, n, -1) == INVALID
        assert _walk(2, n, 3, next0=None) == INVALID
        assert _walk(2, n, 3, trace=None) == INVALID
        for hole in ("last", "at_col", "at_row"):
            assert _walk(2, n, 3, trace=_trace(**{hole: None})) == INVALID, hole
        assert _walk(2, n, 3, stride=n * n - 1) == INVALID
        for cap in (0, -1):
            assert _walk(2, n, 3, cap=cap) == INVALID
        for key in ("mat", "src", "dst", "lens", "paths", "scratch"):
            assert _walk(2, n, 3, **{key: None}) == INVALID, key
        assert _walk(2, n, 0, mat=None, src=None, dst=None, lens=None, paths=None, cap=0, scratch=None) == OK
    assert _walk(2, -1, 3) == INVALID
    assert _walk(1, MAX_N + 1, 3) == UNSUPPORTED
    assert _walk(1, MAX_N + 1, 3, stride=4) == INVALID
    assert _walk(0, 4, 3, next0=None, trace=None) == OK
    assert _walk(2, 0, 3, next0=None, trace=None) == OK


def test_the_mid_entry_points_keep_their_limit():
    """257 is the large family's alone."""
    L = _lib.lib()
    for code in (_lib.FWX_F32, _lib.FWX_F64):
        tr = _trace()
        assert L.fwx_dev_solve_batch_mid_traced(1, 257, code, FAKE, FAKE, FAKE, 257 * 257, ctypes.byref(tr), None,
                                                None) == UNSUPPORTED
        assert L.fwx_dev_solve_batch_traced(1, 257, code, FAKE, FAKE, FAKE, 257 * 257, ctypes.byref(tr), None,
                                            None) == UNSUPPORTED
    tr = _trace()
    assert L.fwx_dev_exact_paths_batch_mid(1, 257, 257 * 257, FAKE, ctypes.byref(tr), 3, FAKE, FAKE, FAKE, FAKE, FAKE, 4,
                                           FAKE, None) == UNSUPPORTED
    assert L.fwx_dev_exact_paths_batch(1, 257, 257 * 257, FAKE, ctypes.byref(tr), 3, FAKE, FAKE, FAKE, FAKE, FAKE, 4,
                                       FAKE, None) == UNSUPPORTED
    it = _items(3, 4)
    for dtype, stem in ((np.float64, "f64"), (np.float32, "f32")):
        rate = np.zeros((1, 257, 257), dtype=dtype)
        nxt = np.zeros((1, 257, 257), dtype=np.int32)
        p = lambda a: a.ctypes.data  # noqa: E731
        for name in ("fwx_solve_batch_mid_lists_", "fwx_solve_batch_lists_"):
            assert getattr(L, name + stem)(1, 257, p(rate), p(nxt), None, None, 3, p(it["mat"]), p(it["src"]),
                                           p(it["dst"]), p(it["len"]), p(it["path"]), 4, None) == UNSUPPORTED, name
    assert (it["len"] == -99).all() and (it["path"] == -7).all()


@NO_GPU
@pytest.mark.parametrize("n", [5, 129, 257, 600, MAX_N])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_valid_call_without_a_device_reports_it_and_leaves_the_arrays_alone(dtype, n):
    rate, nxt, hops = _batch(2, n, dtype)
    rate[1, 2, 3] = np.nan
    before = rate.copy(), nxt.copy(), hops.copy()
    it = _items(4, 6)
    each = np.full(2, 9, dtype=np.uint64)
    assert _host(dtype, 2, n, rate, nxt, hops, 4, it, cap=6, each=each) == NO_DEVICE
    assert _host(dtype, 2, n, rate, nxt, None, 4, it, cap=6, each=each) == NO_DEVICE     # hops absent
    assert _host(dtype, 2, n, rate, nxt, hops, 0, None, each=each) == NO_DEVICE          # a plain batch solve
    for kw in ({"cap": 6}, {"items": ([0], [1], [2]), "cap": 6}):
        with pytest.raises(engine.FwxError) as e:
            engine.solve_batch_large_lists(rate, nxt, hops, count_updates=True, **kw)
        assert e.value.status == NO_DEVICE
    bits = np.uint64 if dtype == np.float64 else np.uint32
    assert np.array_equal(rate.view(bits), before[0].view(bits))
    assert np.array_equal(nxt, before[1]) and np.array_equal(hops, before[2])
    assert list(each) == [9, 9]
    assert (it["len"] == -99).all() and (it["path"] == -7).all()
    assert _walk(2, n, 4) == NO_DEVICE
    assert _walk(2, n, 4, stride=n * n + 7) == NO_DEVICE


def test_python_binding_checks_shapes():
    rate, nxt, hops = _batch(2, 4, np.float64)
    with pytest.raises(ValueError):
        engine.solve_batch_large_lists(rate, None)                     # the lists need next
    with pytest.raises(ValueError):
        engine.solve_batch_large_lists(rate[0], nxt[0])                # one matrix is not a batch
    with pytest.raises(ValueError):
        engine.solve_batch_large_lists(rate, nxt[:, :, :3])
    with pytest.raises(ValueError):
        engine.solve_batch_large_lists(rate.astype(np.float16), nxt)
    with pytest.raises(ValueError):
        engine.solve_batch_large_lists(rate, nxt, items=([0, 1], [0], [1]))
    assert engine.solve_batch_large_lists(np.zeros((0, 600, 600)), np.zeros((0, 600, 600), dtype=np.int32)) == []
    with pytest.raises(engine.FwxError) as e:
        engine.solve_batch_large_lists(np.zeros((1, 1025, 1025)), np.zeros((1, 1025, 1025), dtype=np.int32),
                                       items=([0], [0], [1]), cap=4)
    assert e.value.status == UNSUPPORTED


# ---- the walk's chunk at the new orders ---------------------------------------------------------------
def _chunk(n, cap):
    return int(_lib.lib().fwx_test_batch_lists_chunk(n, cap))


def _fit(n, cap):
    """Items whose lists (cap), stacks (FWX_EXACT_SCRATCH_INTS(n) = 3 (n + 2)) and item arrays (4) fit the budget."""
    return max(1, BUDGET // (4 * (cap + 3 * (n + 2) + 4)))


@pytest.mark.parametrize("n,cap", [(257, 1), (257, 4098), (600, 64), (1023, 4096), (1024, 1), (1024, 8), (1024, 4098),
                                   (1024, 1 << 16), (1024, 1 << 20), (1024, 2**31 - 1)])
def test_chunk_default_is_what_the_budget_holds(n, cap, monkeypatch):
    monkeypatch.delenv("FWX_BATCH_LISTS_CHUNK", raising=False)
    c = _chunk(n, cap)
    assert c == _fit(n, cap) >= 1
    assert c == 1 or c * 4 * (cap + 3 * (n + 2) + 4) <= BUDGET
    assert c < 2**31
