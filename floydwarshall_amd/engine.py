"""Python binding over the libfwx C ABI (include/fwx.h).

This is plumbing for the tests, the benchmark and the multi-GPU driver: numpy arrays for the
host-buffer entry points, raw device pointers for the device step API.  Device memory is owned by
floydwarshall_amd.hip.DeviceArray (the HIP runtime through ctypes: no torch in the process, so libfwx
runs on the runtime it was built against) or, for floydwarshall_amd.dist, by torch tensors; every
function here takes either and allocates its outputs like its inputs.
The functions mirror the reference's seam, floydWarshall = runAlgo 0 . buildMatrix
(/root/reference/src/lib/Algorithms.hs:19-20): `solve` IS runAlgo on the dense form.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import (FWX_ENGINE_AUTO, FWX_ENGINE_FUSED, FWX_ENGINE_PERK, FWX_F32, FWX_F64,
                   FWX_FUSED_BLOCK, FWX_UPDATE_SHARDS, FWX_XCHG_AUTO, FWX_XCHG_PEER, FWX_XCHG_RCCL,
                   FWX_ERR_RCCL, FwxError, FwxOpts, FwxPivots, FwxSlab, check, lib)

__all__ = ["solve", "solve_batch", "dev_solve_batch", "solve_batch_lists", "dev_solve_batch_traced",
           "dev_exact_paths_batch", "solve_batch_mid", "dev_solve_batch_mid", "solve_batch_mid_lists",
           "solve_batch_large", "dev_solve_batch_large", "solve_batch_large_lists", "dev_solve_batch_large_traced",
           "dev_exact_paths_batch_large",
           "dev_solve_batch_mid_traced", "dev_exact_paths_batch_mid", "ragged_plan", "solve_ragged", "solve_ragged_lists", "dev_solve_ragged",
           "dev_exact_paths_ragged", "ragged_mid_plan", "solve_ragged_mid", "solve_ragged_mid_lists",
           "dev_solve_ragged_mid", "dev_exact_paths_ragged_mid", "ragged_large_plan", "solve_ragged_large",
           "solve_ragged_large_lists", "dev_solve_ragged_large", "dev_exact_paths_ragged_large", "follow_path", "dev_follow_paths", "dev_check_nonneg", "dev_domain_bits", "dev_solve_fused",
           "dev_solve", "DeviceMatrix", "dev_relax", "dev_panel", "dev_panel_snap",
           "dev_relax_fused", "FusedWorkspace", "Trace", "FWX_FUSED_BLOCK", "device_count",
           "FwxError", "FWX_ENGINE_AUTO", "FWX_ENGINE_PERK", "FWX_ENGINE_FUSED",
           "FWX_UPDATE_SHARDS", "solve_multi", "FWX_XCHG_AUTO", "FWX_XCHG_PEER", "FWX_XCHG_RCCL", "FWX_ERR_RCCL"]


def device_count():
    return lib().fwx_device_count()


# Launch forms the test hook fwx_test_kernel_forms records, in bit order (FWX_KERNEL_FORM_LIST in
# csrc/fwx_kernels.h): bit i of the mask is KERNEL_FORMS[i].
KERNEL_FORMS = (
    "SMALL_SOLVE", "RELAX_K",
    "ROWPANEL_F32", "ROWPANEL_F64", "COLPANEL_F32", "COLPANEL_F64",
    "PANELS_F32", "PANELS_F64", "PANELS_MAX_F32", "PANELS_MAX_F64",
    "PANELS_NEXT_F32", "PANELS_NEXT_TRACE_F32", "PANELS_NEXT_F32_R32",
    "MAIN_SMALL_F32", "MAIN_LARGE_F32", "MAIN_SMALL_F64", "MAIN_LARGE_F64",
    "MAX_SMALL_F32", "MAX_MID_F32", "MAX_LARGE_F32",
    "ARG_RI4_NP1_F32", "ARG_RI4_NP2_F32", "ARG_RI8_NP1_F32", "ARG_RI8_NP2_F32",
    "MAX_SMALL_F64", "MAX_LARGE_F64",
    "ARG_F64_RI4_NP1", "ARG_F64_RI4_NP2", "ARG_F64_RI2_NP1", "ARG_F64_RI2_NP2",
)


def kernel_forms_seen(reset=False):
    """Names of the launch forms this process has used since the last reset (test hook)."""
    seen = ctypes.c_uint64(0)
    count = lib().fwx_test_kernel_forms(ctypes.byref(seen), 1 if reset else 0)
    assert count == len(KERNEL_FORMS), (count, len(KERNEL_FORMS))
    return {name for i, name in enumerate(KERNEL_FORMS) if seen.value >> i & 1}


def _np_ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _check_arrays(rate, nxt, hops):
    if not (isinstance(rate, np.ndarray) and rate.ndim == 2 and rate.shape[0] == rate.shape[1]):
        raise ValueError("rate must be a square 2-D numpy array")
    if rate.dtype not in (np.float32, np.float64) or not rate.flags.c_contiguous:
        raise ValueError("rate must be C-contiguous float32 or float64")
    for name, a in (("next", nxt), ("hops", hops)):
        if a is not None and not (isinstance(a, np.ndarray) and a.shape == rate.shape
                                  and a.dtype == np.int32 and a.flags.c_contiguous):
            raise ValueError("%s must be a C-contiguous int32 array shaped like rate" % name)
    if hops is not None and nxt is None:
        raise ValueError("hops requires next")


def _opts(device=-1, engine=FWX_ENGINE_AUTO, k_begin=0, k_end=0, block=0, serpentine=True,
          want_updates=False, stream=None):
    """fwx_opts.  stream: a hip.Stream / torch stream handle the (still blocking) call runs on instead
    of a library-owned non-blocking stream."""
    o = FwxOpts()
    o.struct_size = ctypes.sizeof(FwxOpts)
    o.device, o.engine, o.k_begin, o.k_end, o.block = device, engine, k_begin, k_end, block
    o.serpentine = 0 if serpentine else 1
    u = ctypes.c_uint64(0)
    if want_updates:
        o.updates_out = ctypes.pointer(u)
    if stream is not None:
        o.stream = _stream_ptr(stream)
        o.use_stream = 1
    return o, u


def solve(rate, nxt=None, hops=None, *, device=-1, engine=FWX_ENGINE_AUTO, k_begin=0, k_end=0,
          block=0, serpentine=True, count_updates=False):
    """runAlgo (Algorithms.hs:42-61) in place on host numpy arrays, on the GPU.

    Returns U (number of successful relaxations) if count_updates else None."""
    _check_arrays(rate, nxt, hops)
    o, u = _opts(device, engine, k_begin, k_end, block, serpentine, count_updates)
    fn = lib().fwx_solve_f64 if rate.dtype == np.float64 else lib().fwx_solve_f32
    check(fn(rate.shape[0], _np_ptr(rate), _np_ptr(nxt), _np_ptr(hops), ctypes.byref(o)),
          "fwx_solve")
    return int(u.value) if count_updates else None


def solve_batch(rate, nxt=None, hops=None, *, device=-1, k_begin=0, k_end=0, count_updates=False):
    """runAlgo on every matrix of a batch in ONE launch (fwx_solve_batch_f64 / _f32): rate.shape ==
    (count, n, n) with n <= FWX_BATCH_MAX_N, C-contiguous host numpy arrays, solved in place; nxt / hops
    shaped alike.  Every matrix comes back as `solve` of that matrix alone would leave it.

    Returns the per-matrix U as a uint64 array of `count` entries if count_updates else None."""
    return _solve_batch("fwx_solve_batch", rate, nxt, hops, device, k_begin, k_end, count_updates)


def solve_batch_mid(rate, nxt=None, hops=None, *, device=-1, k_begin=0, k_end=0, count_updates=False):
    """solve_batch with the limit at n <= FWX_BATCH_MID_MAX_N (fwx_solve_batch_mid_f64 / _f32): orders from
    FWX_BATCH_MID_MIN_N (environment, default 129) up run the mid tier -- one workgroup per matrix, the matrix
    resident in device memory -- and smaller ones are forwarded to solve_batch's tiers.  Same arrays, same
    results, same return value."""
    return _solve_batch("fwx_solve_batch_mid", rate, nxt, hops, device, k_begin, k_end, count_updates)


def solve_batch_large(rate, nxt=None, hops=None, *, device=-1, k_begin=0, k_end=0, count_updates=False):
    """solve_batch_mid with the limit at n <= FWX_BATCH_LARGE_MAX_N (fwx_solve_batch_large_f64 / _f32): orders from
    FWX_BATCH_LARGE_MIN_N (environment, default 257) up run the large tier -- several workgroups per matrix, two
    launches per 16 pivots over the whole batch -- and smaller ones are forwarded to solve_batch_mid's routing.  Same
    arrays, same results, same return value."""
    return _solve_batch("fwx_solve_batch_large", rate, nxt, hops, device, k_begin, k_end, count_updates)


def _solve_batch(stem, rate, nxt, hops, device, k_begin, k_end, count_updates):
    if not (isinstance(rate, np.ndarray) and rate.ndim == 3 and rate.shape[1] == rate.shape[2]):
        raise ValueError("rate must be a numpy array of shape (count, n, n)")
    if rate.dtype not in (np.float32, np.float64) or not rate.flags.c_contiguous:
        raise ValueError("rate must be C-contiguous float32 or float64")
    for name, a in (("next", nxt), ("hops", hops)):
        if a is not None and not (isinstance(a, np.ndarray) and a.shape == rate.shape
                                  and a.dtype == np.int32 and a.flags.c_contiguous):
            raise ValueError("%s must be a C-contiguous int32 array shaped like rate" % name)
    if hops is not None and nxt is None:
        raise ValueError("hops requires next")
    count, n = rate.shape[0], rate.shape[1]
    o, _ = _opts(device, FWX_ENGINE_AUTO, k_begin, k_end)
    each = np.zeros(count, dtype=np.uint64) if count_updates else None
    fn = getattr(lib(), stem + ("_f64" if rate.dtype == np.float64 else "_f32"))
    check(fn(count, n, _np_ptr(rate), _np_ptr(nxt), _np_ptr(hops), _np_ptr(each), ctypes.byref(o)), stem)
    return each


def dev_solve_batch(rate_t, count, n, *, next_t=None, hops_t=None, stride=None, k_begin=0, k_end=0,
                    updates_t=None, stream=None):
    """fwx_dev_solve_batch: `count` matrices of order n <= FWX_BATCH_MAX_N held in the device array rate_t,
    matrix b at element b * stride (default n * n; the gap is never touched), next_t / hops_t alike, solved
    in place by one launch, asynchronously on `stream` (default: as dev_relax).  updates_t: device array
    of `count` 64-bit counters, counter b is incremented by U of matrix b."""
    _dev_solve_batch("fwx_dev_solve_batch", rate_t, count, n, next_t, hops_t, stride, k_begin, k_end, updates_t,
                     stream)


def dev_solve_batch_mid(rate_t, count, n, *, next_t=None, hops_t=None, stride=None, k_begin=0, k_end=0,
                        updates_t=None, stream=None):
    """fwx_dev_solve_batch_mid: dev_solve_batch with the limit at n <= FWX_BATCH_MID_MAX_N; routing by
    FWX_BATCH_MID_MIN_N as solve_batch_mid.  Same arrays, same results."""
    _dev_solve_batch("fwx_dev_solve_batch_mid", rate_t, count, n, next_t, hops_t, stride, k_begin, k_end, updates_t,
                     stream)


def dev_solve_batch_large(rate_t, count, n, *, next_t=None, hops_t=None, stride=None, k_begin=0, k_end=0,
                          updates_t=None, scratch_t=None, stream=None):
    """fwx_dev_solve_batch_large: dev_solve_batch_mid with the limit at n <= FWX_BATCH_LARGE_MAX_N; routing by
    FWX_BATCH_LARGE_MIN_N as solve_batch_large.  scratch_t: a device array of at least
    _lib.batch_large_scratch_bytes(n) bytes, 16-byte aligned -- the call solves as many matrices at a time as it
    holds; None: one for the whole batch is allocated here.  Returns the scratch array: it must stay alive until the
    stream has run the call."""
    if scratch_t is None:
        scratch_t = _empty_like_device(rate_t, (max(count, 1) * _lib.batch_large_scratch_bytes(n),), "uint8")
    _dev_solve_batch("fwx_dev_solve_batch_large", rate_t, count, n, next_t, hops_t, stride, k_begin, k_end, updates_t,
                     stream, scratch_t)
    return scratch_t


def _dev_solve_batch(name, rate_t, count, n, next_t, hops_t, stride, k_begin, k_end, updates_t, stream,
                     scratch_t=None):
    stride = n * n if stride is None else int(stride)
    need = (count - 1) * stride + n * n if count > 0 else 0
    assert rate_t.is_cuda and rate_t.is_contiguous() and rate_t.numel() >= need
    for t in (next_t, hops_t):
        assert t is None or (t.is_cuda and t.is_contiguous() and _dtype_name(t) == "int32"
                             and t.numel() >= need)
    assert updates_t is None or (updates_t.element_size() == 8 and updates_t.numel() >= count)
    vp = ctypes.c_void_p
    check(getattr(lib(), name)(
        count, n, _tensor_dtype_code(rate_t), vp(rate_t.data_ptr()),
        vp(next_t.data_ptr()) if next_t is not None else None,
        vp(hops_t.data_ptr()) if hops_t is not None else None, stride, k_begin, k_end,
        vp(updates_t.data_ptr()) if updates_t is not None else None,
        *(() if scratch_t is None else (vp(scratch_t.data_ptr()), scratch_t.numel() * scratch_t.element_size())),
        _stream_ptr(stream, rate_t)), name)


def _sweep_csr(per_variant, count, what):
    """(ptr int64[count + 1], the per-variant tuples with empty ones as ()) of a per-variant list."""
    if per_variant is None:
        per_variant = [()] * count
    if len(per_variant) != count:
        raise ValueError("%s must have one entry per variant" % what)
    rows = [() if v is None else tuple(np.atleast_1d(np.asarray(a)) for a in v) for v in per_variant]
    ptr = np.zeros(count + 1, dtype=np.int64)
    for b, v in enumerate(rows):
        if v and any(a.shape != v[0].shape or a.ndim != 1 for a in v):
            raise ValueError("the arrays of %s[%d] must be 1-D and equally long" % (what, b))
        ptr[b + 1] = ptr[b] + (len(v[0]) if v else 0)
    return ptr, rows


def solve_sweep(base_rate, base_next=None, base_hops=None, *, patches, items, device=-1, count_updates=False):
    """A what-if sweep in ONE call (fwx_solve_sweep_f64 / _f32): variant b is base_rate (n x n, n <=
    FWX_SWEEP_MAX_N; base_next / base_hops alike) with patches[b] applied in order, solved whole; only the entries
    items[b] asks for come back.  The base is not written.

    patches: per variant None / () or (index, rate[, next[, hops]]) -- index = i * n + j, a later patch of a cell wins;
    next / hops must be given by every variant that has patches, or by none (then that field of a patched cell
    keeps the base's value).  items: per variant None / () or (src, dst).  len(patches) == len(items) == count
    (either may be None: no patches / no items at all).

    Returns a list with, per variant, the tuple (rate[, next[, hops]]) of arrays over its items (next with base_next,
    hops with base_hops); with count_updates (that list, the per-variant U as a uint64 array)."""
    return _solve_sweep("fwx_solve_sweep", base_rate, base_next, base_hops, patches, items, device, count_updates)


def solve_sweep_mid(base_rate, base_next=None, base_hops=None, *, patches, items, device=-1, count_updates=False):
    """solve_sweep with the limit at n <= FWX_SWEEP_MID_MAX_N (fwx_solve_sweep_mid_f64 / _f32): orders from
    FWX_BATCH_MID_MIN_N (environment, default 129) up are built and solved in workspace slots on the device, one per
    workgroup, whatever the number of variants; smaller ones take solve_sweep's path.  Same arguments, same results,
    same return value."""
    return _solve_sweep("fwx_solve_sweep_mid", base_rate, base_next, base_hops, patches, items, device, count_updates)


def _solve_sweep(stem, base_rate, base_next, base_hops, patches, items, device, count_updates):
    _check_arrays(base_rate, base_next, base_hops)
    if patches is None and items is None:
        raise ValueError("patches or items must say how many variants there are")
    count = len(patches) if patches is not None else len(items)
    n = base_rate.shape[0]
    pptr, prow = _sweep_csr(patches, count, "patches")
    iptr, irow = _sweep_csr(items, count, "items")
    widths = {len(v) for v in prow if v}
    if len(widths) > 1 or (widths and not 2 <= min(widths) <= 4):
        raise ValueError("every patch list is (index, rate[, next[, hops]]), the same fields in all variants")
    if any(len(v) != 2 for v in irow if v):
        raise ValueError("every item list is (src, dst)")
    width = widths.pop() if widths else 2

    def cat(rows, k, dtype):
        parts = [v[k] for v in rows if v]
        return np.ascontiguousarray(np.concatenate(parts), dtype=dtype) if parts else np.zeros(0, dtype=dtype)

    p = _lib.FwxSweepPatches()
    p_arrays = [pptr, cat(prow, 0, np.int64), cat(prow, 1, base_rate.dtype),
                cat(prow, 2, np.int32) if width >= 3 else None, cat(prow, 3, np.int32) if width >= 4 else None]
    p.ptr, p.total = pptr.ctypes.data, int(pptr[-1])
    p.index, p.rate = p_arrays[1].ctypes.data, p_arrays[2].ctypes.data
    p.next = p_arrays[3].ctypes.data if p_arrays[3] is not None else None
    p.hops = p_arrays[4].ctypes.data if p_arrays[4] is not None else None
    it = _lib.FwxSweepItems()
    total = int(iptr[-1])
    src, dst = cat(irow, 0, np.int32), cat(irow, 1, np.int32)
    out = [np.zeros(total, dtype=base_rate.dtype),
           np.zeros(total, dtype=np.int32) if base_next is not None else None,
           np.zeros(total, dtype=np.int32) if base_hops is not None else None]
    it.ptr, it.total, it.src, it.dst, it.rate_out = iptr.ctypes.data, total, src.ctypes.data, dst.ctypes.data, \
        out[0].ctypes.data
    it.next_out = out[1].ctypes.data if out[1] is not None else None
    it.hops_out = out[2].ctypes.data if out[2] is not None else None
    o, _ = _opts(device, FWX_ENGINE_AUTO)
    each = np.zeros(count, dtype=np.uint64) if count_updates else None
    fn = getattr(lib(), stem + ("_f64" if base_rate.dtype == np.float64 else "_f32"))
    check(fn(count, n, _np_ptr(base_rate), _np_ptr(base_next), _np_ptr(base_hops), ctypes.byref(p), ctypes.byref(it),
             _np_ptr(each), ctypes.byref(o)), stem)
    res = [tuple(a[iptr[b]:iptr[b + 1]] for a in out if a is not None) for b in range(count)]
    return (res, each) if count_updates else res


def dev_solve_sweep(base_rate_t, count, n, *, base_next_t=None, base_hops_t=None, patches=None, items=None, full=None,
                    updates_t=None, stream=None):
    """fwx_dev_solve_sweep on device arrays (torch tensors or hip.DeviceArray), asynchronously on `stream` (default: as
    dev_relax): `count` variants of the base (n x n, n <= FWX_SWEEP_MAX_N, never written).

    patches: None or (ptr, index, rate[, next[, hops]]) -- ptr int64[count + 1], index int64, rate as the base, next /
    hops int32 or None; the total is index's length.  items: None or (ptr, src, dst, rate_out[, next_out[,
    hops_out]]) -- src / dst int32, the total is src's length; the outputs are written in place.  full: None or
    (rate, next, hops, stride) with any of the three None; variant b's solved n x n part goes to + b * stride.
    updates_t: device array of `count` 64-bit counters, counter b is incremented by U of variant b."""
    _dev_solve_sweep("fwx_dev_solve_sweep", base_rate_t, count, n, base_next_t, base_hops_t, patches, items, full,
                     updates_t, stream)


def dev_solve_sweep_mid(base_rate_t, count, n, *, base_next_t=None, base_hops_t=None, patches=None, items=None,
                        full=None, updates_t=None, scratch_t=None, stream=None):
    """fwx_dev_solve_sweep_mid: dev_solve_sweep with the limit at n <= FWX_SWEEP_MID_MAX_N; routing by
    FWX_BATCH_MID_MIN_N as solve_sweep_mid.  scratch_t: a device array of at least _lib.sweep_mid_scratch_bytes(n)
    bytes, 16-byte aligned -- the call runs min(count, slots it holds, FWX_SWEEP_MID_SLOTS) workgroups, one slot each;
    None: one for min(count, FWX_SWEEP_MID_SLOTS) slots is allocated here, and none where the order is forwarded to
    dev_solve_sweep's tiers, which use no scratch.  Returns the scratch array (None where none was needed): it must
    stay alive until the stream has run the call."""
    if scratch_t is None and 0 < n <= _lib.FWX_SWEEP_MID_MAX_N and count > 0 and \
            n >= lib().fwx_test_batch_mid_min_n():
        per_slot = _lib.sweep_mid_scratch_bytes(n)
        slots = lib().fwx_test_sweep_mid_slots(count, n, count * per_slot)
        scratch_t = _empty_like_device(base_rate_t, (slots * per_slot,), "uint8")
    _dev_solve_sweep("fwx_dev_solve_sweep_mid", base_rate_t, count, n, base_next_t, base_hops_t, patches, items, full,
                     updates_t, stream, scratch_t if scratch_t is not None else _NO_SCRATCH)
    return scratch_t


class _NoScratch:
    """scratch = NULL, scratch_bytes = 0, in the shape _dev_solve_sweep reads a device array."""

    def data_ptr(self):
        return None

    def numel(self):
        return 0

    def element_size(self):
        return 1


_NO_SCRATCH = _NoScratch()


def _dev_solve_sweep(name, base_rate_t, count, n, base_next_t, base_hops_t, patches, items, full, updates_t, stream,
                     scratch_t=None):
    """scratch_t None: the entry point takes no scratch arguments (fwx_dev_solve_sweep)."""
    def ptr_of(t):
        return None if t is None else t.data_ptr()

    def ints(t, name, least):
        assert t is None or (t.is_cuda and t.is_contiguous() and _dtype_name(t) == name and t.numel() >= least), name
        return t

    assert base_rate_t.is_cuda and base_rate_t.is_contiguous() and base_rate_t.numel() >= n * n
    rate_name = _dtype_name(base_rate_t)
    ints(base_next_t, "int32", n * n), ints(base_hops_t, "int32", n * n)
    p = it = fu = None
    if patches is not None:
        t = tuple(patches) + (None,) * (5 - len(patches))
        total = int(t[1].numel())
        ints(t[0], "int64", count + 1), ints(t[1], "int64", total), ints(t[2], rate_name, total)
        ints(t[3], "int32", total), ints(t[4], "int32", total)
        p = _lib.FwxSweepPatches()
        p.ptr, p.total, p.index, p.rate, p.next, p.hops = ptr_of(t[0]), total, ptr_of(t[1]), ptr_of(t[2]), \
            ptr_of(t[3]), ptr_of(t[4])
    if items is not None:
        t = tuple(items) + (None,) * (6 - len(items))
        total = int(t[1].numel())
        ints(t[0], "int64", count + 1), ints(t[1], "int32", total), ints(t[2], "int32", total)
        ints(t[3], rate_name, total), ints(t[4], "int32", total), ints(t[5], "int32", total)
        it = _lib.FwxSweepItems()
        it.ptr, it.total, it.src, it.dst, it.rate_out, it.next_out, it.hops_out = ptr_of(t[0]), total, ptr_of(t[1]), \
            ptr_of(t[2]), ptr_of(t[3]), ptr_of(t[4]), ptr_of(t[5])
    if full is not None:
        stride = int(full[3])
        need = (count - 1) * stride + n * n if count > 0 else 0
        ints(full[0], rate_name, need), ints(full[1], "int32", need), ints(full[2], "int32", need)
        fu = _lib.FwxSweepFull()
        fu.rate, fu.next, fu.hops, fu.stride = ptr_of(full[0]), ptr_of(full[1]), ptr_of(full[2]), stride
    assert updates_t is None or (updates_t.element_size() == 8 and updates_t.numel() >= count)
    vp = ctypes.c_void_p
    check(getattr(lib(), name)(
        count, n, _tensor_dtype_code(base_rate_t), vp(base_rate_t.data_ptr()), ptr_of(base_next_t), ptr_of(base_hops_t),
        ctypes.byref(p) if p is not None else None, ctypes.byref(it) if it is not None else None,
        ctypes.byref(fu) if fu is not None else None, vp(updates_t.data_ptr()) if updates_t is not None else None,
        *(() if scratch_t is None else (vp(scratch_t.data_ptr()), scratch_t.numel() * scratch_t.element_size())),
        _stream_ptr(stream, base_rate_t)), name)


# solve_batch_lists with cap=None: the first capacity tried, and the last (the lists of an input with arbitrage
# grow with every pivot; past this bound the caller states the cap).
BATCH_LISTS_FIRST_CAP = 64
BATCH_LISTS_MAX_CAP = 1 << 16


def solve_batch_lists(rate, nxt, hops=None, *, items=None, cap=None, device=-1, count_updates=False):
    """solve_batch over the whole pivot range and, in the same call, the reference's exact `_path` lists
    (fwx_solve_batch_lists_f64 / _f32): rate.shape == (count, n, n), nxt required, arrays solved in place.

    items: (mat, src, dst) -- three equally long int32 sequences, item q asks for list (src[q], dst[q]) of matrix
    mat[q]; None means all n * n pairs of every matrix, in the order (b, i, j).
    cap: entries per list.  None: start at BATCH_LISTS_FIRST_CAP and, while an item reports
    FWX_ERR_CAPACITY, double it and ask again for the items that did not fit (the batch is solved again from a
    kept copy of the input), up to BATCH_LISTS_MAX_CAP; a list longer than that raises FwxError.  With
    an explicit cap a list that does not fit raises FwxError at once, as does an item outside the batch.

    Returns the lists as a list of tuples, one per item -- or (lists, U) with U the per-matrix uint64 array if
    count_updates."""
    return _solve_batch_lists("fwx_solve_batch_lists", rate, nxt, hops, items, cap, device, count_updates)


def solve_batch_mid_lists(rate, nxt, hops=None, *, items=None, cap=None, device=-1, count_updates=False):
    """solve_batch_lists with the limit at n <= FWX_BATCH_MID_MAX_N (fwx_solve_batch_mid_lists_f64 / _f32); routing
    by FWX_BATCH_MID_MIN_N as solve_batch_mid.  Same arrays, same lists, same return value."""
    return _solve_batch_lists("fwx_solve_batch_mid_lists", rate, nxt, hops, items, cap, device, count_updates)


def solve_batch_large_lists(rate, nxt, hops=None, *, items=None, cap=None, device=-1, count_updates=False):
    """solve_batch_mid_lists with the limit at n <= FWX_BATCH_LARGE_MAX_N (fwx_solve_batch_large_lists_f64 / _f32);
    routing by FWX_BATCH_LARGE_MIN_N as solve_batch_large.  Same arrays, same lists, same return value."""
    return _solve_batch_lists("fwx_solve_batch_large_lists", rate, nxt, hops, items, cap, device, count_updates)


def _solve_batch_lists(stem, rate, nxt, hops, items, cap, device, count_updates):
    if nxt is None:
        raise ValueError("the exact lists need next")
    if not (isinstance(rate, np.ndarray) and rate.ndim == 3 and rate.shape[1] == rate.shape[2]):
        raise ValueError("rate must be a numpy array of shape (count, n, n)")
    if rate.dtype not in (np.float32, np.float64) or not rate.flags.c_contiguous:
        raise ValueError("rate must be C-contiguous float32 or float64")
    for name, a in (("next", nxt), ("hops", hops)):
        if a is not None and not (isinstance(a, np.ndarray) and a.shape == rate.shape
                                  and a.dtype == np.int32 and a.flags.c_contiguous):
            raise ValueError("%s must be a C-contiguous int32 array shaped like rate" % name)
    count, n = rate.shape[0], rate.shape[1]
    if items is None:
        b, i, j = np.meshgrid(np.arange(count, dtype=np.int32), np.arange(n, dtype=np.int32),
                              np.arange(n, dtype=np.int32), indexing="ij")
        items = (b.reshape(-1), i.reshape(-1), j.reshape(-1))
    mat, src, dst = (np.ascontiguousarray(a, dtype=np.int32) for a in items)
    if not (mat.ndim == 1 and mat.shape == src.shape == dst.shape):
        raise ValueError("items must be three equally long one-dimensional sequences (mat, src, dst)")
    fn = getattr(lib(), stem + ("_f64" if rate.dtype == np.float64 else "_f32"))
    grow = cap is None
    cap = BATCH_LISTS_FIRST_CAP if grow else int(cap)
    kept = (rate.copy(), nxt.copy(), None if hops is None else hops.copy()) if grow else None
    each = np.zeros(count, dtype=np.uint64) if count_updates else None
    o, _ = _opts(device, FWX_ENGINE_AUTO)
    out = [None] * len(mat)
    todo = np.arange(len(mat))
    arrays = (rate, nxt, hops)
    while True:
        lens = np.empty(len(todo), dtype=np.int32)
        paths = np.empty((len(todo), cap), dtype=np.int32)
        m, s, d = (np.ascontiguousarray(a[todo]) for a in (mat, src, dst))
        check(fn(count, n, _np_ptr(arrays[0]), _np_ptr(arrays[1]), _np_ptr(arrays[2]),
                 _np_ptr(each) if arrays[0] is rate else None, len(todo), _np_ptr(m), _np_ptr(s), _np_ptr(d),
                 _np_ptr(lens), _np_ptr(paths), cap, ctypes.byref(o)), stem)
        if count == 0 or n == 0:
            lens[:] = _lib.FWX_ERR_INVALID       # nothing was solved: no item lies in the batch
        short = lens == _lib.FWX_ERR_CAPACITY
        bad = (lens < 0) & ~short
        if bad.any():
            raise FwxError(int(lens[bad][0]), "%s: item %d" % (stem, int(todo[bad][0])))
        for q in np.nonzero(~short)[0]:
            out[todo[q]] = tuple(int(v) for v in paths[q, :lens[q]])
        if not short.any():
            break
        if not grow or cap >= BATCH_LISTS_MAX_CAP:
            raise FwxError(_lib.FWX_ERR_CAPACITY, "%s: item %d does not fit cap %d"
                           % (stem, int(todo[short][0]), cap))
        cap, todo = min(2 * cap, BATCH_LISTS_MAX_CAP), todo[short]
        arrays = tuple(None if a is None else a.copy() for a in kept)     # solved again from the input
    return (out, each) if count_updates else out


def _trace_of(trace, need):
    for t in (trace.last, trace.at_col, trace.at_row):
        assert t.is_cuda and t.is_contiguous() and _dtype_name(t) == "int32" and t.numel() >= need
    return ctypes.byref(trace.c_struct())


def dev_solve_batch_traced(rate_t, count, n, trace, *, next_t, hops_t=None, stride=None, updates_t=None,
                           stream=None):
    """fwx_dev_solve_batch_traced: dev_solve_batch over the whole pivot range that also writes the path trace of
    every matrix to `trace` (an object with last / at_col / at_row device int32 arrays, e.g. Trace), laid out like
    next_t: matrix b at element b * stride, pitch n.  Every cell inside a matrix is written, the gaps never."""
    _dev_solve_batch_traced("fwx_dev_solve_batch_traced", rate_t, count, n, trace, next_t, hops_t, stride, updates_t,
                            stream)


def dev_solve_batch_mid_traced(rate_t, count, n, trace, *, next_t, hops_t=None, stride=None, updates_t=None,
                               stream=None):
    """fwx_dev_solve_batch_mid_traced: dev_solve_batch_traced with the limit at n <= FWX_BATCH_MID_MAX_N; routing by
    FWX_BATCH_MID_MIN_N as solve_batch_mid.  Same arrays, same trace."""
    _dev_solve_batch_traced("fwx_dev_solve_batch_mid_traced", rate_t, count, n, trace, next_t, hops_t, stride,
                            updates_t, stream)


def dev_solve_batch_large_traced(rate_t, count, n, trace, *, next_t, hops_t=None, stride=None, updates_t=None,
                                 scratch_t=None, stream=None):
    """fwx_dev_solve_batch_large_traced: dev_solve_batch_mid_traced with the limit at n <= FWX_BATCH_LARGE_MAX_N;
    routing by FWX_BATCH_LARGE_MIN_N as solve_batch_large, scratch_t as dev_solve_batch_large takes it.  Same arrays,
    same trace.  Returns the scratch array: it must stay alive until the stream has run the call."""
    if scratch_t is None:
        scratch_t = _empty_like_device(rate_t, (max(count, 1) * _lib.batch_large_scratch_bytes(n),), "uint8")
    _dev_solve_batch_traced("fwx_dev_solve_batch_large_traced", rate_t, count, n, trace, next_t, hops_t, stride,
                            updates_t, stream, scratch_t)
    return scratch_t


def _dev_solve_batch_traced(name, rate_t, count, n, trace, next_t, hops_t, stride, updates_t, stream, scratch_t=None):
    stride = n * n if stride is None else int(stride)
    need = (count - 1) * stride + n * n if count > 0 else 0
    assert rate_t.is_cuda and rate_t.is_contiguous() and rate_t.numel() >= need
    for t in (next_t, hops_t):
        assert t is None or (t.is_cuda and t.is_contiguous() and _dtype_name(t) == "int32"
                             and t.numel() >= need)
    assert next_t is not None
    assert updates_t is None or (updates_t.element_size() == 8 and updates_t.numel() >= count)
    vp = ctypes.c_void_p
    check(getattr(lib(), name)(
        count, n, _tensor_dtype_code(rate_t), vp(rate_t.data_ptr()), vp(next_t.data_ptr()),
        vp(hops_t.data_ptr()) if hops_t is not None else None, stride, _trace_of(trace, need),
        vp(updates_t.data_ptr()) if updates_t is not None else None,
        *(() if scratch_t is None else (vp(scratch_t.data_ptr()), scratch_t.numel() * scratch_t.element_size())),
        _stream_ptr(stream, rate_t)), name)


def dev_exact_paths_batch(next0_t, count, n, trace, mat_t, src_t, dst_t, cap, *, stride=None, stream=None):
    """fwx_dev_exact_paths_batch: the exact `_path` lists of the items (mat_t[q], src_t[q], dst_t[q]) of a batch that
    dev_solve_batch_traced solved; next0_t is the caller's copy of the UNSOLVED next-hop array (same layout).
    Asynchronous on `stream`.  Returns (len_t, path_t): device int32 arrays of shape (items,) and (items, cap);
    len_t[q] is the length of list q, FWX_ERR_CAPACITY or FWX_ERR_INVALID, item by item."""
    return _dev_exact_paths_batch("fwx_dev_exact_paths_batch", next0_t, count, n, trace, mat_t, src_t, dst_t, cap,
                                  stride, stream)


def dev_exact_paths_batch_mid(next0_t, count, n, trace, mat_t, src_t, dst_t, cap, *, stride=None, stream=None):
    """fwx_dev_exact_paths_batch_mid: dev_exact_paths_batch over a batch that dev_solve_batch_mid_traced solved,
    n <= FWX_BATCH_MID_MAX_N."""
    return _dev_exact_paths_batch("fwx_dev_exact_paths_batch_mid", next0_t, count, n, trace, mat_t, src_t, dst_t, cap,
                                  stride, stream)


def dev_exact_paths_batch_large(next0_t, count, n, trace, mat_t, src_t, dst_t, cap, *, stride=None, stream=None):
    """fwx_dev_exact_paths_batch_large: dev_exact_paths_batch over a batch that dev_solve_batch_large_traced solved,
    n <= FWX_BATCH_LARGE_MAX_N."""
    return _dev_exact_paths_batch("fwx_dev_exact_paths_batch_large", next0_t, count, n, trace, mat_t, src_t, dst_t,
                                  cap, stride, stream)


def _dev_exact_paths_batch(name, next0_t, count, n, trace, mat_t, src_t, dst_t, cap, stride, stream):
    stride = n * n if stride is None else int(stride)
    need = (count - 1) * stride + n * n if count > 0 else 0
    assert next0_t.is_cuda and next0_t.is_contiguous() and _dtype_name(next0_t) == "int32" and next0_t.numel() >= need
    items = mat_t.numel()
    for t in (mat_t, src_t, dst_t):
        assert t.is_cuda and t.is_contiguous() and _dtype_name(t) == "int32" and t.numel() == items
    len_t = _empty_like_device(mat_t, (items,), "int32")
    path_t = _empty_like_device(mat_t, (items, cap), "int32")
    scratch = _empty_like_device(mat_t, (max(items * 3 * (n + 2), 1),), "int32")
    vp = ctypes.c_void_p
    check(getattr(lib(), name)(
        count, n, stride, vp(next0_t.data_ptr()), _trace_of(trace, need), items, vp(mat_t.data_ptr()),
        vp(src_t.data_ptr()), vp(dst_t.data_ptr()), vp(len_t.data_ptr()), vp(path_t.data_ptr()), cap,
        vp(scratch.data_ptr()), _stream_ptr(stream, mat_t)), name)
    if not _is_torch(mat_t):
        len_t._scratch = scratch              # stays alive until the results are read
    return len_t, path_t


def ragged_plan(n_each):
    """fwx_ragged_plan: (offset, order, tier_count) for a ragged batch of the orders n_each -- the packed offsets
    (int64, count + 1 entries, the total last), the matrices with n >= 1 grouped by tier (wave, 64-wide, 128-wide)
    and by descending order within a tier (int32, count entries, -1 past the listed ones), and the three tier
    sizes (int32).  Needs no device."""
    return _ragged_plan("fwx_ragged_plan", 3, n_each)


def ragged_mid_plan(n_each):
    """fwx_ragged_mid_plan: ragged_plan for orders up to FWX_BATCH_MID_MAX_N, with FOUR tiers -- wave, 64-wide,
    128-wide, mid (orders from FWX_BATCH_MID_MIN_N up) -- and four tier sizes.  Needs no device."""
    return _ragged_plan("fwx_ragged_mid_plan", 4, n_each)


def ragged_large_plan(n_each):
    """fwx_ragged_large_plan: ragged_mid_plan for orders up to FWX_BATCH_LARGE_MAX_N, with FIVE tiers -- the fifth the
    large tier, orders from FWX_BATCH_LARGE_MIN_N up -- and the large tier's work table: (offset, order, tier_count,
    work), work an int64 array of shape (3, count + 1), the orders, panel strips and sweep tiles before each slot of
    the large tier's list.  Needs no device."""
    n_each = np.ascontiguousarray(n_each, dtype=np.int32)
    work = np.zeros((3, max(n_each.size, 0) + 1), dtype=np.int64)
    return _ragged_plan("fwx_ragged_large_plan", 5, n_each, work)


def _ragged_plan(name, ntiers, n_each, work=None):
    n_each = np.ascontiguousarray(n_each, dtype=np.int32)
    if n_each.ndim != 1:
        raise ValueError("n_each must be a one-dimensional sequence of orders")
    count = len(n_each)
    offset = np.zeros(count + 1, dtype=np.int64)
    order = np.full(count, -1, dtype=np.int32)
    tiers = np.zeros(ntiers, dtype=np.int32)
    extra = () if work is None else (_np_ptr(work),)
    check(getattr(lib(), name)(count, _np_ptr(n_each), _np_ptr(offset), _np_ptr(order), _np_ptr(tiers), *extra), name)
    return (offset, order, tiers) if work is None else (offset, order, tiers, work)


def _pack_ragged(rates, nexts, hops):
    """Checks a ragged batch given as sequences of square arrays and packs it: (n_each, rate, next, hops), the three
    arrays one-dimensional with matrix b at the sum of the squares before it (next / hops None where not given)."""
    rates = list(rates)
    for r in rates:
        if not (isinstance(r, np.ndarray) and r.ndim == 2 and r.shape[0] == r.shape[1]):
            raise ValueError("every rate must be a square 2-D numpy array")
    dtypes = {r.dtype for r in rates}
    if len(dtypes) > 1:
        raise ValueError("the matrices of a batch must have one dtype")
    dtype = dtypes.pop() if dtypes else np.dtype(np.float64)
    if dtype not in (np.float32, np.float64):
        raise ValueError("rate must be float32 or float64")
    if hops is not None and nexts is None:
        raise ValueError("hops requires next")
    packed = [np.concatenate([r.reshape(-1) for r in rates]) if rates else np.zeros(0, dtype=dtype)]
    for name, seq in (("next", nexts), ("hops", hops)):
        if seq is None:
            packed.append(None)
            continue
        seq = list(seq)
        if len(seq) != len(rates):
            raise ValueError("%s must hold one array per matrix" % name)
        for a, r in zip(seq, rates):
            if not (isinstance(a, np.ndarray) and a.shape == r.shape and a.dtype == np.int32):
                raise ValueError("every %s must be an int32 array shaped like its rate" % name)
        packed.append(np.concatenate([a.reshape(-1) for a in seq]) if seq else np.zeros(0, dtype=np.int32))
    n_each = np.array([r.shape[0] for r in rates], dtype=np.int32)
    return n_each, packed[0], packed[1], packed[2]


def _unpack_ragged(n_each, packed, into):
    """Writes the packed arrays of a ragged batch back into the caller's matrices, in place."""
    for flat, seq in zip(packed, into):
        if flat is None or seq is None:
            continue
        at = 0
        for n, a in zip(n_each, seq):
            a[...] = flat[at:at + int(n) * int(n)].reshape(int(n), int(n))
            at += int(n) * int(n)


def solve_ragged(rates, nexts=None, hops=None, *, device=-1, count_updates=False):
    """runAlgo on every matrix of a RAGGED batch (fwx_solve_ragged_f64 / _f32): rates is a sequence of square host
    numpy arrays of one dtype and of any orders 0 ... FWX_BATCH_MAX_N, nexts / hops sequences of int32 arrays shaped
    alike.  The batch is packed, solved with one launch per tier, and written back in place.  Every matrix comes back
    as `solve` of that matrix alone would leave it.

    Returns the per-matrix U as a uint64 array if count_updates else None."""
    return _solve_ragged("fwx_solve_ragged", rates, nexts, hops, device, count_updates)


def solve_ragged_mid(rates, nexts=None, hops=None, *, device=-1, count_updates=False):
    """solve_ragged with the limit at FWX_BATCH_MID_MAX_N (fwx_solve_ragged_mid_f64 / _f32): orders 0 ... 256 in one
    call, four tiers, routing by FWX_BATCH_MID_MIN_N.  Same arrays, same return value."""
    return _solve_ragged("fwx_solve_ragged_mid", rates, nexts, hops, device, count_updates)


def solve_ragged_large(rates, nexts=None, hops=None, *, device=-1, count_updates=False):
    """solve_ragged with the limit at FWX_BATCH_LARGE_MAX_N (fwx_solve_ragged_large_f64 / _f32): orders 0 ... 1024 in
    one call, five tiers, routing by FWX_BATCH_MID_MIN_N and FWX_BATCH_LARGE_MIN_N.  Same arrays, same return value."""
    return _solve_ragged("fwx_solve_ragged_large", rates, nexts, hops, device, count_updates)


def _solve_ragged(stem, rates, nexts, hops, device, count_updates):
    rates = list(rates)
    nexts = None if nexts is None else list(nexts)
    hops = None if hops is None else list(hops)
    n_each, rate, nxt, hp = _pack_ragged(rates, nexts, hops)
    o, _ = _opts(device, FWX_ENGINE_AUTO)
    each = np.zeros(len(n_each), dtype=np.uint64) if count_updates else None
    fn = getattr(lib(), stem + ("_f64" if rate.dtype == np.float64 else "_f32"))
    check(fn(len(n_each), _np_ptr(n_each), _np_ptr(rate), _np_ptr(nxt), _np_ptr(hp), _np_ptr(each), ctypes.byref(o)),
          stem)
    _unpack_ragged(n_each, (rate, nxt, hp), (rates, nexts, hops))
    return each


def solve_ragged_lists(rates, nexts, hops=None, *, items=None, cap=None, device=-1, count_updates=False):
    """solve_ragged and, in the same call, the reference's exact `_path` lists (fwx_solve_ragged_lists_f64 / _f32);
    nexts is required.  items, cap and the return value as in solve_batch_lists: items None means all n_b * n_b pairs
    of every matrix in the order (b, i, j); cap None starts at BATCH_LISTS_FIRST_CAP and doubles, solving the batch
    again from a kept copy of the input for the items that did not fit, up to BATCH_LISTS_MAX_CAP."""
    return _solve_ragged_lists("fwx_solve_ragged_lists", rates, nexts, hops, items, cap, device, count_updates)


def solve_ragged_mid_lists(rates, nexts, hops=None, *, items=None, cap=None, device=-1, count_updates=False):
    """solve_ragged_lists with the limit at FWX_BATCH_MID_MAX_N (fwx_solve_ragged_mid_lists_f64 / _f32).  Same arrays,
    same lists, same return value."""
    return _solve_ragged_lists("fwx_solve_ragged_mid_lists", rates, nexts, hops, items, cap, device, count_updates)


def solve_ragged_large_lists(rates, nexts, hops=None, *, items=None, cap=None, device=-1, count_updates=False):
    """solve_ragged_lists with the limit at FWX_BATCH_LARGE_MAX_N (fwx_solve_ragged_large_lists_f64 / _f32).  Same
    arrays, same lists, same return value."""
    return _solve_ragged_lists("fwx_solve_ragged_large_lists", rates, nexts, hops, items, cap, device, count_updates)


def _solve_ragged_lists(stem, rates, nexts, hops, items, cap, device, count_updates):
    if nexts is None:
        raise ValueError("the exact lists need next")
    rates, nexts = list(rates), list(nexts)
    hops = None if hops is None else list(hops)
    n_each, rate, nxt, hp = _pack_ragged(rates, nexts, hops)
    count = len(n_each)
    if items is None:
        trip = [np.stack(np.meshgrid(np.array([b]), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3)
                for b, n in enumerate(n_each)]
        trip = np.concatenate(trip) if trip else np.zeros((0, 3), dtype=np.int32)
        items = (trip[:, 0], trip[:, 1], trip[:, 2])
    mat, src, dst = (np.ascontiguousarray(a, dtype=np.int32) for a in items)
    if not (mat.ndim == 1 and mat.shape == src.shape == dst.shape):
        raise ValueError("items must be three equally long one-dimensional sequences (mat, src, dst)")
    fn = getattr(lib(), stem + ("_f64" if rate.dtype == np.float64 else "_f32"))
    grow = cap is None
    cap = BATCH_LISTS_FIRST_CAP if grow else int(cap)
    kept = (rate.copy(), nxt.copy(), None if hp is None else hp.copy()) if grow else None
    each = np.zeros(count, dtype=np.uint64) if count_updates else None
    o, _ = _opts(device, FWX_ENGINE_AUTO)
    out = [None] * len(mat)
    todo = np.arange(len(mat))
    arrays = (rate, nxt, hp)
    while True:
        lens = np.empty(len(todo), dtype=np.int32)
        paths = np.empty((len(todo), cap), dtype=np.int32)
        m, s, d = (np.ascontiguousarray(a[todo]) for a in (mat, src, dst))
        check(fn(count, _np_ptr(n_each), _np_ptr(arrays[0]), _np_ptr(arrays[1]), _np_ptr(arrays[2]),
                 _np_ptr(each) if arrays[0] is rate else None, len(todo), _np_ptr(m), _np_ptr(s), _np_ptr(d),
                 _np_ptr(lens), _np_ptr(paths), cap, ctypes.byref(o)), stem)
        if count == 0 or not n_each.any():
            lens[:] = _lib.FWX_ERR_INVALID       # nothing was solved: no item lies in the batch
        short = lens == _lib.FWX_ERR_CAPACITY
        bad = (lens < 0) & ~short
        if bad.any():
            raise FwxError(int(lens[bad][0]), "%s: item %d" % (stem, int(todo[bad][0])))
        for q in np.nonzero(~short)[0]:
            out[todo[q]] = tuple(int(v) for v in paths[q, :lens[q]])
        if not short.any():
            break
        if not grow or cap >= BATCH_LISTS_MAX_CAP:
            raise FwxError(_lib.FWX_ERR_CAPACITY, "%s: item %d does not fit cap %d"
                           % (stem, int(todo[short][0]), cap))
        cap, todo = min(2 * cap, BATCH_LISTS_MAX_CAP), todo[short]
        arrays = tuple(None if a is None else a.copy() for a in kept)     # solved again from the input
    _unpack_ragged(n_each, (rate, nxt, hp), (rates, nexts, hops))
    return (out, each) if count_updates else out


def _index_ptr(t, dtype_name, least):
    assert t.is_cuda and t.is_contiguous() and _dtype_name(t) == dtype_name and t.numel() >= least
    return ctypes.c_void_p(t.data_ptr())


def dev_solve_ragged(rate_t, n_each_t, offset_t, order_t, tier_count, *, next_t=None, hops_t=None, trace=None,
                     updates_t=None, stream=None):
    """fwx_dev_solve_ragged: a ragged batch in the device array rate_t (next_t / hops_t and the three arrays of
    `trace` alike), matrix b of order n_each_t[b] at element offset_t[b]; n_each_t (int32), offset_t (int64) and
    order_t (int32) are DEVICE arrays of count entries, order_t / tier_count a plan as ragged_plan gives it.  Gaps
    between the matrices are never touched.  Asynchronous on `stream`.  updates_t: device array of count 64-bit
    counters, counter b is incremented by U of matrix b."""
    _dev_solve_ragged("fwx_dev_solve_ragged", 3, rate_t, n_each_t, offset_t, order_t, tier_count, next_t, hops_t, trace,
                      updates_t, stream)


def dev_solve_ragged_mid(rate_t, n_each_t, offset_t, order_t, tier_count, *, next_t=None, hops_t=None, trace=None,
                         updates_t=None, stream=None):
    """fwx_dev_solve_ragged_mid: dev_solve_ragged for orders up to FWX_BATCH_MID_MAX_N; order_t / tier_count (four
    entries) a plan as ragged_mid_plan gives it.  Same arrays, same trace, same counters."""
    _dev_solve_ragged("fwx_dev_solve_ragged_mid", 4, rate_t, n_each_t, offset_t, order_t, tier_count, next_t, hops_t,
                      trace, updates_t, stream)


def dev_solve_ragged_large(rate_t, n_each_t, offset_t, order_t, tier_count, work, work_t, *, next_t=None, hops_t=None,
                           trace=None, updates_t=None, scratch_t=None, scratch_bytes=None, stream=None):
    """fwx_dev_solve_ragged_large: dev_solve_ragged_mid for orders up to FWX_BATCH_LARGE_MAX_N; order_t / tier_count
    (five entries) and work a plan as ragged_large_plan gives it, work_t a DEVICE int64 array of the same contents.
    scratch_t: a device array for the large tier's panels, 16-byte aligned, of at least
    _lib.batch_large_scratch_bytes(the largest order of the large tier) bytes -- the call solves as many matrices at
    a time as it holds; allocated here, for all of them, when not given.  scratch_bytes: how much of scratch_t the call
    may use (default: all of it).  work / work_t / scratch_t may be None when the large tier lists nothing.  Returns
    the scratch array (or None): it must stay alive until the stream has run the call."""
    tiers = np.ascontiguousarray(tier_count, dtype=np.int32)
    assert tiers.shape == (5,)
    count = n_each_t.numel()
    if work is not None:
        work = np.ascontiguousarray(work, dtype=np.int64)
        assert work.shape == (3, count + 1)
        assert work_t is None or (work_t.is_cuda and work_t.is_contiguous() and _dtype_name(work_t) == "int64"
                                  and work_t.numel() >= work.size)
        if scratch_t is None and tiers[4] > 0:
            scratch_t = _empty_like_device(rate_t, (_lib.batch_large_scratch_bytes(int(work[0, tiers[4]])),), "uint8")
    if scratch_t is not None and scratch_bytes is None:
        scratch_bytes = scratch_t.numel() * scratch_t.element_size()
    vp = ctypes.c_void_p
    large = (_np_ptr(work), vp(work_t.data_ptr()) if work_t is not None else None,
             vp(scratch_t.data_ptr()) if scratch_t is not None else None, int(scratch_bytes or 0))
    _dev_solve_ragged("fwx_dev_solve_ragged_large", 5, rate_t, n_each_t, offset_t, order_t, tiers, next_t, hops_t,
                      trace, updates_t, stream, large)
    return scratch_t


def _dev_solve_ragged(name, ntiers, rate_t, n_each_t, offset_t, order_t, tier_count, next_t, hops_t, trace, updates_t,
                      stream, large=None):
    count = n_each_t.numel()
    tiers = np.ascontiguousarray(tier_count, dtype=np.int32)
    assert tiers.shape == (ntiers,)
    assert rate_t.is_cuda and rate_t.is_contiguous()
    for t in (next_t, hops_t):
        assert t is None or (t.is_cuda and t.is_contiguous() and _dtype_name(t) == "int32")
    assert updates_t is None or (updates_t.element_size() == 8 and updates_t.numel() >= count)
    vp = ctypes.c_void_p
    check(getattr(lib(), name)(
        count, _tensor_dtype_code(rate_t), vp(rate_t.data_ptr()),
        vp(next_t.data_ptr()) if next_t is not None else None,
        vp(hops_t.data_ptr()) if hops_t is not None else None,
        _index_ptr(n_each_t, "int32", count), _index_ptr(offset_t, "int64", count),
        _index_ptr(order_t, "int32", int(tiers.sum())), _np_ptr(tiers), *(() if large is None else large[:2]),
        _trace_of(trace, 0) if trace is not None else None,
        vp(updates_t.data_ptr()) if updates_t is not None else None, *(() if large is None else large[2:]),
        _stream_ptr(stream, rate_t)), name)


def dev_exact_paths_ragged(next0_t, n_each_t, offset_t, n_max, trace, mat_t, src_t, dst_t, cap, *, stream=None):
    """fwx_dev_exact_paths_ragged: the exact `_path` lists of the items (mat_t[q], src_t[q], dst_t[q]) of a ragged
    batch that dev_solve_ragged solved with `trace`; next0_t is the caller's copy of the UNSOLVED next-hop array (same
    offsets), n_max at least the largest order.  Returns (len_t, path_t) as dev_exact_paths_batch."""
    return _dev_exact_paths_ragged("fwx_dev_exact_paths_ragged", next0_t, n_each_t, offset_t, n_max, trace, mat_t,
                                   src_t, dst_t, cap, stream)


def dev_exact_paths_ragged_mid(next0_t, n_each_t, offset_t, n_max, trace, mat_t, src_t, dst_t, cap, *, stream=None):
    """fwx_dev_exact_paths_ragged_mid: dev_exact_paths_ragged over a batch that dev_solve_ragged_mid solved, n_max <=
    FWX_BATCH_MID_MAX_N."""
    return _dev_exact_paths_ragged("fwx_dev_exact_paths_ragged_mid", next0_t, n_each_t, offset_t, n_max, trace, mat_t,
                                   src_t, dst_t, cap, stream)


def dev_exact_paths_ragged_large(next0_t, n_each_t, offset_t, n_max, trace, mat_t, src_t, dst_t, cap, *, stream=None):
    """fwx_dev_exact_paths_ragged_large: dev_exact_paths_ragged over a batch that dev_solve_ragged_large solved, n_max
    <= FWX_BATCH_LARGE_MAX_N."""
    return _dev_exact_paths_ragged("fwx_dev_exact_paths_ragged_large", next0_t, n_each_t, offset_t, n_max, trace, mat_t,
                                   src_t, dst_t, cap, stream)


def _dev_exact_paths_ragged(name, next0_t, n_each_t, offset_t, n_max, trace, mat_t, src_t, dst_t, cap, stream):
    count = n_each_t.numel()
    assert next0_t.is_cuda and next0_t.is_contiguous() and _dtype_name(next0_t) == "int32"
    items = mat_t.numel()
    for t in (mat_t, src_t, dst_t):
        assert t.is_cuda and t.is_contiguous() and _dtype_name(t) == "int32" and t.numel() == items
    len_t = _empty_like_device(mat_t, (items,), "int32")
    path_t = _empty_like_device(mat_t, (items, cap), "int32")
    scratch = _empty_like_device(mat_t, (max(items * 3 * (n_max + 2), 1),), "int32")
    vp = ctypes.c_void_p
    check(getattr(lib(), name)(
        count, _index_ptr(n_each_t, "int32", count), _index_ptr(offset_t, "int64", count), n_max,
        vp(next0_t.data_ptr()), _trace_of(trace, 0), items, vp(mat_t.data_ptr()), vp(src_t.data_ptr()),
        vp(dst_t.data_ptr()), vp(len_t.data_ptr()), vp(path_t.data_ptr()), cap, vp(scratch.data_ptr()),
        _stream_ptr(stream, mat_t)), name)
    if not _is_torch(mat_t):
        len_t._scratch = scratch              # stays alive until the results are read
    return len_t, path_t


def solve_multi(rate, nxt=None, hops=None, *, devices=(0,), exchange=FWX_XCHG_AUTO,
                engine=FWX_ENGINE_AUTO, k_begin=0, k_end=0, count_updates=False):
    """runAlgo in place on host numpy arrays, row-partitioned over `devices` (one partition per
    entry; a device may repeat = logical partitions on one GPU) from ONE process:
    fwx_solve_multi_f64 / _f32."""
    _check_arrays(rate, nxt, hops)
    o, u = _opts(engine=engine, k_begin=k_begin, k_end=k_end, want_updates=count_updates)
    devs = (ctypes.c_int32 * len(devices))(*devices)
    fn = lib().fwx_solve_multi_f64 if rate.dtype == np.float64 else lib().fwx_solve_multi_f32
    check(fn(rate.shape[0], _np_ptr(rate), _np_ptr(nxt), _np_ptr(hops), len(devices), devs, exchange,
             ctypes.byref(o)), "fwx_solve_multi")
    return int(u.value) if count_updates else None


def follow_path(nxt, src, dst):
    """Vertex indices after src up to and including dst; [] when there is no route."""
    n = nxt.shape[0]
    out = np.empty(max(n, 1), dtype=np.int32)
    ln = check(lib().fwx_follow_path(n, _np_ptr(nxt), int(src), int(dst), _np_ptr(out), n),
               "fwx_follow_path")
    return [int(x) for x in out[:ln]]


class DeviceMatrix:
    """fwx_matrix handle: the solved matrix stays in HBM across queries (InSync, Types.hs:35-37)."""

    def __init__(self, n, dtype=np.float64, with_next=True, with_hops=False, device=-1, devices=None,
                 exchange=FWX_XCHG_AUTO):
        """devices: a list of HIP ordinals = a ROW-PARTITIONED handle (fwx_matrix_create_multi), one
        partition per entry, repeats allowed; None = one device."""
        self.n = int(n)
        self.dtype = np.dtype(dtype)
        self.with_next, self.with_hops = bool(with_next), bool(with_hops)
        h = ctypes.c_void_p()
        code = FWX_F64 if self.dtype == np.float64 else FWX_F32
        if devices is None:
            check(lib().fwx_matrix_create(ctypes.byref(h), self.n, code, int(self.with_next),
                                          int(self.with_hops), device), "fwx_matrix_create")
        else:
            devs = (ctypes.c_int32 * len(devices))(*devices)
            check(lib().fwx_matrix_create_multi(ctypes.byref(h), self.n, code, int(self.with_next),
                                                int(self.with_hops), len(devices), devs, exchange),
                  "fwx_matrix_create_multi")
        self._h = h

    def parts(self):
        """(number of row partitions, exchange transport in use)."""
        x = ctypes.c_int32(0)
        p = check(lib().fwx_matrix_parts(self._h, ctypes.byref(x)), "fwx_matrix_parts")
        return p, int(x.value)

    def part_rows(self, part):
        """(row0, rows) of partition `part` (fwx_matrix_part_rows)."""
        r0, rs = ctypes.c_int32(0), ctypes.c_int32(0)
        check(lib().fwx_matrix_part_rows(self._h, int(part), ctypes.byref(r0), ctypes.byref(rs)), "fwx_matrix_part_rows")
        return int(r0.value), int(rs.value)

    def comm_ranks(self):
        """Ranks of the RCCL communicator the partitions exchange panels on (0: not RCCL)."""
        return check(lib().fwx_matrix_comm_ranks(self._h), "fwx_matrix_comm_ranks")

    def set_timing(self, on=True):
        """Per-step event timings of the following solves (partitioned handles; fwx_matrix_set_timing)."""
        check(lib().fwx_matrix_set_timing(self._h, 1 if on else 0), "fwx_matrix_set_timing")

    def timing(self):
        """fwx_multi_timing of the last solve as a dict (microseconds; see include/fwx.h)."""
        from ._lib import FwxMultiTiming
        t = FwxMultiTiming()
        t.struct_size = ctypes.sizeof(FwxMultiTiming)
        check(lib().fwx_matrix_get_timing(self._h, ctypes.byref(t)), "fwx_matrix_get_timing")
        return {name: getattr(t, name) for name, _ in FwxMultiTiming._fields_ if name != "struct_size"}

    def upload(self, rate, nxt=None, hops=None):
        _check_arrays(rate, nxt, hops)
        assert rate.shape[0] == self.n and rate.dtype == self.dtype
        check(lib().fwx_matrix_upload(self._h, _np_ptr(rate), _np_ptr(nxt), _np_ptr(hops)),
              "fwx_matrix_upload")

    def upload_dev(self, rate_d, next_d=None, hops_d=None):
        """Upload from DEVICE arrays (torch tensors or hip.DeviceArray): fwx_matrix_upload takes host
        or device pointers.  The caller must have finished writing them (this call blocks)."""
        ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
        check(lib().fwx_matrix_upload(self._h, ptr(rate_d), ptr(next_d), ptr(hops_d)),
              "fwx_matrix_upload")

    def download_dev(self, rate_d=None, next_d=None, hops_d=None):
        """Copy the handle's arrays into DEVICE arrays."""
        ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
        check(lib().fwx_matrix_download(self._h, ptr(rate_d), ptr(next_d), ptr(hops_d)),
              "fwx_matrix_download")

    def solve(self, **kw):
        count = kw.pop("count_updates", False)
        o, u = _opts(want_updates=count, **kw)
        check(lib().fwx_matrix_solve(self._h, ctypes.byref(o)), "fwx_matrix_solve")
        return int(u.value) if count else None

    def download(self):
        rate = np.empty((self.n, self.n), dtype=self.dtype)
        nxt = np.empty((self.n, self.n), dtype=np.int32) if self.with_next else None
        hops = np.empty((self.n, self.n), dtype=np.int32) if self.with_hops else None
        check(lib().fwx_matrix_download(self._h, _np_ptr(rate), _np_ptr(nxt), _np_ptr(hops)),
              "fwx_matrix_download")
        return rate, nxt, hops

    def query(self, src, dst):
        """(rate, [path indices]) of one entry, read back from the device."""
        r = ctypes.c_double(0.0)
        out = np.empty(max(self.n, 1), dtype=np.int32)
        ln = check(lib().fwx_matrix_query(self._h, int(src), int(dst), ctypes.byref(r),
                                          _np_ptr(out), self.n), "fwx_matrix_query")
        return float(r.value), [int(x) for x in out[:ln]]

    def keep_input(self):
        """Keep the uploaded input on the device (fwx_matrix_keep_input) so that patch_input can
        replace a few entries of it without a new upload."""
        check(lib().fwx_matrix_keep_input(self._h), "fwx_matrix_keep_input")

    def patch_input(self, index, rate_vals, next_vals=None, hops_vals=None):
        """Replace entries index[q] = i*n + j of the KEPT input and make it the unsolved matrix again
        (fwx_matrix_patch_input); follow with solve()."""
        index = np.ascontiguousarray(index, dtype=np.int64)
        rate_vals = np.ascontiguousarray(rate_vals, dtype=self.dtype)
        nv = None if next_vals is None else np.ascontiguousarray(next_vals, dtype=np.int32)
        hv = None if hops_vals is None else np.ascontiguousarray(hops_vals, dtype=np.int32)
        assert index.ndim == 1 and rate_vals.shape == index.shape
        check(lib().fwx_matrix_patch_input(self._h, len(index), _np_ptr(index), _np_ptr(rate_vals),
                                           _np_ptr(nv), _np_ptr(hv)), "fwx_matrix_patch_input")

    def enable_resume(self, checkpoints=7):
        """Keep state checkpoints + the panels of every pivot so that resolve() can resume
        (fwx_matrix_enable_resume); returns the number of checkpoints placed."""
        return check(lib().fwx_matrix_enable_resume(self._h, int(checkpoints)), "fwx_matrix_enable_resume")

    def resolve(self, index, rate_vals, next_vals=None, hops_vals=None, **kw):
        """patch_input + solve in one call, resuming from the last checkpoint the changed entries
        cannot have influenced (fwx_matrix_resolve).  Returns the pivot the solve started at."""
        index = np.ascontiguousarray(index, dtype=np.int64)
        rate_vals = np.ascontiguousarray(rate_vals, dtype=self.dtype)
        nv = None if next_vals is None else np.ascontiguousarray(next_vals, dtype=np.int32)
        hv = None if hops_vals is None else np.ascontiguousarray(hops_vals, dtype=np.int32)
        assert index.ndim == 1 and rate_vals.shape == index.shape
        o, _u = _opts(want_updates=kw.pop("count_updates", False), **kw)   # _u: keeps updates_out alive
        started = ctypes.c_int32(0)
        check(lib().fwx_matrix_resolve(self._h, len(index), _np_ptr(index), _np_ptr(rate_vals), _np_ptr(nv),
                                       _np_ptr(hv), ctypes.byref(o), ctypes.byref(started)),
              "fwx_matrix_resolve")
        return int(started.value)

    def enable_path_log(self):
        """Keep the path trace (three n x n int32 matrices, see fwx.h) so that query_exact can
        rebuild the reference's `_path` lists exactly; a traced solve() needs a fresh upload()."""
        check(lib().fwx_matrix_enable_path_log(self._h), "fwx_matrix_enable_path_log")

    def path_log_count(self):
        c = ctypes.c_uint64(0)
        check(lib().fwx_matrix_path_log_count(self._h, ctypes.byref(c)), "fwx_matrix_path_log_count")
        return int(c.value)

    def query_exact(self, src, dst, cap=None):
        """(rate, the reference's `_path` as vertex indices) -- exact under ties."""
        cap = cap or max(4 * self.n, 64)
        r = ctypes.c_double(0.0)
        out = np.empty(cap, dtype=np.int32)
        ln = check(lib().fwx_matrix_query_exact(self._h, int(src), int(dst), ctypes.byref(r),
                                                _np_ptr(out), cap), "fwx_matrix_query_exact")
        return float(r.value), [int(x) for x in out[:ln]]

    def query_exact_batch(self, src, dst, cap=None):
        """Exact `_path` lists of many (src[q], dst[q]) pairs in one launch -> list of lists
        (FwxError if one does not fit into cap entries)."""
        src = np.ascontiguousarray(src, dtype=np.int32)
        dst = np.ascontiguousarray(dst, dtype=np.int32)
        assert src.shape == dst.shape and src.ndim == 1
        cap = cap or max(4 * self.n, 64)
        lens = np.empty(len(src), dtype=np.int32)
        paths = np.empty((len(src), cap), dtype=np.int32)
        check(lib().fwx_matrix_query_exact_batch(self._h, len(src), _np_ptr(src), _np_ptr(dst),
                                                 _np_ptr(lens), _np_ptr(paths), cap),
              "fwx_matrix_query_exact_batch")
        if len(lens) and int(lens.min()) < 0:
            raise FwxError(int(lens.min()), "fwx_matrix_query_exact_batch: a list did not fit")
        return [[int(v) for v in paths[q, :lens[q]]] for q in range(len(src))]

    def close(self):
        if self._h:
            lib().fwx_matrix_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- device-pointer step API (torch tensors own the memory) -----------------------------------

def _dtype_name(t):
    """'float32' for torch.float32 and numpy float32 alike: the device API takes torch tensors or
    hip.DeviceArray (no torch in the process)."""
    return str(t.dtype).split(".")[-1]


def _tensor_dtype_code(t):
    name = _dtype_name(t)
    if name == "float32":
        return FWX_F32
    if name == "float64":
        return FWX_F64
    raise ValueError("rate tensor must be float32 or float64")


def _slab(rate_t, next_t, hops_t, n, row0):
    assert rate_t.is_cuda and rate_t.is_contiguous() and rate_t.dim() == 2 and rate_t.shape[1] == n
    for t in (next_t, hops_t):
        assert t is None or (t.is_cuda and t.is_contiguous() and _dtype_name(t) == "int32"
                             and tuple(t.shape) == tuple(rate_t.shape))
    s = FwxSlab()
    s.n, s.row0, s.rows, s.dtype = n, row0, rate_t.shape[0], _tensor_dtype_code(rate_t)
    s.rate = rate_t.data_ptr()
    s.next = next_t.data_ptr() if next_t is not None else None
    s.hops = hops_t.data_ptr() if hops_t is not None else None
    return s


def _is_torch(t):
    return type(t).__module__.split(".")[0] == "torch"


def _stream_ptr(stream=None, like=None):
    """hipStream_t for a launch: an explicit hip.Stream / torch stream (or raw handle); else the
    current torch stream if `like` is a torch tensor, else this module's default hip.Stream."""
    if stream is not None:
        h = getattr(stream, "ptr", None)
        if h is None:
            h = getattr(stream, "cuda_stream", stream)
        return h if isinstance(h, ctypes.c_void_p) else ctypes.c_void_p(h)
    if like is not None and _is_torch(like):
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream(like.device).cuda_stream)
    from . import hip
    return hip.default_stream().ptr


def _empty_like_device(like, shape, dtype_name):
    """Uninitialised device array on the device of `like` (torch tensor -> torch tensor, hip.DeviceArray
    -> hip.DeviceArray)."""
    if _is_torch(like):
        import torch
        return torch.empty(tuple(shape), dtype=getattr(torch, dtype_name), device=like.device)
    from . import hip
    return hip.DeviceArray(shape, np.dtype(dtype_name))


def dev_relax(rate_t, n, row0, k_begin, k_end, *, pivots_t=None, pivot_hops_t=None, next_t=None,
              hops_t=None, serpentine=True, updates_t=None, skip=None, pivot_next_t=None,
              stream=None):
    """Apply pivots [k_begin,k_end) to the slab `rate_t` (rows [row0,row0+rows) of the n x n
    matrix) on torch's current stream, asynchronously.  skip = (lo, hi): slab rows [lo, hi)
    (multiples of 4) are left alone -- a look-ahead step has relaxed them already.

    pivots_t None: the slab holds the pivot rows itself (single-GPU solve).  Otherwise pivots_t is
    the (k_end-k_begin) x n panel of time-k snapshots from dev_panel."""
    s = _slab(rate_t, next_t, hops_t, n, row0)
    p = FwxPivots()
    p.k_begin, p.k_end = k_begin, k_end
    if pivots_t is None:
        assert row0 <= k_begin and k_end <= row0 + rate_t.shape[0]
        es = rate_t.element_size()
        p.rate = rate_t.data_ptr() + (k_begin - row0) * n * es
        p.hops = hops_t.data_ptr() + (k_begin - row0) * n * 4 if hops_t is not None else None
        p.next = next_t.data_ptr() + (k_begin - row0) * n * 4 if next_t is not None else None
        p.stride = n
    else:
        assert pivots_t.is_cuda and pivots_t.is_contiguous() and pivots_t.dtype == rate_t.dtype
        assert tuple(pivots_t.shape) == (k_end - k_begin, n)
        p.rate = pivots_t.data_ptr()
        p.hops = pivot_hops_t.data_ptr() if pivot_hops_t is not None else None
        p.next = pivot_next_t.data_ptr() if pivot_next_t is not None else None
        p.stride = n
    upd = ctypes.c_void_p(updates_t.data_ptr()) if updates_t is not None else None
    lo, hi = skip if skip else (0, 0)
    check(lib().fwx_dev_relax_skip(ctypes.byref(s), ctypes.byref(p), int(bool(serpentine)), upd,
                                   int(lo), int(hi), _stream_ptr(stream, rate_t)), "fwx_dev_relax_skip")


def dev_panel(block_rate_t, n, k0, w_rate_t, *, next_t=None, hops_t=None, w_hops_t=None,
              updates_t=None):
    """Owner-side panel phase: evolve pivot rows [k0,k0+B) in place, export time-k snapshots."""
    s = _slab(block_rate_t, next_t, hops_t, n, k0)
    assert w_rate_t.is_cuda and w_rate_t.is_contiguous() and w_rate_t.shape == block_rate_t.shape
    upd = ctypes.c_void_p(updates_t.data_ptr()) if updates_t is not None else None
    wh = ctypes.c_void_p(w_hops_t.data_ptr()) if w_hops_t is not None else None
    check(lib().fwx_dev_panel(ctypes.byref(s), ctypes.c_void_p(w_rate_t.data_ptr()), wh, upd,
                              _stream_ptr(None, block_rate_t)), "fwx_dev_panel")


def _alloc(shape, dtype, device, fill=None):
    """Device array of a torch dtype (on torch `device`) or of a numpy dtype (hip.DeviceArray on the
    current HIP device; `device` is then ignored)."""
    if type(dtype).__module__.split(".")[0] == "torch":
        import torch
        if fill is None:
            return torch.empty(tuple(shape), dtype=dtype, device=device)
        return torch.full(tuple(shape), fill, dtype=dtype, device=device)
    from . import hip
    a = hip.DeviceArray(shape, dtype)
    return a if fill is None else a.fill_(fill)


def _int32_of(dtype):
    if type(dtype).__module__.split(".")[0] == "torch":
        import torch
        return torch.int32
    return np.int32


class FusedWorkspace:
    """Device scratch of the fused engine for slabs of up to `rows` rows: snapshot panels W (two,
    for look-ahead; with hops also their hops panels WH), pivot-column snapshots Ct / CNt / CHt.
    dtype: a torch dtype (arrays are torch tensors on `device`) or a numpy dtype (hip.DeviceArray)."""

    def __init__(self, n, rows, dtype, device=None, with_next=False, with_hops=False):
        B = FWX_FUSED_BLOCK
        i32 = _int32_of(dtype)
        self.w = [_alloc((B, n), dtype, device) for _ in range(2)]
        self.wh = [_alloc((B, n), i32, device) for _ in range(2)] if with_hops else [None, None]
        ld = (max(rows, 1) + 3) & ~3
        self.ld = ld
        self.ct = _alloc((B, ld), dtype, device)
        self.cnt = _alloc((B, ld), i32, device) if with_next else None
        self.cht = _alloc((B, ld), i32, device) if with_hops else None


class Trace:
    """Path trace of a slab (fwx.h fwx_trace): three rows x n int32 device arrays, LOCAL rows, all
    -1 before a solve.  rows(lo, hi) gives the views a panel of pivot rows needs.  device: a
    torch.device (torch tensors) or None (hip.DeviceArray on the current HIP device)."""

    def __init__(self, rows, n, device=None, _views=None):
        if _views is not None:
            self.last, self.at_col, self.at_row = _views
        elif device is not None:
            import torch
            self.last, self.at_col, self.at_row = (torch.full((rows, n), -1, dtype=torch.int32, device=device)
                                                   for _ in range(3))
        else:
            self.last, self.at_col, self.at_row = (_alloc((rows, n), np.int32, None, fill=-1)
                                                   for _ in range(3))

    def rows(self, lo, hi):
        return Trace(0, 0, _views=(self.last[lo:hi], self.at_col[lo:hi], self.at_row[lo:hi]))

    def c_struct(self):
        t = _lib.FwxTrace()
        t.last, t.at_col, t.at_row = self.last.data_ptr(), self.at_col.data_ptr(), self.at_row.data_ptr()
        return t


def _trace_ref(trace):
    return ctypes.byref(trace.c_struct()) if trace is not None else None


def dev_panel_snap(block_rate_t, n, k0, w_rate_t, *, block_next_t=None, block_hops_t=None, w_hops_t=None,
                   trace=None):
    """Snapshot panel of pivot rows [k0, k0+B) (B <= 64): w[t] = row k0+t at time k0+t (and w_hops
    its hops row, if the block carries hops).  The matrix is NOT modified (contrast dev_panel).
    trace: the Trace views OF THE SAME ROWS (Trace.rows); its at_row rows are written."""
    s = _slab(block_rate_t, block_next_t, block_hops_t, n, k0)
    assert w_rate_t.is_cuda and w_rate_t.is_contiguous()
    assert tuple(w_rate_t.shape) == tuple(block_rate_t.shape) and w_rate_t.dtype == block_rate_t.dtype
    wh = None
    if block_hops_t is not None:
        assert w_hops_t is not None and tuple(w_hops_t.shape) == tuple(block_rate_t.shape)
        wh = ctypes.c_void_p(w_hops_t.data_ptr())
    check(lib().fwx_dev_panel_snap(ctypes.byref(s), ctypes.c_void_p(w_rate_t.data_ptr()), wh,
                                   _trace_ref(trace), _stream_ptr(None, block_rate_t)), "fwx_dev_panel_snap")


def dev_domain_bits(rate_t, n, row0=0, next_t=None):
    """Domain check of one slab (fwx.h "Domain"; synchronises): bit 0 = every rate is >= +0.0 and
    not NaN, bit 1 = no entry has a non-zero rate and next < 0 (always set without next_t)."""
    s = _slab(rate_t, next_t, None, n, row0)
    if _is_torch(rate_t):
        import torch
        flag = torch.full((1,), 3, dtype=torch.int32, device=rate_t.device)
        check(lib().fwx_dev_check_nonneg(ctypes.byref(s), ctypes.c_void_p(flag.data_ptr()),
                                         _stream_ptr(None, rate_t)), "fwx_dev_check_nonneg")
        return int(flag.item())
    from . import hip
    st = hip.default_stream()
    flag = hip.DeviceArray.from_numpy(np.full((1,), 3, dtype=np.int32), st)
    check(lib().fwx_dev_check_nonneg(ctypes.byref(s), ctypes.c_void_p(flag.data_ptr()), st.ptr),
          "fwx_dev_check_nonneg")
    return int(flag.numpy(st)[0])


def dev_check_nonneg(rate_t, n, row0=0):
    """True iff every rate of the slab is >= +0.0 and not NaN (synchronises)."""
    return bool(dev_domain_bits(rate_t, n, row0) & 1)


def dev_relax_fused(rate_t, n, row0, k0, k1, w_t, ws, *, next_t=None, hops_t=None, wh_t=None, trace=None,
                    updates_t=None, nonneg=False, skip=None):
    """Apply pivots [k0,k1) (at most 64) to EVERY row of the slab in one pass, from the snapshot
    panel w_t ((k1-k0) x n; wh_t: its hops panel, iff hops_t).  ws: a FusedWorkspace sized for this
    slab.  trace: the slab's Trace.  skip = (lo, hi): slab rows [lo, hi) (multiples of 8) are left
    to an earlier look-ahead step."""
    s = _slab(rate_t, next_t, hops_t, n, row0)
    p = FwxPivots()
    p.k_begin, p.k_end = k0, k1
    assert w_t.is_cuda and w_t.is_contiguous() and w_t.dtype == rate_t.dtype
    assert tuple(w_t.shape) == (k1 - k0, n)
    ld = (rate_t.shape[0] + 3) & ~3
    assert ws.ct.numel() >= FWX_FUSED_BLOCK * ld and ws.ct.dtype == rate_t.dtype
    p.rate, p.hops, p.stride = w_t.data_ptr(), None, n
    sc = _lib.FwxFusedScratch()
    sc.col_rate = ws.ct.data_ptr()
    if next_t is not None:
        assert ws.cnt is not None and ws.cnt.numel() >= FWX_FUSED_BLOCK * ld
        sc.col_next = ws.cnt.data_ptr()
    if hops_t is not None:
        assert wh_t is not None and tuple(wh_t.shape) == (k1 - k0, n) and ws.cht is not None
        p.hops = wh_t.data_ptr()
        sc.col_hops = ws.cht.data_ptr()
    upd = ctypes.c_void_p(updates_t.data_ptr()) if updates_t is not None else None
    lo, hi = skip if skip else (0, 0)
    check(lib().fwx_dev_relax_fused_skip(ctypes.byref(s), ctypes.byref(p), ctypes.byref(sc),
                                         _trace_ref(trace), upd,
                                         _lib.FWX_FLAG_NONNEG if nonneg else 0, int(lo), int(hi),
                                         _stream_ptr(None, rate_t)),
          "fwx_dev_relax_fused_skip")


def dev_solve_fused(rate_t, n, k_begin=0, k_end=None, *, next_t=None, hops_t=None, trace=None, ws=None,
                    updates_t=None, nonneg=None):
    """Single-GPU solve of pivots [k_begin,k_end) with the fused engine on a torch tensor holding
    the whole n x n matrix, one panel + one pass at a time (no look-ahead: fwx_dev_solve has it);
    asynchronous on the current stream (after one small synchronising domain check when `nonneg`
    is not given)."""
    k_end = n if k_end is None else k_end
    if nonneg is None:
        bits = dev_domain_bits(rate_t, n, 0, next_t)
        nonneg = updates_t is None and (bits == 3 if next_t is not None else bool(bits & 1))
    ws = ws or FusedWorkspace(n, n, rate_t.dtype, getattr(rate_t, "device", None),
                              with_next=next_t is not None, with_hops=hops_t is not None)
    B = FWX_FUSED_BLOCK
    for k0 in range(k_begin, k_end, B):
        k1 = min(k_end, k0 + B)
        w = ws.w[0][:k1 - k0]
        wh = ws.wh[0][:k1 - k0] if hops_t is not None else None
        dev_panel_snap(rate_t[k0:k1], n, k0, w,
                       block_next_t=next_t[k0:k1] if next_t is not None else None,
                       block_hops_t=hops_t[k0:k1] if hops_t is not None else None, w_hops_t=wh,
                       trace=trace.rows(k0, k1) if trace is not None else None)
        dev_relax_fused(rate_t, n, 0, k0, k1, w, ws, next_t=next_t, hops_t=hops_t, wh_t=wh, trace=trace,
                        updates_t=updates_t, nonneg=nonneg)
    return ws


def dev_follow_paths(next_t, src_t, dst_t, *, edge_rate_t=None, path_cap=0):
    """Batch path reconstruction on the device (fwx_dev_follow_paths).  next_t: full n x n int32
    next-hop matrix; src_t/dst_t: int32 vectors.  Returns (len, prod or None, paths or None) as
    device arrays of the same kind as next_t; asynchronous on the current / default stream."""
    n = next_t.shape[0]
    assert next_t.is_cuda and next_t.is_contiguous() and _dtype_name(next_t) == "int32"
    assert _dtype_name(src_t) == "int32" and _dtype_name(dst_t) == "int32"
    assert tuple(src_t.shape) == tuple(dst_t.shape)
    count = src_t.numel()
    len_t = _empty_like_device(next_t, (count,), "int32")
    prod_t = _empty_like_device(next_t, (count,), "float64") if edge_rate_t is not None else None
    path_t = _empty_like_device(next_t, (count, path_cap), "int32") if path_cap else None
    code = FWX_F32
    if edge_rate_t is not None:
        assert edge_rate_t.is_cuda and edge_rate_t.is_contiguous()
        assert tuple(edge_rate_t.shape) == tuple(next_t.shape)
        code = _tensor_dtype_code(edge_rate_t)
    vp = ctypes.c_void_p
    check(lib().fwx_dev_follow_paths(
        n, vp(next_t.data_ptr()), count, vp(src_t.data_ptr()), vp(dst_t.data_ptr()),
        vp(len_t.data_ptr()), vp(edge_rate_t.data_ptr()) if edge_rate_t is not None else None, code,
        vp(prod_t.data_ptr()) if prod_t is not None else None,
        vp(path_t.data_ptr()) if path_t is not None else None, path_cap, _stream_ptr(None, next_t)),
        "fwx_dev_follow_paths")
    return len_t, prod_t, path_t


def dev_solve(rate_t, *, next_t=None, hops_t=None, engine=FWX_ENGINE_AUTO, k_begin=0, k_end=0,
              serpentine=True, count_updates=False, stream=None):
    """fwx_dev_solve: whole solve (or a pivot range) on a device array holding the entire n x n
    matrix, in place, BLOCKING.  The fused engine runs with look-ahead on an internal side stream.
    Work queued on the current / default stream must be finished first: this synchronises it."""
    n = rate_t.shape[0]
    assert tuple(rate_t.shape) == (n, n)
    if stream is None:
        if _is_torch(rate_t):
            import torch
            torch.cuda.current_stream(rate_t.device).synchronize()
        else:
            from . import hip
            hip.default_stream().synchronize()
    s = _slab(rate_t, next_t, hops_t, n, 0)
    o, u = _opts(-1, engine, k_begin, k_end, 0, serpentine, count_updates, stream=stream)
    check(lib().fwx_dev_solve(ctypes.byref(s), ctypes.byref(o)), "fwx_dev_solve")
    return int(u.value) if count_updates else None
