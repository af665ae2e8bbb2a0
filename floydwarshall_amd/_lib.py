"""ctypes loader for libfwx.so (the C ABI of include/fwx.h).  Fails loudly: there is no fallback."""
import ctypes
import os

# Multi-process / multi-device GPU work on this pool needs dmabuf IPC: without it RCCL (and any
# device-memory sharing across processes) fails in hipIpcGetMemHandle ("invalid argument").  The HIP
# runtime reads the variable when it initialises, so it is set HERE, at import, before the first HIP
# call any binding of this package can make -- a host that binds libfwx directly (C, Haskell) exports
# it itself (include/fwx.h FWX_XCHG_RCCL).  setdefault: an explicit setting wins.
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

PKG = os.path.dirname(os.path.abspath(__file__))
# FWX_LIB_PATH: developer override, e.g. an experimental build of the same ABI
LIB_PATH = os.environ.get("FWX_LIB_PATH") or os.path.join(PKG, "libfwx.so")

FWX_OK = 0
FWX_ERR_INVALID = -1
FWX_ERR_NO_DEVICE = -2
FWX_ERR_HIP = -3
FWX_ERR_OOM = -4
FWX_ERR_CYCLE = -5
FWX_ERR_CAPACITY = -6
FWX_ERR_UNSUPPORTED = -7
FWX_ERR_RCCL = -8
FWX_ERR_INTERNAL = -9

FWX_ABI_VERSION = 3
FWX_F32, FWX_F64 = 0, 1
FWX_ENGINE_AUTO, FWX_ENGINE_PERK, FWX_ENGINE_FUSED = 0, 1, 2
FWX_UPDATE_SHARDS = 256
FWX_FUSED_BLOCK = 64
FWX_BATCH_MAX_N = 128
FWX_BATCH_MID_MAX_N = 256
FWX_BATCH_LARGE_MAX_N = 1024
FWX_SWEEP_MAX_N = FWX_BATCH_MAX_N
FWX_SWEEP_MID_MAX_N = FWX_BATCH_MID_MAX_N


def batch_large_scratch_bytes(n):
    """FWX_BATCH_LARGE_SCRATCH_BYTES(n) of include/fwx.h: device scratch one matrix of order n needs."""
    return int(n) * 512


def sweep_mid_scratch_bytes(n):
    """FWX_SWEEP_MID_SCRATCH_BYTES(n) of include/fwx.h: one workspace slot of a mid-tier sweep of order n."""
    return int(n) * int(n) * 16


FWX_FLAG_NONNEG = 1
FWX_XCHG_AUTO, FWX_XCHG_PEER, FWX_XCHG_RCCL = 0, 1, 2
FWX_XCHG_CALLBACK = 3
FWX_MAX_PARTS = 32

c_i32 = ctypes.c_int32
c_vp = ctypes.c_void_p
# int exchange(void *ctx, int32 k0, int32 bt, int32 owner, void *w, int32 *wh, int64 count, void *stream)
EXCHANGE_FN = ctypes.CFUNCTYPE(ctypes.c_int, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, ctypes.c_int64, c_vp)


class FwxOpts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("device", c_i32), ("engine", c_i32),
                ("k_begin", c_i32), ("k_end", c_i32), ("block", c_i32), ("serpentine", c_i32),
                ("updates_out", ctypes.POINTER(ctypes.c_uint64)), ("stream", c_vp),
                ("use_stream", c_i32), ("reserved0", c_i32)]


class FwxSlab(ctypes.Structure):
    _fields_ = [("n", c_i32), ("row0", c_i32), ("rows", c_i32), ("dtype", c_i32),
                ("rate", c_vp), ("next", c_vp), ("hops", c_vp)]


class FwxPivots(ctypes.Structure):
    _fields_ = [("k_begin", c_i32), ("k_end", c_i32), ("rate", c_vp), ("hops", c_vp),
                ("stride", ctypes.c_int64), ("next", c_vp)]


class FwxTrace(ctypes.Structure):
    _fields_ = [("last", c_vp), ("at_col", c_vp), ("at_row", c_vp)]


class FwxSweepPatches(ctypes.Structure):
    _fields_ = [("ptr", c_vp), ("total", ctypes.c_int64), ("index", c_vp), ("rate", c_vp), ("next", c_vp),
                ("hops", c_vp)]


class FwxSweepItems(ctypes.Structure):
    _fields_ = [("ptr", c_vp), ("total", ctypes.c_int64), ("src", c_vp), ("dst", c_vp), ("rate_out", c_vp),
                ("next_out", c_vp), ("hops_out", c_vp)]


class FwxSweepFull(ctypes.Structure):
    _fields_ = [("rate", c_vp), ("next", c_vp), ("hops", c_vp), ("stride", ctypes.c_int64)]


class FwxFusedScratch(ctypes.Structure):
    _fields_ = [("col_rate", c_vp), ("col_next", c_vp), ("col_hops", c_vp)]


class FwxMultiTiming(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("steps", c_i32), ("pivots_per_step", c_i32),
                ("partitions", c_i32), ("bulk_us", ctypes.c_float), ("bulk_mean_us", ctypes.c_float),
                ("lookahead_us", ctypes.c_float), ("panel_us", ctypes.c_float),
                ("exchange_us", ctypes.c_float), ("chain_us", ctypes.c_float),
                ("chain_over_bulk", ctypes.c_float)]


class FwxError(RuntimeError):
    def __init__(self, status, what):
        self.status = status
        msg = lib().fwx_strerror(status).decode()
        extra = ""
        if status == FWX_ERR_HIP:
            extra = " (hipError_t %d)" % lib().fwx_last_hip_error()
        super().__init__("%s: %s%s" % (what, msg, extra))


# Every symbol include/fwx.h declares, with its ctypes signature.
SIGNATURES = {
    "fwx_abi_version": (ctypes.c_int, []),
    "fwx_device_count": (ctypes.c_int, []),
    "fwx_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "fwx_last_hip_error": (ctypes.c_int, []),
    "fwx_hip_versions": (ctypes.c_int, [ctypes.POINTER(c_i32), ctypes.POINTER(c_i32)]),
    "fwx_test_fail_after": (ctypes.c_int, [c_i32]),
    "fwx_test_kernel_forms": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]),
    "fwx_test_kernel_form_name": (ctypes.c_char_p, [ctypes.c_int]),
    "fwx_test_perk_pivots": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]),
    "fwx_test_perk_fold": (ctypes.c_int, []),
    "fwx_test_perk_walk": (ctypes.c_int, []),
    "fwx_test_perk_deep": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]),
    "fwx_test_perk_tile": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]),
    "fwx_test_perk_pair": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]),
    "fwx_test_perk_group": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]),
    "fwx_test_perk_group_plan": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                                ctypes.POINTER(ctypes.c_int), ctypes.c_int]),
    "fwx_test_pools": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]),
    "fwx_test_perk_scratch_victim": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int),
                                                    ctypes.c_int, ctypes.c_int]),
    "fwx_test_perk_wide": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]),
    "fwx_solve_f64": (ctypes.c_int, [c_i32, c_vp, c_vp, c_vp, ctypes.POINTER(FwxOpts)]),
    "fwx_solve_f32": (ctypes.c_int, [c_i32, c_vp, c_vp, c_vp, ctypes.POINTER(FwxOpts)]),
    "fwx_follow_path": (ctypes.c_int, [c_i32, c_vp, c_i32, c_i32, c_vp, c_i32]),
    "fwx_matrix_create": (ctypes.c_int, [ctypes.POINTER(c_vp), c_i32, c_i32, c_i32, c_i32, c_i32]),
    "fwx_matrix_upload": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp]),
    "fwx_matrix_solve": (ctypes.c_int, [c_vp, ctypes.POINTER(FwxOpts)]),
    "fwx_matrix_download": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp]),
    "fwx_matrix_query": (ctypes.c_int, [c_vp, c_i32, c_i32, ctypes.POINTER(ctypes.c_double), c_vp,
                                        c_i32]),
    "fwx_matrix_destroy": (ctypes.c_int, [c_vp]),
    "fwx_matrix_keep_input": (ctypes.c_int, [c_vp]),
    "fwx_matrix_patch_input": (ctypes.c_int, [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "fwx_matrix_enable_resume": (ctypes.c_int, [c_vp, c_i32]),
    "fwx_matrix_resume_bytes": (ctypes.c_int, [c_vp, c_i32, ctypes.POINTER(ctypes.c_uint64)]),
    "fwx_device_memory": (ctypes.c_int, [c_i32, ctypes.POINTER(ctypes.c_uint64),
                                         ctypes.POINTER(ctypes.c_uint64)]),
    "fwx_matrix_resolve": (ctypes.c_int, [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, ctypes.POINTER(FwxOpts),
                                          ctypes.POINTER(c_i32)]),
    "fwx_matrix_enable_path_log": (ctypes.c_int, [c_vp]),
    "fwx_matrix_path_log_count": (ctypes.c_int, [c_vp, ctypes.POINTER(ctypes.c_uint64)]),
    "fwx_matrix_query_exact": (ctypes.c_int, [c_vp, c_i32, c_i32, ctypes.POINTER(ctypes.c_double),
                                              c_vp, c_i32]),
    "fwx_matrix_query_exact_batch": (ctypes.c_int, [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_i32]),
    "fwx_matrix_create_multi": (ctypes.c_int, [ctypes.POINTER(c_vp), c_i32, c_i32, c_i32, c_i32, c_i32,
                                               ctypes.POINTER(c_i32), c_i32]),
    "fwx_matrix_create_part": (ctypes.c_int, [ctypes.POINTER(c_vp), c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32,
                                              c_vp, c_vp]),
    "fwx_matrix_part_rows": (ctypes.c_int, [c_vp, c_i32, ctypes.POINTER(c_i32), ctypes.POINTER(c_i32)]),
    "fwx_matrix_domain_bits": (ctypes.c_int, [c_vp, ctypes.POINTER(c_i32)]),
    "fwx_matrix_set_domain": (ctypes.c_int, [c_vp, c_i32]),
    "fwx_matrix_parts": (ctypes.c_int, [c_vp, ctypes.POINTER(c_i32)]),
    "fwx_matrix_set_timing": (ctypes.c_int, [c_vp, c_i32]),
    "fwx_matrix_get_timing": (ctypes.c_int, [c_vp, ctypes.POINTER(FwxMultiTiming)]),
    "fwx_matrix_comm_ranks": (ctypes.c_int, [c_vp]),
    "fwx_solve_multi_f64": (ctypes.c_int, [c_i32, c_vp, c_vp, c_vp, c_i32, ctypes.POINTER(c_i32), c_i32,
                                           ctypes.POINTER(FwxOpts)]),
    "fwx_solve_multi_f32": (ctypes.c_int, [c_i32, c_vp, c_vp, c_vp, c_i32, ctypes.POINTER(c_i32), c_i32,
                                           ctypes.POINTER(FwxOpts)]),
    "fwx_dev_relax": (ctypes.c_int, [ctypes.POINTER(FwxSlab), ctypes.POINTER(FwxPivots), c_i32,
                                     c_vp, c_vp]),
    "fwx_dev_relax_skip": (ctypes.c_int, [ctypes.POINTER(FwxSlab), ctypes.POINTER(FwxPivots), c_i32,
                                          c_vp, c_i32, c_i32, c_vp]),
    "fwx_dev_panel": (ctypes.c_int, [ctypes.POINTER(FwxSlab), c_vp, c_vp, c_vp, c_vp]),
    "fwx_dev_solve": (ctypes.c_int, [ctypes.POINTER(FwxSlab), ctypes.POINTER(FwxOpts)]),
    "fwx_dev_follow_paths": (ctypes.c_int, [c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp,
                                            c_vp, c_i32, c_vp]),
    "fwx_dev_panel_snap": (ctypes.c_int, [ctypes.POINTER(FwxSlab), c_vp, c_vp, ctypes.POINTER(FwxTrace),
                                          c_vp]),
    "fwx_dev_relax_fused": (ctypes.c_int, [ctypes.POINTER(FwxSlab), ctypes.POINTER(FwxPivots),
                                           ctypes.POINTER(FwxFusedScratch), ctypes.POINTER(FwxTrace),
                                           c_vp, c_i32, c_vp]),
    "fwx_dev_relax_fused_skip": (ctypes.c_int, [ctypes.POINTER(FwxSlab), ctypes.POINTER(FwxPivots),
                                                ctypes.POINTER(FwxFusedScratch),
                                                ctypes.POINTER(FwxTrace), c_vp, c_i32, c_i32, c_i32,
                                                c_vp]),
    "fwx_dev_check_nonneg": (ctypes.c_int, [ctypes.POINTER(FwxSlab), c_vp, c_vp]),
}

# The batched solves (csrc/fwx_batch.hip).  Every argument list of the family is put together from these pieces, each
# named once: how a batch is addressed, its three arrays, the items of the exact lists.
_OPTS, _TRACE = ctypes.POINTER(FwxOpts), ctypes.POINTER(FwxTrace)
_UNIFORM = [c_i32, c_i32]                                   # count, n
_RAGGED = [c_i32, c_vp]                                     # count, n_each
_ARRAYS = [c_vp, c_vp, c_vp]                                # rate, next, hops
_ITEMS = [c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32]       # items, mat, src, dst, len_out, path_out, cap
_SCRATCH = [c_vp, ctypes.c_size_t]                          # the large tier's scratch panels
for _stem, _batch in (("batch", _UNIFORM), ("batch_mid", _UNIFORM), ("batch_large", _UNIFORM), ("ragged", _RAGGED),
                      ("ragged_mid", _RAGGED), ("ragged_large", _RAGGED)):
    for _t in ("f64", "f32"):                               # ..., updates_each, [the items,] opts
        SIGNATURES["fwx_solve_%s_%s" % (_stem, _t)] = (ctypes.c_int, _batch + _ARRAYS + [c_vp, _OPTS])
        SIGNATURES["fwx_solve_%s_lists_%s" % (_stem, _t)] = (ctypes.c_int, _batch + _ARRAYS + [c_vp] + _ITEMS + [_OPTS])
for _stem, _extra in (("batch", []), ("batch_mid", []), ("batch_large", _SCRATCH)):
    # count, n, dtype, the arrays, stride, [k_begin, k_end | trace], d_updates_each, [scratch,] stream
    SIGNATURES["fwx_dev_solve_" + _stem] = (
        ctypes.c_int, _UNIFORM + [c_i32] + _ARRAYS + [ctypes.c_int64, c_i32, c_i32, c_vp] + _extra + [c_vp])
    SIGNATURES["fwx_dev_solve_%s_traced" % _stem] = (
        ctypes.c_int, _UNIFORM + [c_i32] + _ARRAYS + [ctypes.c_int64, _TRACE, c_vp] + _extra + [c_vp])
    # count, n, stride, next0, trace, the items, scratch, stream
    SIGNATURES["fwx_dev_exact_paths_" + _stem] = (
        ctypes.c_int, _UNIFORM + [ctypes.c_int64, c_vp, _TRACE] + _ITEMS + [c_vp, c_vp])
for _mid, _work, _extra in (("", [], []), ("_mid", [], []), ("_large", [c_vp], _SCRATCH)):
    # count, n_each, offset_out, order_out, tier_count_out, [work_out]
    SIGNATURES["fwx_ragged%s_plan" % _mid] = (ctypes.c_int, _RAGGED + [c_vp, c_vp, c_vp] + _work)
    # count, dtype, the arrays, d_n_each, d_offset, d_order, tier_count, [work, d_work,] trace, d_updates_each,
    # [scratch,] stream
    SIGNATURES["fwx_dev_solve_ragged" + _mid] = (
        ctypes.c_int, [c_i32, c_i32] + _ARRAYS + [c_vp, c_vp, c_vp, c_vp] + 2 * _work + [_TRACE, c_vp] + _extra + [c_vp])
    # count, d_n_each, d_offset, n_max, next0, trace, the items, scratch, stream
    SIGNATURES["fwx_dev_exact_paths_ragged" + _mid] = (
        ctypes.c_int, _RAGGED + [c_vp, c_i32, c_vp, _TRACE] + _ITEMS + [c_vp, c_vp])
# What-if sweeps: count, n, [dtype,] the base, patches, items, [full,] updates, stream | opts
_SWEEP = [ctypes.POINTER(FwxSweepPatches), ctypes.POINTER(FwxSweepItems)]
SIGNATURES["fwx_dev_solve_sweep"] = (
    ctypes.c_int, _UNIFORM + [c_i32] + _ARRAYS + _SWEEP + [ctypes.POINTER(FwxSweepFull), c_vp, c_vp])
SIGNATURES["fwx_dev_solve_sweep_mid"] = (
    ctypes.c_int, _UNIFORM + [c_i32] + _ARRAYS + _SWEEP + [ctypes.POINTER(FwxSweepFull), c_vp] + _SCRATCH + [c_vp])
for _t in ("f64", "f32"):
    SIGNATURES["fwx_solve_sweep_" + _t] = (ctypes.c_int, _UNIFORM + _ARRAYS + _SWEEP + [c_vp, _OPTS])
    SIGNATURES["fwx_solve_sweep_mid_" + _t] = (ctypes.c_int, _UNIFORM + _ARRAYS + _SWEEP + [c_vp, _OPTS])
SIGNATURES.update({
    "fwx_test_sweep_mid_slots": (ctypes.c_int, [c_i32, c_i32, ctypes.c_size_t]),
    "fwx_test_batch_wave_max_n": (ctypes.c_int, []),
    "fwx_test_batch_mid_min_n": (ctypes.c_int, []),
    "fwx_test_batch_mid_block": (ctypes.c_int, []),
    "fwx_test_batch_large_min_n": (ctypes.c_int, []),
    "fwx_test_batch_large_geometry": (ctypes.c_int, [ctypes.POINTER(c_i32)]),
    "fwx_test_batch_lists_chunk": (ctypes.c_int64, [c_i32, c_i32]),
    # count, large_count, work, scratch_bytes, group_first, cap, totals
    "fwx_test_ragged_large_schedule": (ctypes.c_int, [c_i32, c_i32, c_vp, ctypes.c_size_t, c_vp, c_i32, c_vp]),
})

_LIB = None


def lib():
    """Load libfwx.so from the package directory.  Raises if it has not been built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libfwx.so is missing at %s -- build it with `python -m floydwarshall_amd.build` "
                "(hipcc, gfx950).  floydwarshall_amd has no CPU fallback." % LIB_PATH)
        # One HIP runtime per process, and by default the one libfwx was BUILT AGAINST (/opt/rocm,
        # found through the library's RUNPATH): nothing else is imported here.  torch wheels bundle
        # their own libamdhip64.so.7 (same SONAME, an older ROCm); a program that needs torch in the
        # same process (floydwarshall_amd.dist: torch.distributed) must import torch BEFORE this
        # loader runs, so that libfwx's DT_NEEDED resolves to the copy torch initialises -- the other
        # order leaves torch with "No HIP GPUs are available".  That pairing works but is not the one
        # the library is built and fuzzed on; runtime_versions() reports it and a mismatch is logged
        # once (FWX_STRICT_RUNTIME=1 turns it into an error).
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError here = header/library mismatch
            fn.restype = res
            fn.argtypes = args
        if L.fwx_abi_version() != FWX_ABI_VERSION:
            raise RuntimeError("libfwx ABI version mismatch")
        _LIB = L
        _check_runtime(L)
    return _LIB


def runtime_versions():
    """(HIP_VERSION libfwx was compiled against, version of the HIP runtime it is bound to in this
    process, major.minor agree).  The runtime version is 0 where hipRuntimeGetVersion fails."""
    built, run = c_i32(0), c_i32(0)
    same = lib().fwx_hip_versions(ctypes.byref(built), ctypes.byref(run))
    return int(built.value), int(run.value), bool(same)


def _check_runtime(L):
    built, run = c_i32(0), c_i32(0)
    if L.fwx_hip_versions(ctypes.byref(built), ctypes.byref(run)) or run.value == 0:
        return
    msg = ("libfwx was built against HIP %d but is bound to HIP runtime %d in this process (another "
           "library -- a torch wheel bundles its own libamdhip64 -- was loaded first).  Load "
           "floydwarshall_amd before it, or do not import it at all, to run on the runtime the library "
           "was built and fuzzed on." % (built.value, run.value))
    if os.environ.get("FWX_STRICT_RUNTIME") == "1":
        raise RuntimeError(msg)
    import warnings
    warnings.warn(msg, RuntimeWarning, stacklevel=3)


def check(status, what):
    if status < 0:
        raise FwxError(status, what)
    return status
