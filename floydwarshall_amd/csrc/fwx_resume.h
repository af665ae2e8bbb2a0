// fwx_resume.h -- resumable solves (fwx_matrix_enable_resume / fwx_matrix_resolve, SURVEY.md section 8f row
// f3): what a handle keeps so that a solve of a PATCHED input can start at a stored state instead of at pivot 0,
// and the host code over it.  One copy for both handle kinds: a single-device handle is one slab of all rows, a
// partitioned handle (fwx_multi.hip) is one slab per partition; SlabData is what either owns per slab, and
// fwx_handle.h visits the slabs of a handle.  Not installed, not part of the ABI.
//   panels      the time-k snapshots the fused engine produces anyway, for ALL pivots instead of ping-pong
//               buffers: w[k][j] = row k at time k (every slab keeps all of them: a partition receives them
//               anyway, and the replay of a changed entry (i, j) needs w[k][j] for all k), ct[k][i] = column k at
//               time k for the slab's rows (NaN at i == k), cnt / wh / cht likewise for next-hops and hops
//   checkpoint  a copy of the slab's state (rate, next, hops, the three trace arrays) at the START of step
//               pivot[c], a multiple of 64
// An input entry (i,j) is an OPERAND only in steps i and j, so patched entries cannot influence any
// other entry before step m = min over their indices: the state at a checkpoint <= m is the stored
// one except for the patched entries themselves, and those are replayed through the pivots before
// the checkpoint from the stored panels (their operands (i,k), (k,j), k < m, are not patched).
#ifndef FWX_RESUME_H
#define FWX_RESUME_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <functional>
#include <vector>

#include "fwx_internal.h"

namespace fwxi {

// Replay of patched input entries through the pivots [0, c) they were not part of.  One wave per entry
// (i, j): lane l of chunk q forms the candidate of pivot
// k = 64 q + l from the stored panels, c[k] = ct[k][i] * w[k][j] -- the very operands step k used --
// and the wave folds the chunk at once: on the reference's domain the strict fold of Algorithms.hs:55
// ends at max(x, max_k c[k]) (a NaN candidate never wins), and its LAST update is the FIRST pivot that
// attains that maximum, which gives next = cnt[k*][i], hops = cht[k*][i] + wh[k*][j], last = k*.
// Checkpoints are multiples of 64, so the value at every checkpoint <= c falls on a chunk boundary
// and is written into that checkpoint; the value at time c goes to the live arrays.
struct ReplayTargets {
    enum { MAX = 20 };
    int count;
    int pivot[MAX];
    void *rate[MAX];
    int32_t *next[MAX], *hops[MAX], *last[MAX];
};

template <typename T>
__global__ __launch_bounds__(64) void replay_entries_kernel(const int64_t *index, int n, int ld, int row0, int c,
                                                            const T *rate0, const int32_t *next0,
                                                            const int32_t *hops0, const T *w, const T *ct,
                                                            const int32_t *cnt, const int32_t *wh,
                                                            const int32_t *cht, ReplayTargets tg)
{
    const int64_t idx = index[blockIdx.x];
    // idx: offset in the arrays of this slab (local row * n + column); row0: global index of its first row
    const int i = (int)(idx / n), j = (int)(idx % n), lane = threadIdx.x;
    T x = rate0[idx];
    int nx = next0 ? next0[idx] : -1, hp = hops0 ? hops0[idx] : 0, last = -1;
    int t = 0;
    for (int k0 = 0; k0 <= c; k0 += 64) {
        while (t < tg.count && tg.pivot[t] == k0) {
            if (lane == 0) {
                ((T *)tg.rate[t])[idx] = x;
                if (tg.next[t]) tg.next[t][idx] = nx;
                if (tg.hops[t]) tg.hops[t][idx] = hp;
                if (tg.last[t]) tg.last[t][idx] = last;
            }
            ++t;
        }
        if (k0 == c || i + row0 == j) continue;          // a diagonal entry is never a target (:54)
        const int k = k0 + lane;
        T v = ct[(size_t)k * ld + i] * w[(size_t)k * n + j];
        int arg = k;
        if (!(v == v)) v = -INFINITY;                    // NaN (inf * 0) never wins a strict compare
        for (int d = 1; d < 64; d <<= 1) {               // max, earliest pivot on ties
            const T ov = __shfl_xor(v, d);
            const int oa = __shfl_xor(arg, d);
            if (ov > v || (ov == v && oa < arg)) { v = ov; arg = oa; }
        }
        if (x < v) {
            x = v;
            last = arg;
            if (cnt) nx = cnt[(size_t)arg * ld + i];
            if (cht) hp = cht[(size_t)arg * ld + i] + wh[(size_t)arg * n + j];
        }
    }
}

static_assert(FWX_MAX_CHECKPOINTS < ReplayTargets::MAX, "the replay writes every checkpoint and the live arrays");

// One matrix state: a null member is an array the handle does not carry.
struct Arrays {
    void *rate = nullptr;
    int32_t *next = nullptr, *hops = nullptr, *last = nullptr, *at_col = nullptr, *at_row = nullptr;
};

// What one slab keeps, on the slab's device.  All null: nothing allocated.
struct ResumeStore {
    Arrays cp[FWX_MAX_CHECKPOINTS];                // the checkpoints, Resume::count of them
    void *w = nullptr, *ct = nullptr;              // nd x nd, nd x ct_ld elements of the handle's dtype
    int32_t *cnt = nullptr, *wh = nullptr, *cht = nullptr;
    int64_t *idx = nullptr;                        // FWX_MAX_PATCH entry offsets of a resolve, on the device
};

// The handle-wide bookkeeping (fwx_matrix::resume); the stores are the slabs' (SlabData::store).
struct Resume {
    int count = 0;
    std::vector<int> pivot;                        // ascending, each a multiple of 64 in (0, n)
    int valid_upto = 0;    // panels of pivots [0, valid_upto) and checkpoints with pivot <= valid_upto
                           // belong to the solve of the CURRENT kept input (0: nothing to resume from)
    int state_at = -1;     // the live arrays hold the kept input brought to the start of step state_at
                           // (0 right after an upload / patch; -1: unknown, e.g. solved twice over)
    int checkpoint_at(int k0) const                // index of the checkpoint at pivot k0, or -1
    {
        for (int c = 0; c < count; ++c)
            if (pivot[(size_t)c] == k0) return c;
        return -1;
    }
};

// What a handle owns for rows [row0, row0 + rows) of its nd x nd device matrix, on `device`: a single-device
// handle has one (row0 = 0, rows = nd, ct_ld = (nd + 3) & ~3), a partitioned handle one per partition (Part,
// fwx_multi.hip).  A null array is one the handle does not carry.  (fwx_dev_solve fills one with the caller's
// arrays for the length of the call.)
struct SlabData {
    int device = 0, row0 = 0, rows = 0, ct_ld = 0;
    void *rate = nullptr;
    int32_t *next = nullptr, *hops = nullptr;
    fwx::PathLog plog;                             // the path trace (rows x nd each), or null: not enabled
    int32_t *next0 = nullptr;                      // the uploaded next-hops: the trace's and the kept input's
    void *rate0 = nullptr;                         // the kept input (fwx_matrix_keep_input): rates ...
    int32_t *hops0 = nullptr;                      // ... and hops
    ResumeStore store;                             // checkpoints and all-pivot panels (fwx_matrix_enable_resume)
    hipStream_t main = nullptr;                    // every operation on the slab runs on it: a non-blocking stream
                                                   // of the handle's own, never the legacy null stream
};

// A slab as the functions below take it: the live arrays, the kept input, the geometry.  A view filled at the
// call site; it owns nothing.
struct Slab {
    Arrays live;                                   // the arrays a solve works on, with the trace
    Arrays kept;                                   // the kept input (fwx_matrix_keep_input): rate0 / next0 / hops0
    int rows = 0, row0 = 0, nd = 0, ct_ld = 0;
    size_t es = 0;                                 // bytes per rate element
    hipStream_t s = nullptr;
};
inline Slab slab_of(const SlabData &d, int nd, size_t es)
{
    Slab v;
    v.live = {d.rate, d.next, d.hops, d.plog.last, d.plog.at_col, d.plog.at_row};
    v.kept.rate = d.rate0; v.kept.next = d.next0; v.kept.hops = d.hops0;
    v.rows = d.rows; v.row0 = d.row0; v.nd = nd; v.ct_ld = d.ct_ld;
    v.es = es;
    v.s = d.main;
    return v;
}

// Element counts of what a slab's store holds: per checkpoint array, per column-panel array, per row-panel
// array.  The allocator and fwx_matrix_resume_bytes both go through here.  (An empty partition keeps a
// four-column placeholder.)
struct SlabCells { uint64_t cells, col_cells, w_cells; };
inline SlabCells slab_cells(int rows, int nd, int ct_ld)
{
    return {(uint64_t)rows * (uint64_t)nd, (uint64_t)nd * (uint64_t)(ct_ld ? ct_ld : 4), (uint64_t)nd * (uint64_t)nd};
}

// The checkpoint pivots of a matrix of order n: the multiples of 64 closest to q * n / (checkpoints + 1),
// ascending, inside (0, n), of which `block_start` (if given) keeps those where a pass of the handle begins.
inline std::vector<int> checkpoint_pivots(int n, int checkpoints, const std::function<bool(int)> &block_start = nullptr)
{
    std::vector<int> pivot;
    for (int q = 1; q <= checkpoints; ++q) {
        const int p = (int)(((int64_t)n * q / (checkpoints + 1) + 32) / 64 * 64);
        if (p <= 0 || p >= n || (!pivot.empty() && p <= pivot.back())) continue;
        if (block_start && !block_start(p)) continue;
        pivot.push_back(p);
    }
    return pivot;
}

// dst <- src for every array both carry, on the slab's stream.
inline int copy_arrays(const Slab &v, const Arrays &dst, const Arrays &src)
{
    const size_t cells = (size_t)v.rows * (size_t)v.nd;
    auto copy = [&](void *d, const void *s, size_t es) -> int {
        if (d && s) FWX_HIP(hipMemcpyAsync(d, s, cells * es, hipMemcpyDeviceToDevice, v.s));
        return FWX_OK;
    };
    int rc;
    if ((rc = copy(dst.rate, src.rate, v.es)) || (rc = copy(dst.next, src.next, 4)) || (rc = copy(dst.hops, src.hops, 4)) ||
        (rc = copy(dst.last, src.last, 4)) || (rc = copy(dst.at_col, src.at_col, 4)) ||
        (rc = copy(dst.at_row, src.at_row, 4)))
        return rc;
    return FWX_OK;
}
inline int save_checkpoint(ResumeStore &st, const Slab &v, int c) { return copy_arrays(v, st.cp[c], v.live); }
inline int restore_checkpoint(const ResumeStore &st, const Slab &v, int c) { return copy_arrays(v, v.live, st.cp[c]); }
inline int restore_kept(const Slab &v) { return copy_arrays(v, v.live, v.kept); }   // (the trace is not input)
inline int keep_live(const Slab &v) { return copy_arrays(v, v.kept, v.live); }

// One array of a slab on the current device.  (A zero-size array -- an empty partition -- is 16 bytes.)
template <typename P> inline int slab_array(P **p, uint64_t bytes)
{
    FWX_HIP(hipMalloc((void **)p, bytes ? bytes : 16));
    return FWX_OK;
}

// The path trace of a slab of `cells` entries (fwx_matrix_enable_path_log).  next0 = the UPLOADED next-hops: if
// the arrays hold an unsolved upload (`fresh`), keep it; otherwise a traced solve is refused until the next
// upload, which fills next0.
inline int trace_alloc(SlabData &d, size_t cells, bool fresh)
{
    int rc;
    if ((rc = slab_array(&d.plog.at_col, cells * 4)) || (rc = slab_array(&d.plog.at_row, cells * 4)) ||
        (!d.next0 && (rc = slab_array(&d.next0, cells * 4))) || (rc = slab_array(&d.plog.last, cells * 4)))
        return rc;
    if (fresh) {
        FWX_HIP(hipMemcpyAsync(d.next0, d.next, cells * 4, hipMemcpyDeviceToDevice, d.main));
        FWX_HIP(hipStreamSynchronize(d.main));
    }
    return FWX_OK;
}

// The kept input of a slab (fwx_matrix_keep_input) for the arrays it carries; next0 may be there already, as
// the trace's.
inline int kept_alloc(SlabData &d, size_t cells, size_t es)
{
    int rc;
    if ((rc = slab_array(&d.rate0, cells * es)) || (d.next && !d.next0 && (rc = slab_array(&d.next0, cells * 4))) ||
        (d.hops && (rc = slab_array(&d.hops0, cells * 4))))
        return rc;
    return FWX_OK;
}

// (the store's device must be current)
inline void store_free(ResumeStore &st)
{
    auto drop = [](void *p) { if (p) (void)hipFree(p); };
    for (const Arrays &a : st.cp) { drop(a.rate); drop(a.next); drop(a.hops); drop(a.last); drop(a.at_col); drop(a.at_row); }
    drop(st.w); drop(st.ct); drop(st.cnt); drop(st.wh); drop(st.cht); drop(st.idx);
    st = ResumeStore();
}

// Everything a slab owns: its stream, then its arrays and its store.  The slab's device must be current and
// its streams drained (drain_stream).
inline void slab_release(SlabData &d)
{
    if (d.main) (void)hipStreamDestroy(d.main);
    void *arrays[] = {d.rate, d.next, d.hops, d.plog.last, d.plog.at_col, d.plog.at_row, d.next0, d.rate0, d.hops0};
    for (void *a : arrays)
        if (a) (void)hipFree(a);
    store_free(d.store);
    d = SlabData();
}

// `count` checkpoints of the arrays the slab carries, the all-pivot panels and the index buffer, on the
// current device; a partial set is released again.
inline int store_alloc(ResumeStore &st, const Slab &v, int count)
{
    const SlabCells d = slab_cells(v.rows, v.nd, v.ct_ld);
    auto all = [&]() -> int {
        int rc;
        for (int c = 0; c < count; ++c) {
            Arrays &a = st.cp[c];
            if ((rc = slab_array(&a.rate, d.cells * v.es))) return rc;
            if (v.live.next && (rc = slab_array(&a.next, d.cells * 4))) return rc;
            if (v.live.hops && (rc = slab_array(&a.hops, d.cells * 4))) return rc;
            if (v.live.last && ((rc = slab_array(&a.last, d.cells * 4)) || (rc = slab_array(&a.at_col, d.cells * 4)) ||
                                (rc = slab_array(&a.at_row, d.cells * 4))))
                return rc;
        }
        if ((rc = slab_array(&st.w, d.w_cells * v.es)) || (rc = slab_array(&st.ct, d.col_cells * v.es))) return rc;
        if (v.live.next && (rc = slab_array(&st.cnt, d.col_cells * 4))) return rc;
        if (v.live.hops && ((rc = slab_array(&st.wh, d.w_cells * 4)) || (rc = slab_array(&st.cht, d.col_cells * 4)))) return rc;
        return slab_array(&st.idx, (uint64_t)FWX_MAX_PATCH * 8);
    };
    const int rc = all();
    if (rc) store_free(st);
    return rc;
}

// Rows k0 ... of the all-pivot panels: where the pass that starts at pivot k0 writes (and later reads) them.
struct PanelRows { void *w, *ct; int32_t *cnt, *wh, *cht; };
inline PanelRows store_panels(const ResumeStore &st, const Slab &v, int k0)
{
    const size_t row = (size_t)k0 * (size_t)v.nd, col = (size_t)k0 * (size_t)v.ct_ld;
    return {(char *)st.w + row * v.es, (char *)st.ct + col * v.es, st.cnt ? st.cnt + col : nullptr,
            st.wh ? st.wh + row : nullptr, st.cht ? st.cht + col : nullptr};
}

// Entry q of a patch into the kept input at slab offset `off` (local row * nd + column): plain small copies.
inline int patch_kept(const Slab &v, size_t off, int32_t q, const void *rate_vals, const int32_t *next_vals,
                      const int32_t *hops_vals)
{
    FWX_HIP(hipMemcpyAsync((char *)v.kept.rate + off * v.es, (const char *)rate_vals + (size_t)q * v.es, v.es,
                           hipMemcpyHostToDevice, v.s));
    if (next_vals) FWX_HIP(hipMemcpyAsync(v.kept.next + off, next_vals + q, 4, hipMemcpyHostToDevice, v.s));
    if (hops_vals) FWX_HIP(hipMemcpyAsync(v.kept.hops + off, hops_vals + q, 4, hipMemcpyHostToDevice, v.s));
    return FWX_OK;
}

// The entries at the slab offsets `offs` (patched in the kept input already), replayed from the kept input
// through the stored panels into the live arrays -- which hold checkpoint c_idx -- and into every checkpoint
// up to it, which thereby stay valid for the new input.  Everything is queued on the slab's stream and
// nothing waits: `offs` is read by an asynchronous copy and must stay alive until the stream has been
// synchronised.
template <typename T>
int replay_entries(const ResumeStore &st, const Slab &v, const Resume &R, int c_idx, const int64_t *offs, size_t count)
{
    ReplayTargets tg;
    memset(&tg, 0, sizeof(tg));
    auto target = [&](int pivot, const Arrays &a) {
        const int t = tg.count++;
        tg.pivot[t] = pivot;
        tg.rate[t] = a.rate; tg.next[t] = a.next; tg.hops[t] = a.hops; tg.last[t] = a.last;
    };
    for (int q = 0; q <= c_idx; ++q) target(R.pivot[(size_t)q], st.cp[q]);
    const int c = R.pivot[(size_t)c_idx];
    target(c, v.live);
    FWX_HIP(hipMemcpyAsync(st.idx, offs, count * 8, hipMemcpyHostToDevice, v.s));
    hipLaunchKernelGGL(replay_entries_kernel<T>, dim3((unsigned)count), dim3(64), 0, v.s, st.idx, v.nd, v.ct_ld, v.row0, c,
                       (const T *)v.kept.rate, v.live.next ? v.kept.next : nullptr, v.live.hops ? v.kept.hops : nullptr,
                       (const T *)st.w, (const T *)st.ct, st.cnt, st.wh, st.cht, tg);
    FWX_HIP(hipGetLastError());
    return FWX_OK;
}

}  // namespace fwxi

#endif
