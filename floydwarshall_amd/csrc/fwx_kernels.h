// fwx_kernels.h -- internal launch interface between the C ABI (fwx_api.hip) and the kernels.
#ifndef FWX_KERNELS_H
#define FWX_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

// Must equal FWX_UPDATE_SHARDS of include/fwx.h (power of two).
#define FWX_UPDATE_SHARDS_K 256

namespace fwx {

// Path trace for exact `_path` reconstruction (Algorithms.hs:55 concatenates the time-k paths of
// (i,k) and (k,j) whenever (i,j) improves).
struct PathLog {
    // What the reference's `_path` lists (Algorithms.hs:55) need, without storing a single list or
    // update record: three n x n int32 matrices.
    //   last[i][j]    pivot of the newest successful relaxation of (i,j) in the whole solve, -1 = never
    //   at_col[i][j]  the same, but as it stood at the START of step j  (entry (i,j) as pivot-COLUMN operand)
    //   at_row[i][j]  ...                 at the START of step i        (entry (i,j) as pivot-ROW operand)
    // path(i,j) = path_q(i,q) ++ path_q(q,j) with q = last[i][j]; path_q(i,q) needs the newest update of
    // (i,q) before step q = at_col[i][q], path_q(q,j) needs at_row[q][j]; the recursion only ever asks
    // for an entry "as of the step named by one of its own indices", so these three suffice.
    // Column k and row k of `last` are not modified during step k: the snapshots are plain copies.
    int32_t *last = nullptr;       // (null by default: a PathLog that was never filled in means "no trace")
    int32_t *at_col = nullptr;
    int32_t *at_row = nullptr;
};

// Record of the launch forms a process has used (test hook fwx_test_kernel_forms, fwx.h): one bit per
// form, and within a form one per instantiation that a threshold picks (tile size, passes per launch).
// Every launch site ORs its bit into one process-global word -- one relaxed host atomic per launch,
// nothing on the device; global because the partition sweeps launch from worker threads.  The names
// (fwx_test_kernel_form_name) are what floydwarshall_amd.engine.KERNEL_FORMS must list, in this order.
#define FWX_KERNEL_FORM_LIST(X)                                                                    \
    X(SMALL_SOLVE)          /* small_solve, n <= FWX_SMALL_N */                                    \
    X(RELAX_K)              /* relax_k, the per-k engine */                                        \
    X(ROWPANEL_F32)         /* launch_fused_panel */                                               \
    X(ROWPANEL_F64)                                                                                \
    X(COLPANEL_F32)         /* launch_fused_colpanel */                                            \
    X(COLPANEL_F64)                                                                                \
    X(PANELS_F32)           /* launch_fused_panels: fused_panels, compare form */                  \
    X(PANELS_F64)                                                                                  \
    X(PANELS_MAX_F32)       /* fused_panels, max form (rates only, in the domain) */               \
    X(PANELS_MAX_F64)                                                                              \
    X(PANELS_NEXT_F32)      /* fused_panels_next_f32<false> */                                     \
    X(PANELS_NEXT_TRACE_F32) /* fused_panels_next_f32<true> */                                     \
    X(PANELS_NEXT_F32_R32)  /* fused_panels_next_f32<false, 32>, beside a main launch */           \
    X(MAIN_SMALL_F32)       /* launch_fused_main: generic fused_main, 64 x 64 tiles */             \
    X(MAIN_LARGE_F32)       /* ... 128-row tiles */                                                \
    X(MAIN_SMALL_F64)                                                                              \
    X(MAIN_LARGE_F64)                                                                              \
    X(MAX_SMALL_F32)        /* fused_main_max<4, 1, 4, 1> */                                       \
    X(MAX_MID_F32)          /* fused_main_max<3, 1, 8, 1> */                                       \
    X(MAX_LARGE_F32)        /* fused_main_max<3, 1, 8, 2> */                                       \
    X(ARG_RI4_NP1_F32)      /* fused_main_arg<3, RI, NP> */                                        \
    X(ARG_RI4_NP2_F32)                                                                             \
    X(ARG_RI8_NP1_F32)                                                                             \
    X(ARG_RI8_NP2_F32)                                                                             \
    X(MAX_SMALL_F64)        /* fused_main<double, ..., MAXF = true> */                             \
    X(MAX_LARGE_F64)        /* fused_main_max_f64<2> */                                            \
    X(ARG_F64_RI4_NP1)      /* fused_main_arg_f64<2, 4, NP> (64 x 64 tiles) */                     \
    X(ARG_F64_RI4_NP2)                                                                             \
    X(ARG_F64_RI2_NP1)      /* fused_main_arg_f64<3, 2, NP> (FWX_ARG_F64_SHORT_TILES=1) */         \
    X(ARG_F64_RI2_NP2)

enum KernelForm {
#define FWX_KERNEL_FORM_ENUM(name) KF_##name,
    FWX_KERNEL_FORM_LIST(FWX_KERNEL_FORM_ENUM)
#undef FWX_KERNEL_FORM_ENUM
    KF_COUNT
};
static_assert(KF_COUNT <= 64, "one bit per form in a 64-bit word");

inline std::atomic<uint64_t> g_kernel_forms{0};
inline void note_form(KernelForm f) { g_kernel_forms.fetch_or(1ull << f, std::memory_order_relaxed); }

// Default store granularity of relax_k's rates-only path (RelaxArgs::store_bytes, FWX_PERK_STORE_BYTES):
// one full 64-byte sector per group of 4 lanes (profiles/r06_tune_relax_stores.txt, r06_bench_ab.txt).
#define FWX_PERK_STORE_BYTES_DEFAULT 64

template <typename T> struct RelaxArgs {
    T *rate;                       // slab: rows x n
    int32_t *next;                 // or nullptr
    int32_t *hops;                 // or nullptr
    const T *prow;                 // pivot row k at the start of step k (n elements)
    const int32_t *phops;          // its hops row (iff hops)
    const int32_t *pnext = nullptr;   // its next-hop row, or nullptr.  Algorithms.hs:55 concatenates
                                   // ikPath ++ kjPath: the head is next[i][k] unless ikPath is EMPTY
                                   // (next[i][k] < 0), then it is next[k][j].  nullptr: the caller
                                   // vouches that a winning product never has an empty ikPath (true
                                   // on the reference's domain, see fwx.h "Domain")
    int rows, n, row0, k;
    int flip;                      // 0: tiles in order; 1: reversed; 2: reversed in groups of 8 (XCD kept)
    long long temporal_bytes = -1; // the slab's last rows, this many bytes, are streamed with default-policy
                                   // loads in every launch, all rows before them non-temporally; < 0: all
                                   // default policy
    int store_bytes = 0;           // rates-only store granularity, 16 / 32 / 64 / 128 bytes (relax_k); 0:
                                   // FWX_PERK_STORE_BYTES_DEFAULT
    int skip_lo = 0, skip_hi = 0;  // slab rows [skip_lo, skip_hi) are left alone (multiples of 4):
                                   //   a look-ahead launch has already relaxed them
    unsigned long long *updates;   // FWX_UPDATE_SHARDS_K counters or nullptr
    PathLog plog;                  // plog.last == nullptr: no tracing (per-k engine: the slab must be the
                                   // whole matrix when tracing, the three matrices are indexed by
                                   // global row)
};

template <typename T> hipError_t launch_relax(const RelaxArgs<T> &a, hipStream_t s);

// relax_kt: pivots [k, k+np) on the whole n x n matrix in one streaming pass, rates only, operands from
// the snapshot panels of launch_fused_panels (compare form; the sweep's own fold is chosen per wave, see
// fold_compare).  n must be a multiple of 16 bytes of
// elements, rate and w 16-byte aligned.
#define FWX_PERK_KT_RPB 8          // rows per workgroup and loads in flight per thread: 8 x 8 is 8-10 % faster per
#define FWX_PERK_KT_UNROLL 8       //   pivot than relax_k's 4 x 4 at NP = 8 (profiles/r07_tune_relax_pivots.txt)
#define FWX_PERK_KT16_RPB 16       // the 16-pivot sweep (non-counting f32 only): its geometry
#define FWX_PERK_KT16_UNROLL 8     //   (profiles/r19_tune_relax_pivots.txt)
#define FWX_PERK_WALK_RPB 16       // relax_walk, the 16-pivot sweep since round 23: rows per workgroup, row slots in
#define FWX_PERK_WALK_UNROLL 8     //   flight, cache policy of the stream (WALK_POL_*, fwx_kernels.hip: 0 = default-
#define FWX_PERK_WALK_POL 0        //   policy loads everywhere), slots reloaded one by one behind their folds (1) or
#define FWX_PERK_WALK_ROLL false   //   in batches (0).  What was timed: profiles/r23_tune_relax_pivots.txt
#define FWX_PERK_DEEP_RPB 64       // relax_walk at 32 pivots and 8 bytes of a row per lane (round 25): rows per workgroup
#define FWX_PERK_DEEP_UNROLL 8     //   and row slots in flight.  What was timed: profiles/r25_tune_relax_pivots.txt
template <typename T> struct RelaxKtArgs {
    T *rate;                       // n x n
    const T *w;                    // w[t*n + j]      = row k+t at time k+t          (t < np)
    const T *ct;                   // ct[t*ct_ld + i] = column k+t at time k+t, NaN at i == k+t
    int ct_ld, n, k, np;           // np: 2, 4 or 8; 16 for f32 with updates == nullptr; 32 for that with `walk` as well
    int flip;                      // as RelaxArgs
    long long temporal_bytes = -1;
    int store_bytes = 0;
    bool fold_compare = false;     // true: the compare form of the fold in every tile (FWX_PERK_FOLD=compare); false: each
                                   // wave takes the max form where its operands allow it.  No result bit depends on it
    bool walk = false;             // np == 16: true: relax_walk sweeps (FWX_PERK_WALK); false: relax_kt, round 19's launch.
                                   // No result bit depends on it
    unsigned long long *updates = nullptr;   // FWX_UPDATE_SHARDS_K counters or nullptr
};
template <typename T> hipError_t launch_relax_kt(const RelaxKtArgs<T> &a, hipStream_t s);
// relax_tile (round 26, fwx_fused.hip): pivots [k, k+np) in ONE pass on 128 x 128 register tiles, operands from LDS;
// np a multiple of 64 up to 512 (round 30; w and ct then hold np contiguous rows / lines), f32, updates == nullptr,
// n >= 64.  The fold is chosen per tile and stage (max form where the tile's entries and operands allow it;
// fold_compare forces the compare form).  flip, temporal_bytes, store_bytes and walk are not read: no result bit
// depends on them.
// The tiles of a launch: all; all but the tile rows and tile columns [tx, tx + tw) (the main launch beside a look-ahead
// chain); or only those (the cross: one launch at a raised wave priority), and of those only the tiles whose other
// index is not in [tx - te, tx): what the cross of the band in front has already taken through these pivots.
enum TileSel { TILES_ALL = 0, TILES_EXCEPT = 1, TILES_CROSS = 2 };
hipError_t launch_relax_tile(const RelaxKtArgs<float> &a, hipStream_t s, TileSel sel = TILES_ALL, int tx = 0,
                             int tw = 1, int te = 0);

// Whole solve (pivots [k_begin,k_end)) of an n <= FWX_SMALL_N matrix in one single-workgroup launch.
#define FWX_SMALL_N 128
template <typename T>
hipError_t launch_small_solve(T *rate, int32_t *next, int32_t *hops, int n, int k_begin, int k_end,
                              unsigned long long *updates, PathLog plog, hipStream_t s);

// Batched small solves: `count` matrices of order n <= FWX_SMALL_N, matrix b at rate + b*stride (next / hops
// alike; stride >= n*n elements, the gap is never touched), pivots [k_begin,k_end) of each, in one launch (one per
// 2^21 matrices).  n <= wave_max_n (at most FWX_BATCH_WAVE_N): one wave per matrix, the matrix in registers,
// no LDS; otherwise small_solve's body with one workgroup per matrix.  updates_each: count counters or
// nullptr, counter b is incremented by U of matrix b.  No kernel-form bit is recorded.
// plog (optional; plog.last != nullptr): the path trace of matrix b goes to the three arrays at + b*stride, pitch n
// like next -- every cell of the n x n part is written, the gap never.  Needs next and the whole pivot range
// [0, n) (hipErrorInvalidValue otherwise).
#define FWX_BATCH_WAVE_N 16
template <typename T>
hipError_t launch_batch_solve(T *rate, int32_t *next, int32_t *hops, int count, int n, long long stride,
                              int k_begin, int k_end, unsigned long long *updates_each, int wave_max_n,
                              hipStream_t s, PathLog plog = PathLog());

// What-if sweeps: `count` variants of ONE base matrix of order n <= FWX_SMALL_N (pitch n, never written) in one
// launch (one per 2^21 variants), tiers as launch_batch_solve.  Variant b is the base with the patches [patch_ptr[b],
// patch_ptr[b+1]) applied in list order (patch_next / patch_hops optional: that field of the cell keeps the base's
// value); it answers its items [item_ptr[b], item_ptr[b+1]) into item_rate / item_next / item_hops (the last two
// optional) and, where a full output is given (each optional), stores its whole n x n part at + b*full_stride,
// diagonal included, the gap never.  counter b of updates_each (or nullptr) is incremented by U of variant b.
// Everything is device memory.  The kernels clamp each ptr range into [0, total] and pass over patch indices and
// item vertices that do not belong to the order; what the host arguments decide is hipErrorInvalidValue.
template <typename T> struct SweepTables {
    const int64_t *patch_ptr = nullptr;
    long long patch_total = 0;
    const int64_t *patch_index = nullptr;
    const T *patch_rate = nullptr;
    const int32_t *patch_next = nullptr, *patch_hops = nullptr;
    const int64_t *item_ptr = nullptr;
    long long item_total = 0;
    const int32_t *item_src = nullptr, *item_dst = nullptr;
    T *item_rate = nullptr;
    int32_t *item_next = nullptr, *item_hops = nullptr;
    T *full_rate = nullptr;
    int32_t *full_next = nullptr, *full_hops = nullptr;
    long long full_stride = 0;
};
template <typename T>
hipError_t launch_sweep_solve(const T *base_rate, const int32_t *base_next, const int32_t *base_hops, int count, int n,
                              const SweepTables<T> &t, unsigned long long *updates_each, int wave_max_n, hipStream_t s);

// Mid tier of the batched solves (fwx_mid.hip): `count` matrices of one order n <= FWX_MID_N, same layout and
// counters as launch_batch_solve, one workgroup per matrix, the matrix resident in global memory and FWX_MID_B
// pivots per pass from time-k snapshot panels in LDS.  Any n from 1 up, any stride >= n*n, scalar accesses only.
// plog (optional; plog.last != nullptr): the path trace as launch_batch_solve lays it out -- every cell of the n x n
// part written by the kernel itself, the gap never; needs next and the whole pivot range [0, n)
// (hipErrorInvalidValue otherwise).  One launch per 2^21 matrices.
#define FWX_MID_N 256
#ifndef FWX_MID_B                  // a power of two up to 16 (build variants: -DFWX_MID_B=8)
#define FWX_MID_B 16
#endif
template <typename T>
hipError_t launch_batch_mid(T *rate, int32_t *next, int32_t *hops, int count, int n, long long stride, int k_begin,
                            int k_end, unsigned long long *updates_each, hipStream_t s, PathLog plog = PathLog());

// What-if sweeps on the mid tier (fwx_mid.hip): launch_sweep_solve's contract for n <= FWX_MID_N, the variants built
// and solved in workspace slots.  ONE launch of `slots` workgroups; workgroup s owns slot s of `scratch` (device
// memory, 16-byte aligned, FWX_MID_SWEEP_SLOT_BYTES(n) per slot -- an upper bound over dtype and field set: the rates,
// then next, then hops, each n*n elements at pitch n) and handles the variants s, s + slots, ...: base -> slot, the
// patches in list order, the mid tier's body on the slot, the items and the full outputs from the slot.  Nothing past
// slots x FWX_MID_SWEEP_SLOT_BYTES(n) bytes of the scratch is touched and no result bit depends on `slots`.
// hipErrorInvalidValue for what launch_sweep_solve refuses, for slots < 1 and for scratch that is null or misaligned.
#define FWX_MID_SWEEP_SLOT_BYTES(n) ((size_t)(n) * (n) * 16)
template <typename T>
hipError_t launch_sweep_mid(const T *base_rate, const int32_t *base_next, const int32_t *base_hops, int count, int n,
                            const SweepTables<T> &t, unsigned long long *updates_each, void *scratch, int slots,
                            hipStream_t s);

// Large tier of the batched solves (fwx_large.hip): `count` matrices of one order n <= FWX_LARGE_N, same layout and
// counters as launch_batch_mid, several workgroups per matrix: per block of FWX_LARGE_B pivots one panel launch
// (column strips of FWX_LARGE_S, matrices) that writes the time-k snapshot panels to `scratch`, and one sweep launch
// (column tiles of FWX_LARGE_TC, row tiles of FWX_LARGE_TR, matrices) that folds them into the matrix.  Any n from 1
// up, any stride >= n*n, scalar accesses only.  plog (optional; plog.last != nullptr): the path trace as
// launch_batch_mid lays it out -- `last` filled by a launch of its own before the first block, every cell of the n x n
// part of at_row / at_col written by exactly one panel workgroup, the gap never; needs next and the whole pivot range
// [0, n) (hipErrorInvalidValue otherwise) and no scratch of its own.  scratch: device memory, 16-byte aligned,
// FWX_LARGE_SCRATCH_BYTES(n) per matrix (an upper bound over dtype and field set: W, Ct, WN, CNt, WH, CHt, each
// [B][n]); the batch is solved in groups of scratch_bytes / FWX_LARGE_SCRATCH_BYTES(n) matrices, one after the other
// on s, and nothing past group x per-matrix bytes is touched.  hipErrorInvalidValue for scratch that is null,
// misaligned or smaller than one matrix's -- only with a non-empty pivot range.
#define FWX_LARGE_N 1024
#define FWX_LARGE_B 16             // pivots per block
#define FWX_LARGE_S 48             // B + S = 64: a panel row is one wave
#ifndef FWX_LARGE_TR               // rows of a sweep tile, a multiple of FWX_LARGE_ROWS (build variants: -DFWX_LARGE_TR=32)
#define FWX_LARGE_TR 16
#endif
#ifndef FWX_LARGE_ROWS             // rows a sweep thread folds together
#define FWX_LARGE_ROWS 4
#endif
#ifndef FWX_LARGE_TC               // columns of a sweep tile = threads of a sweep workgroup, a multiple of 64
#define FWX_LARGE_TC 256
#endif
#define FWX_LARGE_SCRATCH_BYTES(n) ((size_t)(n) * (2 * FWX_LARGE_B * 16))
template <typename T>
hipError_t launch_batch_large(T *rate, int32_t *next, int32_t *hops, int count, int n, long long stride, int k_begin,
                              int k_end, unsigned long long *updates_each, void *scratch, size_t scratch_bytes,
                              hipStream_t s, PathLog plog = PathLog());

// Ragged batch: `count` matrices of different orders, matrix id of order n_each[id] <= FWX_SMALL_N at element
// offset[id] of rate (next / hops / the trace arrays alike), pitch n_each[id]; whole pivot range of each.  The three
// index arrays are DEVICE arrays; order / tier_count (host) are what fwx_ragged_plan gives: the matrices grouped by
// tier (wave, 64-wide, 128-wide workgroup).  Up to three launches on s, the 128-wide tier first, each chunked at
// 2^21 workgroups; an empty tier launches nothing.  Nothing outside the n x n cells of a matrix is read or written.
// updates_each: count counters or nullptr, counter id is incremented by U of matrix id.  plog as above.
template <typename T>
hipError_t launch_ragged_solve(T *rate, int32_t *next, int32_t *hops, int count, const int32_t *n_each,
                               const int64_t *offset, const int32_t *order, const int32_t tier_count[3],
                               unsigned long long *updates_each, hipStream_t s, PathLog plog = PathLog());

// The fourth tier of a ragged batch (fwx_mid.hip): the `listed` matrices whose ids stand in `order` (device; the
// mid tier's part of what fwx_ragged_mid_plan gives), each of an order 1 ... FWX_MID_N, one workgroup per matrix on
// launch_batch_mid's body.  Index arrays, layout, counters and plog as launch_ragged_solve.  An id outside
// [0, count) or an order outside 1 ... FWX_MID_N leaves its workgroup idle; a small order is solved like any other.
// One launch per 2^21 matrices.
template <typename T>
hipError_t launch_ragged_mid(T *rate, int32_t *next, int32_t *hops, int count, const int32_t *n_each,
                             const int64_t *offset, const int32_t *order, long long listed,
                             unsigned long long *updates_each, hipStream_t s, PathLog plog = PathLog());

// The fifth tier of a ragged batch (fwx_large.hip): the `listed` matrices whose ids stand in `order` (device; the large
// tier's part of what fwx_ragged_large_plan gives, sorted by descending order), each of an order 1 ... FWX_LARGE_N,
// several workgroups per matrix on launch_batch_large's bodies.  `work` is the plan's work table on the HOST, three
// rows `row` entries apart (RaggedLargeWork), d_work the same contents on the device.  Slot m of the list has the order
// panel[m + 1] - panel[m]; a GROUP is a maximal run of consecutive slots whose panels, 512 bytes per order and slot m
// at 512 * (panel[m] - panel[first slot of the group]), fit scratch_bytes and whose tiles number less than 2^31; the
// groups run one after the other on s.  Per pivot block q of a group, q < ceil(n_first / B), one panel and one sweep
// launch over the ACTIVE PREFIX, the group's slots with n > q * B, each a linear grid of strip[m0 + active] -
// strip[m0] resp. tile[...] workgroups that find their slot by binary search in the device row: 2 * ceil(n_first / B)
// launches per group, and a matrix that is done costs nothing afterwards.  With plog, one launch over the tiles of all
// slots writes -1 to the n x n cells of `last` before the first group.  Index arrays, layout, counters (by matrix id)
// and plog as launch_ragged_mid.  A workgroup whose id lies outside [0, count), whose order lies outside 1 ...
// FWX_LARGE_N or whose panels would end past scratch_bytes stays idle, and none touches anything outside the n x n
// cells of its matrix or the scratch, whatever the device tables hold.  hipErrorInvalidValue for a host table that
// ragged_large_work_ok refuses and for scratch that is null, misaligned or smaller than the first slot's.
struct RaggedLargeWork {
    const int64_t *panel, *strip, *tile;
    RaggedLargeWork(const int64_t *work, long long row) : panel(work), strip(work + row), tile(work + 2 * row) {}
    int order_of(int m) const { return (int)(panel[m + 1] - panel[m]); }
};
// A host table is usable: orders 1 ... FWX_LARGE_N, descending, and the strip and tile rows those of the geometry.
inline bool ragged_large_work_ok(const RaggedLargeWork &w, int listed)
{
    for (int m = 0; m < listed; ++m) {
        const int64_t n = w.panel[m + 1] - w.panel[m];
        if (n < 1 || n > FWX_LARGE_N || (m > 0 && n > w.panel[m] - w.panel[m - 1])) return false;
        const int64_t tiles = ((n + FWX_LARGE_TC - 1) / FWX_LARGE_TC) * ((n + FWX_LARGE_TR - 1) / FWX_LARGE_TR);
        if (w.strip[m + 1] - w.strip[m] != (n + FWX_LARGE_S - 1) / FWX_LARGE_S || w.tile[m + 1] - w.tile[m] != tiles)
            return false;
    }
    return true;
}
// One past the last slot of the group that starts at slot m0 (m0 itself: not even that slot fits).
inline int ragged_large_group_end(const RaggedLargeWork &w, int m0, int listed, size_t scratch_bytes)
{
    int m1 = m0;
    while (m1 < listed && (uint64_t)(w.panel[m1 + 1] - w.panel[m0]) <= scratch_bytes / FWX_LARGE_SCRATCH_BYTES(1) &&
           w.tile[m1 + 1] - w.tile[m0] < ((int64_t)1 << 31))
        ++m1;
    return m1;
}
// f(q, active) for every pivot block q of the group [m0, m1): active = its slots with n > q * B, a prefix.
template <typename F> void ragged_large_blocks(const RaggedLargeWork &w, int m0, int m1, F &&f)
{
    int active = m1 - m0;
    const int blocks = (w.order_of(m0) + FWX_LARGE_B - 1) / FWX_LARGE_B;
    for (int q = 0; q < blocks; ++q) {
        while (active > 0 && w.order_of(m0 + active - 1) <= q * FWX_LARGE_B) --active;
        f(q, active);
    }
}
template <typename T>
hipError_t launch_ragged_large(T *rate, int32_t *next, int32_t *hops, int count, const int32_t *n_each,
                               const int64_t *offset, const int32_t *order, int listed, const int64_t *work,
                               const int64_t *d_work, long long row, unsigned long long *updates_each, void *scratch,
                               size_t scratch_bytes, hipStream_t s, PathLog plog = PathLog());

template <typename T>
hipError_t launch_snapshot_row(T *dst, const T *src, int32_t *hdst, const int32_t *hsrc, int n,
                               hipStream_t s);

// ---- fused engine: FWX_FUSED_B pivots per launch from time-k snapshots ------------------------
#define FWX_FUSED_B 64

template <typename T> struct FusedArgs {
    T *rate;               // slab: rows x n (all rows are relaxed, pivot rows included)
    int32_t *next;         // or nullptr
    int rows, n, row0;
    int k0, bt;            // pivots [k0, k0+bt), bt <= FWX_FUSED_B
    const T *w;            // snapshot panel: w[t*n + j] = row k0+t at time k0+t
    T *ct;                 // scratch bt x rows: ct[t*rows + i] = column k0+t at time k0+t (NaN if i==k)
    int32_t *cnt;          // scratch bt x rows (iff next)
    int32_t *hops = nullptr;      // slab rows x n, or nullptr (needs next): hops' = hops[i][k] + hops[k][j]
    const int32_t *wh = nullptr;  // hops panel: wh[t*n + j] = hops of row k0+t at time k0+t (iff hops)
    int32_t *cht = nullptr;       // scratch bt x rows (iff hops): hops of column k0+t at time k0+t
    int ct_ld;             // leading dimension of ct / cnt (>= rows; a multiple of 4 keeps the
                           // staging loads 16-byte aligned)
    unsigned long long *updates;
    bool nonneg;           // caller verified the domain (fwx.h "Domain"): every matrix entry is >= +0
                           // and not NaN and, if next is carried, no positive rate lacks a path:
                           // the max-form kernels may run (f32: rates only, or rates + next + trace)
    PathLog plog = PathLog();   // path trace (needs next): rows x n like rate / next, LOCAL rows
    bool side = false;     // launch_fused_panels: launched beside a main launch (may pick a form that fits its holes);
                           // launch_fused_main: a launch of the look-ahead chain beside a main launch (the next
                           // blocks' rows and columns) -- its waves run at raised priority (s_setprio 2; the
                           // panel kernels always run at 3), because the chain, not the sweep, bounds mid sizes
};

// Domain check (fwx.h "Domain").  *flag is a device int preset to 3; bit 0 is cleared if any of the
// `count` rates is negative, -0 or NaN; bit 1 is cleared if `next` is given and some entry has a
// non-zero rate with next < 0 (a positive rate without a path).
hipError_t launch_nonneg_check(const float *rate, const int32_t *next, size_t count, int *flag,
                               hipStream_t s);
hipError_t launch_nonneg_check(const double *rate, const int32_t *next, size_t count, int *flag,
                               hipStream_t s);

// colpanel + main: applies the bt pivots to every row of the slab.
template <typename T>
hipError_t launch_fused_relax(const FusedArgs<T> &a, hipStream_t s, int skip_lo = 0, int skip_hi = 0);
// The two halves separately: pivot-column snapshots for all rows of the slab, then the main
// kernel on local rows [r_lo, r_hi) (used by the look-ahead schedule).
template <typename T> hipError_t launch_fused_colpanel(const FusedArgs<T> &a, hipStream_t s);
// Column controls of a main launch (symmetric look-ahead): c_hi > c_lo restricts the launch to the
// columns [c_lo, c_hi) (multiples of 64), skip_hi > skip_lo leaves the columns [skip_lo, skip_hi)
// (multiples of 4) to another launch of the same pass.  Default: all columns.
struct FusedCols {
    int c_lo = 0, c_hi = 0, skip_lo = 0, skip_hi = 0;
    static FusedCols only(int lo, int hi) { FusedCols c; c.c_lo = lo; c.c_hi = hi; return c; }
    static FusedCols except(int lo, int hi) { FusedCols c; c.skip_lo = lo; c.skip_hi = hi; return c; }
};
// True if the main launch these arguments select leaves no room for a panel workgroup when ONE of its own
// workgroups retires (f32 with next-hops on 64 x 64 tiles: four workgroups per CU at 128 registers and 36.5 KB of
// LDS each -- the hole one of them leaves is smaller than a panel workgroup's 48 KB, and before round 4's panel
// rewrite also than its 4 x 48 registers per SIMD): the panels of the look-ahead chain then wait for the
// launch's tail.  A double-pass schedule issues such a main launch as two halves -- the first one's tail lets the
// chain's first panel in, the second one's the other (fused_range in fwx_api.hip, profiles/r04_timeline_*).
template <typename T> bool fused_main_starves_panels(const FusedArgs<T> &a);
// ... unless launch_fused_panels has a form for these arguments that fits the hole (a.side set: f32 with next-hops,
// no trace, no hops -- column workgroups of 32 rows, 32.25 KB of LDS and 32 registers): then the main launch stays
// whole and the chain runs beside it.
template <typename T> bool fused_panels_fit_beside(const FusedArgs<T> &a);
template <typename T>
hipError_t launch_fused_main(const FusedArgs<T> &a, int r_lo, int r_hi, hipStream_t s,
                             int skip_lo = 0, int skip_hi = 0, FusedCols cols = FusedCols());

// rowpanel + colpanel of pass (a.k0, a.bt) in ONE launch, for a slab that is the whole matrix
// (a.rows == a.n, a.row0 == 0): the column panel evolves the diagonal block itself instead of
// reading a finished W, so neither waits for the other.  Writes w_out (and wh_out with hops), a.ct,
// a.cnt, a.cht and the trace's at_row / at_col; a.w / a.wh are not read.
template <typename T>
hipError_t launch_fused_panels(const FusedArgs<T> &a, T *w_out, int32_t *wh_out, hipStream_t s);

// diag + rowpanel: snapshot panel of the pivot rows `rows_base` (bt x n, at time k0); the matrix
// is not modified.  plog: the path trace AT THE SAME ROWS as rows_base (plog.last / plog.at_row
// point at pivot row k0; at_col is not touched).  hops_rows (same rows again) / wh: the hops of the
// pivot rows are carried through the panel and their time-k snapshots exported to wh (bt x n).
template <typename T>
hipError_t launch_fused_panel(const T *rows_base, int n, int k0, int bt, T *w, hipStream_t s,
                              PathLog plog = PathLog(), const int32_t *hops_rows = nullptr,
                              int32_t *wh = nullptr);

}  // namespace fwx
#endif
