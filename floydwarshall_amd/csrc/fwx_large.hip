// fwx_large.hip -- the large tier of the batched solves: `count` matrices of one order n <= FWX_LARGE_N (1024),
// SEVERAL workgroups per matrix.  The scheme is the mid tier's (fwx_mid.hip): pivots are taken FWX_LARGE_B at a time
// from time-k snapshot panels, the matrix resident in global memory.  One workgroup can neither hold the panels of a
// 1024-wide matrix in LDS nor sweep it in reasonable time, so the two phases of a block of pivots become TWO
// LAUNCHES over the whole group of matrices, the matrix index a grid dimension, and the frozen panels travel from
// the first to the second through caller-provided scratch in global memory.
//
// For each block of pivots [k0, k0 + bt), bt <= B, the first block at k_begin:
//   1. large_panel, grid (column strips of width S, matrices), 1024 threads.  Workgroup (s, b) runs the mid tier's
//      panel phase on the index set cross U strip, cross = [k0, k0 + bt), strip = [sS, sS + S) n [0, n): P = B + S
//      positions, position p < B the cross index k0 + p, position B + y the strip index sS + y.  W / WN / WH [t][p] =
//      entry (k0+t, index(p)), C / CN / CH [t][p] = entry (index(p), k0+t), NaN at (k, k) in both and at positions
//      without an index (NaN never wins a compare and no such position is ever an operand).  For t = 0 .. bt-2 row t
//      of both panels is frozen and pivot k0+t applied to the rows u > t: wave w on row u = t + 1 + w, lane on
//      position p, one barrier per pivot.  The operands a strip needs from outside itself are exactly the cross
//      entries C[t][k0+u] and W[t][k0+u] -- positions u < B of its own copy of the cross: every strip workgroup
//      evolves the bt x bt cross block in both forms.  Copies of one entry (in other workgroups, or twice in the
//      strip that overlaps the cross) see the same operands in the same order while unfrozen and stay bit-equal; the
//      mid tier's argument does the rest.  The frozen STRIP positions are written to the matrix's scratch panels,
//      all [B][n]: W, Ct, WN, CNt, WH, CHt.  The matrix is only read; nothing is counted.
//   2. large_sweep, grid (column tiles of TC, row tiles of TR, matrices), 256 threads.  The workgroup stages
//      Ct / CNt / CHt [.][its rows] in LDS (NaN for t >= bt), a thread keeps W[0..B)[its column] in registers, wave w
//      on columns [64w, 64w + 64) of the tile, every wave walking all TR rows, FWX_LARGE_ROWS of them together with t
//      outermost (independent compare chains: a wave alone on its SIMD is bound by them): C[t][i] is a wave-uniform
//      LDS read.
//      Every entry (i, j), i != j, folds C[t][i] * W[t][j] in ascending t with the strict <, keeping the value, the
//      LAST winning t and the count; only an entry that moved is written back, next = CNt[t*][i] if >= 0 else
//      WN[t*][j], hops = CHt[t*][i] + WH[t*][j] (WN / WH read from scratch: only winners need them).  One atomic per
//      workgroup adds the count to updates[b].
// Between launches only STREAM ORDER is relied on: the sweep of a block reads the panels the panel launch before it
// wrote and modifies the matrix, the next panel launch reads the matrix after it.  (One launch could not do both: a
// sweep workgroup that rebuilt its own panels would read pivot rows and columns other workgroups are overwriting.)
// No cooperative launch, no grid barrier, no spin-wait, no flag between workgroups.  Every __syncthreads is reached
// by the whole workgroup with a trip count that is a function of (n, range, geometry) alone; there is no early exit.
// Scalar element accesses only: any n from 1 up (smaller than B, S or a tile included), any stride >= n*n, no
// alignment beyond the element; tiles and strips are ragged at the right and bottom edges.  The gap between
// matrices is never read or written, the diagonal's rate neither.
//
// The path trace (HAS_LAST; PathLog in fwx_kernels.h, whole pivot range only) rides on the two launches as it rides on
// the mid tier's three phases (fwx_mid.hip), and needs no scratch:
//   0. large_fill_last, once per call and before the first block of the first group, writes -1 to the n x n cells of
//      `last` of every matrix of the batch (the caller initialises nothing; the gap is not touched).
//   1. large_panel keeps two more int32 LDS panels, AR and AC [B][pitch]: AR[t][p] = last[k0+t][index(p)] and
//      AC[t][p] = last[index(p)][k0+t], loaded beside the rates -- `last` as it stands at BLOCK START, written by the
//      sweeps before this launch.  A panel-phase win of pivot k0+t on W[u][c] sets AR[u][c] = k0+t, one on C[u][c] sets
//      AC[u][c] = k0+t.  After the pivot loop the frozen STRIP positions -- the positions the rate panels store -- go
//      straight to the caller's trace: at_row[k0+t][x] = AR[t][p], at_col[x][k0+t] = AC[t][p].  Every cell of at_row
//      and at_col belongs to one pivot block and one strip: it is written by exactly one workgroup, exactly once per
//      solve, and no two workgroups ever store to one address.  The copies of a cross cell in other strips see the same
//      wins (the bit-equality argument above) and are dropped.
//   2. large_sweep: a win stores last = k0 + (the last winning t) beside next and hops.
// Stream order between launches is all the trace relies on, as the solve does.
//
// Scratch: FWX_LARGE_SCRATCH_BYTES(n) per matrix of the group, laid out for the dtype and field set of the call
// (W, Ct as T, then the int32 panels), an upper bound: 2 panels x B rows x n columns x 16 bytes.  launch_batch_large
// solves the batch in groups of as many matrices as the scratch holds, one group after the other on the stream.
//
// The ragged form (launch_ragged_large; fwx_kernels.h has the contract): matrices of DIFFERENT orders, the fifth tier of
// a ragged batch.  The bodies of the three kernels are __device__ functions that take what a kernel decides -- n, the
// element offset, the scratch panels, k0, bt, the strip or tile, the counter slot -- by value; the uniform kernels call
// them with what their grid says, large_panel_ragged / large_sweep_ragged / large_fill_last_ragged with what the
// workgroup finds in the plan's tables.  Their grid is LINEAR over the active prefix of one group of the list, which is
// sorted by descending order: at the block that starts at k0 the matrices with n > k0 are a prefix, and a matrix that
// is done gets no workgroup.  Everything such a workgroup decides on is workgroup-uniform and decided before its
// first barrier; the trip counts of the bodies stay functions of (n, k0, geometry) alone.
#include "fwx_kernels.h"

#include <algorithm>

namespace fwx {
namespace {

template <typename T> __device__ __forceinline__ T large_nan();
template <> __device__ __forceinline__ float large_nan<float>() { return __builtin_nanf(""); }
template <> __device__ __forceinline__ double large_nan<double>() { return __builtin_nan(""); }

constexpr int kLargeB = FWX_LARGE_B;
constexpr int kLargeS = FWX_LARGE_S;
constexpr int kLargeTR = FWX_LARGE_TR;
constexpr int kLargeTC = FWX_LARGE_TC;
constexpr int kLargeP = kLargeB + kLargeS;            // positions of a panel workgroup: one wave wide
constexpr int kPanelThreads = 64 * kLargeB;           // one wave per panel row
constexpr int kSweepThreads = kLargeTC;               // one thread per column of the tile
// Pitch of the panel kernel's LDS panels, in elements: the column loads run over t first and store one pitch apart;
// an odd pitch spreads the 16 pivots of a position over the banks where 64 would put them all on one.
constexpr int kLargePitch = kLargeP + 1;
constexpr int kLargeRows = FWX_LARGE_ROWS;            // sweep: rows folded together per thread
static_assert(kLargeP == 64, "a panel row is one wave: lane = position");
static_assert(kLargeB == 16, "t = e & (B - 1) and 16 waves of a 1024-thread workgroup; FWX_LARGE_SCRATCH_BYTES");
static_assert(kLargeTC % 64 == 0 && kLargeTC <= 1024 && kLargeTR % kLargeRows == 0, "waves of whole columns");

// The scratch panels of one matrix, for dtype T: all [B][n], pitch n.
template <typename T> struct LargePanels {
    T *W, *Ct;
    int32_t *WN, *CNt, *WH, *CHt;
};
template <typename T> __device__ __forceinline__ LargePanels<T> large_panels(char *base, int n)
{
    const size_t bn = (size_t)kLargeB * (size_t)n;
    LargePanels<T> p;
    p.W = (T *)base;
    p.Ct = p.W + bn;
    p.WN = (int32_t *)(p.Ct + bn);
    p.CNt = p.WN + bn;
    p.WH = p.CNt + bn;
    p.CHt = p.WH + bn;
    return p;
}

// -1 to the n x n cells of `last` of matrix blockIdx.y, kFillCells cells per workgroup.
constexpr int kFillThreads = 256, kFillCells = 4 * kFillThreads;
__global__ __launch_bounds__(kFillThreads) void large_fill_last(int32_t *last, int n, long long stride)
{
    const size_t cells = (size_t)n * (size_t)n;
    int32_t *m = last + (size_t)blockIdx.y * (size_t)stride;
    const size_t e0 = (size_t)blockIdx.x * kFillCells + threadIdx.x;
#pragma unroll
    for (int q = 0; q < kFillCells / kFillThreads; ++q) {
        const size_t e = e0 + (size_t)q * kFillThreads;
        if (e < cells) m[e] = -1;
    }
}

// ---- the ragged form: where a workgroup of a linear grid works -------------------------------------------------------
// A ragged launch covers the ACTIVE PREFIX of one group of the large tier's list: the slots [m0, m0 + active), sorted
// by descending order, so that the matrices with n > k0 are a prefix.  `base` is a row of the work table
// (fwx_ragged_large_plan: strip_base for the panel launch, tile_base for the sweep and the fill), base[m] the units of
// the slots before m; the grid has base[m0 + active] - base[m0] workgroups.  Workgroup w belongs to the last slot
// of the prefix whose base, counted from the group's, is <= w: a binary search over that prefix only, every load
// through a workgroup-uniform address (scalar loads), ceil(log2(active)) of them whatever the row holds.  `local`
// receives w counted from the slot's own base -- a row that does not belong to the call makes it anything, which the
// callers test against the order of the matrix they find.
__device__ __forceinline__ int large_slot(const int64_t *base, int m0, int active, long long w, long long &local)
{
    const long long b0 = base[m0];
    int lo = 0, hi = active;                                  // the slot is one of [lo, hi)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (base[m0 + mid] - b0 <= w) lo = mid; else hi = mid;
    }
    local = w - (base[m0 + lo] - b0);
    return m0 + lo;
}

// A workgroup-uniform value in scalar registers, whatever the compiler could prove about it: the bodies keep n, the
// offsets and the tile coordinates there in the uniform kernels, and the ragged ones must not spend vector registers
// on them (the sweep sits at 94 of the 96 that five waves per SIMD allow).
__device__ __forceinline__ int large_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ size_t large_uniform(size_t v)
{
    return (size_t)(unsigned)large_uniform((int)(unsigned)v) | (size_t)(unsigned)large_uniform((int)(unsigned)(v >> 32)) << 32;
}

// What a ragged workgroup finds at its slot: the matrix (id, order, element offset) and its scratch panels.  ok is
// false -- the workgroup leaves, before its first barrier and without touching memory -- for an id outside
// [0, count), an order outside 1 ... FWX_LARGE_N, or (with_scratch) panels that would not end within scratch_bytes.
// Everything here is workgroup-uniform.
struct LargeSlot {
    bool ok;
    int id, n;
    size_t off;
    char *panels;
};
__device__ __forceinline__ LargeSlot large_slot_matrix(int m, int m0, int count, const int32_t *n_each,
                                                       const int64_t *offset, const int32_t *order,
                                                       const int64_t *panel_base, char *scratch, size_t scratch_bytes,
                                                       bool with_scratch)
{
    LargeSlot r{false, 0, 0, 0, nullptr};
    r.id = order[m];
    if ((unsigned)r.id >= (unsigned)count) return r;
    r.n = n_each[r.id];
    if (r.n <= 0 || r.n > FWX_LARGE_N) return r;
    r.id = large_uniform(r.id);
    r.n = large_uniform(r.n);
    r.off = large_uniform((size_t)offset[r.id]);
    if (with_scratch) {
        const long long at = panel_base[m] - panel_base[m0];  // orders before the slot, within its group
        const size_t bytes = FWX_LARGE_SCRATCH_BYTES(r.n);
        if (at < 0 || scratch_bytes < bytes || (unsigned long long)at > (scratch_bytes - bytes) / FWX_LARGE_SCRATCH_BYTES(1))
            return r;
        r.panels = scratch + large_uniform((size_t)at * FWX_LARGE_SCRATCH_BYTES(1));
    }
    r.ok = true;
    return r;
}

// Tile `local` of an order-n matrix, its tiles numbered row by row, ceil(n / TC) to a row: false where there is none.
__device__ __forceinline__ bool large_tile_of(int n, long long local, int &tx, int &ty)
{
    const int tcols = (n + kLargeTC - 1) / kLargeTC, trows = (n + kLargeTR - 1) / kLargeTR;
    if (local < 0 || local >= (long long)(tcols * trows)) return false;
    ty = large_uniform((int)local / tcols);
    tx = large_uniform((int)local - ty * tcols);
    return true;
}

// -1 to the cells of `last` of one sweep tile (tx, ty) of the order-n matrix at `last`: the ragged fill, one workgroup
// of kSweepThreads per tile, a row of the tile per pass.
__device__ __forceinline__ void large_fill_tile(int32_t *last, int n, int tx, int ty)
{
    const int j = tx * kLargeTC + (int)threadIdx.x, i0 = ty * kLargeTR;
    if (j >= n) return;
    for (int r = 0; r < kLargeTR && i0 + r < n; ++r) last[(size_t)(i0 + r) * n + j] = -1;
}

// All L slots of the large tier, one workgroup per sweep tile: exactly the n_b x n_b cells of every listed matrix.
__global__ __launch_bounds__(kSweepThreads) void large_fill_last_ragged(int32_t *last, int count,
                                                                        const int32_t *n_each, const int64_t *offset,
                                                                        const int32_t *order,
                                                                        const int64_t *tile_base, int m0, int active)
{
    long long local;
    const int m = large_slot(tile_base, m0, active, (long long)blockIdx.x, local);
    const LargeSlot sl = large_slot_matrix(m, m0, count, n_each, offset, order, nullptr, nullptr, 0, false);
    int tx, ty;
    if (!sl.ok || !large_tile_of(sl.n, local, tx, ty)) return;
    large_fill_tile(last + sl.off, sl.n, tx, ty);
}

// The panel phase of pivot block [k0, k0 + bt) on strip s0 of the order-n matrix at element `off` of the arrays, its
// scratch panels at `panels`.  Shared by the uniform and the ragged kernel: everything a kernel decides comes in by
// value, and every barrier is reached by the whole workgroup with a trip count that depends on bt alone.  The trace
// arguments stand last: an instantiation without HAS_LAST reads none of them.
template <typename T, bool HAS_NEXT, bool HAS_HOPS, bool HAS_LAST>
__device__ __forceinline__ void large_panel_body(const T *rate, const int32_t *next, const int32_t *hops, int n,
                                                 size_t off, char *panels, int k0, int bt, int s0, const PathLog &plog)
{
    static_assert(HAS_NEXT || !HAS_LAST, "the trace goes with next");
    constexpr int B = kLargeB, Q = kLargePitch;
    __shared__ T W[B][Q], C[B][Q];
    __shared__ int32_t WN[HAS_NEXT ? B : 1][HAS_NEXT ? Q : 1], CN[HAS_NEXT ? B : 1][HAS_NEXT ? Q : 1];
    __shared__ int32_t WH[HAS_HOPS ? B : 1][HAS_HOPS ? Q : 1], CH[HAS_HOPS ? B : 1][HAS_HOPS ? Q : 1];
    __shared__ int32_t AR[HAS_LAST ? B : 1][HAS_LAST ? Q : 1], AC[HAS_LAST ? B : 1][HAS_LAST ? Q : 1];

    const int tid = threadIdx.x;
    rate += off;
    if constexpr (HAS_NEXT) next += off;
    if constexpr (HAS_HOPS) hops += off;
    // the index (a row or a column of the matrix) of position p, -1 where it has none
    auto index_of = [&](int p) {
        const int x = p < B ? (p < bt ? k0 + p : -1) : s0 + p - B;
        return x < n ? x : -1;
    };
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;

    // ---- load: pivot rows, wave t on row k0+t, lane on position ---------------------------------------------
    if (wave < bt) {
        const int t = wave, k = k0 + t, x = index_of(lane);
        const size_t e = (size_t)k * n + (x < 0 ? 0 : x);
        W[t][lane] = (x < 0 || x == k) ? large_nan<T>() : rate[e];
        if constexpr (HAS_NEXT) WN[t][lane] = x < 0 ? -1 : next[e];
        if constexpr (HAS_HOPS) WH[t][lane] = x < 0 ? 0 : hops[e];
        if constexpr (HAS_LAST) AR[t][lane] = x < 0 ? -1 : plog.last[off + e];
    }
    // ---- load: pivot columns, thread on (position, t), t fastest: 16 consecutive elements of a row ----------
    {
        const int t = tid & (B - 1), p = tid >> 4;
        if (t < bt) {
            const int k = k0 + t, x = index_of(p);
            const size_t g = (size_t)(x < 0 ? 0 : x) * n + k;
            C[t][p] = (x < 0 || x == k) ? large_nan<T>() : rate[g];
            if constexpr (HAS_NEXT) CN[t][p] = x < 0 ? -1 : next[g];
            if constexpr (HAS_HOPS) CH[t][p] = x < 0 ? 0 : hops[g];
            if constexpr (HAS_LAST) AC[t][p] = x < 0 ? -1 : plog.last[off + g];
        }
    }
    __syncthreads();
    // ---- pivots k0 .. k0+bt-2 on the rows of both panels that are not yet frozen ----------------------------
    for (int t = 0; t + 1 < bt; ++t) {
        const int u = t + 1 + wave;                           // wave-uniform; position u is the cross index k0+u
        if (u < bt) {
            const int c = lane;
            // row k0+u of the matrix: entry (k0+u, index(c)) against (k0+u, k) * (k, index(c))
            const T cand_w = C[t][u] * W[t][c];
            if (W[u][c] < cand_w) {
                W[u][c] = cand_w;
                if constexpr (HAS_NEXT) { const int32_t h = CN[t][u]; WN[u][c] = h >= 0 ? h : WN[t][c]; }
                if constexpr (HAS_HOPS) WH[u][c] = CH[t][u] + WH[t][c];
                if constexpr (HAS_LAST) AR[u][c] = k0 + t;
            }
            // column k0+u of the matrix: entry (index(c), k0+u) against (index(c), k) * (k, k0+u)
            const T cand_c = C[t][c] * W[t][u];
            if (C[u][c] < cand_c) {
                C[u][c] = cand_c;
                if constexpr (HAS_NEXT) { const int32_t h = CN[t][c]; CN[u][c] = h >= 0 ? h : WN[t][u]; }
                if constexpr (HAS_HOPS) CH[u][c] = CH[t][c] + WH[t][u];
                if constexpr (HAS_LAST) AC[u][c] = k0 + t;
            }
        }
        __syncthreads();
    }
    // ---- store the frozen strip positions: wave t on row t of the six panels ---------------------------------
    if (wave < bt && lane >= B) {
        const int x = s0 + lane - B;
        if (x < n) {
            const LargePanels<T> pn = large_panels<T>(panels, n);
            const size_t e = (size_t)wave * n + x;
            pn.W[e] = W[wave][lane];
            pn.Ct[e] = C[wave][lane];
            if constexpr (HAS_NEXT) { pn.WN[e] = WN[wave][lane]; pn.CNt[e] = CN[wave][lane]; }
            if constexpr (HAS_HOPS) { pn.WH[e] = WH[wave][lane]; pn.CHt[e] = CH[wave][lane]; }
            if constexpr (HAS_LAST) plog.at_row[off + (size_t)(k0 + wave) * n + x] = AR[wave][lane];
        }
    }
    // ---- the trace's column cells: thread on (position, t) as in the column load, t fastest -- the 16 pivots of a
    // position are one 64-byte segment of its row of at_col
    if constexpr (HAS_LAST) {
        const int t = tid & (B - 1), p = tid >> 4, x = s0 + p - B;
        if (p >= B && t < bt && x < n) plog.at_col[off + (size_t)x * n + k0 + t] = AC[t][p];
    }
}

template <typename T, bool HAS_NEXT, bool HAS_HOPS, bool HAS_LAST>
__global__ __launch_bounds__(kPanelThreads) void large_panel(const T *rate, const int32_t *next, const int32_t *hops,
                                                             int n, long long stride, int k0, int bt, char *scratch,
                                                             size_t per_matrix, PathLog plog)
{
    large_panel_body<T, HAS_NEXT, HAS_HOPS, HAS_LAST>(rate, next, hops, n, (size_t)blockIdx.y * (size_t)stride,
                                                      scratch + (size_t)blockIdx.y * per_matrix, k0, bt,
                                                      (int)blockIdx.x * kLargeS, plog);
}

// Ragged batch, large tier: workgroup w of the launch on one strip of the matrix large_slot finds for it, of the order
// and at the offset the index arrays give, bt = min(B, n - k0).  Every test is workgroup-uniform and comes before the
// body's first barrier and first memory access: all 1024 threads leave or none does.
template <typename T, bool HAS_NEXT, bool HAS_HOPS, bool HAS_LAST>
__global__ __launch_bounds__(kPanelThreads) void large_panel_ragged(const T *rate, const int32_t *next,
                                                                    const int32_t *hops, int count,
                                                                    const int32_t *n_each, const int64_t *offset,
                                                                    const int32_t *order, const int64_t *panel_base,
                                                                    const int64_t *strip_base, int m0, int active,
                                                                    int k0, char *scratch, size_t scratch_bytes,
                                                                    PathLog plog)
{
    long long local;
    const int m = large_slot(strip_base, m0, active, (long long)blockIdx.x, local);
    const LargeSlot sl = large_slot_matrix(m, m0, count, n_each, offset, order, panel_base, scratch, scratch_bytes, true);
    if (!sl.ok || k0 >= sl.n || local < 0 || local * kLargeS >= sl.n) return;
    large_panel_body<T, HAS_NEXT, HAS_HOPS, HAS_LAST>(rate, next, hops, sl.n, sl.off, sl.panels, k0,
                                                      min(kLargeB, sl.n - k0), large_uniform((int)local * kLargeS), plog);
}

// The sweep of pivot block [k0, k0 + bt) on tile (tx, ty) of the order-n matrix at element `off`, from the panels at
// `panels`; the workgroup's count goes to updates[slot].  Shared by the uniform and the ragged kernel like the panel
// body: i0 < n is the caller's to see to.
template <typename T, bool HAS_NEXT, bool HAS_HOPS, bool HAS_LAST>
__device__ __forceinline__ void large_sweep_body(T *rate, int32_t *next, int32_t *hops, int32_t *last, int n,
                                                 size_t off, char *panels, int k0, int bt, int tx, int ty,
                                                 unsigned long long *updates, unsigned int slot)
{
    static_assert(HAS_NEXT || !HAS_LAST, "the trace goes with next");
    constexpr int B = kLargeB, TR = kLargeTR, TC = kLargeTC;
    __shared__ T C[B][TR];
    __shared__ int32_t CN[HAS_NEXT ? B : 1][HAS_NEXT ? TR : 1], CH[HAS_HOPS ? B : 1][HAS_HOPS ? TR : 1];
    __shared__ unsigned int s_cnt;

    const int tid = threadIdx.x;
    const int j = tx * TC + tid, i0 = ty * TR;
    const int rows = min(TR, n - i0);                         // >= 1: the grid covers [0, n) and no more
    rate += off;
    if constexpr (HAS_NEXT) next += off;
    if constexpr (HAS_HOPS) hops += off;
    if constexpr (HAS_LAST) last += off;
    const LargePanels<T> pn = large_panels<T>(panels, n);

    if (tid == 0) s_cnt = 0;
    for (int e = tid; e < B * TR; e += kSweepThreads) {       // lane on (t, row), row fastest
        const int t = e / TR, r = e - t * TR;
        const bool have = t < bt && r < rows;
        const size_t g = (size_t)t * n + i0 + r;
        C[t][r] = have ? pn.Ct[g] : large_nan<T>();
        if constexpr (HAS_NEXT) CN[t][r] = have ? pn.CNt[g] : -1;
        if constexpr (HAS_HOPS) CH[t][r] = have ? pn.CHt[g] : 0;
    }
    T w[B];
#pragma unroll
    for (int t = 0; t < B; ++t) w[t] = (t < bt && j < n) ? pn.W[(size_t)t * n + j] : large_nan<T>();
    __syncthreads();

    unsigned int mine = 0;                                    // a WAVE total (scalar)
    // a wave whose 64 columns all lie past the edge has nothing to fold (wave-uniform)
    if (tx * TC + (tid & ~63) < n) {
        for (int r0 = 0; r0 < rows; r0 += kLargeRows) {
            // kLargeRows rows together, t outermost: independent compare chains for a wave that is alone on its SIMD.
            // +inf where a lane has no entry (past an edge, or the diagonal's): no candidate compares greater, and the
            // rows of C past the edge are NaN
            T v[kLargeRows];
            int tb[kLargeRows];
#pragma unroll
            for (int m = 0; m < kLargeRows; ++m) {
                const int i = i0 + r0 + m;
                v[m] = (T)__builtin_huge_val();
                tb[m] = -1;
                if (r0 + m < rows && j < n && i != j) v[m] = rate[(size_t)i * n + j];
            }
#pragma unroll
            for (int t = 0; t < B; ++t) {
#pragma unroll
                for (int m = 0; m < kLargeRows; ++m) {
                    const T cand = C[t][r0 + m] * w[t];       // NaN where a skip applies
                    const bool p = v[m] < cand;               // false on NaN
                    v[m] = p ? cand : v[m];
                    tb[m] = p ? t : tb[m];
                    mine += (unsigned int)__builtin_popcountll(__ballot(p));
                }
            }
#pragma unroll
            for (int m = 0; m < kLargeRows; ++m) {
                if (tb[m] >= 0) {
                    const int r = r0 + m;
                    const size_t e = (size_t)(i0 + r) * n + j;
                    rate[e] = v[m];
                    if constexpr (HAS_NEXT) {
                        const int32_t h = CN[tb[m]][r];
                        next[e] = h >= 0 ? h : pn.WN[(size_t)tb[m] * n + j];
                    }
                    if constexpr (HAS_HOPS) hops[e] = CH[tb[m]][r] + pn.WH[(size_t)tb[m] * n + j];
                    if constexpr (HAS_LAST) last[e] = k0 + tb[m];
                }
            }
        }
    }
    if (updates) {                                            // workgroup-uniform
        if (mine && (tid & 63) == 0) atomicAdd(&s_cnt, mine);
        __syncthreads();
        if (tid == 0 && s_cnt) atomicAdd(&updates[slot], (unsigned long long)s_cnt);
    }
}

template <typename T, bool HAS_NEXT, bool HAS_HOPS, bool HAS_LAST>
__global__ __launch_bounds__(kSweepThreads) void large_sweep(T *rate, int32_t *next, int32_t *hops, int n,
                                                             long long stride, int bt, char *scratch,
                                                             size_t per_matrix, unsigned long long *updates,
                                                             int32_t *last, int k0)
{
    large_sweep_body<T, HAS_NEXT, HAS_HOPS, HAS_LAST>(rate, next, hops, last, n, (size_t)blockIdx.z * (size_t)stride,
                                                      scratch + (size_t)blockIdx.z * per_matrix, k0, bt,
                                                      (int)blockIdx.x, (int)blockIdx.y, updates, blockIdx.z);
}

// Ragged batch, large tier: workgroup w of the launch on one tile of its matrix, the tiles of a matrix numbered row by
// row, ceil(n / TC) of its OWN order to a row; U goes to updates[id].  Tests as in large_panel_ragged.
template <typename T, bool HAS_NEXT, bool HAS_HOPS, bool HAS_LAST>
__global__ __launch_bounds__(kSweepThreads) void large_sweep_ragged(T *rate, int32_t *next, int32_t *hops, int count,
                                                                    const int32_t *n_each, const int64_t *offset,
                                                                    const int32_t *order, const int64_t *panel_base,
                                                                    const int64_t *tile_base, int m0, int active,
                                                                    int k0, char *scratch, size_t scratch_bytes,
                                                                    unsigned long long *updates, int32_t *last)
{
    long long local;
    const int m = large_slot(tile_base, m0, active, (long long)blockIdx.x, local);
    const LargeSlot sl = large_slot_matrix(m, m0, count, n_each, offset, order, panel_base, scratch, scratch_bytes, true);
    int tx, ty;
    if (!sl.ok || k0 >= sl.n || !large_tile_of(sl.n, local, tx, ty)) return;
    large_sweep_body<T, HAS_NEXT, HAS_HOPS, HAS_LAST>(rate, next, hops, last, sl.n, sl.off, sl.panels, k0,
                                                      min(kLargeB, sl.n - k0), tx, ty, updates, (unsigned int)sl.id);
}

}  // namespace

template <typename T>
hipError_t launch_batch_large(T *rate, int32_t *next, int32_t *hops, int count, int n, long long stride, int k_begin,
                              int k_end, unsigned long long *updates_each, void *scratch, size_t scratch_bytes,
                              hipStream_t s, PathLog plog)
{
    if (count <= 0 || n <= 0) return hipSuccess;
    const bool traced = plog.last != nullptr;
    if (traced && (!next || !plog.at_col || !plog.at_row || k_begin != 0 || k_end != n)) return hipErrorInvalidValue;
    if (k_end <= k_begin) return hipSuccess;
    if (n > FWX_LARGE_N || (hops && !next) || k_begin < 0 || k_end > n || stride < (long long)n * n)
        return hipErrorInvalidValue;
    const size_t per_matrix = FWX_LARGE_SCRATCH_BYTES(n);
    if (!scratch || ((uintptr_t)scratch & 15) || scratch_bytes < per_matrix) return hipErrorInvalidValue;
    // matrices per group: what the scratch holds, and what one grid dimension does
    const long long group = std::min<long long>((long long)(scratch_bytes / per_matrix), 65535);
    const dim3 strips((n + kLargeS - 1) / kLargeS), tiles((n + kLargeTC - 1) / kLargeTC, (n + kLargeTR - 1) / kLargeTR);
    char *sc = (char *)scratch;
    // the trace's step 0, over every group at once: a later group's `last` is not touched before its own first block
    for (long long b0 = 0; traced && b0 < count; b0 += 65535) {
        const unsigned cnt = (unsigned)std::min<long long>(65535, count - b0);
        const unsigned wgs = (unsigned)(((size_t)n * n + kFillCells - 1) / kFillCells);
        hipLaunchKernelGGL(large_fill_last, dim3(wgs, cnt), dim3(kFillThreads), 0, s,
                           plog.last + (size_t)b0 * (size_t)stride, n, stride);
    }
    for (long long b0 = 0; b0 < count; b0 += group) {
        const unsigned cnt = (unsigned)std::min<long long>(group, count - b0);
        const size_t off = (size_t)b0 * (size_t)stride;
        T *r = rate + off;
        int32_t *nx = next ? next + off : nullptr, *hp = hops ? hops + off : nullptr;
        unsigned long long *u = updates_each ? updates_each + b0 : nullptr;
        PathLog pl;
        if (traced) { pl.last = plog.last + off; pl.at_col = plog.at_col + off; pl.at_row = plog.at_row + off; }
        for (int k0 = k_begin; k0 < k_end; k0 += kLargeB) {
            const int bt = std::min(kLargeB, k_end - k0);
#define FWX_BATCH_LARGE(HN, HH, HL)                                                                                    \
    do {                                                                                                               \
        hipLaunchKernelGGL((large_panel<T, HN, HH, HL>), dim3(strips.x, cnt), dim3(kPanelThreads), 0, s, r, nx, hp, n, \
                           stride, k0, bt, sc, per_matrix, pl);                                                        \
        hipLaunchKernelGGL((large_sweep<T, HN, HH, HL>), dim3(tiles.x, tiles.y, cnt), dim3(kSweepThreads), 0, s, r,    \
                           nx, hp, n, stride, bt, sc, per_matrix, u, pl.last, k0);                                     \
    } while (0)
            if (traced && hops) FWX_BATCH_LARGE(true, true, true);
            else if (traced) FWX_BATCH_LARGE(true, false, true);
            else if (hops) FWX_BATCH_LARGE(true, true, false);
            else if (next) FWX_BATCH_LARGE(true, false, false);
            else FWX_BATCH_LARGE(false, false, false);
#undef FWX_BATCH_LARGE
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

template <typename T>
hipError_t launch_ragged_large(T *rate, int32_t *next, int32_t *hops, int count, const int32_t *n_each,
                               const int64_t *offset, const int32_t *order, int listed, const int64_t *work,
                               const int64_t *d_work, long long row, unsigned long long *updates_each, void *scratch,
                               size_t scratch_bytes, hipStream_t s, PathLog plog)
{
    if (count < 0 || listed < 0 || listed > count || row <= listed || (hops && !next)) return hipErrorInvalidValue;
    if (listed == 0) return hipSuccess;
    const bool traced = plog.last != nullptr;
    if (!rate || !n_each || !offset || !order || !work || !d_work || (traced && (!next || !plog.at_col || !plog.at_row)))
        return hipErrorInvalidValue;
    const RaggedLargeWork w(work, row);
    if (!ragged_large_work_ok(w, listed)) return hipErrorInvalidValue;
    if (!scratch || ((uintptr_t)scratch & 15) || scratch_bytes < FWX_LARGE_SCRATCH_BYTES(w.order_of(0)))
        return hipErrorInvalidValue;
    const int64_t *d_panel = d_work, *d_strip = d_work + row, *d_tile = d_work + 2 * row;
    char *sc = (char *)scratch;
    // the trace's step 0, over every group at once, in runs of less than 2^31 tiles
    for (int m0 = 0; traced && m0 < listed;) {
        const int m1 = ragged_large_group_end(w, m0, listed, ~(size_t)0);
        hipLaunchKernelGGL(large_fill_last_ragged, dim3((unsigned)(w.tile[m1] - w.tile[m0])), dim3(kSweepThreads), 0, s,
                           plog.last, count, n_each, offset, order, d_tile, m0, m1 - m0);
        m0 = m1;
    }
    for (int m0 = 0; m0 < listed;) {
        const int m1 = ragged_large_group_end(w, m0, listed, scratch_bytes);   // > m0: the orders descend
        hipError_t e = hipSuccess;
        ragged_large_blocks(w, m0, m1, [&](int q, int active) {
            if (e != hipSuccess) return;
            const int k0 = q * kLargeB;
            const dim3 strips((unsigned)(w.strip[m0 + active] - w.strip[m0]));
            const dim3 tiles((unsigned)(w.tile[m0 + active] - w.tile[m0]));
#define FWX_RAGGED_LARGE(HN, HH, HL)                                                                                   \
    do {                                                                                                               \
        hipLaunchKernelGGL((large_panel_ragged<T, HN, HH, HL>), strips, dim3(kPanelThreads), 0, s, rate, next, hops,   \
                           count, n_each, offset, order, d_panel, d_strip, m0, active, k0, sc, scratch_bytes, plog);   \
        hipLaunchKernelGGL((large_sweep_ragged<T, HN, HH, HL>), tiles, dim3(kSweepThreads), 0, s, rate, next, hops,    \
                           count, n_each, offset, order, d_panel, d_tile, m0, active, k0, sc, scratch_bytes,           \
                           updates_each, plog.last);                                                                   \
    } while (0)
            if (traced && hops) FWX_RAGGED_LARGE(true, true, true);
            else if (traced) FWX_RAGGED_LARGE(true, false, true);
            else if (hops) FWX_RAGGED_LARGE(true, true, false);
            else if (next) FWX_RAGGED_LARGE(true, false, false);
            else FWX_RAGGED_LARGE(false, false, false);
#undef FWX_RAGGED_LARGE
            e = hipGetLastError();
        });
        if (e != hipSuccess) return e;
        m0 = m1;
    }
    return hipSuccess;
}

template hipError_t launch_ragged_large<float>(float *, int32_t *, int32_t *, int, const int32_t *, const int64_t *,
                                               const int32_t *, int, const int64_t *, const int64_t *, long long,
                                               unsigned long long *, void *, size_t, hipStream_t, PathLog);
template hipError_t launch_ragged_large<double>(double *, int32_t *, int32_t *, int, const int32_t *, const int64_t *,
                                                const int32_t *, int, const int64_t *, const int64_t *, long long,
                                                unsigned long long *, void *, size_t, hipStream_t, PathLog);

template hipError_t launch_batch_large<float>(float *, int32_t *, int32_t *, int, int, long long, int, int,
                                              unsigned long long *, void *, size_t, hipStream_t, PathLog);
template hipError_t launch_batch_large<double>(double *, int32_t *, int32_t *, int, int, long long, int, int,
                                               unsigned long long *, void *, size_t, hipStream_t, PathLog);

}  // namespace fwx
