// fwx_mid.hip -- the mid tier of the batched solves: `count` matrices of order n <= FWX_MID_N (256) -- one order for
// the whole batch (mid_solve_batch) or an order and an offset per matrix (mid_solve_ragged, the fourth tier of the
// ragged batch); both run the one body described here -- one
// workgroup per matrix, the matrix RESIDENT IN GLOBAL MEMORY (a 256 x 256 matrix with next and hops is 1 MiB: it
// fits neither registers nor the CU's 160 KiB of LDS).  Pivots are taken FWX_MID_B at a time from time-k snapshots
// held in LDS -- the fused engine's exactness argument inside one workgroup.
//
// For each block of pivots [k0, k0 + bt), bt <= B, the first block at k_begin:
//   1. panel.  The pivot rows (bt x n) and pivot columns (n x bt, stored transposed) of rate / next / hops are
//      loaded into LDS: W / WN / WH [t][j] = entry (k0+t, j), C / CN / CH [t][i] = entry (i, k0+t).  The diagonal
//      entry (k0+t, k0+t) is not read: both panels hold NaN there, which IS the three skips of the panel phase and
//      two of the sweep's (i == k: C[t][k] is NaN; j == k: W[t][k] is NaN; a diagonal target is NaN and NaN < x is
//      false).  Then for t = 0 .. bt-2, k = k0 + t: row t of W and row t of C as they stand are the time-k
//      snapshots and are frozen; pivot k is applied to the rows t' > t of W (operands C[t][k0+t'], W[t][j]) and of C
//      (operands C[t][i], W[t][k0+t']) -- one multiply, one strict compare, the list rule, hops added.  A cross
//      entry (k0+a, k0+b) lives in both panels; while both copies are unfrozen they see the same operands and stay
//      equal, and once one is frozen it is that panel's snapshot.  The matrix in global memory is not modified and
//      nothing is counted.
//   2. sweep.  Every entry (i, j), i != j, is read from global memory once and folds the candidates
//      C[t][i] * W[t][j] in ascending t with the strict <.  Only the LAST winning t matters for next and hops
//      (every win overwrites both), so the fold keeps x, that t and a count; on a win next = CN[t][i] if that is >= 0
//      else WN[t][j] (Algorithms.hs:55: an empty ikPath takes the head of kjPath), hops = CH[t][i] + WH[t][j], and
//      the entry is written back -- otherwise nothing is stored.  Every successful compare counts one towards U.
//   3. ONE workgroup barrier between the sweep and the next block's panel loads: workgroup-scope visibility of the
//      sweep's global stores (the whole workgroup runs on one CU), and the panels in LDS are free again.
// The path trace (HAS_LAST; PathLog in fwx_kernels.h, whole pivot range only) rides on the same three phases and
// lives in GLOBAL memory throughout -- no LDS copy, so every dtype and field set has one code path and the f64 +
// next + hops form keeps its 133 128 bytes of LDS (two more int32 panels would make 166 408 > 163 840):
//   0. before the first block the workgroup fills last with -1 (every cell, the diagonal's too), one barrier.
//   1. panel load copies last of the pivot rows to at_row and of the pivot columns to at_col -- last as it stands at
//      BLOCK START; a panel-phase win of pivot k0+t on W[u][j] then stores at_row[k0+u][j] = k0+t, one on C[u][i]
//      stores at_col[i][k0+u] = k0+t.  When row u is frozen the cells hold last of the entry at the start of step
//      k0+u, which is what the walk reads.  A cell is written by different waves at different t: the barrier between
//      pivots orders those stores (one CU, one L1, in-order vector memory; the argument of 3. below).
//   2. sweep: a win stores last = k0 + (the last winning t) with next and hops.
// Over the whole range every cell of at_row / at_col is written by exactly one panel load.
// No communication between workgroups, no grid barrier, no spin-wait; every barrier is reached by all 1024 threads
// and its trip count is a function of (n, k_begin, k_end, B) alone.  The ragged kernel's two early exits (an id
// outside the batch, an order outside 1 .. FWX_MID_N) are workgroup-uniform and come before the first barrier: a
// plan that does not belong to the arrays idles workgroups, it cannot hang or misplace one.
//
// Geometry: 1024 threads; thread (rg, c) = (tid / CW, tid % CW) with CW = n rounded up to a multiple of 64, so a wave
// never straddles two row groups (rg is wave-uniform) and at most 63 columns plus one wave idle.  In the sweep a
// thread keeps W[0..B)[c] in registers and walks the rows rg, rg + RGS, ...: C[t][i] is then a wave-uniform LDS
// read (a broadcast) and the global loads / stores of a wave are one row segment.  Scalar element accesses only:
// any pitch n, no alignment beyond the element.  The gap between matrices is never read or written, the
// diagonal's rate neither.
//
// What-if sweeps (mid_solve_sweep): a third kernel on the same body.  A fixed grid of `slots` workgroups; workgroup s
// owns slot s of a scratch buffer -- n*n rates, then n*n next, then n*n hops, pitch n -- and walks the variants
// b = s, s + slots, ... < count.  Per variant: expand (base -> slot, every cell, the diagonal's rate too), patches (in
// list order), solve (the body above on the slot, whole pivot range), answer (items and full outputs read from the
// slot), with a workgroup barrier between the stages and one before the next variant's expand.  A slot is read and
// written by its own workgroup only, so here too there is no communication between workgroups, no grid barrier and no
// spin-wait: every stage hands over to the next through __syncthreads(), the ordering the body already relies on
// between its sweep's stores and its next panel loads (one workgroup, one CU, one L1).  The trip count of the variant
// loop is a function of (blockIdx.x, gridDim.x, count) alone -- workgroup-uniform -- and the kernel has no exit after
// its first barrier.  It declares no LDS of its own.
#include "fwx_kernels.h"

#include <algorithm>

namespace fwx {
namespace {

template <typename T> __device__ __forceinline__ T mid_nan();
template <> __device__ __forceinline__ float mid_nan<float>() { return __builtin_nanf(""); }
template <> __device__ __forceinline__ double mid_nan<double>() { return __builtin_nan(""); }

constexpr int kMidThreads = 1024;
constexpr int kMidB = FWX_MID_B;
static_assert(kMidB >= 1 && kMidB <= 16 && (kMidB & (kMidB - 1)) == 0,
              "a power of two (the column loads split an index by it); 16 fills the LDS of a CU in f64 with next and hops");
// Pitch of the six LDS panels, in elements.  The column panels are filled by lanes that run over t first (a
// wave reads 4 rows x 16 pivots: whole cache lines of the pivot columns) and therefore store kMidPitch elements
// apart: at 260 the 16 pivots of a row land 4 dwords apart (2-way conflicts at the worst) where a pitch of 256 would
// put them all on one bank.
constexpr int kMidPitch = FWX_MID_N + 4;
constexpr int kMidRows = 4;                   // sweep: global loads in flight per thread

// The whole solve of ONE matrix by the workgroup that calls it: rate / next / hops / the three trace arrays of plog
// point at the matrix's first element (pitch n), pivots [k_begin, k_end), U added to updates[slot] (updates may be nullptr).  n and
// the range are workgroup-uniform.  Shared by mid_solve_batch (matrix blockIdx.x of a uniform batch) and
// mid_solve_ragged (its own order and offset per workgroup); inlined into both, everything passed by value.
template <typename T, bool HAS_NEXT, bool HAS_HOPS, bool HAS_LAST>
__device__ __forceinline__ void mid_solve_body(T *rate, int32_t *next, int32_t *hops, int32_t *last, int32_t *at_row,
                                               int32_t *at_col, int n, int k_begin, int k_end,
                                               unsigned long long *updates, unsigned int slot)
{
    static_assert(HAS_NEXT || !HAS_LAST, "the trace goes with next");
    constexpr int B = kMidB, P = kMidPitch;
    __shared__ T W[B][P], C[B][P];
    __shared__ int32_t WN[HAS_NEXT ? B : 1][HAS_NEXT ? P : 1], CN[HAS_NEXT ? B : 1][HAS_NEXT ? P : 1];
    __shared__ int32_t WH[HAS_HOPS ? B : 1][HAS_HOPS ? P : 1], CH[HAS_HOPS ? B : 1][HAS_HOPS ? P : 1];
    __shared__ unsigned int s_cnt;

    const int tid = threadIdx.x;
    const int cw = (n + 63) & ~63;                            // 64 .. 256
    const int rgs = kMidThreads / cw;                         // 16 .. 4 row groups
    const int rg = __builtin_amdgcn_readfirstlane(tid / cw);  // wave-uniform: cw is a multiple of 64
    const int c = tid - rg * cw;
    const bool live = rg < rgs && c < n;                      // 1024 / 192 leaves one wave over
    if (tid == 0) s_cnt = 0;
    if constexpr (HAS_LAST) {                                 // 0. the caller initialises nothing
        for (int e = tid; e < n * n; e += kMidThreads) last[e] = -1;
        __syncthreads();
    }

    unsigned int mine = 0;                                    // a WAVE total (scalar)
    for (int k0 = k_begin; k0 < k_end; k0 += B) {
        const int bt = min(B, k_end - k0);
        // ---- 1. panel: load -------------------------------------------------------------------------------
        if (live) {
            for (int t = rg; t < bt; t += rgs) {              // pivot rows: lane c on column c
                const int k = k0 + t, e = k * n + c;
                W[t][c] = c == k ? mid_nan<T>() : rate[e];
                if constexpr (HAS_NEXT) WN[t][c] = next[e];
                if constexpr (HAS_HOPS) WH[t][c] = hops[e];
                if constexpr (HAS_LAST) at_row[e] = last[e];
            }
        }
        for (int e = tid; e < n * B; e += kMidThreads) {      // pivot columns: lane on (i, t), t fastest
            const int t = e & (B - 1), i = e / B;
            if (t < bt) {
                const int k = k0 + t, g = i * n + k;
                C[t][i] = i == k ? mid_nan<T>() : rate[g];
                if constexpr (HAS_NEXT) CN[t][i] = next[g];
                if constexpr (HAS_HOPS) CH[t][i] = hops[g];
                if constexpr (HAS_LAST) at_col[g] = last[g];
            }
        }
        __syncthreads();
        // ---- 1. panel: pivots k0 .. k0+bt-2 on the rows of both panels that are not yet frozen ------------
        for (int t = 0; t + 1 < bt; ++t) {
            if (live) {
                const T wc = W[t][c], cc = C[t][c];
                int32_t wnc = -1, cnc = -1, whc = 0, chc = 0;
                if constexpr (HAS_NEXT) { wnc = WN[t][c]; cnc = CN[t][c]; }
                if constexpr (HAS_HOPS) { whc = WH[t][c]; chc = CH[t][c]; }
                for (int u = t + 1 + rg; u < bt; u += rgs) {  // u is wave-uniform: the other operand is a broadcast
                    const int ku = k0 + u;
                    // row k0+u of the matrix: entry (ku, c) against (ku, k) * (k, c)
                    const T cand_w = C[t][ku] * wc;
                    if (W[u][c] < cand_w) {
                        W[u][c] = cand_w;
                        if constexpr (HAS_NEXT) { const int32_t h = CN[t][ku]; WN[u][c] = h >= 0 ? h : wnc; }
                        if constexpr (HAS_HOPS) WH[u][c] = CH[t][ku] + whc;
                        if constexpr (HAS_LAST) at_row[ku * n + c] = k0 + t;
                    }
                    // column k0+u of the matrix: entry (c, ku) against (c, k) * (k, ku)
                    const T cand_c = cc * W[t][ku];
                    if (C[u][c] < cand_c) {
                        C[u][c] = cand_c;
                        if constexpr (HAS_NEXT) CN[u][c] = cnc >= 0 ? cnc : WN[t][ku];
                        if constexpr (HAS_HOPS) CH[u][c] = chc + WH[t][ku];
                        if constexpr (HAS_LAST) at_col[c * n + ku] = k0 + t;
                    }
                }
            }
            __syncthreads();
        }
        // ---- 2. sweep --------------------------------------------------------------------------------------
        if (rg < rgs) {                                       // wave-uniform
            T w[B];
#pragma unroll
            for (int t = 0; t < B; ++t) w[t] = (t < bt && c < n) ? W[t][c] : mid_nan<T>();
            for (int i0 = rg; i0 < n; i0 += rgs * kMidRows) {
                T x[kMidRows];
#pragma unroll
                for (int m = 0; m < kMidRows; ++m) {
                    const int i = i0 + m * rgs;
                    // +inf: no candidate compares greater (a lane without an entry, or the diagonal's)
                    x[m] = (T)__builtin_huge_val();
                    if (i < n && c < n && i != c) x[m] = rate[i * n + c];
                }
#pragma unroll
                for (int m = 0; m < kMidRows; ++m) {
                    const int i = i0 + m * rgs;
                    if (i >= n) break;                        // scalar
                    T v = x[m];
                    int tb = -1;
#pragma unroll
                    for (int t = 0; t < B; ++t) {
                        const T cand = C[t][i] * w[t];        // Algorithms.hs:61; NaN where a skip applies
                        const bool p = v < cand;              // :55 (false on NaN)
                        v = p ? cand : v;
                        tb = p ? t : tb;
                        mine += (unsigned int)__builtin_popcountll(__ballot(p));
                    }
                    if (tb >= 0) {
                        const int e = i * n + c;
                        rate[e] = v;
                        if constexpr (HAS_NEXT) { const int32_t h = CN[tb][i]; next[e] = h >= 0 ? h : WN[tb][c]; }
                        if constexpr (HAS_HOPS) hops[e] = CH[tb][i] + WH[tb][c];
                        if constexpr (HAS_LAST) last[e] = k0 + tb;
                    }
                }
            }
        }
        // ---- 3. the sweep's stores before the next block's loads; the panels free again ---------------------
        __syncthreads();
    }
    if (updates) {
        if (mine && (tid & 63) == 0) atomicAdd(&s_cnt, mine);
        __syncthreads();
        if (tid == 0 && s_cnt) atomicAdd(&updates[slot], (unsigned long long)s_cnt);
    }
}

// Uniform batch: workgroup b on matrix b, at b * stride.
template <typename T, bool HAS_NEXT, bool HAS_HOPS, bool HAS_LAST>
__global__ __launch_bounds__(kMidThreads) void mid_solve_batch(T *rate, int32_t *next, int32_t *hops, int n,
                                                               long long stride, int k_begin, int k_end,
                                                               unsigned long long *updates, PathLog plog)
{
    const size_t off = (size_t)blockIdx.x * (size_t)stride;
    mid_solve_body<T, HAS_NEXT, HAS_HOPS, HAS_LAST>(rate + off, HAS_NEXT ? next + off : nullptr,
                                                    HAS_HOPS ? hops + off : nullptr,
                                                    HAS_LAST ? plog.last + off : nullptr,
                                                    HAS_LAST ? plog.at_row + off : nullptr,
                                                    HAS_LAST ? plog.at_col + off : nullptr, n, k_begin, k_end,
                                                    updates, blockIdx.x);
}

// Ragged batch, mid tier: workgroup w of the launch on matrix id = order[w], of order n_each[id], at element
// offset[id] of every array, pitch n_each[id], whole pivot range; U goes to updates[id].  `order` is the mid tier's part
// of a four-tier plan (fwx_ragged_mid_plan).  The three index loads go through workgroup-uniform addresses (scalar
// loads), so n stays a scalar and every trip count of the body one as well.  An id outside [0, count) or an order
// outside [1, FWX_MID_N] (a plan that does not belong to these arrays) makes the whole workgroup leave here -- both
// tests are workgroup-uniform and come before the body's first barrier and first memory access, so all 1024 threads
// leave or none does.  The tile holds every order from 1 up: a small matrix listed here is solved, not skipped.
template <typename T, bool HAS_NEXT, bool HAS_HOPS, bool HAS_LAST>
__global__ __launch_bounds__(kMidThreads) void mid_solve_ragged(T *rate, int32_t *next, int32_t *hops, int count,
                                                                const int32_t *n_each, const int64_t *offset,
                                                                const int32_t *order, unsigned long long *updates,
                                                                PathLog plog)
{
    const int id = order[blockIdx.x];
    if ((unsigned)id >= (unsigned)count) return;              // workgroup-uniform, before any barrier
    const int n = n_each[id];
    if (n <= 0 || n > FWX_MID_N) return;
    const size_t off = (size_t)offset[id];
    mid_solve_body<T, HAS_NEXT, HAS_HOPS, HAS_LAST>(rate + off, HAS_NEXT ? next + off : nullptr,
                                                    HAS_HOPS ? hops + off : nullptr,
                                                    HAS_LAST ? plog.last + off : nullptr,
                                                    HAS_LAST ? plog.at_row + off : nullptr,
                                                    HAS_LAST ? plog.at_col + off : nullptr, n, 0, n,
                                                    updates, (unsigned int)id);
}

// [ptr[b], ptr[b + 1]) clamped into [0, total], as SweepIO::range (fwx_kernels.hip): a descending pair and a null
// table are empty ranges.  b is workgroup-uniform.
__device__ __forceinline__ void sweep_mid_range(const int64_t *ptr, long long b, long long total, long long &lo,
                                                long long &hi)
{
    lo = hi = 0;
    if (!ptr || total <= 0) return;
    long long a = ptr[b], e = ptr[b + 1];
    a = a < 0 ? 0 : a;
    e = e > total ? total : e;
    lo = a;
    hi = e < a ? a : e;
}

// What-if sweep, mid tier: workgroup s of `gridDim.x` slots on the variants s, s + gridDim.x, ... of one base (pitch
// n, const).  Its slot: rate at scratch + s * FWX_MID_SWEEP_SLOT_BYTES(n), next behind the n*n rates, hops behind
// next.  The stages of one variant, a barrier after each:
//   1. expand   e = tid, tid + 1024, ...: the slot's cell e = the base's, every field present.  The diagonal's rate is
//               copied like any cell: the body neither reads nor writes it, so the slot keeps the base's -- or the
//               patched -- value, which is what an item on (i, i) and a full output receive.
//   2. patches  ONE lane (thread 0) walks [p0, p1) in program order, so a later patch of a cell wins by construction;
//               an index outside [0, n*n) is passed over, a null patch_next / patch_hops leaves the expanded value.
//               A sweep has a handful of patches a variant: spreading them over lanes would need a rule for two
//               patches of one cell (the cost of the serial walk was not measured on its own).
//   3. solve    the body on the slot.
//   4. answer   thread t takes the items q0 + t, q0 + t + 1024, ...; an item with src or dst outside [0, n) leaves its
//               outputs alone.  The full outputs given receive the slot's n*n cells, diagonal included, at
//               + b * stride; the gap is never written.
// Nothing of the base is written; nothing outside the tables' stated extents is read.
template <typename T, bool HAS_NEXT, bool HAS_HOPS>
__global__ __launch_bounds__(kMidThreads) void mid_solve_sweep(const T *base_rate, const int32_t *base_next,
                                                               const int32_t *base_hops, int n, int count,
                                                               SweepTables<T> t, unsigned long long *updates,
                                                               char *scratch)
{
    const int tid = threadIdx.x;
    const int cells = n * n;                                  // <= 65536
    T *const rate = (T *)(scratch + (size_t)blockIdx.x * FWX_MID_SWEEP_SLOT_BYTES(n));
    int32_t *const next = (int32_t *)(rate + cells), *const hops = next + cells;
    for (long long b = blockIdx.x; b < count; b += gridDim.x) {
        // ---- 1. expand ---------------------------------------------------------------------------------------
        for (int e = tid; e < cells; e += kMidThreads) {
            rate[e] = base_rate[e];
            if constexpr (HAS_NEXT) next[e] = base_next[e];
            if constexpr (HAS_HOPS) hops[e] = base_hops[e];
        }
        __syncthreads();
        // ---- 2. patches --------------------------------------------------------------------------------------
        if (tid == 0) {
            long long p0, p1;
            sweep_mid_range(t.patch_ptr, b, t.patch_total, p0, p1);
#pragma unroll 1
            for (long long q = p0; q < p1; ++q) {
                const long long idx = t.patch_index[q];
                if (idx < 0 || idx >= cells) continue;
                rate[idx] = t.patch_rate[q];
                if constexpr (HAS_NEXT) { if (t.patch_next) next[idx] = t.patch_next[q]; }
                if constexpr (HAS_HOPS) { if (t.patch_hops) hops[idx] = t.patch_hops[q]; }
            }
        }
        __syncthreads();
        // ---- 3. solve ----------------------------------------------------------------------------------------
        // Safe in a loop: the body's only state outside the slot is its LDS.  (a) s_cnt: thread 0 zeroes it on
        // entry, and thread 0 is also the only reader of the previous call's total (its last statement, program
        // order); this call's atomicAdds come after the pivot loop, which holds at least one barrier (n >= 1), so
        // none can fall before the reset.  (b) the panels: the body's pivot loop ends on a barrier (its step 3), so
        // every read of W / C / ... of this call is over when the call returns, and that barrier is also what makes
        // the sweep's stores to the slot visible to stage 4 -- the same hand-over as from one pivot block to the next.
        mid_solve_body<T, HAS_NEXT, HAS_HOPS, false>(rate, HAS_NEXT ? next : nullptr, HAS_HOPS ? hops : nullptr,
                                                     nullptr, nullptr, nullptr, n, 0, n, updates, (unsigned int)b);
        __syncthreads();
        // ---- 4. answer ---------------------------------------------------------------------------------------
        long long q0, q1;
        sweep_mid_range(t.item_ptr, b, t.item_total, q0, q1);
        for (long long q = q0 + tid; q < q1; q += kMidThreads) {
            const int s = t.item_src[q], d = t.item_dst[q];
            if ((unsigned)s >= (unsigned)n || (unsigned)d >= (unsigned)n) continue;
            const int e = s * n + d;
            t.item_rate[q] = rate[e];
            if constexpr (HAS_NEXT) { if (t.item_next) t.item_next[q] = next[e]; }
            if constexpr (HAS_HOPS) { if (t.item_hops) t.item_hops[q] = hops[e]; }
        }
        const size_t off = (size_t)b * (size_t)t.full_stride;
        if (t.full_rate)
            for (int e = tid; e < cells; e += kMidThreads) t.full_rate[off + e] = rate[e];
        if constexpr (HAS_NEXT) {
            if (t.full_next)
                for (int e = tid; e < cells; e += kMidThreads) t.full_next[off + e] = next[e];
        }
        if constexpr (HAS_HOPS) {
            if (t.full_hops)
                for (int e = tid; e < cells; e += kMidThreads) t.full_hops[off + e] = hops[e];
        }
        // ---- 5. the slot is free for the next variant's expand -------------------------------------------------
        __syncthreads();
    }
}

}  // namespace

template <typename T>
hipError_t launch_batch_mid(T *rate, int32_t *next, int32_t *hops, int count, int n, long long stride, int k_begin,
                            int k_end, unsigned long long *updates_each, hipStream_t s, PathLog plog)
{
    if (count <= 0 || n <= 0) return hipSuccess;
    const bool traced = plog.last != nullptr;
    if (traced && (!next || !plog.at_col || !plog.at_row || k_begin != 0 || k_end != n)) return hipErrorInvalidValue;
    if (k_end <= k_begin) return hipSuccess;
    if (n > FWX_MID_N || (hops && !next) || k_begin < 0 || k_end > n || stride < (long long)n * n)
        return hipErrorInvalidValue;
    constexpr int kChunk = 1 << 21;           // workgroups per launch, as launch_batch_solve
    for (long long b0 = 0; b0 < count; b0 += kChunk) {
        const int cnt = (int)std::min<long long>(kChunk, count - b0);
        const size_t off = (size_t)b0 * (size_t)stride;
        T *r = rate + off;
        int32_t *nx = next ? next + off : nullptr, *hp = hops ? hops + off : nullptr;
        unsigned long long *u = updates_each ? updates_each + b0 : nullptr;
        PathLog pl;
        if (traced) { pl.last = plog.last + off; pl.at_col = plog.at_col + off; pl.at_row = plog.at_row + off; }
#define FWX_BATCH_MID(HN, HH, HL)                                                                  \
    hipLaunchKernelGGL((mid_solve_batch<T, HN, HH, HL>), dim3(cnt), dim3(kMidThreads), 0, s, r, nx, hp, n, stride, \
                       k_begin, k_end, u, pl)
        if (traced && hops) FWX_BATCH_MID(true, true, true);
        else if (traced) FWX_BATCH_MID(true, false, true);
        else if (hops) FWX_BATCH_MID(true, true, false);
        else if (next) FWX_BATCH_MID(true, false, false);
        else FWX_BATCH_MID(false, false, false);
#undef FWX_BATCH_MID
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <typename T>
hipError_t launch_ragged_mid(T *rate, int32_t *next, int32_t *hops, int count, const int32_t *n_each,
                             const int64_t *offset, const int32_t *order, long long listed,
                             unsigned long long *updates_each, hipStream_t s, PathLog plog)
{
    if (count < 0 || listed < 0 || listed > count || (hops && !next)) return hipErrorInvalidValue;
    if (listed == 0) return hipSuccess;
    const bool traced = plog.last != nullptr;
    if (!rate || !n_each || !offset || !order || (traced && (!next || !plog.at_col || !plog.at_row)))
        return hipErrorInvalidValue;
    constexpr int kChunk = 1 << 21;           // workgroups per launch, as launch_batch_mid
    for (long long b0 = 0; b0 < listed; b0 += kChunk) {
        const int cnt = (int)std::min<long long>(kChunk, listed - b0);
        const int32_t *ord = order + b0;
#define FWX_RAGGED_MID(HN, HH, HL)                                                                 \
    hipLaunchKernelGGL((mid_solve_ragged<T, HN, HH, HL>), dim3(cnt), dim3(kMidThreads), 0, s, rate, next, hops, count, \
                       n_each, offset, ord, updates_each, plog)
        if (traced && hops) FWX_RAGGED_MID(true, true, true);
        else if (traced) FWX_RAGGED_MID(true, false, true);
        else if (hops) FWX_RAGGED_MID(true, true, false);
        else if (next) FWX_RAGGED_MID(true, false, false);
        else FWX_RAGGED_MID(false, false, false);
#undef FWX_RAGGED_MID
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <typename T>
hipError_t launch_sweep_mid(const T *base_rate, const int32_t *base_next, const int32_t *base_hops, int count, int n,
                            const SweepTables<T> &t, unsigned long long *updates_each, void *scratch, int slots,
                            hipStream_t s)
{
    if (count <= 0 || n <= 0) return hipSuccess;
    if (n > FWX_MID_N || !base_rate || (base_hops && !base_next) || t.patch_total < 0 || t.item_total < 0 ||
        (t.patch_total > 0 && (!t.patch_ptr || !t.patch_index || !t.patch_rate)) ||
        (t.item_total > 0 && (!t.item_ptr || !t.item_src || !t.item_dst || !t.item_rate)) ||
        ((t.patch_next || t.item_next || t.full_next) && !base_next) ||
        ((t.patch_hops || t.item_hops || t.full_hops) && !base_hops) ||
        ((t.full_rate || t.full_next || t.full_hops) && t.full_stride < (long long)n * n) || slots < 1 || !scratch ||
        ((uintptr_t)scratch & 15))
        return hipErrorInvalidValue;
    const int grid = std::min(slots, count);
#define FWX_SWEEP_MID(HN, HH)                                                                      \
    hipLaunchKernelGGL((mid_solve_sweep<T, HN, HH>), dim3(grid), dim3(kMidThreads), 0, s, base_rate, base_next,    \
                       base_hops, n, count, t, updates_each, (char *)scratch)
    if (base_hops) FWX_SWEEP_MID(true, true);
    else if (base_next) FWX_SWEEP_MID(true, false);
    else FWX_SWEEP_MID(false, false);
#undef FWX_SWEEP_MID
    return hipGetLastError();
}

template hipError_t launch_sweep_mid<float>(const float *, const int32_t *, const int32_t *, int, int,
                                            const SweepTables<float> &, unsigned long long *, void *, int, hipStream_t);
template hipError_t launch_sweep_mid<double>(const double *, const int32_t *, const int32_t *, int, int,
                                             const SweepTables<double> &, unsigned long long *, void *, int,
                                             hipStream_t);

template hipError_t launch_ragged_mid<float>(float *, int32_t *, int32_t *, int, const int32_t *, const int64_t *,
                                             const int32_t *, long long, unsigned long long *, hipStream_t, PathLog);
template hipError_t launch_ragged_mid<double>(double *, int32_t *, int32_t *, int, const int32_t *, const int64_t *,
                                              const int32_t *, long long, unsigned long long *, hipStream_t, PathLog);

template hipError_t launch_batch_mid<float>(float *, int32_t *, int32_t *, int, int, long long, int, int,
                                            unsigned long long *, hipStream_t, PathLog);
template hipError_t launch_batch_mid<double>(double *, int32_t *, int32_t *, int, int, long long, int, int,
                                             unsigned long long *, hipStream_t, PathLog);

}  // namespace fwx
