// fwx_kernels.hip -- hand-written CDNA4 (gfx950) kernels for the max-product Floyd-Warshall
// relaxation  runAlgo  (/root/reference/src/lib/Algorithms.hs:42-61).
//
// Written for MI355X only: 64-lane wavefronts, 16-byte coalesced vector loads (1 KiB per wave
// instruction), pivot column staged in LDS, pivot row segment held in registers, rare-path
// predicated stores.  No MFMA: (max, x) with a strict compare is not a dense contraction.
//
// Kernel 1  relax_k      one launch per pivot k over a slab of rows (HBM-bound streaming read)
//           relax_kt     2, 4, 8, 16 or (relax_walk) 32 neighbouring pivots per launch from time-k snapshots (rates only, whole
//                        matrix in place): the same stream, read once per launch instead of once per pivot
// Kernel 2  snapshot_row copies pivot row k into the snapshot panel (panel phase, multi-GPU)
//
// Exactness rules shared by every kernel:
//   c = r[i][k] * r[k][j]      one IEEE multiply, never contracted        (Algorithms.hs:61)
//   update iff r[i][j] < c     strict ordered compare, false on NaN       (Algorithms.hs:55)
//   skip i == k                                                            (Algorithms.hs:50)
//   skip j == i, j == k                                                    (Algorithms.hs:54)
// The i==k and j==k skips are realised by replacing the operand by NaN (NaN * x = NaN and
// `r < NaN` is false for every r), which costs nothing in the streaming loop; the j==i skip is
// checked only in the rare path that has already found `r < c`.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <type_traits>
#include <utility>

#include "fwx_kernels.h"

#pragma clang fp contract(off)

namespace fwx {

template <typename T, int W> struct VecOf;
template <> struct VecOf<float, 4> { typedef float type __attribute__((ext_vector_type(4))); };
template <> struct VecOf<float, 2> { typedef float type __attribute__((ext_vector_type(2))); };
template <> struct VecOf<double, 2> { typedef double type __attribute__((ext_vector_type(2))); };
template <> struct VecOf<float, 1> { typedef float type; };
template <> struct VecOf<double, 1> { typedef double type; };

template <typename T> __device__ __forceinline__ T quiet_nan();
template <> __device__ __forceinline__ float quiet_nan<float>() { return __builtin_nanf(""); }
template <> __device__ __forceinline__ double quiet_nan<double>() { return __builtin_nan(""); }

template <typename T, int W> struct Lanes {
    using V = typename VecOf<T, W>::type;
    static __device__ __forceinline__ T get(const V &v, int c) { return v[c]; }
    static __device__ __forceinline__ void set(V &v, int c, T x) { v[c] = x; }
    static __device__ __forceinline__ V splat(T x) { V v; for (int c = 0; c < W; ++c) v[c] = x; return v; }
};
template <typename V, bool NT, typename T> __device__ __forceinline__ V load_vec(const T *p)
{
    if (NT) return __builtin_nontemporal_load(reinterpret_cast<const V *>(p));
    return *reinterpret_cast<const V *>(p);
}

// a < b (strict, ordered: false on NaN) as the wave-wide compare: the lane mask of the one v_cmp_lt the plain
// `<` compiles to, in scalar registers.  A lane that is not active has a zero bit, so a caller that hands the
// mask back to the lanes (__builtin_amdgcn_inverse_ballot_w64) or counts its bits must run with every lane of
// the wave active; relax_kt calls it only from workgroup-uniform control flow.
constexpr int FWX_FCMP_OLT = 4;               // llvm::CmpInst::FCMP_OLT, the predicate operand of llvm.amdgcn.fcmp
__device__ __forceinline__ unsigned long long wave_lt(float a, float b)
{
    return __builtin_amdgcn_fcmpf(a, b, FWX_FCMP_OLT);
}
__device__ __forceinline__ unsigned long long wave_lt(double a, double b)
{
    return __builtin_amdgcn_fcmp(a, b, FWX_FCMP_OLT);
}

// Dispatch position -> tile.  flip 0: in order; 1: reversed; 2: reversed in groups of 8, so that a
// tile keeps blockIdx.x % 8 and with it its XCD under round-robin dispatch (needs gridDim.x % 8 == 0,
// the launcher passes 1 otherwise).  Speed only: every mapping is a permutation of the tiles.
__device__ __forceinline__ int visit_tile(int flip)
{
    const int g = (int)gridDim.x, b = (int)blockIdx.x;
    if (flip == 2) return (g / 8 - 1 - b / 8) * 8 + (b & 7);
    return flip ? g - 1 - b : b;
}

template <typename T> struct Lanes<T, 1> {
    using V = T;
    static __device__ __forceinline__ T get(const V &v, int) { return v; }
    static __device__ __forceinline__ void set(V &v, int, T x) { v = x; }
    static __device__ __forceinline__ V splat(T x) { return x; }
};

// -------------------------------------------------------------------------------------------------
// relax_k: step k of runAlgo on `rows` rows of the matrix.
//
// Work decomposition.  A workgroup (256 threads = 4 waves) owns a column strip of
// SW = 256*NV*W elements and a chunk of RPB consecutive rows.  Thread t holds, for the whole
// chunk, the NV vectors of the PIVOT ROW that cover its columns (registers), and the workgroup
// stages the chunk's PIVOT COLUMN values r[i][k] (and next[i][k], hops[i][k]) in LDS with one
// strided gather.  The streaming loop then touches HBM only for r[i][j]: each wave instruction
// reads 1 KiB of one row, UNROLL*NV such loads are in flight per thread.
//
// Stores happen only where r[i][j] < c (about 0.2 % of entries per launch at N = 16384, SURVEY.md
// Appendix B).  With next/hops: one exec-masked 16-byte store of the updated vector plus scalar
// stores of next/hops for the updated components (`SV` = RELAX_SV_LEGACY).  Rates only: the store
// granularity is GL aligned lanes (GL * 16 bytes, RelaxArgs::store_bytes): when any lane of a
// group improved, every lane of the group stores its vector, the lanes that did not improve writing
// back the exact bits they loaded in this launch, so a store covers whole 64-byte sectors / 128-byte
// lines instead of scattered 16-byte pieces of them.  That write-back is
// exact because within one launch every element belongs to exactly one lane and no one else writes
// it: column k gets an identical rewrite under its readers (the pivot-column gathers), row k
// (NaN pivot operand) never improves so its groups never store.  Clamped lanes (past the end of
// the row, duplicating the owner of the last vector) are excluded from every group: their copy is
// stale.  The new vector is built with selects and the group mask comes from a wave ballot
// outside any divergent region; U counts improved components only.
//
// `flip` (visit_tile) reverses the block order: launches alternate direction so that the tiles
// streamed last by pivot k are streamed first by pivot k+1; in groups of 8 (flip 2) they also run on
// the XCD whose L2 still holds them.
//
// `nt_below`: the tiles below it (the slab's first rows) stream r[i][j] with non-temporal loads, the
// rest (its last rows) with default-policy loads, the same rows in every launch whatever the sweep
// order.  Measured 4-5 % faster per launch at N = 16384 (profiles/r05_tune_relax_policy.txt); the
// presumed reason, which no counter shows: non-temporal loads do not allocate in the 256 MiB Infinity
// Cache, so the default-policy rows stay resident there while the rest streams past them.  The pivot
// row, the pivot-column gather and all stores keep the default policy.  A cache hint only: no result
// bit depends on it.
// -------------------------------------------------------------------------------------------------
// Store variants (SV).  The production rates-only path is RELAX_SV_SELECT; next/hops always take
// RELAX_SV_LEGACY.  The others exist for tools/tune_relax.hip `stores` mode only (timing; their
// results are wrong by design): SKIP = SELECT behind a wave-uniform skip of rows where no lane
// compares true, NOSTORE = LEGACY with every store suppressed (its arithmetic and branch kept),
// NORARE = the rare path compiled out (loads and compares kept), NTST = SELECT with non-temporal
// stores everywhere.  NTST_NTROWS = SELECT with non-temporal stores in the rows that are streamed
// with non-temporal loads (`nt_below`), default-policy stores in the temporal tail.
enum { RELAX_SV_SELECT = 0, RELAX_SV_SKIP = 1, RELAX_SV_LEGACY = 2, RELAX_SV_NOSTORE = 3, RELAX_SV_NORARE = 4,
       RELAX_SV_NTST = 5, RELAX_SV_NTST_NTROWS = 6 };

template <typename T, int W, int NV, int RPB, int UNROLL, bool HAS_NEXT, bool HAS_HOPS, bool COUNT,
          int MINW = 1, int GL = 1, int SV = RELAX_SV_SELECT>
__global__ __launch_bounds__(256, MINW) void relax_k(T *rate, int32_t *next, int32_t *hops,
                                               const T *prow, const int32_t *phops,
                                               const int32_t *pnext, int rows,
                                               int n, int row0, int k, int nstrips, int flip,
                                               unsigned long long *updates, PathLog plog,
                                               int skip_lo, int skip_hi, int nt_below)
{
    using L = Lanes<T, W>;
    using V = typename L::V;
    constexpr int SW = 256 * NV * W;

    __shared__ T s_col[RPB];
    __shared__ int32_t s_ncol[HAS_NEXT ? RPB : 1];
    __shared__ int32_t s_hcol[HAS_HOPS ? RPB : 1];
    __shared__ unsigned int s_cnt;

    const int t = threadIdx.x;
    const int bid = visit_tile(flip);
    const int strip = bid % nstrips;
    const int chunk = bid / nstrips;
    const int r_begin = chunk * RPB;
    const int r_cnt = min(RPB, rows - r_begin);
    if (r_begin >= skip_lo && r_begin < skip_hi) return;   // whole workgroup: rows already relaxed

    // Pivot column -> LDS (one strided gather per chunk).  Row k itself gets NaN: skip i == k.
    if (t < r_cnt) {
        const size_t off = (size_t)(r_begin + t) * n + k;
        T v = rate[off];
        if (row0 + r_begin + t == k) v = quiet_nan<T>();
        s_col[t] = v;
        if (HAS_NEXT) s_ncol[t] = next[off];
        if (HAS_HOPS) s_hcol[t] = hops[off];
    }
    if (COUNT && t == 0) s_cnt = 0;
    if (HAS_NEXT && plog.last) {
        // snapshots of `last` for step k (see PathLog): column k by the first strip's workgroups,
        // row k by the first chunk's -- neither is modified during this launch
        if (strip == 0 && t < r_cnt) {
            const size_t off = (size_t)(row0 + r_begin + t) * n + k;
            plog.at_col[off] = plog.last[off];
        }
        if (chunk == 0) {
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int c0 = strip * SW + (v * 256 + t) * W;
#pragma unroll
                for (int c = 0; c < W; ++c)
                    if (c0 + c < n) plog.at_row[(size_t)k * n + c0 + c] = plog.last[(size_t)k * n + c0 + c];
            }
        }
    }

    // Pivot row segment -> registers.  Column k gets NaN: skip j == k.  Columns past the end
    // of the row are CLAMPED to the last in-range vector and their pivot set to NaN: the
    // streaming loads stay unconditional (valid addresses) and such lanes can never update.
    static_assert(GL == 1 || GL == 2 || GL == 4 || GL == 8, "store group: 1, 2, 4 or 8 lanes");
    constexpr bool SEL = !HAS_NEXT && !HAS_HOPS && (SV == RELAX_SV_SELECT || SV == RELAX_SV_SKIP ||
                                                    SV == RELAX_SV_NTST || SV == RELAX_SV_NTST_NTROWS);
    V p[NV];
    int col[NV];
    bool own[NV];             // false: a clamped lane (never stores)
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int c0 = strip * SW + (v * 256 + t) * W;
        own[v] = c0 < n;
        if (c0 < n) {
            col[v] = c0;
            p[v] = *reinterpret_cast<const V *>(prow + c0);
#pragma unroll
            for (int c = 0; c < W; ++c)
                if (c0 + c == k) L::set(p[v], c, quiet_nan<T>());
        } else {
            col[v] = n - W;
            p[v] = L::splat(quiet_nan<T>());
        }
    }
    __syncthreads();

    unsigned int my_updates = 0;
    bool sink = false;        // RELAX_SV_NORARE: keeps the compares alive
    T *const base = rate + (size_t)r_begin * n;
    const int g0 = (int)(__lane_id() & ~(GL - 1));   // first lane of my store group

    // One row of one vector: compare, and in the rare case that something improves, store.
    auto relax_vec = [&](const V &x, const V &pv, int r, int cv, bool mine, auto nt) {
        const T rik = s_col[r];
        bool any = false;
        T cand[W];
#pragma unroll
        for (int c = 0; c < W; ++c) {
            cand[c] = rik * L::get(pv, c);
            any |= (L::get(x, c) < cand[c]);
        }
        if constexpr (SV == RELAX_SV_NORARE) {
            sink |= any;
            return;
        }
        if constexpr (SEL) {
            // All lanes of the wave are active here (r is workgroup-uniform).  Selects, not branches;
            // the diagonal filter and the strict `<` as in the legacy path below.
            if (SV == RELAX_SV_SKIP && !__any(any)) return;   // wave-uniform
            const int i = row0 + r_begin + r;
            V nx = x;
            bool changed = false;
#pragma unroll
            for (int c = 0; c < W; ++c) {
                const bool up = L::get(x, c) < cand[c] && cv + c != i;
                L::set(nx, c, up ? cand[c] : L::get(x, c));
                changed |= up;
                if (COUNT) my_updates += up;
            }
            bool st = changed;
            if constexpr (GL > 1) {
                const unsigned long long m = __ballot(changed);
                st = mine && ((m >> g0) & ((1ull << GL) - 1)) != 0;
            }
            V *const dst = reinterpret_cast<V *>(rate + (size_t)(r_begin + r) * n + cv);
            if (SV == RELAX_SV_NTST || (SV == RELAX_SV_NTST_NTROWS && decltype(nt)::value)) {
                if (st) __builtin_nontemporal_store(nx, dst);
            } else if (st) {
                *dst = nx;
            }
            return;
        }
        if (any) {
            // Rare path: some component improves.  The diagonal (j == i) is filtered here.
            const int i = row0 + r_begin + r;
            V nx = x;
            bool changed = false;
            const size_t off = (size_t)(r_begin + r) * n + cv;
#pragma unroll
            for (int c = 0; c < W; ++c) {
                if (L::get(x, c) < cand[c] && cv + c != i) {
                    L::set(nx, c, cand[c]);
                    changed = true;
                    if (HAS_NEXT) {     // head (ikPath ++ kjPath), Algorithms.hs:55
                        const int32_t nik = s_ncol[r];
                        next[off + c] = (nik >= 0 || !pnext) ? nik : pnext[cv + c];
                    }
                    if (HAS_HOPS) hops[off + c] = s_hcol[r] + phops[cv + c];
                    if (HAS_NEXT && plog.last) plog.last[(size_t)i * n + cv + c] = k;
                    if (COUNT) ++my_updates;
                }
            }
            if (changed && (SV != RELAX_SV_NOSTORE || k < 0)) *reinterpret_cast<V *>(rate + off) = nx;
        }
    };

    auto stream = [&](auto nt) {
        constexpr bool NT = decltype(nt)::value;
        int r = 0;
        // Main loop: UNROLL rows x NV vectors of unconditional 16-byte loads in flight per thread.
        for (; r + UNROLL <= r_cnt; r += UNROLL) {
            V x[UNROLL][NV];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
#pragma unroll
                for (int v = 0; v < NV; ++v)
                    x[u][v] = load_vec<V, NT>(base + (size_t)(r + u) * n + col[v]);
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
#pragma unroll
                for (int v = 0; v < NV; ++v)
                    relax_vec(x[u][v], p[v], r + u, col[v], own[v], nt);
        }
        // Row tail (slab height not a multiple of UNROLL).
        for (; r < r_cnt; ++r) {
            V x[NV];
#pragma unroll
            for (int v = 0; v < NV; ++v)
                x[v] = load_vec<V, NT>(base + (size_t)r * n + col[v]);
#pragma unroll
            for (int v = 0; v < NV; ++v)
                relax_vec(x[v], p[v], r, col[v], own[v], nt);
        }
    };
    // workgroup-uniform: one of the two instantiations, never both
    if (bid < nt_below) stream(std::true_type());
    else stream(std::false_type());
    if (SV == RELAX_SV_NORARE && sink && k < 0) rate[0] = T(0);   // never: k >= 0

    if (COUNT) {
        if (my_updates) atomicAdd(&s_cnt, my_updates);
        __syncthreads();
        if (t == 0 && s_cnt)
            atomicAdd(&updates[bid & (FWX_UPDATE_SHARDS_K - 1)], (unsigned long long)s_cnt);
    }
}

// -------------------------------------------------------------------------------------------------
// relax_kt: steps k .. k+NP-1 of runAlgo on the whole matrix in ONE streaming pass (rates only).
//
// An entry may take several pivots in one visit if each pivot's operands are the snapshots of its row
// and column taken at its own time.  Those come from the panel kernels of the
// fused engine (fwx_fused.hip): w[t][j] = row k+t at time k+t, ct[t][i] = column k+t at time k+t with
// NaN at i == k+t.  The launch reads NOTHING of the live matrix but r[i][j] itself -- rows and columns
// k .. k+NP-1 are rewritten by their owners during the launch and are no operands here (DESIGN.md
// section 3, consequence (2)) -- so it is race-free, and the exact write-back of unchanged lanes holds
// as in relax_k: every element belongs to exactly one lane and nobody else reads or writes it.
//
// Shaped like relax_k: 256 threads with one 16-byte vector each, RPB rows per workgroup, UNROLL rows of
// unconditional loads in flight, the same visit_tile mapping, `nt_below` split and GL-lane group store.
// A thread keeps its slice of the NP pivot rows in registers (NaN at column k+t: skip j == k; NaN in
// clamped lanes), the workgroup stages ct[t][rows] in LDS, row-major (s_ct[row][t], so a row's NP values
// are one or two 16-byte reads; contiguous reads of the panel: no strided gather).  Each loaded vector
// is folded through t = 0 .. NP-1 in ascending order with
//   x = x < c ? c : x,   c = ct[t][i] * w[t][j]
// -- one IEEE multiply, the strict ordered compare -- or, bit for bit the same, through the maximum of the NP
// candidates and ONE compare, exactly where the operands allow it (round 14, below).  No domain assumption enters
// the per-k engine: the condition is read off the operands a wave has loaded, and x may be anything.  The compare
// form's fold step is three vector instructions and nothing else (round 10): the diagonal (j == i
// never updates) is protected outside the per-pivot loop, by folding that one component from +inf and
// giving it its loaded bits back, and only in the tiles whose rows meet their columns (DIAG, a
// workgroup-uniform choice like the cache-policy one); whether a vector changed is read off afterwards,
// from an integer comparison with the loaded bits.  A group stores once if any of its lanes ended
// different from what it loaded.  U counts every improvement of every fold step, which is what NP
// launches of relax_k count (the +inf component never counts).
//
// Round 13.  (1) The tile index is split into (strip, chunk) by a multiply-high with a constant the launcher
// passes (`strip_magic`) instead of an integer division, which the compiler expands into a float
// reciprocal in vector registers, a readfirstlane and some twenty dependent scalar instructions in front
// of the first address of every workgroup: that chain, not the instruction count, is what the sweep
// gained from.  (2) The COUNTING instantiation alone keeps its masks in scalar
// registers: its fold compares with the wave-wide compare (wave_lt), U is the sum of the set bits of those
// masks, one scalar count per wave, and its store rule is evaluated on the wave mask with scalar shifts.
// That needs every lane of the wave active in relax_vec: its callers are workgroup-uniform (`r`, `r_cnt`,
// `head` and the instantiation choice depend on the tile only, the row tail included), and the one
// divergent statement, the store, reconverges before the next row.  The non-counting instantiation (what
// a whole solve runs) has round 10's fold and store rule: the scalar forms compile to the same fold there
// and gain nothing measurable (profiles/r13_tune_relax_pivots.txt).
// The NaN patch of W runs in every strip, although only a strip that meets the pivot columns or the end of
// the row has a lane that needs it: without the selects the kernel was measured slower (DESIGN.md section
// 4.1, round 13).  Rows are still addressed with 64-bit vector adds: the compiler re-forms base + lane
// offset + row stride into a per-lane address chain (profiles/r13_experiments_not_adopted.txt).
//
// Round 14: the max form.  If every candidate of an entry is NaN or has its sign bit clear -- true whenever every
// w[t][j] and ct[t][i] it is built from is -- then with m = maxNum(c_0 .. c_NP-1), `x < m ? m : x` is the sequential
// fold bit for bit for every x.  The non-counting f32 instantiations (MAXF) carry both forms; a
// WAVE takes the max form iff no value of W in its lanes after the NaN patch and no staged Ct value of the tile has its
// sign bit set (one OR chain and a ballot behind the prologue's loads; FWX_PERK_FOLD=compare, the kernel argument
// `fold_compare`, forces the compare form).  Per row-vector: NP * W multiplies, a v_max3_f32 per two candidates, W
// compares, which are `changed` as well; 63 vector instructions per row for 107.  The counting instantiation keeps the
// compare form (U counts every improving step), f64 too (no max form is written for it), and so does a ragged last row
// chunk (the max form has no row-by-row tail).  These kernels of the production geometry ask for four waves per SIMD
// in their launch bound where a store group is at most four lanes (relax_kt_min_waves, below).
//
// Round 19: NP = 16, non-counting f32 only (relax_kt_wide; the schedule: relax_range_kt, FWX_PERK_WIDE).  The same
// kernel text: the NaN patch at column k + t for all 16 t, 64 registers of W, a staged row of Ct is four 16-byte
// reads, the vote reads the RPB * NP > 64 staged values back from LDS, the max form is 64 multiplies, 28 v_max3_f32
// and 4 v_max_f32 per row-vector, the compare form 16 steps.  Nothing but r[i][j] is read of the live matrix, so the
// race-freedom argument holds for 16 consecutive snapshots as for 8.  Two waves per SIMD, 16 rows per workgroup, 8
// in flight (profiles/r19_relax_kt16_isa.txt, r19_tune_relax_pivots.txt).
//
// The prologue issues every load a workgroup starts with back to back -- its pivot-column value, the NP
// vectors of W and the first UNROLL rows of the stream, all from addresses valid in every lane -- and
// patches the NaNs in with selects, so the barrier waits for one overlapped group of loads (round 10;
// before, NP exec-masked loads each waited for alone, and the stream started after the barrier).
// -------------------------------------------------------------------------------------------------
// Which element types have a max form of relax_kt's fold: f32.  f64 has the compare form alone; a max form for it
// is not written.
template <typename T> constexpr bool relax_kt_max_form() { return sizeof(T) == 4; }

// max(c[0], ..., c[N-1]) as IEEE maxNum (a NaN operand is ignored; NaN if all are): two operands per
// v_max3_f32, a lone last one by v_max_f32.  By inline asm, like fmax_t in fwx_fused.hip, for another reason: a
// chain of __builtin_fmaxf is a horizontal reduction to the SLP vectoriser, which then forms the NP products as
// one vector, multiplies with v_pk_mul_f32 on register pairs and pads every pair with s_nop (576 v_pk_mul_f32
// and 1281 s_nop in the NP = 8 kernel, profiles/r14_relax_kt_isa.txt).  The operands are products, quiet
// already, so nothing needs quieting.  VALU results feeding a VALU need no wait states.
template <int N> __device__ __forceinline__ float max_of(const float (&c)[N])
{
    float m = c[0];
    int i = 1;
#pragma unroll
    for (; i + 1 < N; i += 2) asm("v_max3_f32 %0, %1, %2, %3" : "=v"(m) : "v"(m), "v"(c[i]), "v"(c[i + 1]));
    if (i < N) asm("v_max_f32 %0, %1, %2" : "=v"(m) : "v"(m), "v"(c[i]));
    return m;
}

// Waves per SIMD the launch bound asks for.  With both forms of the fold inside, the production geometry takes 133
// VGPRs under the plain bound, for a peak in the rarely run tail loop; asked for four waves it stays at 128 without a
// spill.  Not where a group is 8 lanes (FWX_PERK_STORE_BYTES=128): that kernel spills 8 bytes under the bound and
// takes 133 VGPRs without it.  Not in the other geometries (tools/tune_relax.hip), which are timed as the compiler
// makes them (profiles/r14_relax_kt_isa.txt).
// The 16-pivot kernels (round 19) hold 64 registers of W and ask for two waves: under a bound of three or four every
// geometry spills (profiles/r19_relax_kt16_isa.txt).
template <typename T, int RPB, int UNROLL, bool COUNT, int GL, int NP = 8> constexpr int relax_kt_min_waves()
{
    if (NP > 8) return 2;
    return !COUNT && relax_kt_max_form<T>() && RPB == FWX_PERK_KT_RPB && UNROLL == FWX_PERK_KT_UNROLL && GL < 8 ? 4 : 1;
}

template <typename T, int W, int RPB, int UNROLL, bool COUNT, int GL, int NP>
__global__ __launch_bounds__(256, (relax_kt_min_waves<T, RPB, UNROLL, COUNT, GL, NP>()))
void relax_kt(T *rate, const T *w, const T *ct, int ct_ld, int n, int k,
                                                int nstrips, int flip, unsigned long long *updates,
                                                int nt_below, unsigned strip_magic, int fold_compare)
{
    using L = Lanes<T, W>;
    using V = typename L::V;
    using Bits = std::conditional_t<sizeof(T) == 4, uint32_t, uint64_t>;
    constexpr int SW = 256 * W;
    // The instantiations that carry the max form of the fold beside the compare form (header, round 14).
    constexpr bool MAXF = !COUNT && relax_kt_max_form<T>();
    static_assert(GL == 1 || GL == 2 || GL == 4 || GL == 8, "store group: 1, 2, 4 or 8 lanes");
    static_assert(NP * RPB <= 256, "one thread per staged pivot-column value");
    static_assert(64 % (NP * RPB) == 0 || NP * RPB % 64 == 0, "the fold vote: staged values per wave");

    __shared__ __attribute__((aligned(16))) T s_ct[RPB][NP];
    __shared__ unsigned int s_cnt;

    const int t = threadIdx.x;
    const int bid = visit_tile(flip);
    // Tile -> (strip, chunk).  strip_magic = ceil(2^32 / nstrips): the high word of bid * strip_magic is
    // bid / nstrips exactly while bid * nstrips < 2^32 (the launcher checks the whole grid; it passes 0 for one
    // strip and for a grid past that bound, and the division below stays for those).  Three scalar
    // instructions; the division is a float reciprocal in vector registers, a readfirstlane and a score of
    // dependent scalar instructions, and every address of the prologue's loads waits for it.
    int strip, chunk;
    if (strip_magic) {
        chunk = (int)__umulhi((unsigned)bid, strip_magic);
        strip = bid - chunk * nstrips;
    } else {
        strip = bid % nstrips;
        chunk = bid / nstrips;
    }
    const int r_begin = chunk * RPB;
    const int r_cnt = min(RPB, n - r_begin);
    if (COUNT && t == 0) s_cnt = 0;

    // My 16-byte column slice, clamped past the end of the row as in relax_k.
    const int c0 = strip * SW + t * W;
    const bool own = c0 < n;                  // false: a clamped lane (never stores)
    const int col = own ? c0 : n - W;
    // Row r of the tile is at a workgroup-uniform base plus my 32-bit byte offset: a form the compiler can
    // address with a scalar base and one offset register (it does for the W loads) instead of keeping a
    // 64-bit address per row in flight.
    const unsigned boff = (unsigned)col * (unsigned)sizeof(T);
    auto at = [&](const T *q, int r) {
        const char *const row = reinterpret_cast<const char *>(q + (size_t)r * n);
        return const_cast<T *>(reinterpret_cast<const T *>(row + boff));
    };
    T *const base = rate + (size_t)r_begin * n;
    const int g0 = (int)(__lane_id() & ~(GL - 1));   // first lane of my store group
    unsigned int wave_updates = 0;            // COUNT: U of my wave, the set bits of every compare mask (scalar)
    V p[NP];                                  // my slice of the NP pivot rows

    // The store rule on my own `changed`: a group of GL aligned lanes stores if any of its lanes changed, clamped
    // lanes never.  All lanes of the wave are active.
    auto group_stores = [&](bool changed) {
        if constexpr (GL == 1) return changed;
        const unsigned long long m = __ballot(changed);
        return own && ((m >> g0) & ((1ull << GL) - 1)) != 0;
    };

    // One row of one vector through the NP pivots, MAX FORM: only where every operand of the wave -- its lanes'
    // slices of W after the NaN patch, the tile's staged Ct -- is NaN or has its sign bit clear (`max_form`
    // below).  Then no candidate is -0 or negative, candidates that compare equal have equal bits, and with m
    // the maxNum of the NP candidates `x < m ? m : x` is the sequential fold bit for bit for EVERY loaded x:
    // where nothing beats x both keep the loaded bits (x NaN with any payload, x = -0 against m = +0), otherwise
    // both end at the bits of the numeric maximum.  m needs no x, so the row's load is
    // waited for in front of the W compares and not in front of the multiplies; the compare is `changed` as well.
    // DIAG: the component on the diagonal is masked out of the compare, so it keeps its bits and never counts.
    auto relax_vec_max = [&](const V &x, int r, auto dg) {
      if constexpr (MAXF) {
        constexpr bool DIAG = decltype(dg)::value;
        const int d = r_begin + r - col;
        T cik[NP];
#pragma unroll
        for (int tt = 0; tt < NP; ++tt) cik[tt] = s_ct[r][tt];
        T m[W];
        bool up[W];
#pragma unroll
        for (int c = 0; c < W; ++c) {
            T cand[NP];
#pragma unroll
            for (int tt = 0; tt < NP; ++tt) cand[tt] = cik[tt] * L::get(p[tt], c);
            m[c] = max_of(cand);
        }
#pragma unroll
        for (int c = 0; c < W; ++c) {
            up[c] = L::get(x, c) < m[c];
            if constexpr (DIAG) up[c] = up[c] && c != d;
        }
        // All W compares before the first select, as in the compare form.
        __builtin_amdgcn_sched_barrier(0);
        V nx;
        bool changed = false;
#pragma unroll
        for (int c = 0; c < W; ++c) {
            L::set(nx, c, up[c] ? m[c] : L::get(x, c));
            changed = changed || up[c];
        }
        if (group_stores(changed)) *reinterpret_cast<V *>(at(base, r)) = nx;
      }
    };

    // One row of one vector through the NP pivots, COMPARE FORM; all lanes of the wave are active (r is uniform).
    // DIAG: the tile may hold diagonal elements (j == i never updates).  Such a component folds from +inf,
    // which no candidate beats (`+inf < c` is false for every c, NaN included), and gets its loaded bits
    // back afterwards; the fold step itself carries no diagonal term.
    auto relax_vec = [&](const V &x, int r, auto dg) {
        constexpr bool DIAG = decltype(dg)::value;
        const int d = r_begin + r - col;      // the component of mine on the diagonal, if 0 <= d < W
        V nx = x;
        if constexpr (DIAG) {
#pragma unroll
            for (int c = 0; c < W; ++c)
                L::set(nx, c, c == d ? (T)__builtin_huge_val() : L::get(x, c));
        }
        T cik[NP];
#pragma unroll
        for (int tt = 0; tt < NP; ++tt) cik[tt] = s_ct[r][tt];
#pragma unroll
        for (int tt = 0; tt < NP; ++tt) {
            T cand[W];
            bool up[W];
            unsigned long long upm[COUNT ? W : 1];   // COUNT: the compare's lane mask, for the scalar count
#pragma unroll
            for (int c = 0; c < W; ++c) {
                cand[c] = cik[tt] * L::get(p[tt], c);
                if constexpr (COUNT) {
                    upm[c] = wave_lt(L::get(nx, c), cand[c]);
                    up[c] = __builtin_amdgcn_inverse_ballot_w64(upm[c]);
                } else {
                    up[c] = L::get(nx, c) < cand[c];
                }
            }
            // All W compares before the first select: a select that directly follows the compare whose
            // mask it reads costs idle issue slots (the compiler pads the pair with s_nop).
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int c = 0; c < W; ++c) {
                L::set(nx, c, up[c] ? cand[c] : L::get(nx, c));
                if constexpr (COUNT) wave_updates += (unsigned)__builtin_popcountll(upm[c]);
            }
        }
        // The fold is monotone under the strict compare: a component improved at some step exactly when
        // its final bits differ from the loaded ones (a NaN or -0.0 that no candidate beats keeps its bits).
        if constexpr (DIAG) {
#pragma unroll
            for (int c = 0; c < W; ++c) L::set(nx, c, c == d ? L::get(x, c) : L::get(nx, c));
        }
        bool st;
        if constexpr (GL == 1 || !COUNT) {
            Bits diff = 0;
#pragma unroll
            for (int c = 0; c < W; ++c)
                diff |= __builtin_bit_cast(Bits, L::get(nx, c)) ^ __builtin_bit_cast(Bits, L::get(x, c));
            st = group_stores(diff != 0);
        } else {
            // COUNT: the group rule ("any lane of my aligned GL-lane group changed") on the wave mask itself, in
            // scalar registers: the W integer compares each leave a lane mask, their OR is `changed` of the
            // whole wave; bit l of m becomes the OR of the bits l .. l+GL-1, the first lane of every group keeps
            // its bit and hands it to the group's other lanes, and the result is the wave's store predicate.
            constexpr unsigned long long FIRST = GL == 2 ? 0x5555555555555555ull
                                               : GL == 4 ? 0x1111111111111111ull : 0x0101010101010101ull;
            unsigned long long m = 0;
#pragma unroll
            for (int c = 0; c < W; ++c)
                m |= __builtin_amdgcn_ballot_w64(__builtin_bit_cast(Bits, L::get(nx, c)) !=
                                                 __builtin_bit_cast(Bits, L::get(x, c)));
            m |= m >> 1;
            if constexpr (GL >= 4) m |= m >> 2;
            if constexpr (GL >= 8) m |= m >> 4;
            m &= FIRST;
            m |= m << 1;
            if constexpr (GL >= 4) m |= m << 2;
            if constexpr (GL >= 8) m |= m << 4;
            st = own && __builtin_amdgcn_inverse_ballot_w64(m);
        }
        if (st) *reinterpret_cast<V *>(at(base, r)) = nx;
        // COUNT: one running count, added up row by row.  The value is uniform already; the readfirstlane is a fence
        // for the optimiser only (it costs one scalar move): without it the NP * W popcounts of every row are
        // reassociated into one sum over the whole tile, every compare mask stays live to the end and is
        // spilled lane by lane into vector registers (profiles/r13_relax_kt_isa.txt, counting kernels).
        if constexpr (COUNT) wave_updates = (unsigned)__builtin_amdgcn_readfirstlane((int)wave_updates);
    };

    auto stream = [&](auto nt, auto dg) {
        constexpr bool NT = decltype(nt)::value;
        int r = 0;
        // Prologue: everything the workgroup's first fold needs is requested back to back, from addresses
        // that are valid in every lane -- the staged pivot-column value, the NP vectors of W (from the
        // clamped column) and the first UNROLL rows of the stream, which depend on none of the others --
        // so that one wait covers one overlapped group of loads.  The NaN patches are selects afterwards.
        const int stt = t / RPB % NP, sr = min(t % RPB, r_cnt - 1);
        const T cv = ct[(size_t)stt * ct_ld + r_begin + sr];
#pragma unroll
        for (int tt = 0; tt < NP; ++tt) p[tt] = *reinterpret_cast<const V *>(at(w, tt));
        const bool head = UNROLL <= r_cnt;    // workgroup-uniform
        V x0[UNROLL];
        if (head) {
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) x0[u] = load_vec<V, NT>(at(base, u));
        }
        // Pivot columns -> LDS (row k+t of the panel already holds NaN: skip i == k).
        // Rows of a ragged chunk past the end of the matrix get the last row's values again (cv is loaded from the
        // clamped row): no fold reads them, each cell has one writer, and the store needs no row compare.  With the
        // compare the default kernel spills 4 bytes in its tail loop (profiles/r14_relax_kt_isa.txt).
        if (t < NP * RPB) s_ct[t % RPB][stt] = cv;
        // NaN at column k+t: skip j == k; NaN everywhere in a clamped lane.  In every strip, also where no
        // lane can need it (a strip that meets neither the pivot columns nor the end of the row): leaving the
        // selects out of those strips was measured slower (round 13).
#pragma unroll
        for (int tt = 0; tt < NP; ++tt)
#pragma unroll
            for (int c = 0; c < W; ++c)
                L::set(p[tt], c, !own || col + c == k + tt ? quiet_nan<T>() : L::get(p[tt], c));
        // The fold's form, per wave, from what the wave has loaded: the max form iff no operand of its rows has
        // its sign bit set (a negative NaN included: conservative and exact).  After the patch column k + t and
        // clamped lanes hold the positive quiet NaN, so a hostile r[k][k] disqualifies nobody.  The RPB x NP staged
        // Ct values lie across the wave's lanes already, in `cv` (t -> (stt, sr) has the period RPB * NP, which divides
        // 64, and sr is clamped to the tile's rows); a larger tile reads the staged rows back from LDS behind the
        // barrier.  A ragged chunk keeps the compare form.
        __syncthreads();
        bool max_form = false;
        if constexpr (MAXF) {
            // The OR is written as the instruction itself and takes the values as floats: any integer use of p[]
            // or of the loaded vectors makes the optimiser pair the multiplies of the compare form's diagonal copies
            // into v_pk_mul_f32, every pair padded with s_nop (profiles/r14_relax_kt_isa.txt).
            static_assert(!MAXF || (sizeof(T) == 4 && W == 4), "the vote is written for four 32-bit components");
            T signs = cv;
#pragma unroll
            for (int tt = 0; tt < NP; ++tt)
                asm("v_or3_b32 %0, %0, %1, %2\n\tv_or3_b32 %0, %0, %3, %4"
                    : "+v"(signs)
                    : "v"(L::get(p[tt], 0)), "v"(L::get(p[tt], 1)), "v"(L::get(p[tt], 2)), "v"(L::get(p[tt], 3)));
            if constexpr (RPB * NP > 64) {
#pragma unroll
                for (int i = 0; i < RPB * NP; i += 64) {
                    const T v = (&s_ct[0][0])[i + (int)__lane_id()];     // rows past r_cnt repeat the last row
                    asm("v_or_b32 %0, %1, %2" : "=v"(signs) : "v"(signs), "v"(v));
                }
            }
            const bool any = __builtin_amdgcn_ballot_w64(__builtin_signbit(signs)) != 0;
            max_form = !fold_compare && !any && r_cnt % UNROLL == 0;
        }
        auto rows = [&](auto vec, auto tl) {
            if (head) {
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) vec(x0[u], u, dg);
                r = UNROLL;
            }
            if constexpr (RPB > UNROLL) {
                for (; r + UNROLL <= r_cnt; r += UNROLL) {
                    V x[UNROLL];
#pragma unroll
                    for (int u = 0; u < UNROLL; ++u) x[u] = load_vec<V, NT>(at(base, r + u));
#pragma unroll
                    for (int u = 0; u < UNROLL; ++u) vec(x[u], r + u, dg);
                }
            }
            // The row-by-row tail (a ragged last chunk), in the compare form only; rare, and kept rolled: unrolled it
            // sets the kernel's register peak (profiles/r14_relax_kt_isa.txt).
            if constexpr (decltype(tl)::value)
#pragma unroll 1
                for (; __builtin_expect(r < r_cnt, 0); ++r) vec(load_vec<V, NT>(at(base, r)), r, dg);
        };
        // wave-uniform: one of the two, never both
        if constexpr (MAXF) {
            if (max_form) { rows(relax_vec_max, std::false_type()); return; }
        }
        rows(relax_vec, std::true_type());
    };
    // workgroup-uniform: one of the four instantiations, never two.  Only a tile whose rows meet its
    // columns holds diagonal elements (one strip in sixteen at N = 16384).
    const bool diag = r_begin < (strip + 1) * SW && r_begin + r_cnt > strip * SW;
    if (bid < nt_below) {
        if (diag) stream(std::true_type(), std::true_type());
        else stream(std::true_type(), std::false_type());
    } else {
        if (diag) stream(std::false_type(), std::true_type());
        else stream(std::false_type(), std::false_type());
    }

    if (COUNT) {
        if (__lane_id() == 0 && wave_updates) atomicAdd(&s_cnt, wave_updates);
        __syncthreads();
        if (t == 0 && s_cnt)
            atomicAdd(&updates[bid & (FWX_UPDATE_SHARDS_K - 1)], (unsigned long long)s_cnt);
    }
}

// -------------------------------------------------------------------------------------------------
// relax_walk (round 23): the 16-pivot sweep of the non-counting f32 solve, relax_kt<float, 4, ., ., false, GL, 16>
// word for word in what it computes -- operands from the snapshot panels only, the NaN patch at column k + t and in
// clamped lanes, the per-wave vote between the max form and the compare form, the diagonal never updates, the group
// store with exact write-back, visit_tile, strip_magic, `nt_below` -- in another shape:
//
// ONE body.  relax_kt is four copies of `stream` (cache policy x diagonal), and the compiler hoists the 16 loads of W
// in front of them and patches the NaNs into registers of each copy's own: 247 VGPRs, two waves per SIMD
// (profiles/r19_relax_kt16_isa.txt).  Here W is loaded and patched once, in place; the diagonal is a run-time term
// of the fold and the cache policy is chosen at the load.  160 VGPRs with 8 row slots, three waves per SIMD
// (profiles/r23_relax_walk_isa.txt).
// The diagonal term: a tile starts at a multiple of 4 rows and a lane at a multiple of 4 columns, so the component
// of row r on the diagonal is r % 4 in whichever lane holds it, and r % 4 is the slot's number % 4, a constant of the
// unrolled body: ONE component per row carries `&& d != c` (d: this lane's diagonal component of the row, -1 in a
// tile off the diagonal), one v_cmp_ne and one scalar AND per row.
//
// What ships is this body with relax_kt's geometry and row loop (16 rows per workgroup, 8 loaded together and folded
// together, twice; !ROLL) and default-policy loads everywhere (WALK_POL_PLAIN): 223.8 us per pass late in the solve
// at N = 16384 against relax_kt's 257.5 (profiles/r23_tune_relax_pivots.txt).  The other values of ROLL and POL are
// what was timed against it and lost (tools/tune_relax.hip `pivots`, profiles/r23_experiments_not_adopted.txt):
//
// The WALK (ROLL).  A workgroup owns RPB rows of its strip, RPB a multiple of UNROLL up to 64, and keeps W for all of
// them.  UNROLL row slots are in flight; a slot is reloaded with the row UNROLL further on right after its fold and
// its store, UNCONDITIONALLY, and the last batch is peeled without a reload.  In that shape, from RPB = 32 and with
// WALK_POL_PLAIN, the compiler's waits are exact: one s_waitcnt vmcnt(UNROLL - 1) per row in front of the row's
// compares, so UNROLL - 1 rows stay in flight under every fold.  A reload behind a uniform `if (more)` gets one
// vmcnt(0) per batch instead (the wait pass merges the path on which no later load was issued), which is what the
// compare form's loop below has: it is the rare form and keeps the simple loop.  The walk was slower than the batches
// in every window, the more rows the slower: the exposed wait was not what the pass was short of.
//
// The cache policy (POL), what `nt_below` means to the loads of r[i][j]:
//   WALK_POL_PLAIN  default-policy loads everywhere (the split of round 5 dropped)
//   WALK_POL_FENCE  one load, its policy chosen at run time; the non-temporal arm stands between two empty asm
//                   statements, without which the optimiser merges the two arms into one plain load.  Two
//                   conditional blocks per load, and one vmcnt(0) per batch in the walk
//   WALK_POL_LOOP   two copies of the steady loop alone, one per policy; the head loads as WALK_POL_FENCE.  Spills
// No result bit depends on it.
//
// Staging: thread t stages the cells t, t + 256, ... of the RPB x NP values of Ct, one writer per cell.  The race-
// freedom and write-back arguments are relax_kt's: every element belongs to exactly one lane of one workgroup.
//
// Round 25: NP = 32 with W = 2.  A lane owns 8 bytes of a row instead of 16, so 32 rows of W are the same 64 registers
// and the kernel stays at three waves; the strip is 512 columns, the diagonal component of row r is r % 2, a store
// group of G bytes is G / 8 lanes, a staged row of Ct is eight 16-byte reads.  Per row-vector the max form is the same
// 64 multiplies, 30 v_max3_f32, 2 v_max_f32 and 2 compares; the compare form is 32 steps of two chains, with the next
// step's multiplies between a step's compares and its selects (vec_cmp).  The matrix is streamed once per 32 pivots.
// What ships: 64 rows per workgroup, 8 slots, batches, plain loads (profiles/r25_tune_relax_pivots.txt,
// r25_relax_walk_isa.txt); the schedule: relax_range_kt, FWX_PERK_DEEP.
// -------------------------------------------------------------------------------------------------
enum { WALK_POL_PLAIN = 0, WALK_POL_FENCE = 1, WALK_POL_LOOP = 2 };

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): a loop whose index is a constant of each step
template <typename F, int... U> __device__ __forceinline__ void for_slots_seq(F &&f, std::integer_sequence<int, U...>)
{
    (f(std::integral_constant<int, U>()), ...);
}
template <int N, typename F> __device__ __forceinline__ void for_slots(F &&f)
{
    for_slots_seq(f, std::make_integer_sequence<int, N>());
}

template <int UNROLL> constexpr int relax_walk_min_waves() { return UNROLL <= 4 ? 4 : 3; }

template <int RPB, int UNROLL, int GL, int POL, bool ROLL, int NP = 16, int W = 4>
__global__ __launch_bounds__(256, (relax_walk_min_waves<UNROLL>()))
void relax_walk(float *rate, const float *w, const float *ct, int ct_ld, int n, int k, int nstrips, int flip,
                int nt_below, unsigned strip_magic, int fold_compare)
{
    constexpr int SW = 256 * W;
    constexpr int STAGE = (RPB * NP + 255) / 256;     // staged values per thread
    using L = Lanes<float, W>;
    using V = typename L::V;
    static_assert((NP == 16 && W == 4) || (NP == 32 && W == 2), "16 pivots on 16 bytes of a row or 32 on 8: 64 registers of W");
    static_assert(GL * W == 4 || GL * W == 8 || GL * W == 16 || GL * W == 32, "store group: 16, 32, 64 or 128 bytes");
    static_assert(UNROLL % 4 == 0 && RPB % UNROLL == 0 && RPB * NP % 256 == 0, "slots and rows");

    __shared__ __attribute__((aligned(16))) float s_ct[RPB][NP];

    const int t = threadIdx.x;
    const int bid = visit_tile(flip);
    int strip, chunk;                         // as relax_kt
    if (strip_magic) {
        chunk = (int)__umulhi((unsigned)bid, strip_magic);
        strip = bid - chunk * nstrips;
    } else {
        strip = bid % nstrips;
        chunk = bid / nstrips;
    }
    const int r_begin = chunk * RPB;
    const int r_cnt = min(RPB, n - r_begin);
    const int c0 = strip * SW + t * W;
    const bool own = c0 < n;                  // false: a clamped lane (never stores)
    const int col = own ? c0 : n - W;
    const unsigned boff = (unsigned)col * (unsigned)sizeof(float);
    auto at = [&](const float *q, int r) {
        const char *const row = reinterpret_cast<const char *>(q + (size_t)r * n);
        return const_cast<float *>(reinterpret_cast<const float *>(row + boff));
    };
    float *const base = rate + (size_t)r_begin * n;
    const int g0 = (int)(__lane_id() & ~(GL - 1));
    const bool nt = bid < nt_below;           // workgroup-uniform
    const bool diag = r_begin < (strip + 1) * SW && r_begin + r_cnt > strip * SW;
    const int d0 = diag ? r_begin - col : -1 - RPB;   // row r of the tile: my diagonal component is d0 + r if in [0, W)

    auto ld_nt = [&](const float *q) { return __builtin_nontemporal_load(reinterpret_cast<const V *>(q)); };
    auto ld_t = [&](const float *q) { return *reinterpret_cast<const V *>(q); };
    // the policy chosen at the load; the fences keep the two arms apart (header)
    auto ld = [&](const float *q) -> V {
        if constexpr (POL == WALK_POL_PLAIN) return ld_t(q);
        V v;
        if (nt) { asm volatile(""); v = ld_nt(q); asm volatile(""); }
        else v = ld_t(q);
        return v;
    };
    auto group_stores = [&](bool changed) {
        if constexpr (GL == 1) return changed;
        const unsigned long long m = __ballot(changed);
        return own && ((m >> g0) & ((1ull << GL) - 1)) != 0;
    };

    // Prologue: every load the first fold needs back to back (relax_kt's), then the NaN patch of W in place.
    float cv[STAGE];
#pragma unroll
    for (int i = 0; i < STAGE; ++i) {
        const int id = t + 256 * i;
        cv[i] = ct[(size_t)(id / RPB % NP) * ct_ld + r_begin + min(id % RPB, r_cnt - 1)];
    }
    V p[NP];
#pragma unroll
    for (int tt = 0; tt < NP; ++tt) p[tt] = *reinterpret_cast<const V *>(at(w, tt));
    const bool head = UNROLL <= r_cnt;        // workgroup-uniform
    V x[UNROLL];
    if (head) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) x[u] = ld(at(base, u));
    }
    // rows of a ragged chunk past the end of the matrix get the last row's values again; one writer per cell
#pragma unroll
    for (int i = 0; i < STAGE; ++i) {
        const int id = t + 256 * i;
        s_ct[id % RPB][id / RPB % NP] = cv[i];
    }
#pragma unroll
    for (int tt = 0; tt < NP; ++tt)
#pragma unroll
        for (int c = 0; c < W; ++c)
            L::set(p[tt], c, !own || col + c == k + tt ? quiet_nan<float>() : L::get(p[tt], c));
    __syncthreads();
    // The vote, per wave (relax_kt's): the max form iff no value of W in my lanes after the patch and no staged Ct
    // value of the tile has its sign bit set.  A ragged chunk keeps the compare form.
    float signs = 0.f;
#pragma unroll
    for (int tt = 0; tt < NP; ++tt) {
        if constexpr (W == 4)
            asm("v_or3_b32 %0, %0, %1, %2\n\tv_or3_b32 %0, %0, %3, %4"
                : "+v"(signs)
                : "v"(L::get(p[tt], 0)), "v"(L::get(p[tt], 1)), "v"(L::get(p[tt], 2)), "v"(L::get(p[tt], 3)));
        else
            asm("v_or3_b32 %0, %0, %1, %2" : "+v"(signs) : "v"(L::get(p[tt], 0)), "v"(L::get(p[tt], 1)));
    }
#pragma unroll
    for (int i = 0; i < RPB * NP; i += 64) {
        const float v = (&s_ct[0][0])[i + (int)__lane_id()];         // rows past r_cnt repeat the last row
        asm("v_or_b32 %0, %1, %2" : "=v"(signs) : "v"(signs), "v"(v));
    }
    const bool any = __builtin_amdgcn_ballot_w64(__builtin_signbit(signs)) != 0;
    const bool max_form = !fold_compare && !any && r_cnt % UNROLL == 0;

    // One row through the NP pivots, max form (relax_kt's relax_vec_max).  CD = r % W: the one component of the row
    // that can lie on the diagonal.
    auto vec_max = [&](const V &xv, int r, auto cd) {
        constexpr int CD = decltype(cd)::value;
        float cik[NP];
#pragma unroll
        for (int tt = 0; tt < NP; ++tt) cik[tt] = s_ct[r][tt];
        float m[W];
        bool up[W];
#pragma unroll
        for (int c = 0; c < W; ++c) {
            float cand[NP];
#pragma unroll
            for (int tt = 0; tt < NP; ++tt) cand[tt] = cik[tt] * L::get(p[tt], c);
            m[c] = max_of(cand);
        }
#pragma unroll
        for (int c = 0; c < W; ++c) {
            up[c] = L::get(xv, c) < m[c];
            if (c == CD) up[c] = up[c] && d0 + r != CD;
        }
        __builtin_amdgcn_sched_barrier(0);
        V nx;
        bool changed = false;
#pragma unroll
        for (int c = 0; c < W; ++c) {
            L::set(nx, c, up[c] ? m[c] : L::get(xv, c));
            changed = changed || up[c];
        }
        if (group_stores(changed)) *reinterpret_cast<V *>(at(base, r)) = nx;
    };
    // ... compare form (relax_kt's relax_vec with the diagonal as a run-time term).
    auto vec_cmp = [&](const V &xv, int r) {
        const int d = d0 + r;
        V nx;
#pragma unroll
        for (int c = 0; c < W; ++c) L::set(nx, c, c == d ? __builtin_huge_valf() : L::get(xv, c));
        float cik[NP];
#pragma unroll
        for (int tt = 0; tt < NP; ++tt) cik[tt] = s_ct[r][tt];
        if constexpr (W == 2) {
            // Two components are two compares: a select would follow the compare that feeds it at a distance of one
            // instruction and get a wait state.  The next step's two multiplies, which do not depend on this step,
            // stand between them instead.
            float cand[W];
#pragma unroll
            for (int c = 0; c < W; ++c) cand[c] = cik[0] * L::get(p[0], c);
#pragma unroll
            for (int tt = 0; tt < NP; ++tt) {
                float next[W];
                bool up[W];
#pragma unroll
                for (int c = 0; c < W; ++c) up[c] = L::get(nx, c) < cand[c];
                __builtin_amdgcn_sched_barrier(0);
                if (tt + 1 < NP) {
#pragma unroll
                    for (int c = 0; c < W; ++c) next[c] = cik[tt + 1] * L::get(p[tt + 1], c);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int c = 0; c < W; ++c) L::set(nx, c, up[c] ? cand[c] : L::get(nx, c));
                if (tt + 1 < NP) {
#pragma unroll
                    for (int c = 0; c < W; ++c) cand[c] = next[c];
                }
            }
        } else {
#pragma unroll
            for (int tt = 0; tt < NP; ++tt) {
                float cand[W];
                bool up[W];
#pragma unroll
                for (int c = 0; c < W; ++c) {
                    cand[c] = cik[tt] * L::get(p[tt], c);
                    up[c] = L::get(nx, c) < cand[c];
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int c = 0; c < W; ++c) L::set(nx, c, up[c] ? cand[c] : L::get(nx, c));
            }
        }
#pragma unroll
        for (int c = 0; c < W; ++c) L::set(nx, c, c == d ? L::get(xv, c) : L::get(nx, c));
        uint32_t diff = 0;
#pragma unroll
        for (int c = 0; c < W; ++c)
            diff |= __builtin_bit_cast(uint32_t, L::get(nx, c)) ^ __builtin_bit_cast(uint32_t, L::get(xv, c));
        if (group_stores(diff != 0)) *reinterpret_cast<V *>(at(base, r)) = nx;
    };

    if (max_form) {                           // wave-uniform; r_cnt is a multiple of UNROLL here, so `head` holds
        int rb = 0;
        if constexpr (ROLL) {
            // steady state: fold slot u (row rb + u), reload it with row rb + UNROLL + u, unconditionally
            auto steady = [&](auto load) {
#pragma unroll 1
                for (; rb + UNROLL < r_cnt; rb += UNROLL) {
                    for_slots<UNROLL>([&](auto uc) {
                        constexpr int u = decltype(uc)::value;
                        vec_max(x[u], rb + u, std::integral_constant<int, u % W>());
                        x[u] = load(at(base, rb + UNROLL + u));
                    });
                }
            };
            if constexpr (POL == WALK_POL_LOOP) {
                if (nt) steady(ld_nt); else steady(ld_t);
            } else {
                steady(ld);
            }
        } else {
#pragma unroll 1
            for (; rb + UNROLL < r_cnt; rb += UNROLL) {
                for_slots<UNROLL>([&](auto uc) {
                    constexpr int u = decltype(uc)::value;
                    vec_max(x[u], rb + u, std::integral_constant<int, u % W>());
                });
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) x[u] = ld(at(base, rb + UNROLL + u));
            }
        }
        // the last batch, peeled: no reload
        for_slots<UNROLL>([&](auto uc) {
            constexpr int u = decltype(uc)::value;
            vec_max(x[u], rb + u, std::integral_constant<int, u % W>());
        });
        return;
    }
    int r = 0;
    if (head) {
#pragma unroll 1
        for (int rb = 0; rb + UNROLL <= r_cnt; rb += UNROLL) {
            const bool more = rb + 2 * UNROLL <= r_cnt;
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                vec_cmp(x[u], rb + u);
                if (more) x[u] = ld(at(base, rb + UNROLL + u));
            }
            r = rb + UNROLL;
        }
    }
    // the row-by-row tail of a ragged last chunk, rolled
#pragma unroll 1
    for (; __builtin_expect(r < r_cnt, 0); ++r) vec_cmp(ld(at(base, r)), r);
}

// -------------------------------------------------------------------------------------------------
// Where the matrix of a small solve comes from and where it goes: the load stage and the store stage of
// small_solve_body and wave_solve_body, which hold the one pivot loop in between.
//   InPlaceIO  the matrix is solved where it lies (small_solve, the batch and the ragged kernels).  The register of
//              a diagonal entry holds +inf and its value in memory is left alone.
//   SweepIO    variant b of a what-if sweep (small_solve_sweep, wave_solve_sweep): the entries are the BASE's (const,
//              the same for every variant), then the variant's patches in list order; nothing goes back to the base.
//              The items of the variant are answered from the registers, the whole matrix goes to the full outputs
//              if there are any.  There is no memory left alone here, so the (patched) diagonal rate is kept aside
//              by the thread that owns it -- `dg` in the bodies -- and is what an item on (i, i) and a full output
//              receive.
// in_base / out_base: element offsets the wave body adds (its loads and stores keep one scalar base each); the
// workgroup body is handed pointers that include them and passes 0.
// The bodies know their layout: they hand patches() a `put` and items() a `get`, both an unrolled select over the
// thread's entries (no register array is indexed dynamically); the policy walks the tables, through wave-uniform
// addresses, and holds the defence against tables that do not belong to the arrays.
// -------------------------------------------------------------------------------------------------
template <typename T> struct InPlaceIO {
    static constexpr bool SWEEP = false;
    T *in_rate;
    int32_t *in_next, *in_hops;
    T *out_rate;
    int32_t *out_next, *out_hops;
    size_t in_base, out_base;
    __device__ __forceinline__ InPlaceIO(T *rate, int32_t *next, int32_t *hops, size_t base = 0)
        : in_rate(rate), in_next(next), in_hops(hops), out_rate(rate), out_next(next), out_hops(hops), in_base(base),
          out_base(base) {}
    __device__ __forceinline__ void put_rate(size_t off, T v, bool diag, T) const { if (!diag) out_rate[off] = v; }
    __device__ __forceinline__ void put_next(size_t off, int32_t v) const { out_next[off] = v; }
    __device__ __forceinline__ void put_hops(size_t off, int32_t v) const { out_hops[off] = v; }
};

__device__ __forceinline__ long long uniform64(long long v)
{
    return (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
                       (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)v));
}

template <typename T> struct SweepIO {
    static constexpr bool SWEEP = true;
    const T *in_rate;                          // the base, pitch n
    const int32_t *in_next, *in_hops;
    T *out_rate;                               // the full outputs of this variant, each optional
    int32_t *out_next, *out_hops;
    size_t in_base, out_base;
    int n;
    const int64_t *patch_index;                // this variant's patches: [p0, p1) of the patch arrays
    const T *patch_rate;
    const int32_t *patch_next, *patch_hops;    // optional
    long long p0, p1;
    const int32_t *item_src, *item_dst;        // this variant's items: [q0, q1) of the item arrays
    T *item_rate;
    int32_t *item_next, *item_hops;            // optional
    long long q0, q1;

    // [ptr[b], ptr[b + 1]) clamped into [0, total]; a descending pair and a null table are empty ranges
    __device__ __forceinline__ static void range(const int64_t *ptr, long long b, long long total, long long &lo,
                                                 long long &hi)
    {
        lo = hi = 0;
        if (!ptr || total <= 0) return;
        long long a = uniform64(ptr[b]), e = uniform64(ptr[b + 1]);
        a = a < 0 ? 0 : a;
        e = e > total ? total : e;
        lo = a;
        hi = e < a ? a : e;
    }
    // put(cell, rate, has_next, next, has_hops, hops) for every patch in list order; an index outside [0, n * n) is
    // ignored
    template <typename Put> __device__ __forceinline__ void patches(Put &&put) const
    {
        const long long cells = (long long)n * n;
#pragma unroll 1
        for (long long q = p0; q < p1; ++q) {
            const long long idx = uniform64(patch_index[q]);
            if (idx < 0 || idx >= cells) continue;
            int32_t pn = -1, ph = 0;
            if (patch_next) pn = patch_next[q];
            if (patch_hops) ph = patch_hops[q];
            put((int)idx, patch_rate[q], patch_next != nullptr, pn, patch_hops != nullptr, ph);
        }
    }
    // get(src, dst, rate, next, hops) -> "this thread holds the entry"; it writes the item's outputs.  An item whose
    // src or dst is outside [0, n) leaves them untouched.
    template <typename Get> __device__ __forceinline__ void items(Get &&get) const
    {
#pragma unroll 1
        for (long long q = q0; q < q1; ++q) {
            const int s = __builtin_amdgcn_readfirstlane(item_src[q]), d = __builtin_amdgcn_readfirstlane(item_dst[q]);
            if ((unsigned)s >= (unsigned)n || (unsigned)d >= (unsigned)n) continue;
            T v;
            int32_t nv = -1, hv = 0;
            if (get(s, d, v, nv, hv)) {
                item_rate[q] = v;
                if (item_next) item_next[q] = nv;
                if (item_hops) item_hops[q] = hv;
            }
        }
    }
    __device__ __forceinline__ void put_rate(size_t off, T v, bool diag, T dg) const
    {
        if (out_rate) out_rate[off] = diag ? dg : v;
    }
    __device__ __forceinline__ void put_next(size_t off, int32_t v) const { if (out_next) out_next[off] = v; }
    __device__ __forceinline__ void put_hops(size_t off, int32_t v) const { if (out_hops) out_hops[off] = v; }
};

// -------------------------------------------------------------------------------------------------
// small_solve: the whole of runAlgo for n <= 128 in ONE launch of one workgroup -- the reference's
// own regime (its tests stop at 4 x 4, src/test/AlgorithmsTest.hs:66-77; the README session has 4
// vertices; a market of 10 exchanges x 12 currencies has 120).  The matrix is padded with NaN to
// M x M (M = 64 or 128) and lives in REGISTERS for the entire solve (1024 threads; the 128-wide
// tile keeps its index matrices in LDS): thread (r0, c) holds column c of the rows r0, r0+RG, ...  Only pivot row k and pivot column k pass through LDS, double
// buffered: during step k the threads that own entries of row k+1 / column k+1 publish their
// post-step values (= the time-(k+1) operands) into the other buffer, so one barrier per pivot is
// enough.  Row k and column k are fixed points of step k, so what step k reads are exactly the
// step-start operands (Algorithms.hs:58-60).
//
// The body is shared by the kernels small_solve (one matrix, one workgroup), small_solve_batch (the workgroup tier
// of the batched solve: workgroup b solves matrix b of a batch), small_solve_ragged and small_solve_sweep (workgroup
// b solves variant b of one base matrix); `io` (InPlaceIO or SweepIO, above) is its load and its store stage.
// -------------------------------------------------------------------------------------------------
template <typename T, int M, int RG, bool HAS_NEXT, bool HAS_HOPS, bool LOG, typename IO>
__device__ __forceinline__ void small_solve_body(const IO &io, int n, int k_begin, int k_end,
                                                 unsigned long long *updates, PathLog plog)
{
    constexpr int E = M / RG;                 // entries per thread; rows r = r0 + RG*m
    constexpr int G = 4;                      // entries per branch-free group
    constexpr int LOG_M = M == 64 ? 6 : 7;
    // Where next / hops live.  64-wide tile: in registers like the rates (4 entries per thread).
    // 128-wide tile: 16 entries per thread and 128 registers each, so the two index matrices
    // stay in LDS (2 x 66 KB of the CU's 160 KB) and only the rates are in registers; row k and
    // column k of an LDS-resident matrix are read in place (they are not written during step k).
    constexpr bool IDXL = M == 128;
    constexpr bool NXL = IDXL && HAS_NEXT, HPL = IDXL && HAS_HOPS;
    static_assert(M == 64 || M == 128, "M");
    static_assert(E % G == 0, "E");
    __shared__ T rowR[2][M], colR[2][M];      // pivot row k / pivot column k at time k
    __shared__ int32_t rowH[2][HAS_HOPS && !IDXL ? M : 1], colH[2][HAS_HOPS && !IDXL ? M : 1];
    __shared__ int32_t colN[2][HAS_NEXT && !IDXL ? M : 1], rowN[2][HAS_NEXT && !IDXL ? M : 1];
    __shared__ int32_t NX[NXL ? M : 1][NXL ? M + 1 : 1], HP[HPL ? M : 1][HPL ? M + 1 : 1];
    __shared__ unsigned int s_cnt;
    const int tid = threadIdx.x;
    // a wave never straddles two rows: r0 is wave-uniform, say so (scalar row tests, fewer VGPRs)
    const int c = tid & (M - 1), r0 = __builtin_amdgcn_readfirstlane(tid >> LOG_M);
    if (tid == 0) s_cnt = 0;
    const int off0 = r0 * n + c, off_step = RG * n;   // entry (r0 + RG*m, c) is at off0 + m*off_step
    // LOG: the path trace (see PathLog).  hd[m] = pivot of the newest update of this thread's m-th
    // entry; its snapshots for step k are stored by the owners of row k / column k when they
    // publish their operands, the final values at the end.

    T x[E];
    int32_t nx[HAS_NEXT && !IDXL ? E : 1], hp[HAS_HOPS && !IDXL ? E : 1], hd[LOG ? E : 1];
    [[maybe_unused]] T dg = quiet_nan<T>();   // sweep: my diagonal entry's rate (a thread owns at most one)
    auto publish = [&](int k, int b) {        // my entries of row k / column k -> buffer b
#pragma unroll
        for (int m = 0; m < E; ++m) {
            if (r0 + RG * m == k) {           // scalar
                rowR[b][c] = x[m];
                if constexpr (HAS_NEXT && !IDXL) rowN[b][c] = nx[m];
                if constexpr (HAS_HOPS && !IDXL) rowH[b][c] = hp[m];
                if constexpr (LOG) { if (c < n) plog.at_row[(size_t)k * n + c] = hd[m]; }
            }
        }
        if (c == k) {                         // one lane of the wave that holds column k
#pragma unroll
            for (int m = 0; m < E; ++m) {
                const int r = r0 + RG * m;
                colR[b][r] = r == k ? quiet_nan<T>() : x[m];   // skip i == k: NaN at the source
                if constexpr (HAS_NEXT && !IDXL) colN[b][r] = nx[m];
                if constexpr (HAS_HOPS && !IDXL) colH[b][r] = hp[m];
                if constexpr (LOG) { if (r < n) plog.at_col[(size_t)r * n + k] = hd[m]; }
            }
        }
    };
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int r = r0 + RG * m;
        const bool in = r < n && c < n;
        x[m] = in ? io.in_rate[off0 + m * off_step] : quiet_nan<T>();
        if constexpr (IO::SWEEP) { if (r == c) dg = x[m]; }
        // skip j == i: a diagonal entry is never an operand (it could only be one in the steps
        // that skip it) and never a target, so its register holds +inf -- no candidate compares
        // greater -- and the value in memory is left as it is
        if (r == c) x[m] = (T)__builtin_huge_val();
        if constexpr (HAS_NEXT) {
            const int32_t v = in ? io.in_next[off0 + m * off_step] : -1;
            if constexpr (IDXL) NX[r][c] = v; else nx[m] = v;
        }
        if constexpr (HAS_HOPS) {
            const int32_t v = in ? io.in_hops[off0 + m * off_step] : 0;
            if constexpr (IDXL) HP[r][c] = v; else hp[m] = v;
        }
        if constexpr (LOG) hd[m] = -1;
    }
    if constexpr (IO::SWEEP) {
        // the variant's patches: the thread that owns the cell takes the value (a diagonal rate goes aside, its
        // register stays +inf); NX / HP are written by their owner before the first barrier
        io.patches([&](int cell, T v, bool hn, int32_t pn, bool hh, int32_t ph) {
#pragma unroll
            for (int m = 0; m < E; ++m) {
                const int r = r0 + RG * m;
                const bool hit = r < n && c < n && cell == off0 + m * off_step;
                dg = hit && r == c ? v : dg;
                x[m] = hit && r != c ? v : x[m];
                if constexpr (NXL) { if (hit && hn) NX[r][c] = pn; }
                else if constexpr (HAS_NEXT) nx[m] = hit && hn ? pn : nx[m];
                if constexpr (HPL) { if (hit && hh) HP[r][c] = ph; }
                else if constexpr (HAS_HOPS) hp[m] = hit && hh ? ph : hp[m];
            }
        });
    }
    publish(k_begin, k_begin & 1);
    __syncthreads();

    unsigned int mine = 0;
    for (int k = k_begin; k < k_end; ++k) {
        const int b = k & 1;
        T rkc = rowR[b][c];
        int32_t hkc = 0, nkc = -1;
        if constexpr (HPL) hkc = HP[k][c];
        else if constexpr (HAS_HOPS) hkc = rowH[b][c];
        // head kjPath, for the (off-domain) case of an update whose ikPath is empty
        if constexpr (NXL) nkc = NX[k][c];
        else if constexpr (HAS_NEXT) nkc = rowN[b][c];
        if (c == k) rkc = quiet_nan<T>();                     // skip j == k
#pragma unroll
        for (int g = 0; g < E; g += G) {
            if (r0 + RG * g >= n) break;                      // scalar: nothing but padding rows left
            // G entries: the pivot-column operands are read unconditionally (so the LDS reads of
            // the group overlap) and the update is a select / predicated store, exactly
            //   if (x < cand) { x = cand; next = next[i][k]; hops = hops[i][k] + hops[k][j]; }
#pragma unroll
            for (int m = g; m < g + G; ++m) {
                const int r = r0 + RG * m;
                const T raw = colR[b][r];                     // wave-uniform address: LDS broadcast
                int32_t cn = 0, ch = 0;
                if constexpr (NXL) cn = NX[r][k]; else if constexpr (HAS_NEXT) cn = colN[b][r];
                if constexpr (HAS_NEXT) {
                    // head (ikPath ++ kjPath): next[i][k] unless ikPath is empty (Algorithms.hs:55).
                    // r is wave-uniform, so this is a scalar test and a rarely taken move.
                    if (__builtin_amdgcn_readfirstlane(cn) < 0) cn = nkc;
                }
                if constexpr (HPL) ch = HP[r][k]; else if constexpr (HAS_HOPS) ch = colH[b][r];
                const T cand = raw * rkc;                     // Algorithms.hs:61
                const bool p = x[m] < cand;                   // :55 (false on NaN)
                x[m] = p ? cand : x[m];
                if constexpr (!IDXL) {
                    if constexpr (HAS_NEXT) nx[m] = p ? cn : nx[m];
                    if constexpr (HAS_HOPS) hp[m] = p ? ch + hkc : hp[m];
                } else if (p) {
                    if constexpr (HAS_NEXT) NX[r][c] = cn;
                    if constexpr (HAS_HOPS) HP[r][c] = ch + hkc;
                }
                mine += (unsigned int)__builtin_popcountll(__ballot(p));   // scalar; wave total
                if constexpr (LOG) hd[m] = p ? k : hd[m];
            }
        }
        if (k + 1 < k_end) publish(k + 1, b ^ 1);
        __syncthreads();
    }
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int r = r0 + RG * m;
        if (r < n && c < n) {
            io.put_rate(off0 + m * off_step, x[m], r == c, dg);
            if constexpr (NXL) io.put_next(off0 + m * off_step, NX[r][c]);
            else if constexpr (HAS_NEXT) io.put_next(off0 + m * off_step, nx[m]);
            if constexpr (HPL) io.put_hops(off0 + m * off_step, HP[r][c]);
            else if constexpr (HAS_HOPS) io.put_hops(off0 + m * off_step, hp[m]);
            if constexpr (LOG) plog.last[off0 + m * off_step] = hd[m];
        }
    }
    if constexpr (IO::SWEEP) {
        // the variant's items: entry (s, d) is register s / RG of the thread (s % RG, d)
        io.items([&](int s, int d, T &v, int32_t &nv, int32_t &hv) -> bool {
            const int ms = s / RG;
            const bool own = c == d && r0 == (s & (RG - 1));
            T xv = dg;                        // s == d: the diagonal entry of the thread that holds it
            // the index is a constant of each step from the start: a rolled `m == ms ? x[m] : xv` comes back
            // from the optimiser as x[ms], and the array with it as LDS or scratch
            for_slots<E>([&](auto mc) {
                constexpr int m = decltype(mc)::value;
                const bool at = m == ms;      // scalar
                xv = at && s != d ? x[m] : xv;
                if constexpr (HAS_NEXT && !IDXL) nv = at ? nx[m] : nv;
                if constexpr (HAS_HOPS && !IDXL) hv = at ? hp[m] : hv;
            });
            v = xv;
            if constexpr (NXL) { if (own) nv = NX[s][d]; }
            if constexpr (HPL) { if (own) hv = HP[s][d]; }
            return own;
        });
    }
    if (updates) {
        if (mine && (tid & 63) == 0) atomicAdd(&s_cnt, mine);   // `mine` is a wave total
        __syncthreads();
        if (tid == 0 && s_cnt) atomicAdd(&updates[0], (unsigned long long)s_cnt);
    }
}

template <typename T, int M, int RG, bool HAS_NEXT, bool HAS_HOPS, bool LOG>
__global__ __launch_bounds__(M * RG) void small_solve(T *rate, int32_t *next, int32_t *hops, int n,
                                                      int k_begin, int k_end,
                                                      unsigned long long *updates, PathLog plog)
{
    small_solve_body<T, M, RG, HAS_NEXT, HAS_HOPS, LOG>(InPlaceIO<T>(rate, next, hops), n, k_begin, k_end, updates, plog);
}

// -------------------------------------------------------------------------------------------------
// Batched small solves: `count` independent matrices of one order n <= 128 in one launch, matrix b at
// rate + b*stride (next / hops alike), U of matrix b added to updates[b].  LOG: the path trace of matrix b
// (PathLog) goes to plog's three arrays at + b*stride, pitch n like next; whole pivot range only (the launcher
// sees to that), every cell of the n x n part written, the gap never.
//
// Workgroup tier (any n <= 128): small_solve's body, workgroup b on matrix b.
// -------------------------------------------------------------------------------------------------
template <typename T, int M, int RG, bool HAS_NEXT, bool HAS_HOPS, bool LOG>
__global__ __launch_bounds__(M * RG) void small_solve_batch(T *rate, int32_t *next, int32_t *hops, int n,
                                                            long long stride, int k_begin, int k_end,
                                                            unsigned long long *updates, PathLog plog)
{
    const size_t off = (size_t)blockIdx.x * (size_t)stride;
    if constexpr (LOG) { plog.last += off; plog.at_col += off; plog.at_row += off; }
    small_solve_body<T, M, RG, HAS_NEXT, HAS_HOPS, LOG>(InPlaceIO<T>(rate + off, HAS_NEXT ? next + off : nullptr,
                                                                     HAS_HOPS ? hops + off : nullptr),
                                                        n, k_begin, k_end, updates ? updates + blockIdx.x : nullptr,
                                                        plog);
}

// -------------------------------------------------------------------------------------------------
// Wave tier (n <= 16): one WAVE per matrix, four matrices per 256-thread workgroup; no LDS, no barrier.
// The matrix is a NaN-padded 16 x 16 tile in registers: lane l holds column c = l & 15 of the rows
// q + 4m (q = l >> 4, m = 0..3), next and hops alike.  Row k = 4*mk + kq is register mk of the 16 lanes
// with q == kq; column k is lane (q*16 + k) of every row group.  Step k reads its operands -- r[k][c],
// next[k][c], hops[k][c] from lane kq*16 + c, and r[i][k], next[i][k], hops[i][k] from lane (l & 48) | k
// for each of the lane's rows -- with cross-lane reads (ds_bpermute_b32: the sources differ per lane),
// ALL of them before any register of the step is updated, so every operand is the step-start value
// (Algorithms.hs:58-60).  The pivot loop is fully unrolled: which register holds row k is then a
// compile-time fact and no register array is indexed dynamically (no scratch).  Skips as everywhere:
// NaN in place of r[k][k]-column / row operands (i == k, j == k), +inf in the register of a diagonal
// entry (never a target; never an operand, because the only steps that would read it skip it), whose
// value in memory is left alone.  Row groups and pivots that are padding only are skipped by
// wave-uniform tests.  A wave past `count` leaves at once: there is no barrier it could be missed at.
//
// LOG (the path trace, see PathLog): hd[m] = pivot of the newest update of the lane's m-th entry, -1 = none,
// selected beside x / nx / hp.  The snapshots of step k are two stores: the 16 lanes that hold row k store
// hd[mk] to at_row[k][c], the four lanes that hold column k store hd[m] to at_col[r][k] for their rows.  Row k
// and column k are fixed points of step k (their row / column operand is NaN), so hd of these entries does not
// change inside the step and "the start of step k" is anywhere in it: the stores are issued at the top,
// before the cross-lane reads, and drain behind them.  `last` is stored with the results.
//
// The body is shared by three kernels: wave_solve_batch (wave b on matrix b, at b*stride), wave_solve_ragged (the
// wave tier of the ragged batch: its own order and offset per wave) and wave_solve_sweep (wave b on variant b of one
// base matrix).  n is wave-uniform in all; `io` (InPlaceIO or SweepIO) is the load and the store stage: the matrix
// is read at + io.in_base and written at + io.out_base, the trace at + io.out_base; its U goes to updates[b].
// -------------------------------------------------------------------------------------------------
template <typename T, bool HAS_NEXT, bool HAS_HOPS, bool LOG, typename IO>
__device__ __forceinline__ void wave_solve_body(const IO &io, int n, long long b, int k_begin, int k_end,
                                                unsigned long long *updates, PathLog plog)
{
    constexpr int E = 4;                      // rows per lane: q, q + 4, q + 8, q + 12
    const int lane = threadIdx.x & 63;
    const int c = lane & 15, q = lane >> 4;

    T x[E];
    int32_t nx[E], hp[E], hd[LOG ? E : 1];
    [[maybe_unused]] T dg = quiet_nan<T>();   // sweep: my diagonal entry's rate (a lane owns at most one)
    if constexpr (LOG) { plog.last += io.out_base; plog.at_col += io.out_base; plog.at_row += io.out_base; }
    const int qn = q * n;
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int r = q + 4 * m;
        const bool in = r < n && c < n;
        const size_t off = io.in_base + (size_t)(r * n + c);
        if constexpr (LOG) hd[m] = -1;
        x[m] = in ? io.in_rate[off] : quiet_nan<T>();
        if constexpr (IO::SWEEP) { if (r == c) dg = x[m]; }
        if (r == c) x[m] = (T)__builtin_huge_val();           // skip j == i (see small_solve)
        nx[m] = -1;
        hp[m] = 0;
        if constexpr (HAS_NEXT) { if (in) nx[m] = io.in_next[off]; }
        if constexpr (HAS_HOPS) { if (in) hp[m] = io.in_hops[off]; }
    }
    if constexpr (IO::SWEEP) {                // the variant's patches (see small_solve_body)
        io.patches([&](int cell, T v, bool hn, int32_t pn, bool hh, int32_t ph) {
#pragma unroll
            for (int m = 0; m < E; ++m) {
                const int r = q + 4 * m;
                const bool hit = r < n && c < n && cell == r * n + c;
                dg = hit && r == c ? v : dg;
                x[m] = hit && r != c ? v : x[m];
                if constexpr (HAS_NEXT) nx[m] = hit && hn ? pn : nx[m];
                if constexpr (HAS_HOPS) hp[m] = hit && hh ? ph : hp[m];
            }
        });
    }

    unsigned int mine = 0;
#pragma unroll
    for (int mk = 0; mk < E; ++mk) {
#pragma unroll
        for (int kq = 0; kq < 4; ++kq) {
            const int k = 4 * mk + kq;
            if (k < k_begin || k >= k_end) continue;          // scalar (k_end <= n)
            if constexpr (LOG) {                              // the snapshots of step k (k < n)
                // scalar bases, one vector offset each (c, q * n): no address lives across steps
                if (q == kq && c < n) (plog.at_row + k * n)[c] = hd[mk];
                if (c == k) {
#pragma unroll
                    for (int m = 0; m < E; ++m)
                        if (q + 4 * m < n) (plog.at_col + (4 * m * n + k))[qn] = hd[m];
                }
            }
            // every operand of step k, before any register changes
            const int rsrc = kq * 16 + c;
            T rkc = __shfl(x[mk], rsrc, 64);
            int32_t nkc = -1, hkc = 0;
            if constexpr (HAS_NEXT) nkc = __shfl(nx[mk], rsrc, 64);
            if constexpr (HAS_HOPS) hkc = __shfl(hp[mk], rsrc, 64);
            if (c == k) rkc = quiet_nan<T>();                 // skip j == k
            const int csrc = (lane & 48) | k;
            T cr[E];
            int32_t cn[E], ch[E];
#pragma unroll
            for (int m = 0; m < E; ++m) {
                cr[m] = quiet_nan<T>();
                cn[m] = -1;
                ch[m] = 0;
                if (4 * m >= n) continue;                     // scalar: padding rows only
                cr[m] = __shfl(x[m], csrc, 64);
                if (q + 4 * m == k) cr[m] = quiet_nan<T>();   // skip i == k
                if constexpr (HAS_NEXT) cn[m] = __shfl(nx[m], csrc, 64);
                if constexpr (HAS_HOPS) ch[m] = __shfl(hp[m], csrc, 64);
            }
#pragma unroll
            for (int m = 0; m < E; ++m) {
                if (4 * m >= n) continue;
                const T cand = cr[m] * rkc;                   // Algorithms.hs:61
                const bool p = x[m] < cand;                   // :55 (false on NaN)
                x[m] = p ? cand : x[m];
                // head (ikPath ++ kjPath): next[i][k] unless ikPath is empty, then next[k][j]
                if constexpr (HAS_NEXT) nx[m] = p ? (cn[m] < 0 ? nkc : cn[m]) : nx[m];
                if constexpr (HAS_HOPS) hp[m] = p ? ch[m] + hkc : hp[m];
                if constexpr (LOG) hd[m] = p ? k : hd[m];
                mine += (unsigned int)__builtin_popcountll(__ballot(p));   // scalar; wave total
            }
        }
    }

#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int r = q + 4 * m;
        if (r < n && c < n) {
            const size_t off = io.out_base + (size_t)(r * n + c);
            io.put_rate(off, x[m], r == c, dg);
            if constexpr (HAS_NEXT) io.put_next(off, nx[m]);
            if constexpr (HAS_HOPS) io.put_hops(off, hp[m]);
            if constexpr (LOG) (plog.last + 4 * m * n)[qn + c] = hd[m];
        }
    }
    if constexpr (IO::SWEEP) {                // the variant's items: entry (s, d) is register s / 4 of lane (s % 4, d)
        io.items([&](int s, int d, T &v, int32_t &nv, int32_t &hv) -> bool {
            const int ms = s >> 2;
            T xv = dg;
            for_slots<E>([&](auto mc) {       // constant indices from the start, as in small_solve_body
                constexpr int m = decltype(mc)::value;
                const bool at = m == ms;      // scalar
                xv = at && s != d ? x[m] : xv;
                if constexpr (HAS_NEXT) nv = at ? nx[m] : nv;
                if constexpr (HAS_HOPS) hv = at ? hp[m] : hv;
            });
            v = xv;
            return lane == ((s & 3) << 4 | d);
        });
    }
    if (updates && mine && lane == 0) atomicAdd(&updates[b], (unsigned long long)mine);
}

template <typename T, bool HAS_NEXT, bool HAS_HOPS, bool LOG>
__global__ __launch_bounds__(256) void wave_solve_batch(T *rate, int32_t *next, int32_t *hops, int n,
                                                        long long stride, int count, int k_begin,
                                                        int k_end, unsigned long long *updates, PathLog plog)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const long long b = (long long)blockIdx.x * 4 + wave;
    if (b >= count) return;                   // wave-uniform
    wave_solve_body<T, HAS_NEXT, HAS_HOPS, LOG>(InPlaceIO<T>(rate, next, hops, (size_t)b * (size_t)stride), n, b, k_begin,
                                                k_end, updates, plog);
}

// -------------------------------------------------------------------------------------------------
// Ragged batch: matrices of DIFFERENT orders in one call.  Matrix id has order n_each[id] and starts at element
// offset[id] of rate (next, hops and the three trace arrays alike), pitch n_each[id]; U of matrix id is added to
// updates[id].  `order` lists the matrices of ONE tier (fwx_ragged_plan groups them; the launcher passes the tier's
// part of the list): launch item w takes matrix order[w].  Whole pivot range only.  Order and offset are read
// through wave-uniform addresses (scalar loads), so n stays a scalar in both bodies: every row / pivot skip is
// still a scalar test.  An id outside [0, count) or an order that does not fit the tier's tile (a plan that does not
// belong to these arrays) makes the workgroup / wave leave before it touches memory or reaches a barrier.
// -------------------------------------------------------------------------------------------------
template <typename T, int M, int RG, bool HAS_NEXT, bool HAS_HOPS, bool LOG>
__global__ __launch_bounds__(M * RG) void small_solve_ragged(T *rate, int32_t *next, int32_t *hops, int count,
                                                             const int32_t *n_each, const int64_t *offset,
                                                             const int32_t *order, unsigned long long *updates,
                                                             PathLog plog)
{
    const int id = order[blockIdx.x];
    if ((unsigned)id >= (unsigned)count) return;              // workgroup-uniform, before any barrier
    const int n = n_each[id];
    if (n <= 0 || n > M) return;
    const size_t off = (size_t)offset[id];
    if constexpr (LOG) { plog.last += off; plog.at_col += off; plog.at_row += off; }
    small_solve_body<T, M, RG, HAS_NEXT, HAS_HOPS, LOG>(InPlaceIO<T>(rate + off, HAS_NEXT ? next + off : nullptr,
                                                                     HAS_HOPS ? hops + off : nullptr),
                                                        n, 0, n, updates ? updates + id : nullptr, plog);
}

// Wave tier: wave w of the launch (four per workgroup) on matrix order[w]; a wave past tier_count leaves at once.
template <typename T, bool HAS_NEXT, bool HAS_HOPS, bool LOG>
__global__ __launch_bounds__(256) void wave_solve_ragged(T *rate, int32_t *next, int32_t *hops, int count,
                                                         const int32_t *n_each, const int64_t *offset,
                                                         const int32_t *order, int tier_count,
                                                         unsigned long long *updates, PathLog plog)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const long long w = (long long)blockIdx.x * 4 + wave;
    if (w >= tier_count) return;              // wave-uniform
    const int id = __builtin_amdgcn_readfirstlane(order[w]);
    if ((unsigned)id >= (unsigned)count) return;
    const int n = __builtin_amdgcn_readfirstlane(n_each[id]);
    if (n <= 0 || n > FWX_BATCH_WAVE_N) return;
    const int64_t off = offset[id];            // wave-uniform too: the base of every load and store of the body
    const size_t base =((size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(off >> 32)) << 32) |
                        (size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)off);
    wave_solve_body<T, HAS_NEXT, HAS_HOPS, LOG>(InPlaceIO<T>(rate, next, hops, base), n, (long long)id, 0, n, updates, plog);
}

template <typename T>
hipError_t launch_batch_solve(T *rate, int32_t *next, int32_t *hops, int count, int n, long long stride,
                              int k_begin, int k_end, unsigned long long *updates_each, int wave_max_n,
                              hipStream_t s, PathLog plog)
{
    if (count <= 0 || n <= 0 || k_end <= k_begin) return hipSuccess;
    if (n > FWX_SMALL_N || (hops && !next) || k_begin < 0 || k_end > n || stride < (long long)n * n)
        return hipErrorInvalidValue;
    const bool lg = plog.last != nullptr;
    if (lg && (!next || !plog.at_col || !plog.at_row || k_begin != 0 || k_end != n)) return hipErrorInvalidValue;
    const bool wave = n <= wave_max_n && n <= FWX_BATCH_WAVE_N;
    // One launch; a launch is limited to 2^32 - 1 threads, so a batch of more than kChunk matrices
    // (2^21 workgroups of 1024 threads) takes one launch per kChunk.
    constexpr int kChunk = 1 << 21;
    for (long long b0 = 0; b0 < count; b0 += kChunk) {
        const int cnt = (int)std::min<long long>(kChunk, count - b0);
        const size_t off = (size_t)b0 * (size_t)stride;
        T *r = rate + off;
        int32_t *nx = next ? next + off : nullptr, *hp = hops ? hops + off : nullptr;
        unsigned long long *u = updates_each ? updates_each + b0 : nullptr;
        PathLog pl;
        if (lg) { pl.last = plog.last + off; pl.at_col = plog.at_col + off; pl.at_row = plog.at_row + off; }
#define FWX_BATCH_WAVE(HN, HH, LG)                                                                 \
    hipLaunchKernelGGL((wave_solve_batch<T, HN, HH, LG>), dim3((cnt + 3) / 4), dim3(256), 0, s, r, nx, hp, n, \
                       stride, cnt, k_begin, k_end, u, pl)
#define FWX_BATCH_WG(M, RG, HN, HH, LG)                                                            \
    hipLaunchKernelGGL((small_solve_batch<T, M, RG, HN, HH, LG>), dim3(cnt), dim3(M * RG), 0, s, r, nx, hp, n, \
                       stride, k_begin, k_end, u, pl)
#define FWX_BATCH_FIELDS(LAUNCH, ...)                                                              \
    do {                                                                                           \
        if (hops) { if (lg) LAUNCH(__VA_ARGS__ true, true, true); else LAUNCH(__VA_ARGS__ true, true, false); }   \
        else if (next) { if (lg) LAUNCH(__VA_ARGS__ true, false, true); else LAUNCH(__VA_ARGS__ true, false, false); } \
        else LAUNCH(__VA_ARGS__ false, false, false);                                              \
    } while (0)
        if (wave) FWX_BATCH_FIELDS(FWX_BATCH_WAVE);
        else if (n <= 64) FWX_BATCH_FIELDS(FWX_BATCH_WG, 64, 16,);
        else FWX_BATCH_FIELDS(FWX_BATCH_WG, 128, 8,);
#undef FWX_BATCH_FIELDS
#undef FWX_BATCH_WG
#undef FWX_BATCH_WAVE
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template hipError_t launch_batch_solve<float>(float *, int32_t *, int32_t *, int, int, long long, int, int,
                                              unsigned long long *, int, hipStream_t, PathLog);
template hipError_t launch_batch_solve<double>(double *, int32_t *, int32_t *, int, int, long long, int, int,
                                               unsigned long long *, int, hipStream_t, PathLog);

// -------------------------------------------------------------------------------------------------
// What-if sweeps: `count` variants of ONE base matrix of order n <= 128 in one launch.  Variant b is the base (pitch
// n, const, the same for every variant) with the patches [patch_ptr[b], patch_ptr[b+1]) applied in list order: patch
// q puts patch_rate[q] -- and patch_next[q] / patch_hops[q] where those arrays are given -- at cell patch_index[q] =
// i*n + j; a later patch of a cell wins.  The solved variant answers its items [item_ptr[b], item_ptr[b+1]): entry
// (item_src[q], item_dst[q]) goes to out.item_rate[q] (item_next, item_hops alike, optional), and, where a full
// output is given, its whole n x n part goes there at + b*stride, diagonal included, the gap never.  U of variant b
// is added to out.updates[b].  Whole pivot range, no trace.
//
// The kernels are the batch kernels with SweepIO in place of InPlaceIO: small_solve_sweep is workgroup b on variant b,
// wave_solve_sweep wave b (four per workgroup; a wave past `count` leaves at once).  The tables are read through
// wave-uniform addresses; their pointers are __restrict__ so that the item loads, which follow stores, stay scalar.
// The device form cannot see the tables: each [ptr[b], ptr[b+1]) is clamped into [0, total] (a descending pair is
// empty), a patch index outside [0, n*n) is ignored and an item whose src or dst is outside [0, n) leaves its
// outputs alone, so nothing outside the arrays' stated extents is read or written whatever the tables hold.
// -------------------------------------------------------------------------------------------------
template <typename T> struct SweepOut {
    T *item_rate;
    int32_t *item_next, *item_hops;
    T *full_rate;
    int32_t *full_next, *full_hops;
    long long stride;
    unsigned long long *updates;
};

#define FWX_SWEEP_PARAMS                                                                                           \
    const T *__restrict__ base_rate, const int32_t *__restrict__ base_next, const int32_t *__restrict__ base_hops, \
        int n, int count, const int64_t *__restrict__ patch_ptr, long long patch_total,                            \
        const int64_t *__restrict__ patch_index, const T *__restrict__ patch_rate,                                 \
        const int32_t *__restrict__ patch_next, const int32_t *__restrict__ patch_hops,                            \
        const int64_t *__restrict__ item_ptr, long long item_total, const int32_t *__restrict__ item_src,          \
        const int32_t *__restrict__ item_dst, SweepOut<T> out

// Variant b's policy; full_off: what the body does not add to the full outputs itself.
#define FWX_SWEEP_IO(io, b, full_off, body_off)                                                                    \
    SweepIO<T> io;                                                                                                 \
    io.in_rate = base_rate; io.in_next = base_next; io.in_hops = base_hops;                                        \
    io.out_rate = out.full_rate ? out.full_rate + (full_off) : nullptr;                                            \
    io.out_next = out.full_next ? out.full_next + (full_off) : nullptr;                                            \
    io.out_hops = out.full_hops ? out.full_hops + (full_off) : nullptr;                                            \
    io.in_base = 0; io.out_base = (body_off); io.n = n;                                                            \
    io.patch_index = patch_index; io.patch_rate = patch_rate; io.patch_next = patch_next; io.patch_hops = patch_hops; \
    io.item_src = item_src; io.item_dst = item_dst;                                                                \
    io.item_rate = out.item_rate; io.item_next = out.item_next; io.item_hops = out.item_hops;                      \
    SweepIO<T>::range(patch_ptr, (b), patch_total, io.p0, io.p1);                                                  \
    SweepIO<T>::range(item_ptr, (b), item_total, io.q0, io.q1)

template <typename T, int M, int RG, bool HAS_NEXT, bool HAS_HOPS>
__global__ __launch_bounds__(M * RG) void small_solve_sweep(FWX_SWEEP_PARAMS)
{
    const size_t off = (size_t)blockIdx.x * (size_t)out.stride;
    FWX_SWEEP_IO(io, (long long)blockIdx.x, off, (size_t)0);
    small_solve_body<T, M, RG, HAS_NEXT, HAS_HOPS, false>(io, n, 0, n, out.updates ? out.updates + blockIdx.x : nullptr,
                                                          PathLog{});
}

template <typename T, bool HAS_NEXT, bool HAS_HOPS>
__global__ __launch_bounds__(256) void wave_solve_sweep(FWX_SWEEP_PARAMS)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const long long b = (long long)blockIdx.x * 4 + wave;
    if (b >= count) return;                   // wave-uniform
    FWX_SWEEP_IO(io, b, (size_t)0, (size_t)b * (size_t)out.stride);
    wave_solve_body<T, HAS_NEXT, HAS_HOPS, false>(io, n, b, 0, n, out.updates, PathLog{});
}
#undef FWX_SWEEP_IO
#undef FWX_SWEEP_PARAMS

template <typename T>
hipError_t launch_sweep_solve(const T *base_rate, const int32_t *base_next, const int32_t *base_hops, int count, int n,
                              const SweepTables<T> &t, unsigned long long *updates_each, int wave_max_n, hipStream_t s)
{
    if (count <= 0 || n <= 0) return hipSuccess;
    if (n > FWX_SMALL_N || !base_rate || (base_hops && !base_next) || t.patch_total < 0 || t.item_total < 0 ||
        (t.patch_total > 0 && (!t.patch_ptr || !t.patch_index || !t.patch_rate)) ||
        (t.item_total > 0 && (!t.item_ptr || !t.item_src || !t.item_dst || !t.item_rate)) ||
        ((t.patch_next || t.item_next || t.full_next) && !base_next) ||
        ((t.patch_hops || t.item_hops || t.full_hops) && !base_hops) ||
        ((t.full_rate || t.full_next || t.full_hops) && t.full_stride < (long long)n * n))
        return hipErrorInvalidValue;
    const bool wave = n <= wave_max_n && n <= FWX_BATCH_WAVE_N;
    constexpr int kChunk = 1 << 21;           // workgroups per launch, as launch_batch_solve
    for (long long b0 = 0; b0 < count; b0 += kChunk) {
        const int cnt = (int)std::min<long long>(kChunk, count - b0);
        const size_t off = (size_t)b0 * (size_t)t.full_stride;
        const SweepOut<T> out = {t.item_rate, t.item_next, t.item_hops, t.full_rate ? t.full_rate + off : nullptr,
                                 t.full_next ? t.full_next + off : nullptr, t.full_hops ? t.full_hops + off : nullptr,
                                 t.full_stride, updates_each ? updates_each + b0 : nullptr};
        const int64_t *pp = t.patch_total > 0 ? t.patch_ptr + b0 : nullptr, *ip = t.item_total > 0 ? t.item_ptr + b0 : nullptr;
#define FWX_SWEEP_ARGS                                                                                             \
    base_rate, base_next, base_hops, n, cnt, pp, (long long)t.patch_total, t.patch_index, t.patch_rate,            \
        t.patch_next, t.patch_hops, ip, (long long)t.item_total, t.item_src, t.item_dst, out
#define FWX_SWEEP_WAVE(HN, HH)                                                                     \
    hipLaunchKernelGGL((wave_solve_sweep<T, HN, HH>), dim3((cnt + 3) / 4), dim3(256), 0, s, FWX_SWEEP_ARGS)
#define FWX_SWEEP_WG(M, RG, HN, HH)                                                                \
    hipLaunchKernelGGL((small_solve_sweep<T, M, RG, HN, HH>), dim3(cnt), dim3(M * RG), 0, s, FWX_SWEEP_ARGS)
#define FWX_SWEEP_FIELDS(LAUNCH, ...)                                                              \
    do {                                                                                           \
        if (base_hops) LAUNCH(__VA_ARGS__ true, true);                                             \
        else if (base_next) LAUNCH(__VA_ARGS__ true, false);                                       \
        else LAUNCH(__VA_ARGS__ false, false);                                                     \
    } while (0)
        if (wave) FWX_SWEEP_FIELDS(FWX_SWEEP_WAVE);
        else if (n <= 64) FWX_SWEEP_FIELDS(FWX_SWEEP_WG, 64, 16,);
        else FWX_SWEEP_FIELDS(FWX_SWEEP_WG, 128, 8,);
#undef FWX_SWEEP_FIELDS
#undef FWX_SWEEP_WG
#undef FWX_SWEEP_WAVE
#undef FWX_SWEEP_ARGS
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template hipError_t launch_sweep_solve<float>(const float *, const int32_t *, const int32_t *, int, int,
                                              const SweepTables<float> &, unsigned long long *, int, hipStream_t);
template hipError_t launch_sweep_solve<double>(const double *, const int32_t *, const int32_t *, int, int,
                                               const SweepTables<double> &, unsigned long long *, int, hipStream_t);

template <typename T>
hipError_t launch_ragged_solve(T *rate, int32_t *next, int32_t *hops, int count, const int32_t *n_each,
                               const int64_t *offset, const int32_t *order, const int32_t tier_count[3],
                               unsigned long long *updates_each, hipStream_t s, PathLog plog)
{
    const long long tiers[3] = {tier_count[0], tier_count[1], tier_count[2]};
    if (count < 0 || tiers[0] < 0 || tiers[1] < 0 || tiers[2] < 0 || tiers[0] + tiers[1] + tiers[2] > count ||
        (hops && !next))
        return hipErrorInvalidValue;
    if (tiers[0] + tiers[1] + tiers[2] == 0) return hipSuccess;
    const bool lg = plog.last != nullptr;
    if (!rate || !n_each || !offset || !order || (lg && (!next || !plog.at_col || !plog.at_row)))
        return hipErrorInvalidValue;
    constexpr int kChunk = 1 << 21;           // workgroups per launch, as launch_batch_solve
#define FWX_RAGGED_WAVE(HN, HH, LG)                                                                \
    hipLaunchKernelGGL((wave_solve_ragged<T, HN, HH, LG>), dim3((cnt + 3) / 4), dim3(256), 0, s, rate, next, hops, \
                       count, n_each, offset, ord, cnt, updates_each, plog)
#define FWX_RAGGED_WG(M, RG, HN, HH, LG)                                                           \
    hipLaunchKernelGGL((small_solve_ragged<T, M, RG, HN, HH, LG>), dim3(cnt), dim3(M * RG), 0, s, rate, next, hops, \
                       count, n_each, offset, ord, updates_each, plog)
#define FWX_RAGGED_FIELDS(LAUNCH, ...)                                                             \
    do {                                                                                           \
        if (hops) { if (lg) LAUNCH(__VA_ARGS__ true, true, true); else LAUNCH(__VA_ARGS__ true, true, false); }   \
        else if (next) { if (lg) LAUNCH(__VA_ARGS__ true, false, true); else LAUNCH(__VA_ARGS__ true, false, false); } \
        else LAUNCH(__VA_ARGS__ false, false, false);                                              \
    } while (0)
    // the 128-wide tier first: its workgroups run longest
    for (int tier = 2; tier >= 0; --tier) {
        const long long first = tier == 2 ? tiers[0] + tiers[1] : tier == 1 ? tiers[0] : 0;
        const long long per = tier == 0 ? 4LL * kChunk : kChunk;     // matrices per launch: four waves a workgroup
        for (long long b0 = 0; b0 < tiers[tier]; b0 += per) {
            const int cnt = (int)std::min<long long>(per, tiers[tier] - b0);
            const int32_t *ord = order + first + b0;
            if (tier == 0) FWX_RAGGED_FIELDS(FWX_RAGGED_WAVE);
            else if (tier == 1) FWX_RAGGED_FIELDS(FWX_RAGGED_WG, 64, 16,);
            else FWX_RAGGED_FIELDS(FWX_RAGGED_WG, 128, 8,);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
    }
#undef FWX_RAGGED_FIELDS
#undef FWX_RAGGED_WG
#undef FWX_RAGGED_WAVE
    return hipSuccess;
}

template hipError_t launch_ragged_solve<float>(float *, int32_t *, int32_t *, int, const int32_t *, const int64_t *,
                                               const int32_t *, const int32_t *, unsigned long long *, hipStream_t,
                                               PathLog);
template hipError_t launch_ragged_solve<double>(double *, int32_t *, int32_t *, int, const int32_t *, const int64_t *,
                                                const int32_t *, const int32_t *, unsigned long long *, hipStream_t,
                                                PathLog);

template <typename T>
hipError_t launch_small_solve(T *rate, int32_t *next, int32_t *hops, int n, int k_begin, int k_end,
                              unsigned long long *updates, PathLog plog, hipStream_t s)
{
    if (n <= 0 || k_end <= k_begin) return hipSuccess;
    if (n > FWX_SMALL_N || (hops && !next) || k_begin < 0 || k_end > n) return hipErrorInvalidValue;
    note_form(KF_SMALL_SOLVE);
#define FWX_SMALL(M, RG, HN, HH, LG)                                                               \
    hipLaunchKernelGGL((small_solve<T, M, RG, HN, HH, LG>), dim3(1), dim3(M * RG), 0, s, rate,     \
                       next, hops, n, k_begin, k_end, updates, plog)
#define FWX_SMALL_M(M, RG)                                                                         \
    do {                                                                                           \
        const bool lg = next && plog.last;                                                         \
        if (hops) { if (lg) FWX_SMALL(M, RG, true, true, true); else FWX_SMALL(M, RG, true, true, false); }    \
        else if (next) { if (lg) FWX_SMALL(M, RG, true, false, true); else FWX_SMALL(M, RG, true, false, false); } \
        else FWX_SMALL(M, RG, false, false, false);                                                \
    } while (0)
    if (n <= 64) FWX_SMALL_M(64, 16);         // 1024 threads x 4 entries: 4 waves per SIMD hide
    else FWX_SMALL_M(128, 8);                 //   the LDS latency; 1024 threads x 16 entries
#undef FWX_SMALL_M
#undef FWX_SMALL
    return hipGetLastError();
}

template hipError_t launch_small_solve<float>(float *, int32_t *, int32_t *, int, int, int,
                                              unsigned long long *, PathLog, hipStream_t);
template hipError_t launch_small_solve<double>(double *, int32_t *, int32_t *, int, int, int,
                                               unsigned long long *, PathLog, hipStream_t);

template <typename T>
__global__ __launch_bounds__(256) void snapshot_row(T *dst, const T *src, int32_t *hdst,
                                                    const int32_t *hsrc, int n)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < n) {
        dst[j] = src[j];
        if (hdst) hdst[j] = hsrc[j];
    }
}

// -------------------------------------------------------------------------------------------------
// Host-side launchers
// -------------------------------------------------------------------------------------------------
template <typename T, int W, int NV, int RPB, int UNROLL, int MINW = 1, int SV = RELAX_SV_SELECT>
static hipError_t launch_relax_cfg(const RelaxArgs<T> &a, hipStream_t s)
{
    constexpr int SW = 256 * NV * W;
    const int nstrips = (a.n + SW - 1) / SW;
    const int nchunks = (a.rows + RPB - 1) / RPB;
    const dim3 grid((unsigned)(nstrips * nchunks)), block(256);
    if (grid.x == 0) return hipSuccess;
    if (a.skip_hi > a.skip_lo && (a.skip_lo % RPB || a.skip_hi % RPB)) return hipErrorInvalidValue;
    const int flip = a.flip == 2 && grid.x % 8 ? 1 : a.flip;
    // Cache policy split: the tiles that hold the last `temporal_bytes` of the slab load with the
    // default policy, all before them non-temporally (relax_k, `nt_below`).
    int nt_below = 0;
    const double slab = (double)a.rows * a.n * sizeof(T);
    if (a.temporal_bytes >= 0 && slab > (double)a.temporal_bytes) {
        const double tail = std::ceil((double)a.temporal_bytes / slab * grid.x);
        nt_below = (int)grid.x - (int)std::min(tail, (double)grid.x);
    }
    // Store group of the rates-only path in lanes of 16 bytes (the scalar path stores per lane).
    const int sb = a.store_bytes > 0 ? a.store_bytes : FWX_PERK_STORE_BYTES_DEFAULT;
    const int gl = sb >= 128 ? 8 : sb >= 64 ? 4 : sb >= 32 ? 2 : 1;
#define FWX_LAUNCH(HN, HH, CN, GL)                                                                 \
    hipLaunchKernelGGL((relax_k<T, W, NV, RPB, UNROLL, HN, HH, CN, MINW, GL, SV>), grid, block, 0, s, \
                       a.rate, a.next, a.hops, a.prow, a.phops, a.pnext, a.rows, a.n, a.row0, a.k,  \
                       nstrips, flip, a.updates, a.plog, a.skip_lo, a.skip_hi, nt_below)
#define FWX_LAUNCH_GL(CN)                                                                          \
    do {                                                                                           \
        if constexpr (W * sizeof(T) == 16) {                                                       \
            if (gl == 8) { FWX_LAUNCH(false, false, CN, 8); break; }                               \
            if (gl == 4) { FWX_LAUNCH(false, false, CN, 4); break; }                               \
            if (gl == 2) { FWX_LAUNCH(false, false, CN, 2); break; }                               \
        }                                                                                          \
        FWX_LAUNCH(false, false, CN, 1);                                                           \
    } while (0)
    const bool hn = a.next != nullptr, hh = a.hops != nullptr, cn = a.updates != nullptr;
    note_form(KF_RELAX_K);
    if (hh) {
        if (cn) FWX_LAUNCH(true, true, true, 1); else FWX_LAUNCH(true, true, false, 1);
    } else if (hn) {
        if (cn) FWX_LAUNCH(true, false, true, 1); else FWX_LAUNCH(true, false, false, 1);
    } else {
        if (cn) FWX_LAUNCH_GL(true); else FWX_LAUNCH_GL(false);
    }
#undef FWX_LAUNCH_GL
#undef FWX_LAUNCH
    return hipGetLastError();
}

template <typename T> hipError_t launch_relax(const RelaxArgs<T> &a, hipStream_t s)
{
    constexpr int WV = 16 / (int)sizeof(T);
    const bool vec_ok = (a.n % WV == 0) && ((uintptr_t)a.rate % 16 == 0) &&
                        ((uintptr_t)a.prow % 16 == 0);
    if (a.hops && !a.next) return hipErrorInvalidValue;  // hops ride on the next-hop path
    // Launch geometry from the sweep in tools/tune_relax.hip (profiles/r01_tune_relax_sweep1.txt ... _sweep3.txt):
    // one 16-byte vector per thread (strip = 1024 f32 / 512 f64 columns), 4 rows per workgroup,
    // 4 loads in flight per thread.  Many small workgroups beat fewer large ones by 10-15 % at
    // N = 16384: the resident set then covers a compact band of rows (DRAM page locality) and
    // the tail of the launch is short.
    if (!vec_ok) return launch_relax_cfg<T, 1, 1, 4, 4>(a, s);
    return launch_relax_cfg<T, WV, 1, 4, 4>(a, s);
}

template hipError_t launch_relax<float>(const RelaxArgs<float> &, hipStream_t);
template hipError_t launch_relax<double>(const RelaxArgs<double> &, hipStream_t);

// The geometries in which the 16-pivot sweep exists: non-counting f32 (the only instantiation with a max form; a
// counting call and f64 stay 8 wide, round 19), 8 or 16 rows per workgroup, 4 or 8 rows in flight.
template <typename T, int RPB, int UNROLL> constexpr bool relax_kt_wide()
{
    return relax_kt_max_form<T>() && (RPB == 8 || RPB == 16) && (UNROLL == 4 || UNROLL == 8);
}

// relax_kt with the geometry (RPB, UNROLL); the tile order, the cache-policy split and the store group
// are chosen exactly as launch_relax_cfg chooses them for relax_k.  np == 16 is taken only where the kernel exists
// (relax_kt_wide, uncounted).  NARROW / WIDE: which kernels this instantiation carries, np 2, 4 and 8 / np 16; the
// library asks for one of the two in each of its two geometries, tools/tune_relax.hip for both.
template <typename T, int RPB, int UNROLL, bool NARROW = true, bool WIDE = relax_kt_wide<T, RPB, UNROLL>()>
static hipError_t launch_relax_kt_cfg(const RelaxKtArgs<T> &a, hipStream_t s)
{
    constexpr int W = 16 / (int)sizeof(T), SW = 256 * W;
    static_assert(!WIDE || relax_kt_wide<T, RPB, UNROLL>(), "no 16-pivot kernel in this geometry");
    if (a.n <= 0) return hipSuccess;
    const bool narrow = NARROW && (a.np == 2 || a.np == 4 || a.np == 8);
    const bool wide = WIDE && a.np == 16 && !a.updates;
    if (a.n % W || (uintptr_t)a.rate % 16 || (uintptr_t)a.w % 16 || a.ct_ld < a.n || a.k < 0 ||
        a.k + a.np > a.n || !(narrow || wide))
        return hipErrorInvalidValue;
    const int nstrips = (a.n + SW - 1) / SW;
    const int nchunks = (a.n + RPB - 1) / RPB;
    // ceil(2^32 / nstrips) for the kernel's tile -> (strip, chunk); 0 (the kernel divides) for one strip and
    // for a grid on which the multiply-high is not proven exact
    unsigned strip_magic = 0;
    if (nstrips >= 2 && (unsigned long long)nstrips * nchunks * nstrips < (1ull << 32))
        strip_magic = (unsigned)(0xffffffffull / (unsigned)nstrips) + 1u;
    const dim3 grid((unsigned)(nstrips * nchunks)), block(256);
    const int flip = a.flip == 2 && grid.x % 8 ? 1 : a.flip;
    int nt_below = 0;
    const double slab = (double)a.n * a.n * sizeof(T);
    if (a.temporal_bytes >= 0 && slab > (double)a.temporal_bytes) {
        const double tail = std::ceil((double)a.temporal_bytes / slab * grid.x);
        nt_below = (int)grid.x - (int)std::min(tail, (double)grid.x);
    }
    const int sb = a.store_bytes > 0 ? a.store_bytes : FWX_PERK_STORE_BYTES_DEFAULT;
    const int gl = sb >= 128 ? 8 : sb >= 64 ? 4 : sb >= 32 ? 2 : 1;
#define FWX_LAUNCH_KT(CN, GL, NP)                                                                  \
    hipLaunchKernelGGL((relax_kt<T, W, RPB, UNROLL, CN, GL, NP>), grid, block, 0, s, a.rate, a.w, a.ct, \
                       a.ct_ld, a.n, a.k, nstrips, flip, a.updates, nt_below, strip_magic, a.fold_compare ? 1 : 0)
#define FWX_LAUNCH_KT_NP(CN, GL)                                                                   \
    do {                                                                                           \
        if constexpr (WIDE && !CN) {                                                               \
            if (a.np == 16) FWX_LAUNCH_KT(CN, GL, 16);                                             \
        }                                                                                          \
        if constexpr (NARROW) {                                                                    \
            if (a.np == 8) FWX_LAUNCH_KT(CN, GL, 8);                                               \
            else if (a.np == 4) FWX_LAUNCH_KT(CN, GL, 4);                                          \
            else if (a.np == 2) FWX_LAUNCH_KT(CN, GL, 2);                                          \
        }                                                                                          \
    } while (0)
#define FWX_LAUNCH_KT_GL(CN)                                                                       \
    do {                                                                                           \
        if (gl == 8) FWX_LAUNCH_KT_NP(CN, 8);                                                      \
        else if (gl == 4) FWX_LAUNCH_KT_NP(CN, 4);                                                 \
        else if (gl == 2) FWX_LAUNCH_KT_NP(CN, 2);                                                 \
        else FWX_LAUNCH_KT_NP(CN, 1);                                                              \
    } while (0)
    // The form RELAX_K stands for the per-k engine, whichever of its two kernels sweeps: relax_kt has no
    // bit of its own, its launches are counted by width instead (fwx_test_perk_pivots).
    note_form(KF_RELAX_K);
    if (a.updates) FWX_LAUNCH_KT_GL(true); else FWX_LAUNCH_KT_GL(false);
#undef FWX_LAUNCH_KT_GL
#undef FWX_LAUNCH_KT_NP
#undef FWX_LAUNCH_KT
    return hipGetLastError();
}

// relax_walk with the geometry (RPB rows per workgroup, UNROLL slots), the policy POL and the walk ROLL: np == NP,
// uncounted f32.  The tile order, the cache-policy split and the store group are chosen as launch_relax_kt_cfg chooses
// them, in tiles of RPB rows.  ALLGL: every store group; otherwise the default one alone (tools/tune_relax.hip).
// NP = 32 (round 25): 8 bytes of a row per lane, strips of 512 columns, a store group of the same bytes is twice the
// lanes.  The matrix keeps the 16-byte rules of every relax_kt launch (n a multiple of 4, 16-byte aligned).
template <int RPB, int UNROLL, int POL, bool ROLL, bool ALLGL = false, int NP = 16>
static hipError_t launch_relax_walk_cfg(const RelaxKtArgs<float> &a, hipStream_t s)
{
    constexpr int W = 64 / NP, SW = 256 * W, LG = 4 / W;      // LG: lanes per 16 bytes
    if (a.n <= 0) return hipSuccess;
    if (a.n % 4 || (uintptr_t)a.rate % 16 || (uintptr_t)a.w % 16 || a.ct_ld < a.n || a.k < 0 || a.np != NP ||
        a.k + a.np > a.n || a.updates)
        return hipErrorInvalidValue;
    const int nstrips = (a.n + SW - 1) / SW;
    const int nchunks = (a.n + RPB - 1) / RPB;
    unsigned strip_magic = 0;
    if (nstrips >= 2 && (unsigned long long)nstrips * nchunks * nstrips < (1ull << 32))
        strip_magic = (unsigned)(0xffffffffull / (unsigned)nstrips) + 1u;
    const dim3 grid((unsigned)(nstrips * nchunks)), block(256);
    const int flip = a.flip == 2 && grid.x % 8 ? 1 : a.flip;
    int nt_below = 0;
    const double slab = (double)a.n * a.n * sizeof(float);
    if (a.temporal_bytes >= 0 && slab > (double)a.temporal_bytes) {
        const double tail = std::ceil((double)a.temporal_bytes / slab * grid.x);
        nt_below = (int)grid.x - (int)std::min(tail, (double)grid.x);
    }
    const int sb = a.store_bytes > 0 ? a.store_bytes : FWX_PERK_STORE_BYTES_DEFAULT;
    const int gl = sb >= 128 ? 8 : sb >= 64 ? 4 : sb >= 32 ? 2 : 1;
#define FWX_LAUNCH_WALK(GL)                                                                        \
    hipLaunchKernelGGL((relax_walk<RPB, UNROLL, (GL) * LG, POL, ROLL, NP, W>), grid, block, 0, s, a.rate, a.w, a.ct,  \
                       a.ct_ld, a.n, a.k, nstrips, flip, nt_below, strip_magic, a.fold_compare ? 1 : 0)
    note_form(KF_RELAX_K);
    if (gl == 4) FWX_LAUNCH_WALK(4);
    else if constexpr (ALLGL) {
        if (gl == 8) FWX_LAUNCH_WALK(8);
        else if (gl == 2) FWX_LAUNCH_WALK(2);
        else FWX_LAUNCH_WALK(1);
    } else {
        return hipErrorInvalidValue;
    }
#undef FWX_LAUNCH_WALK
    return hipGetLastError();
}

template <typename T> hipError_t launch_relax_kt(const RelaxKtArgs<T> &a, hipStream_t s)
{
    if (a.np == 32) {
        if constexpr (std::is_same<T, float>::value) {
            if (a.walk && !a.updates)
                return launch_relax_walk_cfg<FWX_PERK_DEEP_RPB, FWX_PERK_DEEP_UNROLL, WALK_POL_PLAIN, false, true, 32>(a, s);
        }
        return hipErrorInvalidValue;
    }
    if (a.np == 16) {
        if constexpr (std::is_same<T, float>::value) {
            if (a.walk && !a.updates)
                return launch_relax_walk_cfg<FWX_PERK_WALK_RPB, FWX_PERK_WALK_UNROLL, FWX_PERK_WALK_POL,
                                             FWX_PERK_WALK_ROLL, true>(a, s);
        }
        if constexpr (relax_kt_wide<T, FWX_PERK_KT16_RPB, FWX_PERK_KT16_UNROLL>())
            return launch_relax_kt_cfg<T, FWX_PERK_KT16_RPB, FWX_PERK_KT16_UNROLL, false, true>(a, s);
        return hipErrorInvalidValue;
    }
    return launch_relax_kt_cfg<T, FWX_PERK_KT_RPB, FWX_PERK_KT_UNROLL, true, false>(a, s);
}

template hipError_t launch_relax_kt<float>(const RelaxKtArgs<float> &, hipStream_t);
template hipError_t launch_relax_kt<double>(const RelaxKtArgs<double> &, hipStream_t);

template <typename T>
hipError_t launch_snapshot_row(T *dst, const T *src, int32_t *hdst, const int32_t *hsrc, int n,
                               hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL((snapshot_row<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dst,
                       src, hdst, hsrc, n);
    return hipGetLastError();
}

template hipError_t launch_snapshot_row<float>(float *, const float *, int32_t *, const int32_t *,
                                               int, hipStream_t);
template hipError_t launch_snapshot_row<double>(double *, const double *, int32_t *,
                                                const int32_t *, int, hipStream_t);

}  // namespace fwx
