// fwx_batch.hip -- the batched solves of the C ABI (include/fwx.h): fwx_solve_batch_* / fwx_solve_ragged_* with
// their _mid, _large and _lists forms, the device forms fwx_dev_solve_batch* / fwx_dev_solve_ragged* /
// fwx_dev_exact_paths_*, the ragged plans and the fwx_test_batch_* hooks.  Host code only: the kernels and their
// launchers are fwx_kernels.hip, fwx_mid.hip and fwx_large.hip, the exact walk (launch_exact_batch,
// launch_exact_ragged; fwx_query.h) is fwx_api.hip, which the handles share it with.
//
// A family of entry points is one BatchFamily value; every contract has one body that takes it:
//   dev_solve_uniform      fwx_dev_solve_batch{,_mid,_large}{,_traced}
//   dev_solve_ragged       fwx_dev_solve_ragged{,_mid,_large}
//   dev_exact_paths_batch  fwx_dev_exact_paths_batch{,_mid,_large}
//   dev_exact_paths_ragged fwx_dev_exact_paths_ragged{,_mid,_large}
//   solve_batch_host       every host form
//   dev_solve_sweep        fwx_dev_solve_sweep{,_mid}
//   solve_sweep_host       fwx_solve_sweep{,_mid}_*
// and the tier of an order is decided in one place, BatchFamily::tier, which run_uniform acts on.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "fwx.h"
#include "fwx_guard.h"
#include "fwx_internal.h"
#include "fwx_kernels.h"
#include "fwx_query.h"

using namespace fwxi;

static_assert(FWX_BATCH_MID_MAX_N == FWX_MID_N, "fwx.h states the largest order of the mid tier");
static_assert(FWX_BATCH_LARGE_MAX_N <= FWX_LARGE_N, "fwx.h states no order the large tier cannot take");
static_assert(FWX_RAGGED_LARGE_WORK_ENTRIES(7) == 3 * 8, "three rows of count + 1 entries");
static_assert(FWX_BATCH_LARGE_SCRATCH_BYTES(1000) == FWX_LARGE_SCRATCH_BYTES(1000) &&
                  FWX_BATCH_LARGE_SCRATCH_BYTES(1) == FWX_LARGE_SCRATCH_BYTES(1),
              "fwx.h states the scratch the large tier lays out");
static_assert(FWX_SWEEP_MID_SCRATCH_BYTES(255) == FWX_MID_SWEEP_SLOT_BYTES(255) && FWX_SWEEP_MID_MAX_N == FWX_MID_N,
              "fwx.h states the slot the mid tier's sweep lays out");

namespace {

// Tier choice of the batched small solves (fwx_solve_batch_*, fwx_dev_solve_batch): matrices of order n <=
// FWX_BATCH_WAVE_MAX_N take the wave tier (one wave per matrix, registers only), larger ones the workgroup
// tier (small_solve's body, one workgroup per matrix).  An integer 0 ... FWX_BATCH_WAVE_N, read on every
// call; 0 turns the wave tier off; any other value: the default.  No result bit depends on it.
#define FWX_BATCH_WAVE_MAX_N_DEFAULT FWX_BATCH_WAVE_N
int batch_wave_max_n()
{
    return (int)env_digits("FWX_BATCH_WAVE_MAX_N", 0, FWX_BATCH_WAVE_N, FWX_BATCH_WAVE_MAX_N_DEFAULT);
}

// Routing of the mid-size batch entry points (fwx_solve_batch_mid_*, fwx_dev_solve_batch_mid): orders below
// FWX_BATCH_MID_MIN_N are forwarded to the tiers above, orders from it up to FWX_BATCH_MID_MAX_N run the mid
// tier (fwx_mid.hip).  An integer 1 ... FWX_BATCH_MAX_N + 1, read on every call; any other value: the default,
// FWX_BATCH_MAX_N + 1 (only what the small tiers cannot take).  No result bit depends on it.
// fwx_ragged_mid_plan and the host forms fwx_solve_ragged_mid_* read it too, as the boundary of the plan's fourth tier
// (the plan reads it and only the plan: the device form takes the tier counts it is given).
#define FWX_BATCH_MID_MIN_N_DEFAULT (FWX_BATCH_MAX_N + 1)
int batch_mid_min_n()
{
    return (int)env_digits("FWX_BATCH_MID_MIN_N", 1, FWX_BATCH_MID_MIN_N_DEFAULT, FWX_BATCH_MID_MIN_N_DEFAULT);
}

// Routing of the large batch entry points (fwx_solve_batch_large_*, fwx_dev_solve_batch_large): orders below
// FWX_BATCH_LARGE_MIN_N are forwarded to the mid entry path (which forwards further by FWX_BATCH_MID_MIN_N), orders
// from it up to FWX_BATCH_LARGE_MAX_N run the large tier (fwx_large.hip).  An integer 1 ... FWX_BATCH_MID_MAX_N + 1,
// read on every call; any other value: the default, FWX_BATCH_MID_MAX_N + 1.  No result bit depends on it.
#define FWX_BATCH_LARGE_MIN_N_DEFAULT (FWX_BATCH_MID_MAX_N + 1)
int batch_large_min_n()
{
    return (int)env_digits("FWX_BATCH_LARGE_MIN_N", 1, FWX_BATCH_LARGE_MIN_N_DEFAULT, FWX_BATCH_LARGE_MIN_N_DEFAULT);
}

// fwx_solve_batch_lists_*: items walked per launch.  The lists (cap int32 per item), the walk stacks
// (FWX_EXACT_SCRATCH_INTS(n)) and the item triples + lengths (4) of one launch stay within
// FWX_BATCH_LISTS_BUDGET_BYTES of device memory; FWX_BATCH_LISTS_CHUNK (environment, read per call: digits only,
// >= 1, anything else means the default) asks for fewer.  At least one item per launch.  No result depends on it.
#define FWX_BATCH_LISTS_BUDGET_BYTES ((long long)64 << 20)
long long batch_lists_chunk(int n, int cap)
{
    const long long per_item = 4ll * ((long long)cap + 3ll * ((long long)n + 2) + 4);
    long long fit = FWX_BATCH_LISTS_BUDGET_BYTES / per_item;
    if (fit < 1) fit = 1;
    return env_digits("FWX_BATCH_LISTS_CHUNK", 1, fit - 1, fit);
}

enum Tier { TIER_SMALL, TIER_MID, TIER_LARGE };

// One family of entry points: the largest order it takes, the tiers it may route to beyond the small ones (the
// wave and workgroup tiers of fwx_kernels.hip, which every family has) and the tiers of its ragged plan --
// ragged_tiers == 0: the family has no ragged form.
struct BatchFamily {
    int32_t max_n;
    bool mid, large;
    int ragged_tiers;
    // Where a uniform batch of order n runs: orders from FWX_BATCH_LARGE_MIN_N up the large tier, below it from
    // FWX_BATCH_MID_MIN_N up the mid tier, the rest the small tiers -- the same bits wherever.
    Tier tier(int32_t n) const
    {
        return large && n >= batch_large_min_n() ? TIER_LARGE : mid && n >= batch_mid_min_n() ? TIER_MID : TIER_SMALL;
    }
    // The large tier's scratch panels are used, and judged, only by a call routed there with pivots to apply.
    bool needs_scratch(int32_t n, int32_t k_begin, int32_t k_end) const
    {
        return tier(n) == TIER_LARGE && k_end > k_begin;
    }
};
constexpr BatchFamily kPlain = {FWX_BATCH_MAX_N, false, false, 3};
constexpr BatchFamily kMid = {FWX_BATCH_MID_MAX_N, true, false, 4};
constexpr BatchFamily kLarge = {FWX_BATCH_LARGE_MAX_N, true, true, 5};

// body(rate as double * or float *), by the dtype code of a device form (checked by the caller).
template <typename F> int with_dtype(int32_t dtype, void *rate, F &&body)
{
    return dtype == FWX_F64 ? body((double *)rate) : body((float *)rate);
}

bool trace_complete(const fwx_trace *t) { return t && t->last && t->at_col && t->at_row; }

// A null trace: no trace.
fwx::PathLog plog_of(const fwx_trace *t)
{
    fwx::PathLog plog{};
    if (t) {
        plog.last = t->last;
        plog.at_col = t->at_col;
        plog.at_row = t->at_row;
    }
    return plog;
}

bool large_scratch_ok(int32_t n, const void *scratch, size_t bytes)
{
    return scratch && !((uintptr_t)scratch & 15) && bytes >= FWX_BATCH_LARGE_SCRATCH_BYTES((size_t)n);
}

// What a launcher refuses (a trace without next or over a part of the pivots, scratch it cannot use) is the caller's
// mistake.
int launch_status(hipError_t e)
{
    if (e == hipErrorInvalidValue) return FWX_ERR_INVALID;
    FWX_HIP(e);
    return FWX_OK;
}

// What the batch entry points decide before any device call (fwx.h): the pivot range against n, then the
// order against the family's limit.  k_end <= 0 means n.
int batch_range(const BatchFamily &f, int32_t n, int32_t k_begin, int32_t &k_end)
{
    if (k_end <= 0) k_end = n;
    if (k_begin < 0 || k_begin > k_end || k_end > n) return FWX_ERR_INVALID;
    return n > f.max_n ? FWX_ERR_UNSUPPORTED : FWX_OK;
}

// `count` matrices of one order on the tier the family routes it to, queued on s.  The large tier runs groups of as
// many matrices as the scratch holds, one after the other; plog: the path trace, whole pivot range only.
template <typename T>
int run_uniform(const BatchFamily &f, int32_t count, int32_t n, T *rate, int32_t *next, int32_t *hops, int64_t stride,
                int32_t k_begin, int32_t k_end, unsigned long long *d_updates_each, void *scratch, size_t scratch_bytes,
                hipStream_t s, const fwx::PathLog &plog)
{
    switch (f.tier(n)) {
    case TIER_LARGE:
        return launch_status(fwx::launch_batch_large<T>(rate, next, hops, count, n, (long long)stride, k_begin, k_end,
                                                        d_updates_each, scratch, scratch_bytes, s, plog));
    case TIER_MID:
        return launch_status(fwx::launch_batch_mid<T>(rate, next, hops, count, n, (long long)stride, k_begin, k_end,
                                                      d_updates_each, s, plog));
    default:
        return launch_status(fwx::launch_batch_solve<T>(rate, next, hops, count, n, (long long)stride, k_begin, k_end,
                                                        d_updates_each, batch_wave_max_n(), s, plog));
    }
}

// What the fifth tier of a ragged batch runs on (fwx_dev_solve_ragged_large): the plan's work table on the host and on
// the device, 3 * (count + 1) entries each, and the scratch panels.  Unused with fewer tiers.
struct RaggedLarge {
    const int64_t *work = nullptr, *d_work = nullptr;
    void *scratch = nullptr;
    size_t scratch_bytes = 0;
};

// A planned ragged batch, queued on s.  From four tiers up the mid tier first -- its workgroups run longest -- then the
// three small tiers; with five the large tier's chain of launches (launch_ragged_large) behind them.
template <typename T>
int run_ragged(int tiers, int32_t count, T *rate, int32_t *next, int32_t *hops, const int32_t *d_n_each,
               const int64_t *d_offset, const int32_t *d_order, const int32_t *tier_count,
               unsigned long long *d_updates_each, const RaggedLarge &lg, hipStream_t s, const fwx::PathLog &plog)
{
    const long long small = (long long)tier_count[0] + tier_count[1] + tier_count[2];
    int rc = FWX_OK;
    if (tiers >= 4)
        rc = launch_status(fwx::launch_ragged_mid<T>(rate, next, hops, count, d_n_each, d_offset, d_order + small,
                                                     tier_count[3], d_updates_each, s, plog));
    if (!rc && (tiers < 4 || small > 0))
        rc = launch_status(fwx::launch_ragged_solve<T>(rate, next, hops, count, d_n_each, d_offset, d_order, tier_count,
                                                       d_updates_each, s, plog));
    if (!rc && tiers >= 5 && tier_count[4] > 0)
        rc = launch_status(fwx::launch_ragged_large<T>(rate, next, hops, count, d_n_each, d_offset,
                                                       d_order + small + tier_count[3], tier_count[4], lg.work,
                                                       lg.d_work, (long long)count + 1, d_updates_each, lg.scratch,
                                                       lg.scratch_bytes, s, plog));
    return rc;
}

// Ragged batches: what the orders alone decide.  FWX_ERR_INVALID for a negative order; n_max is the largest
// order, whatever it is -- the caller compares it with the family's limit.
int ragged_orders(int32_t count, const int32_t *n_each, int32_t &n_max)
{
    n_max = 0;
    for (int32_t b = 0; b < count; ++b) {
        if (n_each[b] < 0) return FWX_ERR_INVALID;
        n_max = std::max(n_max, n_each[b]);
    }
    return FWX_OK;
}

// The plan of a family's ragged form (fwx_ragged_plan: three tiers, fwx_ragged_mid_plan: four, fwx_ragged_large_plan:
// five -- large, n >= FWX_BATCH_LARGE_MIN_N, which wins over the mid tier as that does over the wave tier) for orders that
// ragged_orders accepted and the family's limit admits: the packed offsets (count + 1 entries), the matrices with
// n >= 1 grouped by tier -- wave (n <= FWX_BATCH_WAVE_MAX_N), 64-wide, 128-wide and, with four tiers, mid (n >=
// FWX_BATCH_MID_MIN_N, which wins where the wave tier claims the order too) -- and within a tier by descending order,
// ties by ascending index (a counting sort over the orders: the tier is monotone in the order), the rest of `order`
// -1.  tier_count has f.ragged_tiers entries.  work (five tiers only): the large tier's work table, three rows of
// count + 1 entries -- before slot m of its list the orders (row 0), the panel strips (row 1) and the sweep tiles
// (row 2), the entries past the list repeating the totals.  Any output may be null.
void ragged_plan(const BatchFamily &f, int32_t count, const int32_t *n_each, int64_t *offset, int32_t *order,
                 int32_t *tier_count, int64_t *work = nullptr)
{
    const int ntiers = f.ragged_tiers, wave_max_n = batch_wave_max_n(), mid_min_n = batch_mid_min_n();
    const int large_min_n = batch_large_min_n();
    auto tier_of = [&](int n) {
        return ntiers >= 5 && n >= large_min_n ? 4 : ntiers >= 4 && n >= mid_min_n ? 3 : n <= wave_max_n ? 0 : n <= 64 ? 1 : 2;
    };
    int64_t at[FWX_BATCH_LARGE_MAX_N + 2] = {0};  // at[n]: matrices of order n, then where the next one of order n goes
    int32_t tiers[5] = {0, 0, 0, 0, 0};
    int64_t cells = 0;
    for (int32_t b = 0; b < count; ++b) {
        const int n = n_each[b];
        if (offset) offset[b] = cells;
        cells += (int64_t)n * n;
        if (n >= 1) { ++at[n]; ++tiers[tier_of(n)]; }
    }
    if (offset) offset[count] = cells;
    if (tier_count) std::copy(tiers, tiers + ntiers, tier_count);
    if (work && ntiers >= 5) {                  // the large list is the orders from the limit down, at[n] of each
        int64_t *panel = work, *strip = work + count + 1, *tile = strip + count + 1;
        int64_t m = 0;
        panel[0] = strip[0] = tile[0] = 0;
        for (int64_t n = f.max_n; n >= large_min_n; --n)
            for (int64_t c = 0; c < at[n]; ++c, ++m) {
                panel[m + 1] = panel[m] + n;
                strip[m + 1] = strip[m] + (n + FWX_LARGE_S - 1) / FWX_LARGE_S;
                tile[m + 1] = tile[m] + ((n + FWX_LARGE_TC - 1) / FWX_LARGE_TC) * ((n + FWX_LARGE_TR - 1) / FWX_LARGE_TR);
            }
        for (; m < count; ++m) { panel[m + 1] = panel[m]; strip[m + 1] = strip[m]; tile[m + 1] = tile[m]; }
    }
    if (!order) return;
    int64_t pos = 0;
    for (int tier = 0; tier < ntiers; ++tier)
        for (int n = f.max_n; n >= 1; --n)
            if (tier_of(n) == tier) { const int64_t c = at[n]; at[n] = pos; pos += c; }
    for (int32_t b = 0; b < count; ++b)
        if (n_each[b] >= 1) order[at[n_each[b]]++] = b;
    for (int64_t i = pos; i < count; ++i) order[i] = -1;
}

// fwx_ragged_plan, fwx_ragged_mid_plan and fwx_ragged_large_plan.
int ragged_plan_checked(const BatchFamily &f, int32_t count, const int32_t *n_each, int64_t *offset_out,
                        int32_t *order_out, int32_t *tier_count_out, int64_t *work_out = nullptr)
{
    return guarded([&]() -> int {
        int32_t n_max = 0;
        if (count < 0 || (count > 0 && !n_each) || ragged_orders(count, n_each, n_max)) return FWX_ERR_INVALID;
        if (n_max > f.max_n) return FWX_ERR_UNSUPPORTED;
        ragged_plan(f, count, n_each, offset_out, order_out, tier_count_out, work_out);
        return FWX_OK;
    });
}

// fwx_dev_solve_batch{,_mid,_large} (traced = false; trace, and scratch outside the large family, unused) and their
// _traced forms (traced: next and a complete trace are required and the pivot range is whole, k_begin = 0 and k_end = n
// from the entry point): one contract, the family apart.  The order of the checks is fwx.h's: the arguments and the
// pivot range (FWX_ERR_INVALID), the order against the limit (FWX_ERR_UNSUPPORTED), the scratch where it is used
// (FWX_ERR_INVALID), the device (FWX_ERR_NO_DEVICE).
int dev_solve_uniform(const BatchFamily &f, int32_t count, int32_t n, int32_t dtype, void *rate, int32_t *next,
                      int32_t *hops, int64_t stride, int32_t k_begin, int32_t k_end, bool traced, const fwx_trace *trace,
                      unsigned long long *d_updates_each, void *scratch, size_t scratch_bytes, void *stream)
{
    return guarded([&]() -> int {
        if (count < 0 || n < 0 || (dtype != FWX_F32 && dtype != FWX_F64)) return FWX_ERR_INVALID;
        if (count == 0 || n == 0) return FWX_OK;
        if (!rate || (hops && !next) || stride < (int64_t)n * n) return FWX_ERR_INVALID;
        if (traced && (!next || !trace_complete(trace))) return FWX_ERR_INVALID;
        const int rc = batch_range(f, n, k_begin, k_end);
        if (rc) return rc;
        if (f.needs_scratch(n, k_begin, k_end) && !large_scratch_ok(n, scratch, scratch_bytes)) return FWX_ERR_INVALID;
        if (device_count() <= 0) return FWX_ERR_NO_DEVICE;
        return with_dtype(dtype, rate, [&](auto *r) {
            return run_uniform(f, count, n, r, next, hops, stride, k_begin, k_end, d_updates_each, scratch, scratch_bytes,
                               (hipStream_t)stream, plog_of(traced ? trace : nullptr));
        });
    });
}

// A host work table and scratch the large tier can run `listed` slots of a batch of `count` on (fwx.h).
bool ragged_large_ok(int32_t count, int32_t listed, const RaggedLarge &lg)
{
    if (!lg.work || !lg.d_work) return false;
    const fwx::RaggedLargeWork w(lg.work, (long long)count + 1);
    return fwx::ragged_large_work_ok(w, listed) && large_scratch_ok(w.order_of(0), lg.scratch, lg.scratch_bytes);
}

// fwx_dev_solve_ragged, fwx_dev_solve_ragged_mid and fwx_dev_solve_ragged_large: one contract, the number of tiers
// apart (lg: what the fifth runs on, judged only when it lists a matrix).  The device forms cannot read the orders:
// what they can decide is decided from the host arguments, and the kernels leave a matrix alone whose order does not
// fit the tier it is listed in.
int dev_solve_ragged(const BatchFamily &f, int32_t count, int32_t dtype, void *rate, int32_t *next, int32_t *hops,
                     const int32_t *d_n_each, const int64_t *d_offset, const int32_t *d_order,
                     const int32_t *tier_count, const fwx_trace *trace, unsigned long long *d_updates_each,
                     void *stream, const RaggedLarge &lg = RaggedLarge())
{
    return guarded([&]() -> int {
        if (count < 0 || !tier_count || (dtype != FWX_F32 && dtype != FWX_F64)) return FWX_ERR_INVALID;
        int64_t listed = 0;
        for (int t = 0; t < f.ragged_tiers; ++t) {
            if (tier_count[t] < 0) return FWX_ERR_INVALID;
            listed += tier_count[t];
        }
        if (listed > count) return FWX_ERR_INVALID;
        if (listed == 0) return FWX_OK;
        if (!rate || !d_n_each || !d_offset || !d_order || (hops && !next)) return FWX_ERR_INVALID;
        if (trace && (!next || !trace_complete(trace))) return FWX_ERR_INVALID;
        if (f.ragged_tiers >= 5 && tier_count[4] > 0 && !ragged_large_ok(count, tier_count[4], lg)) return FWX_ERR_INVALID;
        if (device_count() <= 0) return FWX_ERR_NO_DEVICE;
        return with_dtype(dtype, rate, [&](auto *r) {
            return run_ragged(f.ragged_tiers, count, r, next, hops, d_n_each, d_offset, d_order, tier_count,
                              d_updates_each, lg, (hipStream_t)stream, plog_of(trace));
        });
    });
}

// fwx_dev_exact_paths_batch{,_mid,_large}: one walk, the limit apart.
int dev_exact_paths_batch(const BatchFamily &f, int32_t count, int32_t n, int64_t stride, const int32_t *next0,
                          const fwx_trace *trace, int32_t items, const int32_t *mat, const int32_t *src,
                          const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap, int32_t *scratch,
                          void *stream)
{
    return guarded([&]() -> int {
        if (count < 0 || n < 0 || items < 0) return FWX_ERR_INVALID;
        if (count == 0 || n == 0 || items == 0) return FWX_OK;
        if (!next0 || !trace_complete(trace) || stride < (int64_t)n * n || cap < 1 || !mat || !src || !dst ||
            !len_out || !path_out || !scratch)
            return FWX_ERR_INVALID;
        if (n > f.max_n) return FWX_ERR_UNSUPPORTED;
        if (device_count() <= 0) return FWX_ERR_NO_DEVICE;
        return launch_exact_batch(count, n, (long long)stride, next0, plog_of(trace), items, mat, src, dst, len_out,
                                  path_out, cap, scratch, (hipStream_t)stream);
    });
}

// fwx_dev_exact_paths_ragged{,_mid,_large}: the same over a ragged batch, n_max against the limit.
int dev_exact_paths_ragged(const BatchFamily &f, int32_t count, const int32_t *d_n_each, const int64_t *d_offset,
                           int32_t n_max, const int32_t *next0, const fwx_trace *trace, int32_t items,
                           const int32_t *mat, const int32_t *src, const int32_t *dst, int32_t *len_out,
                           int32_t *path_out, int32_t cap, int32_t *scratch, void *stream)
{
    return guarded([&]() -> int {
        if (count < 0 || n_max < 0 || items < 0) return FWX_ERR_INVALID;
        if (count == 0 || n_max == 0 || items == 0) return FWX_OK;
        if (!d_n_each || !d_offset || !next0 || !trace_complete(trace) || cap < 1 || !mat || !src || !dst ||
            !len_out || !path_out || !scratch)
            return FWX_ERR_INVALID;
        if (n_max > f.max_n) return FWX_ERR_UNSUPPORTED;
        if (device_count() <= 0) return FWX_ERR_NO_DEVICE;
        return launch_exact_ragged(count, d_n_each, d_offset, n_max, next0, plog_of(trace), items, mat, src, dst,
                                   len_out, path_out, cap, scratch, (hipStream_t)stream);
    });
}

// What the _lists forms add to a batch solve: the exact lists of `items` triples, host arrays.
struct BatchLists {
    int32_t items;
    const int32_t *mat, *src, *dst;
    int32_t *len_out, *path_out;
    int32_t cap;
};

// Which host form a call is: the family; ragged (fwx_solve_ragged_*: matrix b has order n_each[b] and the batch is
// packed, matrix b at the sum of the squares before it; only families with ragged_tiers != 0); lists (null: none).
struct HostForm {
    BatchFamily family;
    bool ragged;
    const int32_t *n_each;
    const BatchLists *lists;
};

constexpr size_t kBatchLargeScratchCap = (size_t)256 << 20;
static_assert(FWX_BATCH_LARGE_SCRATCH_BYTES(1) % 16 == 0, "what follows the scratch panels stays 16-byte aligned");

// One call of a host form: `count` matrices from / to host arrays, pitch n, no padding (the batch kernels load
// scalars), the arrays of the batch back to back on the device.  run() is the stages in order.  Every reservation of
// the pooled context, each behind its fail_point(), lies in reserve_and_upload, and nothing of the caller's is
// written before the last of them.
template <typename T> struct HostCall {
    const HostForm &form;
    int32_t count, n;                  // ragged: n becomes the largest order (the walk's stacks and chunks go by it)
    T *rate;
    int32_t *next, *hops;
    uint64_t *updates_each;
    const BatchLists *const ls = form.lists;

    Opts op{};
    DeviceGuard g{};
    CtxLease lease{};
    hipStream_t s = nullptr;
    size_t cells = 0;
    // rate, next, hops (CallCtx::RATE + f): the caller's array (null: not given), its copy on the device and, while the
    // whole batch fits the pinned staging (see solve_host), in there
    struct Field { void *host; size_t bytes; void *dev; char *stage; } fld[3] = {};
    bool staged = false;
    // ragged: the plan, packed for one copy -- count offsets, then count orders and the tier list (count) as int32,
    // then, with five tiers, the large tier's work table -- and where it lies in the context's workspace, behind the
    // counters
    std::vector<int64_t> plan{};
    int32_t tiers[5] = {0, 0, 0, 0, 0};
    size_t work_at = 0;                // of the work table in `plan`, in entries
    const int64_t *d_work = nullptr;
    const int64_t *d_offset = nullptr;
    const int32_t *d_n_each = nullptr, *d_order = nullptr;
    bool counting = false;
    std::vector<unsigned long long> h_upd{};
    unsigned long long *d_upd = nullptr;
    void *d_scratch = nullptr;
    size_t b_scratch = 0;
    // lists: the unsolved next-hops and the trace, then the walk's memory for one chunk of items
    fwx::PathLog plog{};
    int32_t *d_next0 = nullptr, *d_walk = nullptr;
    long long chunk = 0;

    // 1. What is decided before any device call, in fwx.h's order; FWX_OK with done set: nothing to do.
    int validate(const fwx_opts *o, bool &done)
    {
        const bool ragged = form.ragged;
        done = true;
        if (count < 0 || (!ragged && n < 0) || (ls && ls->items < 0)) return FWX_ERR_INVALID;
        if (count == 0 || (!ragged && n == 0)) return FWX_OK;
        if (ragged) {
            if (!form.n_each || ragged_orders(count, form.n_each, n)) return FWX_ERR_INVALID;
            if (n == 0) return FWX_OK;
        }
        if (!rate || (hops && !next)) return FWX_ERR_INVALID;
        if (ls && (!next || (ls->items > 0 && (ls->cap < 1 || !ls->mat || !ls->src || !ls->dst || !ls->len_out ||
                                               !ls->path_out))))
            return FWX_ERR_INVALID;
        int rc = read_opts(o, n, op);
        if (rc) return rc;
        if (ls && (op.k_begin != 0 || op.k_end != n)) return FWX_ERR_INVALID;      // the trace covers whole solves only
        if (ragged && o && (o->k_begin != 0 || o->k_end > 0)) return FWX_ERR_INVALID;   // one range does not fit all orders
        if ((rc = batch_range(form.family, n, op.k_begin, op.k_end))) return rc;
        if (op.engine != FWX_ENGINE_AUTO) return FWX_ERR_UNSUPPORTED;
        done = false;
        return FWX_OK;
    }

    // 2. The cells of the batch and, ragged, the plan.
    void plan_batch()
    {
        cells = (size_t)count * (size_t)n * (size_t)n;
        if (!form.ragged) return;
        std::vector<int64_t> offs((size_t)count + 1);
        const bool five = form.family.ragged_tiers >= 5;
        work_at = 2 * (size_t)count;
        plan.resize(work_at + (five ? FWX_RAGGED_LARGE_WORK_ENTRIES(count) : 0));
        int32_t *h_n = (int32_t *)(plan.data() + count), *h_order = h_n + count;
        ragged_plan(form.family, count, form.n_each, offs.data(), h_order, tiers, five ? plan.data() + work_at : nullptr);
        std::copy(offs.begin(), offs.end() - 1, plan.begin());
        std::copy(form.n_each, form.n_each + count, h_n);
        cells = (size_t)offs[(size_t)count];
    }

    // 3. The context's buffers and the input on its way to them.
    int reserve_and_upload()
    {
        int rc;
        if ((rc = lease.open())) return rc;
        CallCtx &cx = *lease.c;
        if (op.has_stream) cx.uses_stream(op.stream);
        s = op.has_stream ? op.stream : cx.s;
        fld[0] = {rate, cells * sizeof(T), nullptr, nullptr};
        fld[1] = {next, cells * sizeof(int32_t), nullptr, nullptr};
        fld[2] = {hops, cells * sizeof(int32_t), nullptr, nullptr};
        size_t b_total = 0;
        for (int f = 0; f < 3; ++f) {                // a point for each of the three, given or not
            fail_point();
            if (!fld[f].host) continue;
            if ((rc = cx.reserve(CallCtx::RATE + f, fld[f].bytes, &fld[f].dev))) return rc;
            b_total += fld[f].bytes;
        }
        const size_t b_upd = counting ? (size_t)count * sizeof(unsigned long long) : 0;
        if (counting || form.ragged) {               // one counter per matrix, then the plan: the context's workspace
            fail_point();
            void *ws = nullptr;
            if ((rc = cx.reserve(CallCtx::WS, b_upd + plan.size() * sizeof(int64_t), &ws))) return rc;
            if (counting) {
                h_upd.resize((size_t)count);
                d_upd = (unsigned long long *)ws;
                FWX_HIP(hipMemsetAsync(d_upd, 0, b_upd, s));
            }
            if (form.ragged) {
                d_offset = (const int64_t *)((char *)ws + b_upd);
                d_n_each = (const int32_t *)(d_offset + count);
                d_order = d_n_each + count;
                d_work = d_offset + work_at;
                FWX_HIP(hipMemcpyAsync((void *)d_offset, plan.data(), plan.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
            }
        }
        staged = b_total <= CallCtx::kStageBytes;    // straight copies above that
        if (staged) {
            void *pinned = nullptr;
            fail_point();
            if ((rc = cx.reserve_pinned(b_total, &pinned))) return rc;
            char *at = (char *)pinned;
            for (Field &a : fld)
                if (a.host) { a.stage = at; at += a.bytes; memcpy(a.stage, a.host, a.bytes); }
        }
        for (const Field &a : fld)
            if (a.host) FWX_HIP(hipMemcpyAsync(a.dev, staged ? a.stage : a.host, a.bytes, hipMemcpyHostToDevice, s));

        // the context's SMALL buffer, ONE reservation: the large tier's scratch panels first -- at most
        // kBatchLargeScratchCap, larger batches run in groups; the buffer's own alignment, and every matrix's part a
        // multiple of 16 bytes -- then, with lists, the unsolved next-hops, the three trace arrays and the walk's
        // memory for one chunk of items (triples and lengths, lists, stacks)
        // (ragged: the panels of every slot of the large tier -- there is one iff the largest order is routed there)
        const size_t per_large = FWX_BATCH_LARGE_SCRATCH_BYTES((size_t)n);
        if (form.family.needs_scratch(n, op.k_begin, op.k_end))
            b_scratch = form.ragged
                ? std::min(FWX_BATCH_LARGE_SCRATCH_BYTES((size_t)plan[work_at + (size_t)tiers[4]]),
                           std::max(per_large, kBatchLargeScratchCap))
                : per_large * std::min<size_t>((size_t)count, std::max<size_t>(1, kBatchLargeScratchCap / per_large));
        if (ls) {
            void *p = nullptr;
            chunk = std::min<long long>(batch_lists_chunk(n, ls->cap), ls->items);
            const size_t walk_ints = (size_t)chunk * (4 + (size_t)ls->cap + FWX_EXACT_SCRATCH_INTS((size_t)n));
            fail_point();
            if ((rc = cx.reserve(CallCtx::SMALL, b_scratch + (4 * cells + walk_ints) * sizeof(int32_t), &p))) return rc;
            if (b_scratch) d_scratch = p;
            d_next0 = (int32_t *)((char *)p + b_scratch);
            plog.last = d_next0 + cells;
            plog.at_col = plog.last + cells;
            plog.at_row = plog.at_col + cells;
            d_walk = plog.at_row + cells;
            FWX_HIP(hipMemcpyAsync(d_next0, fld[1].dev, fld[1].bytes, hipMemcpyDeviceToDevice, s));
        } else if (form.family.tier(n) == TIER_LARGE) {     // a point of its own, scratch or none (an empty pivot range)
            fail_point();
            if (b_scratch && (rc = cx.reserve(CallCtx::SMALL, b_scratch, &d_scratch))) return rc;
        }
        return FWX_OK;
    }

    // 4. The solve, queued.
    int solve()
    {
        T *r = (T *)fld[0].dev;
        int32_t *x = (int32_t *)fld[1].dev, *h = (int32_t *)fld[2].dev;
        if (form.ragged) {
            RaggedLarge lg;
            if (tiers[4] > 0) lg = {plan.data() + work_at, d_work, d_scratch, b_scratch};
            return run_ragged(form.family.ragged_tiers, count, r, x, h, d_n_each, d_offset, d_order, tiers, d_upd, lg, s,
                              plog);
        }
        return run_uniform(form.family, count, n, r, x, h, (int64_t)n * n, op.k_begin, op.k_end, d_upd, d_scratch,
                           b_scratch, s, plog);
    }

    // 5. The results on their way back (queued before the walk, which reads none of them), then the lists,
    //    batch_lists_chunk items per launch.
    int download_and_walk()
    {
        for (const Field &a : fld)
            if (a.host) FWX_HIP(hipMemcpyAsync(staged ? a.stage : a.host, a.dev, a.bytes, hipMemcpyDeviceToHost, s));
        if (counting)
            FWX_HIP(hipMemcpyAsync(h_upd.data(), d_upd, (size_t)count * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        for (long long q0 = 0; ls && q0 < ls->items; q0 += chunk) {
            const size_t c = (size_t)std::min<long long>(chunk, ls->items - q0), cap = (size_t)ls->cap;
            int32_t *d_mat = d_walk, *d_src = d_mat + c, *d_dst = d_src + c, *d_len = d_dst + c, *d_paths = d_len + c,
                    *d_stacks = d_paths + c * cap;
            FWX_HIP(hipMemcpyAsync(d_mat, ls->mat + q0, c * 4, hipMemcpyHostToDevice, s));
            FWX_HIP(hipMemcpyAsync(d_src, ls->src + q0, c * 4, hipMemcpyHostToDevice, s));
            FWX_HIP(hipMemcpyAsync(d_dst, ls->dst + q0, c * 4, hipMemcpyHostToDevice, s));
            const int rc = form.ragged
                ? launch_exact_ragged(count, d_n_each, d_offset, n, d_next0, plog, (int)c, d_mat, d_src, d_dst, d_len,
                                      d_paths, ls->cap, d_stacks, s)
                : launch_exact_batch(count, n, (long long)n * n, d_next0, plog, (int)c, d_mat, d_src, d_dst, d_len,
                                     d_paths, ls->cap, d_stacks, s);
            if (rc) return rc;
            FWX_HIP(hipMemcpyAsync(ls->len_out + q0, d_len, c * 4, hipMemcpyDeviceToHost, s));
            FWX_HIP(hipMemcpyAsync(ls->path_out + (size_t)q0 * cap, d_paths, c * cap * 4, hipMemcpyDeviceToHost, s));
        }
        return FWX_OK;
    }

    // 6. Everything has arrived: the caller's arrays out of the staging, the counters.
    int finish()
    {
        FWX_HIP(hipStreamSynchronize(s));
        for (const Field &a : fld)
            if (staged && a.host) memcpy(a.host, a.stage, a.bytes);
        uint64_t sum = 0;
        for (int32_t b = 0; counting && b < count; ++b) {
            sum += h_upd[(size_t)b];
            if (updates_each) updates_each[b] = h_upd[(size_t)b];
        }
        if (op.updates_out) *op.updates_out = sum;
        return FWX_OK;
    }

    int run(const fwx_opts *o)
    {
        bool done = false;
        int rc = validate(o, done);
        if (rc || done) return rc;
        if ((rc = g.enter(op.device))) return rc;
        plan_batch();
        counting = updates_each || op.updates_out;
        if ((rc = reserve_and_upload())) return rc;
        if ((rc = solve())) return rc;
        if ((rc = download_and_walk())) return rc;
        return finish();
    }
};

template <typename T>
int solve_batch_host(const HostForm &form, int32_t count, int32_t n, T *rate, int32_t *next, int32_t *hops,
                     uint64_t *updates_each, const fwx_opts *o)
{
    return guarded([&]() -> int { return HostCall<T>{form, count, n, rate, next, hops, updates_each}.run(o); });
}

// ---- what-if sweeps ---------------------------------------------------------------------------------------------------

// Workgroups (= workspace slots) of a mid-tier sweep: FWX_SWEEP_MID_SLOTS, environment, read once per call: digits
// only, >= 1, anything else means the default -- two 1024-thread workgroups on each of the 256 CUs, the most that can
// be resident.  No result bit depends on it.
#define FWX_SWEEP_MID_SLOTS_DEFAULT 512
int sweep_mid_slots(int32_t count, int32_t n, size_t scratch_bytes)
{
    if (count <= 0 || n <= 0) return 0;
    const long long cap = env_digits("FWX_SWEEP_MID_SLOTS", 1, INT32_MAX, FWX_SWEEP_MID_SLOTS_DEFAULT);
    const size_t fit = scratch_bytes / FWX_SWEEP_MID_SCRATCH_BYTES((size_t)n);
    return (int)std::min<unsigned long long>({(unsigned long long)count, (unsigned long long)fit, (unsigned long long)cap});
}

// Where a sweep of order n runs and what it needs there.  `limit` is the family's largest order; a family with the
// mid tier (limit FWX_SWEEP_MID_MAX_N) routes by FWX_BATCH_MID_MIN_N as fwx_solve_batch_mid_*, read once here.
struct SweepRoute {
    bool mid;
    SweepRoute(int32_t limit, int32_t n) : mid(limit > FWX_SWEEP_MAX_N && n >= batch_mid_min_n()) {}
    // the launcher of the tier: scratch and slots are the mid tier's and unused otherwise
    template <typename T>
    hipError_t launch(const T *rate, const int32_t *next, const int32_t *hops, int32_t count, int32_t n,
                      const fwx::SweepTables<T> &t, unsigned long long *d_updates_each, void *scratch, int slots,
                      hipStream_t s) const
    {
        return mid ? fwx::launch_sweep_mid<T>(rate, next, hops, count, n, t, d_updates_each, scratch, slots, s)
                   : fwx::launch_sweep_solve<T>(rate, next, hops, count, n, t, d_updates_each, batch_wave_max_n(), s);
    }
};

// What both sweep forms decide from their host arguments, in fwx.h's order (the dtype is the caller's; limit: the
// family's largest order); FWX_OK with done set: nothing to do.
int sweep_args(int32_t limit, int32_t count, int32_t n, const void *base_rate, const int32_t *base_next,
               const int32_t *base_hops, const fwx_sweep_patches *p, const fwx_sweep_items *it, const fwx_sweep_full *fu,
               bool &done)
{
    done = true;
    if (count < 0 || n < 0) return FWX_ERR_INVALID;
    if (count == 0 || n == 0) return FWX_OK;
    if (!base_rate || (base_hops && !base_next)) return FWX_ERR_INVALID;
    if (p) {
        if ((p->next && !base_next) || (p->hops && !base_hops) || p->total < 0) return FWX_ERR_INVALID;
        if (p->total > 0 && (!p->ptr || !p->index || !p->rate)) return FWX_ERR_INVALID;
    }
    if (it) {
        if ((it->next_out && !base_next) || (it->hops_out && !base_hops) || it->total < 0) return FWX_ERR_INVALID;
        if (it->total > 0 && (!it->ptr || !it->src || !it->dst || !it->rate_out)) return FWX_ERR_INVALID;
    }
    if (fu) {
        if ((fu->next && !base_next) || (fu->hops && !base_hops)) return FWX_ERR_INVALID;
        if ((fu->rate || fu->next || fu->hops) && fu->stride < (int64_t)n * n) return FWX_ERR_INVALID;
    }
    if (n > limit) return FWX_ERR_UNSUPPORTED;
    done = false;
    return FWX_OK;
}

// The launcher's tables from the ABI's structs (any may be null), rates as T.
template <typename T>
fwx::SweepTables<T> sweep_tables(const fwx_sweep_patches *p, const fwx_sweep_items *it, const fwx_sweep_full *fu)
{
    fwx::SweepTables<T> t;
    if (p && p->total > 0) {
        t.patch_ptr = p->ptr;
        t.patch_total = p->total;
        t.patch_index = p->index;
        t.patch_rate = (const T *)p->rate;
        t.patch_next = p->next;
        t.patch_hops = p->hops;
    }
    if (it && it->total > 0) {
        t.item_ptr = it->ptr;
        t.item_total = it->total;
        t.item_src = it->src;
        t.item_dst = it->dst;
        t.item_rate = (T *)it->rate_out;
        t.item_next = it->next_out;
        t.item_hops = it->hops_out;
    }
    if (fu) {
        t.full_rate = (T *)fu->rate;
        t.full_next = fu->next;
        t.full_hops = fu->hops;
        t.full_stride = fu->stride;
    }
    return t;
}

// A host table the kernels would have to defend against: ptr[0] != 0, a descending ptr, ptr[count] != total.
bool sweep_ptr_ok(const int64_t *ptr, int32_t count, int64_t total)
{
    if (ptr[0] != 0 || ptr[count] != total) return false;
    for (int32_t b = 0; b < count; ++b)
        if (ptr[b + 1] < ptr[b]) return false;
    return true;
}

// fwx_solve_sweep_*: the base, the patch arrays and the item arrays go up once into ONE reservation of the pooled
// context, the item outputs and the counters come down.  Nothing of the caller's is written before the reservation.
// limit: the family's largest order (fwx_solve_sweep_*: FWX_SWEEP_MAX_N, fwx_solve_sweep_mid_*: FWX_SWEEP_MID_MAX_N);
// a call routed to the mid tier takes its slots from the context's SMALL buffer, as many as fit under
// kBatchLargeScratchCap (one at least), capped by sweep_mid_slots' rule.
template <typename T>
int solve_sweep_host(int32_t limit, int32_t count, int32_t n, const T *base_rate, const int32_t *base_next,
                     const int32_t *base_hops, const fwx_sweep_patches *p, const fwx_sweep_items *it,
                     uint64_t *updates_each, const fwx_opts *o)
{
    return guarded([&]() -> int {
        bool done = false;
        int rc = sweep_args(limit, count, n, base_rate, base_next, base_hops, p, it, nullptr, done);
        if (rc || done) return rc;
        const SweepRoute route(limit, n);
        Opts op{};
        if ((rc = read_opts(o, n, op))) return rc;
        if (op.k_begin != 0 || op.k_end != n) return FWX_ERR_INVALID;
        if (op.engine != FWX_ENGINE_AUTO) return FWX_ERR_UNSUPPORTED;
        const int64_t np = p ? p->total : 0, ni = it ? it->total : 0, cells = (int64_t)n * n;
        if (np > 0) {
            if (!sweep_ptr_ok(p->ptr, count, np)) return FWX_ERR_INVALID;
            for (int64_t q = 0; q < np; ++q)
                if (p->index[q] < 0 || p->index[q] >= cells) return FWX_ERR_INVALID;
        }
        if (ni > 0) {
            if (!sweep_ptr_ok(it->ptr, count, ni)) return FWX_ERR_INVALID;
            for (int64_t q = 0; q < ni; ++q)
                if (it->src[q] < 0 || it->src[q] >= n || it->dst[q] < 0 || it->dst[q] >= n) return FWX_ERR_INVALID;
        }
        DeviceGuard g{};
        if ((rc = g.enter(op.device))) return rc;
        CtxLease lease{};
        if ((rc = lease.open())) return rc;
        CallCtx &cx = *lease.c;
        if (op.has_stream) cx.uses_stream(op.stream);
        hipStream_t s = op.has_stream ? op.stream : cx.s;

        // the pieces of the reservation, each 16-byte aligned: inputs (host != null: copied up), outputs, counters
        struct Piece { const void *host; size_t bytes; char *dev; };
        const size_t ptr_bytes = ((size_t)count + 1) * sizeof(int64_t);
        const bool counting = updates_each || op.updates_out;
        enum { BR, BN, BH, PP, PI, PR, PN, PH, IP, IS, ID, OR, ON, OH, UP, NPIECE };
        Piece pc[NPIECE] = {};
        pc[BR] = {base_rate, (size_t)cells * sizeof(T), nullptr};
        pc[BN] = {base_next, base_next ? (size_t)cells * 4 : 0, nullptr};
        pc[BH] = {base_hops, base_hops ? (size_t)cells * 4 : 0, nullptr};
        if (np > 0) {
            pc[PP] = {p->ptr, ptr_bytes, nullptr};
            pc[PI] = {p->index, (size_t)np * sizeof(int64_t), nullptr};
            pc[PR] = {p->rate, (size_t)np * sizeof(T), nullptr};
            pc[PN] = {p->next, p->next ? (size_t)np * 4 : 0, nullptr};
            pc[PH] = {p->hops, p->hops ? (size_t)np * 4 : 0, nullptr};
        }
        if (ni > 0) {
            pc[IP] = {it->ptr, ptr_bytes, nullptr};
            pc[IS] = {it->src, (size_t)ni * 4, nullptr};
            pc[ID] = {it->dst, (size_t)ni * 4, nullptr};
            pc[OR] = {nullptr, (size_t)ni * sizeof(T), nullptr};
            pc[ON] = {nullptr, it->next_out ? (size_t)ni * 4 : 0, nullptr};
            pc[OH] = {nullptr, it->hops_out ? (size_t)ni * 4 : 0, nullptr};
        }
        pc[UP] = {nullptr, counting ? (size_t)count * sizeof(unsigned long long) : 0, nullptr};
        size_t total = 0;
        for (Piece &a : pc) total += (a.bytes + 15) & ~(size_t)15;
        void *buf = nullptr;
        fail_point();
        if ((rc = cx.reserve(CallCtx::RATE, total, &buf))) return rc;
        void *d_scratch = nullptr;             // mid tier: the slots, a reservation (and a point) of their own
        int slots = 0;
        if (route.mid) {
            const size_t per_slot = FWX_SWEEP_MID_SCRATCH_BYTES((size_t)n);
            slots = sweep_mid_slots(count, n, std::max(per_slot, kBatchLargeScratchCap));
            fail_point();
            if ((rc = cx.reserve(CallCtx::SMALL, (size_t)slots * per_slot, &d_scratch))) return rc;
        }
        char *at = (char *)buf;
        for (Piece &a : pc) {
            if (!a.bytes) continue;
            a.dev = at;
            at += (a.bytes + 15) & ~(size_t)15;
            if (a.host) FWX_HIP(hipMemcpyAsync(a.dev, a.host, a.bytes, hipMemcpyHostToDevice, s));
        }
        if (counting) FWX_HIP(hipMemsetAsync(pc[UP].dev, 0, pc[UP].bytes, s));
        // the tables passed the checks above, so every item's outputs are written by its variant

        fwx::SweepTables<T> t;
        if (np > 0) {
            t.patch_ptr = (const int64_t *)pc[PP].dev;
            t.patch_total = np;
            t.patch_index = (const int64_t *)pc[PI].dev;
            t.patch_rate = (const T *)pc[PR].dev;
            t.patch_next = (const int32_t *)pc[PN].dev;
            t.patch_hops = (const int32_t *)pc[PH].dev;
        }
        if (ni > 0) {
            t.item_ptr = (const int64_t *)pc[IP].dev;
            t.item_total = ni;
            t.item_src = (const int32_t *)pc[IS].dev;
            t.item_dst = (const int32_t *)pc[ID].dev;
            t.item_rate = (T *)pc[OR].dev;
            t.item_next = (int32_t *)pc[ON].dev;
            t.item_hops = (int32_t *)pc[OH].dev;
        }
        if ((rc = launch_status(route.launch<T>((const T *)pc[BR].dev, (const int32_t *)pc[BN].dev,
                                                (const int32_t *)pc[BH].dev, count, n, t,
                                                (unsigned long long *)pc[UP].dev, d_scratch, slots, s))))
            return rc;
        std::vector<unsigned long long> h_upd(counting ? (size_t)count : 0);
        if (ni > 0) {
            FWX_HIP(hipMemcpyAsync(it->rate_out, pc[OR].dev, pc[OR].bytes, hipMemcpyDeviceToHost, s));
            if (it->next_out) FWX_HIP(hipMemcpyAsync(it->next_out, pc[ON].dev, pc[ON].bytes, hipMemcpyDeviceToHost, s));
            if (it->hops_out) FWX_HIP(hipMemcpyAsync(it->hops_out, pc[OH].dev, pc[OH].bytes, hipMemcpyDeviceToHost, s));
        }
        if (counting) FWX_HIP(hipMemcpyAsync(h_upd.data(), pc[UP].dev, pc[UP].bytes, hipMemcpyDeviceToHost, s));
        FWX_HIP(hipStreamSynchronize(s));
        uint64_t sum = 0;
        for (int32_t b = 0; counting && b < count; ++b) {
            sum += h_upd[(size_t)b];
            if (updates_each) updates_each[b] = h_upd[(size_t)b];
        }
        if (op.updates_out) *op.updates_out = sum;
        return FWX_OK;
    });
}

// fwx_dev_solve_sweep (limit FWX_SWEEP_MAX_N; scratch unused) and fwx_dev_solve_sweep_mid: one contract, the limit
// apart.  The order of the checks is fwx.h's: the dtype and the arguments (FWX_ERR_INVALID), the order against the limit
// (FWX_ERR_UNSUPPORTED), the scratch where the call is routed to the mid tier (FWX_ERR_INVALID), the device.
int dev_solve_sweep(int32_t limit, int32_t count, int32_t n, int32_t dtype, const void *base_rate,
                    const int32_t *base_next, const int32_t *base_hops, const fwx_sweep_patches *patches,
                    const fwx_sweep_items *items, const fwx_sweep_full *full, unsigned long long *d_updates_each,
                    void *scratch, size_t scratch_bytes, void *stream)
{
    return guarded([&]() -> int {
        if (dtype != FWX_F32 && dtype != FWX_F64) return FWX_ERR_INVALID;
        bool done = false;
        const int rc = sweep_args(limit, count, n, base_rate, base_next, base_hops, patches, items, full, done);
        if (rc || done) return rc;
        const SweepRoute route(limit, n);
        int slots = 0;
        if (route.mid) {
            if (!scratch || ((uintptr_t)scratch & 15) || scratch_bytes < FWX_SWEEP_MID_SCRATCH_BYTES((size_t)n))
                return FWX_ERR_INVALID;
            slots = sweep_mid_slots(count, n, scratch_bytes);
        }
        if (device_count() <= 0) return FWX_ERR_NO_DEVICE;
        return with_dtype(dtype, (void *)base_rate, [&](auto *r) {
            using T = std::remove_pointer_t<decltype(r)>;
            return launch_status(route.launch<T>(r, base_next, base_hops, count, n, sweep_tables<T>(patches, items, full),
                                                 d_updates_each, scratch, slots, (hipStream_t)stream));
        });
    });
}

}  // namespace

extern "C" {

// ---- what-if sweeps ---------------------------------------------------------------------------------------------------

int fwx_dev_solve_sweep(int32_t count, int32_t n, int32_t dtype, const void *base_rate, const int32_t *base_next,
                        const int32_t *base_hops, const fwx_sweep_patches *patches, const fwx_sweep_items *items,
                        const fwx_sweep_full *full, unsigned long long *d_updates_each, void *stream)
{
    return dev_solve_sweep(FWX_SWEEP_MAX_N, count, n, dtype, base_rate, base_next, base_hops, patches, items, full,
                           d_updates_each, nullptr, 0, stream);
}

int fwx_solve_sweep_f64(int32_t count, int32_t n, const double *base_rate, const int32_t *base_next,
                        const int32_t *base_hops, const fwx_sweep_patches *patches, const fwx_sweep_items *items,
                        uint64_t *updates_each, const fwx_opts *opts)
{
    return solve_sweep_host<double>(FWX_SWEEP_MAX_N, count, n, base_rate, base_next, base_hops, patches, items,
                                    updates_each, opts);
}

int fwx_solve_sweep_f32(int32_t count, int32_t n, const float *base_rate, const int32_t *base_next,
                        const int32_t *base_hops, const fwx_sweep_patches *patches, const fwx_sweep_items *items,
                        uint64_t *updates_each, const fwx_opts *opts)
{
    return solve_sweep_host<float>(FWX_SWEEP_MAX_N, count, n, base_rate, base_next, base_hops, patches, items,
                                   updates_each, opts);
}

int fwx_dev_solve_sweep_mid(int32_t count, int32_t n, int32_t dtype, const void *base_rate, const int32_t *base_next,
                            const int32_t *base_hops, const fwx_sweep_patches *patches, const fwx_sweep_items *items,
                            const fwx_sweep_full *full, unsigned long long *d_updates_each, void *scratch,
                            size_t scratch_bytes, void *stream)
{
    return dev_solve_sweep(FWX_SWEEP_MID_MAX_N, count, n, dtype, base_rate, base_next, base_hops, patches, items, full,
                           d_updates_each, scratch, scratch_bytes, stream);
}

int fwx_solve_sweep_mid_f64(int32_t count, int32_t n, const double *base_rate, const int32_t *base_next,
                            const int32_t *base_hops, const fwx_sweep_patches *patches, const fwx_sweep_items *items,
                            uint64_t *updates_each, const fwx_opts *opts)
{
    return solve_sweep_host<double>(FWX_SWEEP_MID_MAX_N, count, n, base_rate, base_next, base_hops, patches, items,
                                    updates_each, opts);
}

int fwx_solve_sweep_mid_f32(int32_t count, int32_t n, const float *base_rate, const int32_t *base_next,
                            const int32_t *base_hops, const fwx_sweep_patches *patches, const fwx_sweep_items *items,
                            uint64_t *updates_each, const fwx_opts *opts)
{
    return solve_sweep_host<float>(FWX_SWEEP_MID_MAX_N, count, n, base_rate, base_next, base_hops, patches, items,
                                   updates_each, opts);
}

// ---- uniform batches: host forms ----------------------------------------------------------------------------------

int fwx_solve_batch_f64(int32_t count, int32_t n, double *rate, int32_t *next, int32_t *hops,
                        uint64_t *updates_each, const fwx_opts *opts)
{
    return solve_batch_host<double>({kPlain, false, nullptr, nullptr}, count, n, rate, next, hops, updates_each, opts);
}

int fwx_solve_batch_f32(int32_t count, int32_t n, float *rate, int32_t *next, int32_t *hops,
                        uint64_t *updates_each, const fwx_opts *opts)
{
    return solve_batch_host<float>({kPlain, false, nullptr, nullptr}, count, n, rate, next, hops, updates_each, opts);
}

int fwx_solve_batch_mid_f64(int32_t count, int32_t n, double *rate, int32_t *next, int32_t *hops,
                            uint64_t *updates_each, const fwx_opts *opts)
{
    return solve_batch_host<double>({kMid, false, nullptr, nullptr}, count, n, rate, next, hops, updates_each, opts);
}

int fwx_solve_batch_mid_f32(int32_t count, int32_t n, float *rate, int32_t *next, int32_t *hops,
                            uint64_t *updates_each, const fwx_opts *opts)
{
    return solve_batch_host<float>({kMid, false, nullptr, nullptr}, count, n, rate, next, hops, updates_each, opts);
}

int fwx_solve_batch_large_f64(int32_t count, int32_t n, double *rate, int32_t *next, int32_t *hops,
                              uint64_t *updates_each, const fwx_opts *opts)
{
    return solve_batch_host<double>({kLarge, false, nullptr, nullptr}, count, n, rate, next, hops, updates_each, opts);
}

int fwx_solve_batch_large_f32(int32_t count, int32_t n, float *rate, int32_t *next, int32_t *hops,
                              uint64_t *updates_each, const fwx_opts *opts)
{
    return solve_batch_host<float>({kLarge, false, nullptr, nullptr}, count, n, rate, next, hops, updates_each, opts);
}

int fwx_solve_batch_lists_f64(int32_t count, int32_t n, double *rate, int32_t *next, int32_t *hops,
                              uint64_t *updates_each, int32_t items, const int32_t *mat, const int32_t *src,
                              const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap,
                              const fwx_opts *opts)
{
    const BatchLists ls = {items, mat, src, dst, len_out, path_out, cap};
    return solve_batch_host<double>({kPlain, false, nullptr, &ls}, count, n, rate, next, hops, updates_each, opts);
}

int fwx_solve_batch_lists_f32(int32_t count, int32_t n, float *rate, int32_t *next, int32_t *hops,
                              uint64_t *updates_each, int32_t items, const int32_t *mat, const int32_t *src,
                              const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap,
                              const fwx_opts *opts)
{
    const BatchLists ls = {items, mat, src, dst, len_out, path_out, cap};
    return solve_batch_host<float>({kPlain, false, nullptr, &ls}, count, n, rate, next, hops, updates_each, opts);
}

int fwx_solve_batch_mid_lists_f64(int32_t count, int32_t n, double *rate, int32_t *next, int32_t *hops,
                                  uint64_t *updates_each, int32_t items, const int32_t *mat, const int32_t *src,
                                  const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap,
                                  const fwx_opts *opts)
{
    const BatchLists ls = {items, mat, src, dst, len_out, path_out, cap};
    return solve_batch_host<double>({kMid, false, nullptr, &ls}, count, n, rate, next, hops, updates_each, opts);
}

int fwx_solve_batch_mid_lists_f32(int32_t count, int32_t n, float *rate, int32_t *next, int32_t *hops,
                                  uint64_t *updates_each, int32_t items, const int32_t *mat, const int32_t *src,
                                  const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap,
                                  const fwx_opts *opts)
{
    const BatchLists ls = {items, mat, src, dst, len_out, path_out, cap};
    return solve_batch_host<float>({kMid, false, nullptr, &ls}, count, n, rate, next, hops, updates_each, opts);
}

int fwx_solve_batch_large_lists_f64(int32_t count, int32_t n, double *rate, int32_t *next, int32_t *hops,
                                    uint64_t *updates_each, int32_t items, const int32_t *mat, const int32_t *src,
                                    const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap,
                                    const fwx_opts *opts)
{
    const BatchLists ls = {items, mat, src, dst, len_out, path_out, cap};
    return solve_batch_host<double>({kLarge, false, nullptr, &ls}, count, n, rate, next, hops, updates_each, opts);
}

int fwx_solve_batch_large_lists_f32(int32_t count, int32_t n, float *rate, int32_t *next, int32_t *hops,
                                    uint64_t *updates_each, int32_t items, const int32_t *mat, const int32_t *src,
                                    const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap,
                                    const fwx_opts *opts)
{
    const BatchLists ls = {items, mat, src, dst, len_out, path_out, cap};
    return solve_batch_host<float>({kLarge, false, nullptr, &ls}, count, n, rate, next, hops, updates_each, opts);
}

// ---- uniform batches: device forms --------------------------------------------------------------------------------

int fwx_dev_solve_batch(int32_t count, int32_t n, int32_t dtype, void *rate, int32_t *next, int32_t *hops,
                        int64_t stride, int32_t k_begin, int32_t k_end, unsigned long long *d_updates_each,
                        void *stream)
{
    return dev_solve_uniform(kPlain, count, n, dtype, rate, next, hops, stride, k_begin, k_end, false, nullptr,
                             d_updates_each, nullptr, 0, stream);
}

int fwx_dev_solve_batch_mid(int32_t count, int32_t n, int32_t dtype, void *rate, int32_t *next, int32_t *hops,
                            int64_t stride, int32_t k_begin, int32_t k_end, unsigned long long *d_updates_each,
                            void *stream)
{
    return dev_solve_uniform(kMid, count, n, dtype, rate, next, hops, stride, k_begin, k_end, false, nullptr,
                             d_updates_each, nullptr, 0, stream);
}

int fwx_dev_solve_batch_large(int32_t count, int32_t n, int32_t dtype, void *rate, int32_t *next, int32_t *hops,
                              int64_t stride, int32_t k_begin, int32_t k_end, unsigned long long *d_updates_each,
                              void *scratch, size_t scratch_bytes, void *stream)
{
    return dev_solve_uniform(kLarge, count, n, dtype, rate, next, hops, stride, k_begin, k_end, false, nullptr,
                             d_updates_each, scratch, scratch_bytes, stream);
}

int fwx_dev_solve_batch_traced(int32_t count, int32_t n, int32_t dtype, void *rate, int32_t *next, int32_t *hops,
                               int64_t stride, const fwx_trace *trace, unsigned long long *d_updates_each,
                               void *stream)
{
    return dev_solve_uniform(kPlain, count, n, dtype, rate, next, hops, stride, 0, n, true, trace, d_updates_each,
                             nullptr, 0, stream);
}

int fwx_dev_solve_batch_mid_traced(int32_t count, int32_t n, int32_t dtype, void *rate, int32_t *next, int32_t *hops,
                                   int64_t stride, const fwx_trace *trace, unsigned long long *d_updates_each,
                                   void *stream)
{
    return dev_solve_uniform(kMid, count, n, dtype, rate, next, hops, stride, 0, n, true, trace, d_updates_each,
                             nullptr, 0, stream);
}

int fwx_dev_solve_batch_large_traced(int32_t count, int32_t n, int32_t dtype, void *rate, int32_t *next, int32_t *hops,
                                     int64_t stride, const fwx_trace *trace, unsigned long long *d_updates_each,
                                     void *scratch, size_t scratch_bytes, void *stream)
{
    return dev_solve_uniform(kLarge, count, n, dtype, rate, next, hops, stride, 0, n, true, trace, d_updates_each,
                             scratch, scratch_bytes, stream);
}

int fwx_dev_exact_paths_batch(int32_t count, int32_t n, int64_t stride, const int32_t *next0,
                              const fwx_trace *trace, int32_t items, const int32_t *mat, const int32_t *src,
                              const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap,
                              int32_t *scratch, void *stream)
{
    return dev_exact_paths_batch(kPlain, count, n, stride, next0, trace, items, mat, src, dst, len_out, path_out, cap,
                                 scratch, stream);
}

int fwx_dev_exact_paths_batch_mid(int32_t count, int32_t n, int64_t stride, const int32_t *next0,
                                  const fwx_trace *trace, int32_t items, const int32_t *mat, const int32_t *src,
                                  const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap,
                                  int32_t *scratch, void *stream)
{
    return dev_exact_paths_batch(kMid, count, n, stride, next0, trace, items, mat, src, dst, len_out, path_out, cap,
                                 scratch, stream);
}

int fwx_dev_exact_paths_batch_large(int32_t count, int32_t n, int64_t stride, const int32_t *next0,
                                    const fwx_trace *trace, int32_t items, const int32_t *mat, const int32_t *src,
                                    const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap,
                                    int32_t *scratch, void *stream)
{
    return dev_exact_paths_batch(kLarge, count, n, stride, next0, trace, items, mat, src, dst, len_out, path_out, cap,
                                 scratch, stream);
}

// ---- ragged batches -----------------------------------------------------------------------------------------------

int fwx_ragged_plan(int32_t count, const int32_t *n_each, int64_t *offset_out, int32_t *order_out,
                    int32_t tier_count_out[3])
{
    return ragged_plan_checked(kPlain, count, n_each, offset_out, order_out, tier_count_out);
}

int fwx_ragged_mid_plan(int32_t count, const int32_t *n_each, int64_t *offset_out, int32_t *order_out,
                        int32_t tier_count_out[4])
{
    return ragged_plan_checked(kMid, count, n_each, offset_out, order_out, tier_count_out);
}

int fwx_solve_ragged_f64(int32_t count, const int32_t *n_each, double *rate, int32_t *next, int32_t *hops,
                         uint64_t *updates_each, const fwx_opts *opts)
{
    return solve_batch_host<double>({kPlain, true, n_each, nullptr}, count, 0, rate, next, hops, updates_each, opts);
}

int fwx_solve_ragged_f32(int32_t count, const int32_t *n_each, float *rate, int32_t *next, int32_t *hops,
                         uint64_t *updates_each, const fwx_opts *opts)
{
    return solve_batch_host<float>({kPlain, true, n_each, nullptr}, count, 0, rate, next, hops, updates_each, opts);
}

int fwx_solve_ragged_mid_f64(int32_t count, const int32_t *n_each, double *rate, int32_t *next, int32_t *hops,
                             uint64_t *updates_each, const fwx_opts *opts)
{
    return solve_batch_host<double>({kMid, true, n_each, nullptr}, count, 0, rate, next, hops, updates_each, opts);
}

int fwx_solve_ragged_mid_f32(int32_t count, const int32_t *n_each, float *rate, int32_t *next, int32_t *hops,
                             uint64_t *updates_each, const fwx_opts *opts)
{
    return solve_batch_host<float>({kMid, true, n_each, nullptr}, count, 0, rate, next, hops, updates_each, opts);
}

int fwx_solve_ragged_lists_f64(int32_t count, const int32_t *n_each, double *rate, int32_t *next, int32_t *hops,
                               uint64_t *updates_each, int32_t items, const int32_t *mat, const int32_t *src,
                               const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap,
                               const fwx_opts *opts)
{
    const BatchLists ls = {items, mat, src, dst, len_out, path_out, cap};
    return solve_batch_host<double>({kPlain, true, n_each, &ls}, count, 0, rate, next, hops, updates_each, opts);
}

int fwx_solve_ragged_lists_f32(int32_t count, const int32_t *n_each, float *rate, int32_t *next, int32_t *hops,
                               uint64_t *updates_each, int32_t items, const int32_t *mat, const int32_t *src,
                               const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap,
                               const fwx_opts *opts)
{
    const BatchLists ls = {items, mat, src, dst, len_out, path_out, cap};
    return solve_batch_host<float>({kPlain, true, n_each, &ls}, count, 0, rate, next, hops, updates_each, opts);
}

int fwx_solve_ragged_mid_lists_f64(int32_t count, const int32_t *n_each, double *rate, int32_t *next, int32_t *hops,
                                   uint64_t *updates_each, int32_t items, const int32_t *mat, const int32_t *src,
                                   const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap,
                                   const fwx_opts *opts)
{
    const BatchLists ls = {items, mat, src, dst, len_out, path_out, cap};
    return solve_batch_host<double>({kMid, true, n_each, &ls}, count, 0, rate, next, hops, updates_each, opts);
}

int fwx_solve_ragged_mid_lists_f32(int32_t count, const int32_t *n_each, float *rate, int32_t *next, int32_t *hops,
                                   uint64_t *updates_each, int32_t items, const int32_t *mat, const int32_t *src,
                                   const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap,
                                   const fwx_opts *opts)
{
    const BatchLists ls = {items, mat, src, dst, len_out, path_out, cap};
    return solve_batch_host<float>({kMid, true, n_each, &ls}, count, 0, rate, next, hops, updates_each, opts);
}

int fwx_dev_solve_ragged(int32_t count, int32_t dtype, void *rate, int32_t *next, int32_t *hops,
                         const int32_t *d_n_each, const int64_t *d_offset, const int32_t *d_order,
                         const int32_t tier_count[3], const fwx_trace *trace, unsigned long long *d_updates_each,
                         void *stream)
{
    return dev_solve_ragged(kPlain, count, dtype, rate, next, hops, d_n_each, d_offset, d_order, tier_count, trace,
                            d_updates_each, stream);
}

int fwx_dev_solve_ragged_mid(int32_t count, int32_t dtype, void *rate, int32_t *next, int32_t *hops,
                             const int32_t *d_n_each, const int64_t *d_offset, const int32_t *d_order,
                             const int32_t tier_count[4], const fwx_trace *trace,
                             unsigned long long *d_updates_each, void *stream)
{
    return dev_solve_ragged(kMid, count, dtype, rate, next, hops, d_n_each, d_offset, d_order, tier_count, trace,
                            d_updates_each, stream);
}

int fwx_dev_exact_paths_ragged(int32_t count, const int32_t *d_n_each, const int64_t *d_offset, int32_t n_max,
                               const int32_t *next0, const fwx_trace *trace, int32_t items, const int32_t *mat,
                               const int32_t *src, const int32_t *dst, int32_t *len_out, int32_t *path_out,
                               int32_t cap, int32_t *scratch, void *stream)
{
    return dev_exact_paths_ragged(kPlain, count, d_n_each, d_offset, n_max, next0, trace, items, mat, src, dst, len_out,
                                  path_out, cap, scratch, stream);
}

int fwx_dev_exact_paths_ragged_mid(int32_t count, const int32_t *d_n_each, const int64_t *d_offset, int32_t n_max,
                                   const int32_t *next0, const fwx_trace *trace, int32_t items, const int32_t *mat,
                                   const int32_t *src, const int32_t *dst, int32_t *len_out, int32_t *path_out,
                                   int32_t cap, int32_t *scratch, void *stream)
{
    return dev_exact_paths_ragged(kMid, count, d_n_each, d_offset, n_max, next0, trace, items, mat, src, dst, len_out,
                                  path_out, cap, scratch, stream);
}

// ---- ragged batches up to FWX_BATCH_LARGE_MAX_N: the fifth tier -----------------------------------------------------

int fwx_ragged_large_plan(int32_t count, const int32_t *n_each, int64_t *offset_out, int32_t *order_out,
                          int32_t tier_count_out[5], int64_t *work_out)
{
    return ragged_plan_checked(kLarge, count, n_each, offset_out, order_out, tier_count_out, work_out);
}

int fwx_solve_ragged_large_f64(int32_t count, const int32_t *n_each, double *rate, int32_t *next, int32_t *hops,
                               uint64_t *updates_each, const fwx_opts *opts)
{
    return solve_batch_host<double>({kLarge, true, n_each, nullptr}, count, 0, rate, next, hops, updates_each, opts);
}

int fwx_solve_ragged_large_f32(int32_t count, const int32_t *n_each, float *rate, int32_t *next, int32_t *hops,
                               uint64_t *updates_each, const fwx_opts *opts)
{
    return solve_batch_host<float>({kLarge, true, n_each, nullptr}, count, 0, rate, next, hops, updates_each, opts);
}

int fwx_solve_ragged_large_lists_f64(int32_t count, const int32_t *n_each, double *rate, int32_t *next, int32_t *hops,
                                     uint64_t *updates_each, int32_t items, const int32_t *mat, const int32_t *src,
                                     const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap,
                                     const fwx_opts *opts)
{
    const BatchLists ls = {items, mat, src, dst, len_out, path_out, cap};
    return solve_batch_host<double>({kLarge, true, n_each, &ls}, count, 0, rate, next, hops, updates_each, opts);
}

int fwx_solve_ragged_large_lists_f32(int32_t count, const int32_t *n_each, float *rate, int32_t *next, int32_t *hops,
                                     uint64_t *updates_each, int32_t items, const int32_t *mat, const int32_t *src,
                                     const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap,
                                     const fwx_opts *opts)
{
    const BatchLists ls = {items, mat, src, dst, len_out, path_out, cap};
    return solve_batch_host<float>({kLarge, true, n_each, &ls}, count, 0, rate, next, hops, updates_each, opts);
}

int fwx_dev_solve_ragged_large(int32_t count, int32_t dtype, void *rate, int32_t *next, int32_t *hops,
                               const int32_t *d_n_each, const int64_t *d_offset, const int32_t *d_order,
                               const int32_t tier_count[5], const int64_t *work, const int64_t *d_work,
                               const fwx_trace *trace, unsigned long long *d_updates_each, void *scratch,
                               size_t scratch_bytes, void *stream)
{
    RaggedLarge lg;
    lg.work = work;
    lg.d_work = d_work;
    lg.scratch = scratch;
    lg.scratch_bytes = scratch_bytes;
    return dev_solve_ragged(kLarge, count, dtype, rate, next, hops, d_n_each, d_offset, d_order, tier_count, trace,
                            d_updates_each, stream, lg);
}

int fwx_dev_exact_paths_ragged_large(int32_t count, const int32_t *d_n_each, const int64_t *d_offset, int32_t n_max,
                                     const int32_t *next0, const fwx_trace *trace, int32_t items, const int32_t *mat,
                                     const int32_t *src, const int32_t *dst, int32_t *len_out, int32_t *path_out,
                                     int32_t cap, int32_t *scratch, void *stream)
{
    return dev_exact_paths_ragged(kLarge, count, d_n_each, d_offset, n_max, next0, trace, items, mat, src, dst, len_out,
                                  path_out, cap, scratch, stream);
}

// ---- test hooks ---------------------------------------------------------------------------------------------------

// The groups and grids launch_ragged_large makes of a host work table, counted with its own helpers.
int fwx_test_ragged_large_schedule(int32_t count, int32_t large_count, const int64_t *work, size_t scratch_bytes,
                                   int32_t *group_first, int32_t cap, int64_t totals[3])
{
    return guarded([&]() -> int {
        if (count < 0 || large_count < 0 || large_count > count || cap < 0 || (cap > 0 && !group_first))
            return FWX_ERR_INVALID;
        int64_t sum[3] = {0, 0, 0};
        int groups = 0;
        if (large_count > 0) {
            if (!work) return FWX_ERR_INVALID;
            const fwx::RaggedLargeWork w(work, (long long)count + 1);
            if (!fwx::ragged_large_work_ok(w, large_count) ||
                scratch_bytes < FWX_BATCH_LARGE_SCRATCH_BYTES((size_t)w.order_of(0)))
                return FWX_ERR_INVALID;
            for (int m0 = 0; m0 < large_count; ++groups) {
                const int m1 = fwx::ragged_large_group_end(w, m0, large_count, scratch_bytes);
                if (groups < cap) group_first[groups] = m0;
                fwx::ragged_large_blocks(w, m0, m1, [&](int, int active) {
                    sum[0] += 2;
                    sum[1] += w.strip[m0 + active] - w.strip[m0];
                    sum[2] += w.tile[m0 + active] - w.tile[m0];
                });
                m0 = m1;
            }
        }
        if (totals) std::copy(sum, sum + 3, totals);
        return groups;
    });
}

int fwx_test_batch_wave_max_n(void) { return batch_wave_max_n(); }

int fwx_test_batch_mid_min_n(void) { return batch_mid_min_n(); }

int fwx_test_batch_mid_block(void) { return FWX_MID_B; }

int fwx_test_batch_large_min_n(void) { return batch_large_min_n(); }

int fwx_test_batch_large_geometry(int32_t out[4])
{
    if (!out) return FWX_ERR_INVALID;
    out[0] = FWX_LARGE_B;
    out[1] = FWX_LARGE_S;
    out[2] = FWX_LARGE_TR;
    out[3] = FWX_LARGE_TC;
    return FWX_OK;
}

int fwx_test_sweep_mid_slots(int32_t count, int32_t n, size_t scratch_bytes)
{
    if (count < 0 || n < 0) return FWX_ERR_INVALID;
    if (n > FWX_SWEEP_MID_MAX_N) return FWX_ERR_UNSUPPORTED;
    return sweep_mid_slots(count, n, scratch_bytes);
}

int64_t fwx_test_batch_lists_chunk(int32_t n, int32_t cap)
{
    return n < 0 || cap < 1 ? (int64_t)FWX_ERR_INVALID : (int64_t)batch_lists_chunk(n, cap);
}

}  // extern "C"
