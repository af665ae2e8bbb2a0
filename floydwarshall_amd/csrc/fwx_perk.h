// fwx_perk.h -- the per-k engine's host side (fwx_perk.hip) as fwx_api.hip and fwx_multi.hip see it: the range entry,
// the size of its scratch and the capacity of its pool.  Not installed, not part of the ABI.
#ifndef FWX_PERK_H
#define FWX_PERK_H

#include "fwx_internal.h"

namespace fwxi {

constexpr size_t kPerkScratchMax = 16;         // PerkScratch keeps this many streams' buffers (fwx_test_pools)

// Snapshot panels (W and Ct of one 64-pivot block) of the multi-pivot schedule: what PerkRange::kt_ws holds.
template <typename T> inline size_t perk_kt_ws_bytes(int n)
{
    const size_t ld = ((size_t)n + 3) & ~(size_t)3;
    return (size_t)FWX_FUSED_B * ((size_t)n + ld) * sizeof(T);
}

// Pivots [k_begin, k_end) over a slab; pivot k's row (and its hops / next-hops, where the slab has them) at
// `prow0 + (k - k_begin) * stride`.
template <typename T> struct PerkRange {
    T *rate = nullptr;                             // the slab: rows x n entries, its first row is row0 of the matrix
    int32_t *next = nullptr, *hops = nullptr;
    int rows = 0, n = 0, row0 = 0;
    const T *prow0 = nullptr;                      // the pivot rows
    const int32_t *phops0 = nullptr, *pnext0 = nullptr;
    int64_t stride = 0;
    int k_begin = 0, k_end = 0, serpentine = 0;
    unsigned long long *d_updates = nullptr;
    hipStream_t stream = nullptr;
    fwx::PathLog plog = fwx::PathLog();
    int skip_lo = 0, skip_hi = 0;                  // rows [skip_lo, skip_hi) of the slab are left alone
    // perk_kt_ws_bytes of device scratch for the multi-pivot schedule that the caller keeps until the launches have
    // run, or null: the stream's buffer of PerkScratch
    void *kt_ws = nullptr;

    // the whole matrix in place, the pivots its own rows
    static PerkRange whole(T *rate, int32_t *next, int32_t *hops, int n, int k_begin, int k_end)
    {
        const size_t off = (size_t)k_begin * n;
        PerkRange r;
        r.rate = rate; r.next = next; r.hops = hops; r.rows = n; r.n = n;
        r.prow0 = rate + off; r.phops0 = hops ? hops + off : nullptr; r.pnext0 = next ? next + off : nullptr;
        r.stride = n; r.k_begin = k_begin; r.k_end = k_end;
        return r;
    }
};

// One launch per pivot; a rates-only call on the whole matrix in place with the pivots its own rows takes the
// multi-pivot schedule instead (fwx_perk.hip).  Instantiated for float and double.
template <typename T> int relax_range(const PerkRange<T> &r);

}  // namespace fwxi

#endif
