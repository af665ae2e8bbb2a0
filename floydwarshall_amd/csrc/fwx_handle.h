// fwx_handle.h -- the handle behind fwx_matrix_* and the one way its operations visit what it holds.  A handle
// is a set of slabs (SlabData, fwx_resume.h): one of all rows for a single-device handle, one per partition
// that lives in this process for a row-partitioned one.  The data operations of fwx_api.hip (upload, download,
// keep / patch, trace, resume, resolve) are loops over those slabs and exist once; what only partitions have
// (panels, events, the exchange, the engines) stays in fwx_multi.hip.  Not installed, not part of the ABI.
#ifndef FWX_HANDLE_H
#define FWX_HANDLE_H

#include "fwx_resume.h"

namespace fwxi {
struct MultiState;   // fwx_multi.hip: the partitions of a row-partitioned handle
}

struct fwx_matrix {
    int32_t n, dtype, device;
    int32_t nd;            // device order = pitch of every array of every slab: n rounded up to a multiple of 16
                           // bytes of rate elements, so that the fused engine reads any n.  The padding
                           // (rate +0.0, next -1, hops 0, trace -1) is inert: a padding index is never a pivot,
                           // and a +0.0 target never improves (0 < +-0 and 0 < NaN are false) -- as in fwx_solve_*
    int32_t with_next, with_hops;   // the handle carries next-hops / path lengths
    int32_t traced;        // the path trace for exact `_path` lists is enabled (fwx_matrix_enable_path_log)
    fwxi::SlabData slab;   // a single-device handle's one slab: all nd rows on `device` (the padding written
                           // once, at create).  Empty on a partitioned handle, whose slabs are its partitions
    int32_t *scratch;
    unsigned long long *upd;
    int32_t keep;          // the input is kept on the device
    int32_t kept_valid;    // ... and holds an upload
    int32_t *walk;         // scratch of the exact-path walk (output, then a stack sized by the order)
    int32_t walk_cap;      // capacity (path entries) `walk` was sized for
    int32_t rec_ready;     // a traced solve of the current upload has completed
    int32_t fresh;         // the arrays hold an uploaded input that has not been solved yet
    unsigned long long last_u;   // U of the last traced solve
    void *ws;              // fused-engine workspace, allocated by the first fused solve and kept
    size_t ws_bytes;
    fwxi::SideStream *side;      // look-ahead stream + events of the fused engine, kept likewise
    int *flag;             // device int for the domain check (null: a view of caller-owned memory, fwx_dev_solve)
    int32_t dom_known;     // dom_bits is the domain check's answer for what the arrays hold now.  The
    int32_t dom_bits;      // domain (fwx.h) is closed under the algorithm -- products of non-negative
                           // rates are >= +0 or NaN (which never wins), and a relaxation only succeeds
                           // through a non-zero r[i][k], whose next-hop it copies -- so only an upload
                           // or a patch can change the answer: the upload forgets it, a patch whose
                           // values are themselves inside the domain keeps a "3".
    fwxi::MultiState *multi;   // non-null: a row-partitioned handle (fwx_matrix_create_multi / _create_part)
    fwxi::Resume *resume;  // non-null: panels of all pivots + state checkpoints are kept (f3, fwx_resume.h)
};

namespace fwxi {

// fwx_multi.hip: the partitions of a partitioned handle as slabs.  multi_slab(m, p) for p < multi_parts(m);
// with multi_self(m) >= 0 only that one lives in this process (fwx_matrix_create_part) and the others are
// row bounds without arrays.
int multi_parts(const fwx_matrix *m);
int multi_self(const fwx_matrix *m);
SlabData &multi_slab(const fwx_matrix *m, int p);
// ... and what fwx_api.hip calls for a handle with m->multi
int multi_solve(fwx_matrix *m, const Opts &op, bool resumed = false);
int multi_query(fwx_matrix *m, int32_t src, int32_t dst, double *rate_out, int32_t *path_out, int32_t cap);
int multi_query_exact(fwx_matrix *m, int32_t src, int32_t dst, double *rate_out, int32_t *path_out,
                      int32_t cap);
int multi_query_exact_batch(fwx_matrix *m, int32_t count, const int32_t *src, const int32_t *dst,
                            int32_t *len_out, int32_t *path_out, int32_t cap);
void multi_destroy(fwx_matrix *m);

// fn(SlabData &, int p) for every slab of the handle that lives in this process, in row order, with the
// slab's device current; stops at the first error.  A single-device handle's device is current since
// DeviceGuard::enter; g == nullptr: fn makes no device call.
// (M: fwx_matrix or const fwx_matrix, which hands out const slabs.)
template <typename M, typename F> int each_slab(M *m, DeviceGuard *g, F &&fn)
{
    const int parts = m->multi ? multi_parts(m) : 1, self = m->multi ? multi_self(m) : -1;
    for (int p = 0; p < parts; ++p) {
        if (self >= 0 && p != self) continue;
        auto &d = m->multi ? multi_slab(m, p) : m->slab;
        int rc = g && m->multi ? g->set(d.device) : FWX_OK;
        if (rc || (rc = fn(d, p))) return rc;
    }
    return FWX_OK;
}

// Waits for the stream of every such slab.
inline int sync_slabs(fwx_matrix *m, DeviceGuard &g)
{
    return each_slab(m, &g, [](SlabData &d, int) -> int {
        FWX_HIP(hipStreamSynchronize(d.main));
        return FWX_OK;
    });
}

// First row of the slab that holds `row`, wherever that slab lives.
inline int slab_row0_of(const fwx_matrix *m, int row)
{
    int row0 = 0;
    for (int p = 0; m->multi && p < multi_parts(m); ++p)
        if (multi_slab(m, p).rows > 0 && row >= multi_slab(m, p).row0) row0 = multi_slab(m, p).row0;
    return row0;
}

// Does a patch with these values keep a matrix inside the domain (fwx.h) inside it?  rate >= +0 and not
// NaN; a non-zero rate comes with a next-hop >= 0 on a handle that carries next-hops.
inline bool patch_keeps_domain(const fwx_matrix *m, int32_t count, const void *rate_vals, const int32_t *next_vals)
{
    for (int32_t q = 0; q < count; ++q) {
        const double r = m->dtype == FWX_F64 ? ((const double *)rate_vals)[q] : (double)((const float *)rate_vals)[q];
        if (r != r || r < 0.0 || (r == 0.0 && 1.0 / r < 0.0)) return false;       // NaN, negative, -0.0
        if (m->with_next && r != 0.0 && !(next_vals && next_vals[q] >= 0)) return false;
    }
    const int want = m->with_next ? 3 : 1;
    return (m->dom_bits & want) == want;
}

}  // namespace fwxi

#endif
