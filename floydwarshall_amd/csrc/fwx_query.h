// fwx_query.h -- the path queries of a handle (fwx_matrix_query, fwx_matrix_query_exact and its batch form),
// one copy for both handle kinds: a query kernel addresses entry (a, b) through a table of row partitions, and
// a single-device handle (fwx_api.hip) is the table with one partition of all rows.  The walks, their kernels
// and the host drivers are defined once, in fwx_api.hip.  Not installed, not part of the ABI.
#ifndef FWX_QUERY_H
#define FWX_QUERY_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "fwx_internal.h"

namespace fwxi {

// Which of the three trace matrices holds the pivot of an entry the exact walk asks for (PathLog, fwx_kernels.h).
enum WalkKind { WALK_FINAL = 0, WALK_AS_COLUMN = 1, WALK_AS_ROW = 2 };

// Everything a query kernel needs to address entry (a, b) of a handle's matrix: partition p holds rows
// [row0[p], row0[p + 1]) at pitch nd.  Passed by value (about 1.4 KB of kernel arguments).
// The exact walk (exact_walk, fwx_api.hip) reads a table through three members only -- cell(a, b), pivot(cell, kind)
// and edge(cell), the leaf test on the unsolved next-hops -- so that BatchTab below can stand in for it.
struct EntryTab {
    int parts, nd;                             // nd = device pitch (fwx_matrix::nd), not the caller's n
    int row0[FWX_MAX_PARTS + 1];
    const int32_t *next[FWX_MAX_PARTS], *last[FWX_MAX_PARTS], *at_col[FWX_MAX_PARTS],
        *at_row[FWX_MAX_PARTS], *next0[FWX_MAX_PARTS];
    __device__ __forceinline__ size_t locate(int a, int b, int &p) const
    {
        p = 0;
        while (p + 1 < parts && a >= row0[p + 1]) ++p;
        return (size_t)(a - row0[p]) * nd + b;
    }
    struct Cell { int p; size_t off; };
    __device__ __forceinline__ Cell cell(int a, int b) const
    {
        Cell c;
        c.off = locate(a, b, c.p);
        return c;
    }
    __device__ __forceinline__ int pivot(const Cell &c, int kind) const
    {
        return kind == WALK_FINAL ? last[c.p][c.off] : kind == WALK_AS_COLUMN ? at_col[c.p][c.off] : at_row[c.p][c.off];
    }
    __device__ __forceinline__ bool edge(const Cell &c) const { return next0[c.p][c.off] >= 0; }
};

// The same three reads for ONE matrix of a traced batch (fwx_dev_solve_batch_traced): order n, pitch n, the four
// arrays already offset to the matrix (mat * stride).  Built per item by the batch kernel.
struct BatchTab {
    int n;
    const int32_t *last, *at_col, *at_row, *next0;
    typedef size_t Cell;
    __device__ __forceinline__ Cell cell(int a, int b) const { return (size_t)a * n + b; }
    __device__ __forceinline__ int pivot(Cell c, int kind) const
    {
        return kind == WALK_FINAL ? last[c] : kind == WALK_AS_COLUMN ? at_col[c] : at_row[c];
    }
    __device__ __forceinline__ bool edge(Cell c) const { return next0[c] >= 0; }
};

// One rate entry as a double.  queue() puts the copy on `s` (f32: into the first half of *rate_out); once
// something has synchronised `s`, done() widens an f32 in place.  A null rate_out makes both no-ops.
struct RateRead {
    double *out = nullptr;
    bool f32 = false;
    int queue(const void *base, size_t off, int dtype, hipStream_t s, double *rate_out)
    {
        if (!(out = rate_out)) return FWX_OK;
        f32 = dtype != FWX_F64;
        const size_t es = f32 ? 4 : 8;
        FWX_HIP(hipMemcpyAsync(out, (const char *)base + off * es, es, hipMemcpyDeviceToHost, s));
        return FWX_OK;
    }
    void done() const
    {
        float f;
        if (out && f32) { memcpy(&f, out, 4); *out = (double)f; }
    }
};

// The drivers (fwx_api.hip).  The caller has selected the device of `s` and of the scratch; n_real is the
// caller's matrix order.  Both block until the answer is in the caller's memory.
// Next-hop walk src -> dst: the length, 0 (no path) or an error; scratch: n_real + 2 ints on the device.
int run_follow(const EntryTab &tab, int n_real, hipStream_t s, int32_t *scratch, int32_t src, int32_t dst,
               int32_t *path_out, int32_t cap);
// `count` exact `_path` lists, device scratch from a pooled per-call context: len_out[q] is the length of list
// q or its error, path_out + q * cap the list.
int run_exact_batch(const EntryTab &tab, int n_real, hipStream_t s, int32_t count, const int32_t *src,
                    const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap);

// For the batched solves (fwx_batch.hip; defined in fwx_api.hip beside the walk they share with the handles).
// The exact lists of `items` triples (mat, src, dst) of a traced batch, everything on the device, one launch on `s`,
// nothing allocated or synchronised: len_out[q] = length or the error of item q, paths + q * cap its list;
// stacks: items * 3 * (n + 2) ints.
int launch_exact_batch(int count, int n, long long stride, const int32_t *next0, const fwx::PathLog &plog,
                       int items, const int32_t *mat, const int32_t *src, const int32_t *dst, int32_t *len_out,
                       int32_t *paths, int cap, int32_t *stacks, hipStream_t s);
// The same over a traced ragged batch: matrix m of order n_each[m] at + offset[m] (device arrays), pitch n_each[m];
// stacks: items * 3 * (n_max + 2) ints, n_max at least the largest order of the batch.
int launch_exact_ragged(int count, const int32_t *n_each, const int64_t *offset, int n_max, const int32_t *next0,
                        const fwx::PathLog &plog, int items, const int32_t *mat, const int32_t *src,
                        const int32_t *dst, int32_t *len_out, int32_t *paths, int cap, int32_t *stacks, hipStream_t s);

}  // namespace fwxi

#endif
