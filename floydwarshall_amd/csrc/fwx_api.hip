// fwx_api.hip -- the C ABI of libfwx (include/fwx.h) over the gfx950 kernels.
//
// Replaces runAlgo (/root/reference/src/lib/Algorithms.hs:42-61) behind floydWarshall (:19-20).
// No CPU fallback: every solve entry point needs a HIP device and says so when there is none.
// The batched solves (fwx_solve_batch_*, fwx_solve_ragged_*, their device forms) are fwx_batch.hip; the kernels of
// their exact walk are here, beside the handles' (fwx_query.h).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <new>

#include "fwx.h"
#include "fwx_guard.h"
#include "fwx_handle.h"
#include "fwx_internal.h"
#include "fwx_kernels.h"
#include "fwx_perk.h"
#include "fwx_query.h"

using namespace fwxi;

namespace {

template <typename T>
int fused_block(const fwx_slab *sl, int k0, int bt, const T *w, const int32_t *wh,
                const fwx_fused_scratch *sc, const fwx_trace *tr, unsigned long long *d_updates,
                bool nonneg, hipStream_t s, int skip_lo = 0, int skip_hi = 0)
{
    fwx::FusedArgs<T> a;
    a.nonneg = nonneg;
    a.rate = (T *)sl->rate; a.next = sl->next; a.rows = sl->rows; a.n = sl->n; a.row0 = sl->row0;
    a.k0 = k0; a.bt = bt; a.w = w; a.ct = (T *)sc->col_rate; a.cnt = sc->col_next; a.updates = d_updates;
    a.ct_ld = (sl->rows + 3) & ~3;
    a.hops = sl->hops; a.wh = wh; a.cht = sc->col_hops;
    if (tr) { a.plog.last = tr->last; a.plog.at_col = tr->at_col; a.plog.at_row = tr->at_row; }
    hipError_t e = fwx::launch_fused_relax<T>(a, s, skip_lo, skip_hi);
    if (e == hipErrorInvalidValue) return FWX_ERR_INVALID;
    FWX_HIP(e);
    return FWX_OK;
}

// Can the fused kernels read this matrix?  (16-byte vectors along rows.)
template <typename T> bool fused_dims_ok(int n, const void *rate)
{
    return n % (16 / (int)sizeof(T)) == 0 && ((uintptr_t)rate % 16) == 0;
}
template <typename T> bool fused_ok(int n, const void *rate, const int32_t *)
{
    return fused_dims_ok<T>(n, rate);
}

// Single-GPU solve of pivots [k_begin,k_end) with the fused engine.  Per block of <= 64 pivots:
// snapshot panel W_b (rowpanel), pivot-column snapshots for all rows (colpanel), main kernel over
// all rows.  Three schedules:
//   serial: ONE fused_panels launch (row panel + column panel as one grid) and ONE main launch
//     per pass, in one stream.  While a main launch is not much longer than a panel kernel
//     (20-40 us) any look-ahead costs more -- an extra latency-bound launch and two cross-stream
//     event hops (6 + 12 us) -- than its overlap gives: N = 1024 f32 1.08 ms (rows-only look-ahead)
//     -> 0.73 (serial, three launches) -> 0.52 (panels merged); and because the panels then run on
//     an idle chip (25 us instead of 75 us beside a main launch) it stays level with the look-ahead
//     forms up to the largest sizes for rates-only solves.
//   symmetric look-ahead (large matrices with next-hops, 64-aligned blocks): the panel chain of
//     block b+1 only needs the 64 pivot ROWS and the 64 pivot COLUMNS of b+1 as pass b leaves them.
//     The side stream relaxes exactly those with pass b's panels, then runs fused_panels(b+1) --
//     all of it beside main(b), which leaves those rows and columns alone.  The main stream carries
//     nothing but main kernels back to back (gap 44 -> 12.5 us).
//   rows-only look-ahead (the fallback for pivot ranges that do not start on a multiple of 64):
//     main(b) on the next block's rows first, their rowpanel on the side stream while main(b)
//     sweeps the rest; colpanel(b+1) follows main(b).
// Crossovers (serial vs symmetric, ms; gpurun_out/r02_run37.log, r02_run38.log): f32 rates 8192:
// 21.6 / 22.3, 12288: 69.1 / 69.9, 16384: 156.3 / 157.0 -> always serial; f32 + next 8192: 39.5 / 39.6,
// 12288: 117.0 / 117.5, 16384: 266.3 / 262.2; + trace 8192: 46.1 / 45.8, 10240: 84.6 / 83.6, 16384:
// 316.2 / 305.0; f64 + trace 8192: 137.9 / 132.6.
// ws: see fused_ws_bytes.
//   double pass (inside the domain -- the max-form and the arg kernels --, 64-aligned blocks, large
//     matrices): the main kernel applies TWO passes (128 pivots) per launch, which halves the tile
//     traffic and the per-tile overhead that kept it at 0.75 of its issue bound (the arg kernels run
//     their two passes one after the other on the tile they keep in registers).  It needs the
//     panels of both passes up front, so the look-ahead is two deep: beside main(P) -- which leaves
//     the 128 rows and 128 columns of the NEXT pair of blocks alone -- the side stream brings
//     exactly that cross up to date with the pair being applied (two launches of 128 pivots), runs
//     the panels of the first block of the next pair, applies that one pass to the rows and columns
//     of the second block, and runs its panels.  An entry that main(P+1) then folds again with a
//     pass it has already seen does not move (max is idempotent; the compare form would not move or
//     count it either -- and an entry that does not move is no item of the arg re-scan: its next-hop,
//     path length and trace stay), so main(P+1) simply covers everything but the cross after it.
constexpr int kLookaheadMinN = INT32_MAX, kLookaheadMinNWithNext = 16384, kLookaheadMinNWithTrace = 8192;
// The double-pass crossovers (kDoublePassMinN, kDoublePassNextMinN) and env_threshold: fwx_internal.h.

template <typename T>
int fused_range(T *rate, int32_t *next, int32_t *hops, int n, int k_begin, int k_end, void *ws,
                unsigned long long *d_updates, hipStream_t s, fwx::PathLog plog, bool nonneg,
                SideStream *kept_side = nullptr, Resume *rec = nullptr, ResumeStore *store = nullptr)
{
    char *p = (char *)ws;
    const int ld = (n + 3) & ~3;
    T *wbuf[2], *ctbuf[2];
    int32_t *cntbuf[2];
    int32_t *whbuf[2] = {nullptr, nullptr}, *chtbuf[2] = {nullptr, nullptr};
    for (int b = 0; b < 2; ++b) { wbuf[b] = (T *)p;          p += (size_t)FWX_FUSED_B * n * sizeof(T); }
    for (int b = 0; b < 2; ++b) { ctbuf[b] = (T *)p;         p += (size_t)FWX_FUSED_B * ld * sizeof(T); }
    for (int b = 0; b < 2; ++b) { cntbuf[b] = (int32_t *)p;  p += (size_t)FWX_FUSED_B * ld * sizeof(int32_t); }
    if (hops) {                    // hops panels of the pivot rows + hops of the pivot columns
        for (int b = 0; b < 2; ++b) { whbuf[b] = (int32_t *)p;  p += (size_t)FWX_FUSED_B * n * sizeof(int32_t); }
        for (int b = 0; b < 2; ++b) { chtbuf[b] = (int32_t *)p; p += (size_t)FWX_FUSED_B * ld * sizeof(int32_t); }
    }
    if (k_end <= k_begin) return FWX_OK;
    // Resumable handle: every pass writes its panels to their place in the all-pivot arrays (row k of
    // each = pivot k) instead of a ping-pong buffer, and the state is copied at the checkpoint pivots.
    if (rec && k_begin % FWX_FUSED_B) rec = nullptr;      // passes must start on multiples of 64
    Slab whole;                                           // the matrix as one slab (fwx_resume.h)
    whole.live = {rate, next, hops, plog.last, plog.at_col, plog.at_row};
    whole.rows = whole.nd = n; whole.ct_ld = ld; whole.es = sizeof(T); whole.s = s;
    auto panel_set = [&](int k0, int b) {
        if (!rec) return;
        const PanelRows pr = store_panels(*store, whole, k0);
        wbuf[b] = (T *)pr.w; ctbuf[b] = (T *)pr.ct; cntbuf[b] = pr.cnt; whbuf[b] = pr.wh; chtbuf[b] = pr.cht;
    };
    auto checkpoint = [&](int k0) -> int {        // the state at the START of step k0, if it is one
        const int c = rec ? rec->checkpoint_at(k0) : -1;
        return c < 0 ? FWX_OK : save_checkpoint(*store, whole, c);
    };
    SideStream local_side;
    SideStream &side = kept_side ? *kept_side : local_side;
    if (!side.s) {
        const int rc = side.init();
        if (rc) return rc;
    }
    Throttle thr;

    fwx::FusedArgs<T> a;
    a.rate = rate; a.next = next; a.rows = n; a.n = n; a.row0 = 0;
    a.ct_ld = ld; a.updates = d_updates;
    a.nonneg = nonneg;     // the caller has run the domain check (route_solve)
    a.plog = plog;         // path trace: kept by all three kernels of a pass (needs next)
    a.hops = hops;         // hops: carried by the panels, written by the main kernel (needs next)
    auto bind = [&](int k0, int bt, int bi) {       // pass (k0, bt) reads / writes buffer set bi
        panel_set(k0, bi);
        a.k0 = k0; a.bt = bt; a.w = wbuf[bi]; a.wh = whbuf[bi];
        a.ct = ctbuf[bi]; a.cnt = next ? cntbuf[bi] : nullptr; a.cht = chtbuf[bi];
    };
    auto rowpanel = [&](int k0, int bt, int bi, hipStream_t st) {
        panel_set(k0, bi);
        return fwx::launch_fused_panel<T>(rate + (size_t)k0 * n, n, k0, bt, wbuf[bi], st,
                                          plog_rows(plog, (size_t)k0 * n),
                                          hops ? hops + (size_t)k0 * n : nullptr, whbuf[bi]);
    };
    const bool lookahead = n >= env_threshold("FWX_LOOKAHEAD_MIN_N",
                                               !next ? kLookaheadMinN
                                                     : plog.last ? kLookaheadMinNWithTrace : kLookaheadMinNWithNext);
    const bool symmetric_ok = n >= env_threshold("FWX_SYMMETRIC_MIN_N", 0) && k_begin % FWX_FUSED_B == 0;

    auto panels = [&](int k0, int bt, int bi, hipStream_t st) {   // both panels of a pass, one launch
        bind(k0, bt, bi);
        return fwx::launch_fused_panels<T>(a, wbuf[bi], whbuf[bi], st);
    };

    // ---- double pass: see the header comment ----------------------------------------------------
    if (nonneg && !d_updates && !rec && k_begin % FWX_FUSED_B == 0 &&
        n >= (next ? env_threshold("FWX_DOUBLE_PASS_NEXT_MIN_N", sizeof(T) == 4 ? kDoublePassNextMinN : INT32_MAX)
                   : env_threshold("FWX_DOUBLE_PASS_MIN_N", kDoublePassMinN)) &&
        k_end - k_begin >= 4 * FWX_FUSED_B) {
        constexpr int Bq = FWX_FUSED_B;
        const int nb = (k_end - k_begin) / Bq;          // full blocks; a ragged tail is handled below
        const int pairs = nb / 2;
        // four panel sets, as two adjacent pairs: block q lives in set q & 3, so a pair (2P, 2P + 1)
        // is contiguous in W (128 rows), in Ct (128 lines) and likewise in CNt, WH, CHt
        char *q4 = (char *)ws;
        T *w4 = (T *)q4;                 q4 += (size_t)4 * Bq * n * sizeof(T);
        T *ct4 = (T *)q4;                q4 += (size_t)4 * Bq * ld * sizeof(T);
        int32_t *cnt4 = (int32_t *)q4;   q4 += (size_t)4 * Bq * ld * sizeof(int32_t);
        int32_t *wh4 = nullptr, *cht4 = nullptr;
        if (hops) {
            wh4 = (int32_t *)q4;         q4 += (size_t)4 * Bq * n * sizeof(int32_t);
            cht4 = (int32_t *)q4;
        }
        auto set_of = [&](int q) { return q & 3; };
        auto wh_of = [&](int q) { return wh4 ? wh4 + (size_t)set_of(q) * Bq * n : nullptr; };
        auto bind4 = [&](int q, int blocks) {           // pivots of `blocks` blocks starting at block q
            a.k0 = k_begin + q * Bq; a.bt = blocks * Bq;
            a.w = w4 + (size_t)set_of(q) * Bq * n; a.wh = wh_of(q);
            a.ct = ct4 + (size_t)set_of(q) * Bq * ld;
            a.cnt = next ? cnt4 + (size_t)set_of(q) * Bq * ld : nullptr;
            a.cht = cht4 ? cht4 + (size_t)set_of(q) * Bq * ld : nullptr;
        };
        auto panels4 = [&](int q, hipStream_t st) {
            bind4(q, 1);
            a.side = st != s;                       // beside a main launch: the panel kernels may pick a leaner form
            const hipError_t e = fwx::launch_fused_panels<T>(a, w4 + (size_t)set_of(q) * Bq * n, wh_of(q), st);
            a.side = false;
            return e;
        };
        // pivots of `blocks` blocks from block q onto the rows [lo, hi) (all columns) and the columns
        // [lo, hi) (the other rows)
        auto cross = [&](int q, int blocks, int lo, int hi, hipStream_t st) -> hipError_t {
            if (hi <= lo) return hipSuccess;
            bind4(q, blocks);
            a.side = true;
            hipError_t e = fwx::launch_fused_main<T>(a, lo, hi, st);
            if (e == hipSuccess) e = fwx::launch_fused_main<T>(a, 0, n, st, lo, hi, fwx::FusedCols::only(lo, hi));
            a.side = false;
            return e;
        };
        auto rows_of = [&](int q) { return k_begin + q * Bq; };
        // chain(0): panels of block 0, that pass onto block 1's rows and columns, panels of block 1
        FWX_HIP(panels4(0, s));
        FWX_HIP(cross(0, 1, rows_of(1), rows_of(2), s));
        FWX_HIP(panels4(1, s));
        for (int P = 0; P < pairs; ++P) {
            const int q = 2 * P;
            const int q_lo = q + 2, q_hi = q + 4 < nb ? q + 4 : nb;     // blocks of the next pair (or the odd last one)
            const int x_lo = rows_of(q_lo), x_hi = rows_of(q_hi);
            if (q_hi > q_lo) {
                FWX_HIP(hipEventRecord(side.main_done, s));       // main(P - 1) and chain(P) precede
                FWX_HIP(hipStreamWaitEvent(side.s, side.main_done, 0));
                FWX_HIP(cross(q, 2, x_lo, x_hi, side.s));         // the pair being applied onto the next cross
                FWX_HIP(panels4(q_lo, side.s));
                if (q_hi - q_lo == 2) {
                    FWX_HIP(cross(q_lo, 1, rows_of(q_lo + 1), x_hi, side.s));
                    FWX_HIP(panels4(q_lo + 1, side.s));
                }
                FWX_HIP(hipEventRecord(side.panel_done, side.s));
                bind4(q, 2);
                // a main launch whose retiring workgroups leave no room for a panel workgroup -- and for which the panel
                // kernels have no form that fits the hole (the path trace) -- goes out as two halves: the chain's
                // panels get in at each half's tail instead of at the end of the whole launch (N = 8192 + next-hops:
                // gap between main launches 77 -> 20 us; FWX_SPLIT_MAIN=0: A/B)
                static const bool split_ok = [] { const char *e = getenv("FWX_SPLIT_MAIN"); return !(e && *e == '0'); }();
                const int h = n / 2 / 128 * 128;
                if (split_ok && h > 0 && fwx::fused_main_starves_panels<T>(a) && !fwx::fused_panels_fit_beside<T>(a)) {
                    FWX_HIP(fwx::launch_fused_main<T>(a, 0, h, s, x_lo, x_hi, fwx::FusedCols::except(x_lo, x_hi)));
                    FWX_HIP(fwx::launch_fused_main<T>(a, h, n, s, x_lo, x_hi, fwx::FusedCols::except(x_lo, x_hi)));
                } else {
                    FWX_HIP(fwx::launch_fused_main<T>(a, 0, n, s, x_lo, x_hi, fwx::FusedCols::except(x_lo, x_hi)));
                }
                FWX_HIP(hipStreamWaitEvent(s, side.panel_done, 0));
            } else {
                bind4(q, 2);
                FWX_HIP(fwx::launch_fused_main<T>(a, 0, n, s));
            }
            const int rc = thr.tick(s, 8);
            if (rc) return rc;
        }
        if (nb & 1) {                                   // the odd last block: its panels are ready
            bind4(nb - 1, 1);
            FWX_HIP(fwx::launch_fused_main<T>(a, 0, n, s));
        }
        FWX_HIP(hipStreamSynchronize(s));
        k_begin += nb * Bq;                             // a ragged tail (< 64 pivots) takes the serial form
        if (k_end <= k_begin) return FWX_OK;
        bind(k_begin, k_end - k_begin, 0);              // (restores the two-set bindings below)
    }

    int bi = 0;
    bool col_ready = false;        // colpanel of the current pass already ran
    {
        const int bt = k_end - k_begin < FWX_FUSED_B ? k_end - k_begin : FWX_FUSED_B;
        if (!lookahead) {
            FWX_HIP(panels(k_begin, bt, 0, s));
            col_ready = true;
        } else {
            FWX_HIP(rowpanel(k_begin, bt, 0, s));
        }
    }
    for (int k0 = k_begin; k0 < k_end; k0 += FWX_FUSED_B, bi ^= 1) {
        const int bt = k_end - k0 < FWX_FUSED_B ? k_end - k0 : FWX_FUSED_B;
        const int k1 = k0 + bt;
        // everything queued on `s` so far (the previous pass, whose side chain `s` has waited for)
        // precedes this copy; this pass's panels only READ the matrix
        if (k0 > k_begin) { const int rc = checkpoint(k0); if (rc) return rc; }
        bind(k0, bt, bi);
        if (!col_ready) FWX_HIP(fwx::launch_fused_colpanel<T>(a, s));
        col_ready = false;
        if (k1 < k_end && !lookahead) {
            const int bt1 = k_end - k1 < FWX_FUSED_B ? k_end - k1 : FWX_FUSED_B;
            FWX_HIP(fwx::launch_fused_main<T>(a, 0, n, s));
            FWX_HIP(panels(k1, bt1, bi ^ 1, s));
            col_ready = true;
        } else if (k1 < k_end) {
            const int bt1 = k_end - k1 < FWX_FUSED_B ? k_end - k1 : FWX_FUSED_B;
            if (symmetric_ok && bt1 == FWX_FUSED_B) {
                // everything up to here (the previous main, this pass's panels) precedes the side chain
                FWX_HIP(hipEventRecord(side.main_done, s));
                FWX_HIP(hipStreamWaitEvent(side.s, side.main_done, 0));
                // side: pass b on the next block's rows (all columns), then on its columns (the
                // other rows) ...
                a.side = true;
                hipError_t se = fwx::launch_fused_main<T>(a, k1, k1 + bt1, side.s);
                if (se == hipSuccess)
                    se = fwx::launch_fused_main<T>(a, 0, n, side.s, k1, k1 + bt1, fwx::FusedCols::only(k1, k1 + bt1));
                a.side = false;
                FWX_HIP(se);
                // ... then the next pass's panels (one launch) into the other buffer set
                FWX_HIP(panels(k1, bt1, bi ^ 1, side.s));
                FWX_HIP(hipEventRecord(side.panel_done, side.s));
                // main: pass b everywhere else
                bind(k0, bt, bi);
                FWX_HIP(fwx::launch_fused_main<T>(a, 0, n, s, k1, k1 + bt1,
                                                  fwx::FusedCols::except(k1, k1 + bt1)));
                FWX_HIP(hipStreamWaitEvent(s, side.panel_done, 0));
                col_ready = true;
            } else {
                // the next panel's rows first ...
                FWX_HIP(fwx::launch_fused_main<T>(a, k1, k1 + bt1, s));
                FWX_HIP(hipEventRecord(side.rows_done, s));
                FWX_HIP(hipStreamWaitEvent(side.s, side.rows_done, 0));
                // ... their snapshot panel on the side stream ...
                FWX_HIP(rowpanel(k1, bt1, bi ^ 1, side.s));
                FWX_HIP(hipEventRecord(side.panel_done, side.s));
                // ... while the rest of the matrix is relaxed on the main stream
                if (k1 % 8 == 0 && bt1 % 8 == 0) {
                    FWX_HIP(fwx::launch_fused_main<T>(a, 0, n, s, k1, k1 + bt1));   // one launch, rows skipped
                } else {
                    FWX_HIP(fwx::launch_fused_main<T>(a, 0, k1, s));
                    FWX_HIP(fwx::launch_fused_main<T>(a, k1 + bt1, n, s));
                }
                FWX_HIP(hipStreamWaitEvent(s, side.panel_done, 0));
            }
        } else {
            FWX_HIP(fwx::launch_fused_main<T>(a, 0, n, s));
        }
        const int rc = thr.tick(s, 6);
        if (rc) return rc;
    }
    // the side stream's work is ordered before `s` by the last panel_done wait (or it never ran)
    FWX_HIP(hipStreamSynchronize(s));
    return FWX_OK;
}

// AUTO: the single-launch kernel up to its 64 x 64 form, the fused engine above wherever it applies.
constexpr int kSmallSolveAutoMax = 64;
template <typename T> bool pick_fused(int engine, int n, int nd, const void *rate, const int32_t *hops)
{
    if (engine == FWX_ENGINE_PERK) return false;
    if (!fused_ok<T>(nd, rate, hops)) return false;
    // tools/measure_small.py (profiles/r02_small_sizes.txt): with the serial two-launch schedule
    // the fused engine beats the per-k engine at every order, and the single-launch kernel above
    // its 64 x 64 register form (n = 72 f64 + next: 0.13 ms against 0.20; n = 128: 0.18 / 0.36)
    return engine == FWX_ENGINE_FUSED || n > kSmallSolveAutoMax;
}

// Which engine runs a solve of pivots [k_begin, k_end) of a matrix of order n held on the device at
// order (= pitch) nd >= n: the host-buffer path and the handles pad an odd order with inert entries
// (fwx_matrix::nd), every engine then runs the nd x nd arrays over the real pivots only.
enum Route { ROUTE_SMALL, ROUTE_PERK, ROUTE_FUSED };
template <typename T>
int route_solve(const Opts &op, int n, int nd, const T *rate, const int32_t *next,
                const int32_t *hops, bool counting, int *d_flag, hipStream_t s, Route &route,
                bool &nonneg, fwx_matrix *cache = nullptr)
{
    nonneg = false;
    if (op.engine == FWX_ENGINE_FUSED && !fused_ok<T>(nd, rate, hops)) return FWX_ERR_UNSUPPORTED;
    // AUTO below the fused engine's range, or where it cannot read the matrix / the input lies outside
    // its domain: the single-launch kernel while it fits (nd <= FWX_SMALL_N), else one launch per pivot
    const Route fallback = (op.engine == FWX_ENGINE_AUTO && nd <= FWX_SMALL_N) ? ROUTE_SMALL : ROUTE_PERK;
    if (op.engine == FWX_ENGINE_AUTO && n <= kSmallSolveAutoMax) { route = ROUTE_SMALL; return FWX_OK; }
    if (!pick_fused<T>(op.engine, n, nd, rate, hops)) { route = fallback; return FWX_OK; }
    // The fused kernels take next[i][k] as the head of ikPath ++ kjPath (Algorithms.hs:55), which
    // is the reference's list head only while a winning product never has an empty ikPath -- true
    // on the reference's own domain, checked here.  Outside it the per-k engine, which reads the
    // pivot row's next-hops for exactly that case, runs the solve (same bits as the reference).
    int bits = 0;
    if (next || !counting) {
        // a handle remembers the answer for its arrays (fwx_matrix::dom_known); with next-hops the
        // check reads both arrays, without them only bit 0 is meaningful -- a cached answer taken
        // with next-hops serves both
        if (cache && cache->dom_known) {
            bits = cache->dom_bits;
        } else {
            const int rc = domain_bits<T>(rate, next, (size_t)nd * nd, d_flag, s, bits);
            if (rc) return rc;
            if (cache && (next || !cache->with_next)) { cache->dom_bits = bits; cache->dom_known = 1; }
        }
    }
    if (next && bits != 3) { route = fallback; return FWX_OK; }
    nonneg = !counting && (next ? bits == 3 : (bits & 1) != 0);   // max-form kernels allowed
    route = ROUTE_FUSED;
    return FWX_OK;
}

template <typename T>
int solve_host(int32_t n, T *rate, int32_t *next, int32_t *hops, const fwx_opts *o)
{
    if (n < 0) return FWX_ERR_INVALID;
    if (n == 0) return FWX_OK;  // empty map -> empty matrix (AlgorithmsTest.hs:62-64)
    if (!rate) return FWX_ERR_INVALID;
    if (hops && !next) return FWX_ERR_INVALID;
    Opts op;
    int rc = read_opts(o, n, op);
    if (rc) return rc;
    DeviceGuard g;
    if ((rc = g.enter(op.device))) return rc;

    // Device order of the matrix.  The fused engine needs rows that are a multiple of 16 bytes; an
    // odd-sized matrix headed for it is PADDED on the device with +0.0 rows and columns.  Padding
    // never reaches a real entry -- step k reads r[i][k] and r[k][j] of real pivots k only, and a
    // padding entry is never a pivot row or column -- and a +0.0 target is never improved
    // (0 < +-0 and 0 < NaN are false), so U is unchanged too.  The caller's arrays stay n x n.
    constexpr int VW = 16 / (int)sizeof(T);
    const bool to_fused = op.engine == FWX_ENGINE_FUSED || (op.engine == FWX_ENGINE_AUTO && n > kSmallSolveAutoMax);
    const int nd = (to_fused && n % VW) ? (n + VW - 1) / VW * VW : n;
    const size_t nn = (size_t)nd * (size_t)nd;
    // stream, look-ahead stream, device buffers, workspace: a pooled per-call context (CallCtx)
    CtxLease lease;
    if ((rc = lease.open())) return rc;
    CallCtx &cx = *lease.c;
    if (op.has_stream) cx.uses_stream(op.stream);   // drained before the context's buffers are reused
    struct { void *p = nullptr; } d_rate, d_next, d_hops, d_upd;
    if ((rc = cx.reserve(CallCtx::RATE, nn * sizeof(T), &d_rate.p))) return rc;
    if (next && (rc = cx.reserve(CallCtx::NEXT, nn * sizeof(int32_t), &d_next.p))) return rc;
    if (hops && (rc = cx.reserve(CallCtx::HOPS, nn * sizeof(int32_t), &d_hops.p))) return rc;
    if ((rc = cx.reserve(CallCtx::SMALL, (FWX_UPDATE_SHARDS + 2) * sizeof(unsigned long long), &d_upd.p))) return rc;
    int *d_flag = (int *)((unsigned long long *)d_upd.p + FWX_UPDATE_SHARDS);

    hipStream_t s = op.has_stream ? op.stream : cx.s;   // a non-blocking stream, never the null stream
    auto copy2d = [&](void *dst, size_t dpitch, const void *src, size_t spitch, size_t es,
                      hipMemcpyKind kind) -> int {
        if (dpitch == spitch)
            FWX_HIP(hipMemcpyAsync(dst, src, (size_t)n * (size_t)n * es, kind, s));
        else
            FWX_HIP(hipMemcpy2DAsync(dst, dpitch * es, src, spitch * es, (size_t)n * es, (size_t)n, kind, s));
        return FWX_OK;
    };
    if (nd != n) {
        FWX_HIP(hipMemsetAsync(d_rate.p, 0, nn * sizeof(T), s));                  // +0.0
        if (next) FWX_HIP(hipMemsetAsync(d_next.p, 0xFF, nn * sizeof(int32_t), s));   // -1
        if (hops) FWX_HIP(hipMemsetAsync(d_hops.p, 0, nn * sizeof(int32_t), s));
    }
    // Small matrices travel through the context's pinned staging buffer and a plain memcpy: an
    // asynchronous copy from / to pageable memory makes the runtime pin and unpin the caller's pages
    // per call, which costs more than the transfer itself for small arrays (fwx_solve_f64 with next +
    // hops, n = 4: 0.079 -> 0.048 ms, n = 64: 0.155 -> 0.123, n = 256: 1.04 -> 0.92); larger ones go
    // straight from / to the caller's arrays (CallCtx::kStageBytes).
    const size_t b_rate = (size_t)n * n * sizeof(T), b_idx = (size_t)n * n * sizeof(int32_t);
    const size_t b_total = b_rate + (next ? b_idx : 0) + (hops ? b_idx : 0);
    const bool staged = b_total <= CallCtx::kStageBytes;
    char *st_rate = nullptr, *st_next = nullptr, *st_hops = nullptr;
    if (staged) {
        void *pinned = nullptr;
        if ((rc = cx.reserve_pinned(b_total, &pinned))) return rc;
        st_rate = (char *)pinned;
        st_next = st_rate + b_rate;
        st_hops = st_next + (next ? b_idx : 0);
        memcpy(st_rate, rate, b_rate);
        if (next) memcpy(st_next, next, b_idx);
        if (hops) memcpy(st_hops, hops, b_idx);
    }
    if ((rc = copy2d(d_rate.p, nd, staged ? (const void *)st_rate : (const void *)rate, n, sizeof(T), hipMemcpyHostToDevice))) return rc;
    if (next && (rc = copy2d(d_next.p, nd, staged ? (const void *)st_next : (const void *)next, n, sizeof(int32_t), hipMemcpyHostToDevice))) return rc;
    if (hops && (rc = copy2d(d_hops.p, nd, staged ? (const void *)st_hops : (const void *)hops, n, sizeof(int32_t), hipMemcpyHostToDevice))) return rc;
    FWX_HIP(hipMemsetAsync(d_upd.p, 0, FWX_UPDATE_SHARDS * sizeof(unsigned long long), s));

    T *dr = (T *)d_rate.p;
    int32_t *dn = (int32_t *)d_next.p, *dh = (int32_t *)d_hops.p;
    unsigned long long *upd = op.updates_out ? (unsigned long long *)d_upd.p : nullptr;
    Route route;
    bool nonneg = false;
    // (a padded matrix is routed by its real order n and solved over its real pivots only: the padding
    // is inert)
    if ((rc = route_solve<T>(op, n, nd, dr, dn, dh, upd != nullptr, d_flag, s, route, nonneg))) return rc;
    if (route == ROUTE_SMALL) {
        // the reference's own regime: the whole solve in one single-workgroup launch
        FWX_HIP(fwx::launch_small_solve<T>(dr, dn, dh, nd, op.k_begin, op.k_end, upd, fwx::PathLog(), s));
    } else if (route == ROUTE_FUSED) {
        void *ws = nullptr;
        if ((rc = cx.reserve(CallCtx::WS, fused_ws_bytes(nd, sizeof(T), dh != nullptr), &ws))) return rc;
        rc = fused_range<T>(dr, dn, dh, nd, op.k_begin, op.k_end, ws, upd, s, fwx::PathLog(), nonneg, &cx.side);
        if (rc) return rc;
    } else {
        // per-k engine; pitch nd (a matrix padded for the fused engine but found outside its domain)
        void *ws = nullptr;      // snapshot panels of the multi-pivot schedule (rates only): the context's
        if (!dn && !dh && (rc = cx.reserve(CallCtx::WS, perk_kt_ws_bytes<T>(nd), &ws))) return rc;
        PerkRange<T> pr = PerkRange<T>::whole(dr, dn, dh, nd, op.k_begin, op.k_end);
        pr.serpentine = op.serpentine; pr.d_updates = upd; pr.stream = s; pr.kt_ws = ws;
        if ((rc = relax_range<T>(pr))) return rc;
    }

    if ((rc = copy2d(staged ? (void *)st_rate : (void *)rate, n, d_rate.p, nd, sizeof(T), hipMemcpyDeviceToHost))) return rc;
    if (next && (rc = copy2d(staged ? (void *)st_next : (void *)next, n, d_next.p, nd, sizeof(int32_t), hipMemcpyDeviceToHost))) return rc;
    if (hops && (rc = copy2d(staged ? (void *)st_hops : (void *)hops, n, d_hops.p, nd, sizeof(int32_t), hipMemcpyDeviceToHost))) return rc;
    FWX_HIP(hipStreamSynchronize(s));
    if (staged) {
        memcpy(rate, st_rate, b_rate);
        if (next) memcpy(next, st_next, b_idx);
        if (hops) memcpy(hops, st_hops, b_idx);
    }
    if (op.updates_out) {
        if ((rc = sum_updates((unsigned long long *)d_upd.p, op.updates_out, s))) return rc;
    }
    return FWX_OK;
}

template <typename T>
int matrix_solve_typed(fwx_matrix *m, const Opts &op, unsigned long long *upd, hipStream_t s,
                       CallCtx *cx = nullptr);

// One thread per (src, dst) pair: batch path reconstruction from the next-hop matrix.
template <typename T>
__global__ __launch_bounds__(256) void follow_paths_kernel(const int32_t *next, int n, int count,
                                                           const int32_t *src, const int32_t *dst,
                                                           int32_t *len_out, const T *edge,
                                                           double *prod_out, int32_t *path_out,
                                                           int cap)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= count) return;
    const int s = src[q], d = dst[q];
    int len = 0, cur = s;
    double prod = 1.0;
    if (s < 0 || d < 0 || s >= n || d >= n) {
        len_out[q] = FWX_ERR_INVALID;
        return;
    }
    while (true) {
        const int nx = next[(size_t)cur * n + d];
        if (nx < 0) {
            if (len) len = FWX_ERR_CYCLE;    // a broken walk: only possible on inconsistent input
            break;
        }
        if (nx >= n || len >= n) { len = FWX_ERR_CYCLE; break; }
        if (edge) prod *= (double)edge[(size_t)cur * n + nx];
        if (path_out && len < cap) path_out[(size_t)q * cap + len] = nx;
        ++len;
        cur = nx;
        if (cur == d) break;
    }
    len_out[q] = len;
    if (prod_out) prod_out[q] = len > 0 ? prod : 0.0;
}

int check_slab(const fwx_slab *s)
{
    if (!s || s->n < 0 || s->rows < 0 || s->row0 < 0 || (int64_t)s->row0 + s->rows > s->n ||
        (s->dtype != FWX_F32 && s->dtype != FWX_F64) || (s->hops && !s->next))
        return FWX_ERR_INVALID;
    if (s->rows > 0 && s->n > 0 && !s->rate) return FWX_ERR_INVALID;
    return FWX_OK;
}

template <typename T>
int panel_impl(const fwx_slab *b, T *w, int32_t *w_hops, unsigned long long *d_updates,
                      hipStream_t s)
{
    const int n = b->n, k0 = b->row0, B = b->rows;
    T *rows = (T *)b->rate;
    fwx::RelaxArgs<T> a;
    a.rate = rows; a.next = b->next; a.hops = b->hops;
    a.rows = B; a.n = n; a.row0 = k0; a.updates = d_updates; a.flip = 0; a.plog = fwx::PathLog();
    for (int t = 0; t < B; ++t) {
        // Time-k snapshot of pivot row k = k0+t: every pivot < k has been applied, pivot k
        // leaves row k unchanged (Algorithms.hs:50), later pivots will change it.
        FWX_HIP(fwx::launch_snapshot_row<T>(w + (size_t)t * n, rows + (size_t)t * n,
                                            b->hops ? w_hops + (size_t)t * n : nullptr,
                                            b->hops ? b->hops + (size_t)t * n : nullptr, n, s));
        a.prow = w + (size_t)t * n;
        a.phops = b->hops ? w_hops + (size_t)t * n : nullptr;
        // the list rule in full (an empty ikPath takes next[k][j]): next-hop row k at time k is the block's own
        // row t, which step k leaves alone
        a.pnext = b->next ? b->next + (size_t)t * n : nullptr;
        a.k = k0 + t;
        FWX_HIP(fwx::launch_relax<T>(a, s));
    }
    return FWX_OK;
}

}  // namespace

// ---- path queries of both handle kinds (fwx_query.h) ------------------------------------------------
namespace fwxi {

// Single-thread device walk of the next-hop matrix (fwx_matrix_query).
__global__ void follow_path_kernel(EntryTab t, int n_real, int src, int dst, int32_t *out, int cap,
                                   int32_t *len_out)
{
    int len = 0, cur = src, p;
    {
        const size_t off = t.locate(src, dst, p);
        if (t.next[p][off] < 0) { *len_out = 0; return; }
    }
    while (cur != dst || len == 0) {
        const size_t off = t.locate(cur, dst, p);
        const int nx = t.next[p][off];
        if (nx < 0 || nx >= n_real || len >= n_real) { *len_out = FWX_ERR_CYCLE; return; }
        if (len >= cap) { *len_out = FWX_ERR_CAPACITY; return; }
        out[len++] = nx;
        cur = nx;
    }
    *len_out = len;
}

// The reference's `_path` list of entry (src,dst), rebuilt from the path trace exactly as
// Algorithms.hs:55 built it: the newest update of (a,b) before time T, by pivot q, splits the path
// into path_q(a,q) ++ path_q(q,b); an entry with no update before T still has its buildMatrix path
// ([b] if next0[a][b] >= 0, else []).  T is the end of the solve for the query itself (`last`), and
// for every sub-entry it is the step named by one of its own indices: (a,q) at time q is read from
// at_col, (q,b) at time q from at_row.  Iterative, one thread: the list goes to out (cap entries), the
// stack holds (a, b, kind) triples.  The length, or FWX_ERR_CAPACITY if the LIST is longer than cap.
//
// The stack is sized by the order, not by cap (exact_stack_triples).  Along any descent the pivots strictly
// decrease -- at_col[a][q] and at_row[q][b] are pivots applied before step q -- so an item at depth d has d + 1
// distinct pivots above it, d <= n - 1, and with one pending sibling per level the stack never holds more than
// n + 1 triples.  cap cannot bound it: on the reference's domain every pending item yields at least one list
// entry, outside it (a leaf with next0 < 0, an update whose ikPath was empty) a pending item can yield nothing,
// and a list of length L can need more than L triples.  The depth test below cannot fire on a trace a solve
// wrote; it keeps a corrupted one inside the scratch.
__host__ __device__ constexpr size_t exact_stack_triples(int n_real) { return (size_t)n_real + 2; }
static_assert(FWX_EXACT_SCRATCH_INTS(128) == 3 * exact_stack_triples(128), "fwx.h states the walk's scratch per item");
static_assert(FWX_EXACT_SCRATCH_INTS(FWX_BATCH_MID_MAX_N) == 3 * exact_stack_triples(FWX_BATCH_MID_MAX_N),
              "... at the mid tier's largest order too (fwx_dev_exact_paths_batch_mid)");
static_assert(FWX_EXACT_SCRATCH_INTS(FWX_BATCH_LARGE_MAX_N) == 3 * exact_stack_triples(FWX_BATCH_LARGE_MAX_N),
              "... and at the large tier's (fwx_dev_exact_paths_batch_large)");

template <typename Tab>
__device__ int exact_walk(const Tab &t, int n_real, int src, int dst, int32_t *out, int32_t *stack, int cap)
{
    enum { FINAL = WALK_FINAL, AS_COLUMN = WALK_AS_COLUMN, AS_ROW = WALK_AS_ROW };
    const int scap = (int)exact_stack_triples(n_real);
    int sp = 0, len = 0;
    stack[0] = src; stack[1] = dst; stack[2] = FINAL; sp = 1;
    while (sp > 0) {
        --sp;
        const int a = stack[3 * sp], b = stack[3 * sp + 1], kind = stack[3 * sp + 2];
        const typename Tab::Cell cell = t.cell(a, b);
        const int q = t.pivot(cell, kind);
        if (q < 0) {
            if (t.edge(cell)) {
                if (len >= cap) return FWX_ERR_CAPACITY;
                out[len++] = b;
            }
        } else {
            if (sp + 2 > scap || q >= n_real) return FWX_ERR_CYCLE;
            stack[3 * sp] = q; stack[3 * sp + 1] = b; stack[3 * sp + 2] = AS_ROW; ++sp;      // second half
            stack[3 * sp] = a; stack[3 * sp + 1] = q; stack[3 * sp + 2] = AS_COLUMN; ++sp;   // first half
        }
    }
    return len;
}

// Batch form: one thread per (src[q], dst[q]); query q writes its list to paths + q*cap and uses
// stacks + q * 3 * exact_stack_triples(n_real) as its stack.  len_out[q] = length, or the error of that item.
__global__ __launch_bounds__(64) void exact_paths_kernel(EntryTab t, int n_real, int count, const int32_t *src,
                                                         const int32_t *dst, int32_t *paths, int32_t *stacks,
                                                         int cap, int32_t *len_out)
{
    const int qi = blockIdx.x * 64 + threadIdx.x;
    if (qi >= count) return;
    const int s0 = src[qi], d0 = dst[qi];
    if (s0 < 0 || d0 < 0 || s0 >= n_real || d0 >= n_real) { len_out[qi] = FWX_ERR_INVALID; return; }
    len_out[qi] = exact_walk(t, n_real, s0, d0, paths + (size_t)qi * cap,
                             stacks + (size_t)qi * 3 * exact_stack_triples(n_real), cap);
}

// One list of the order-n matrix that starts at element `off` of the four arrays of a traced batch, pitch n.
__device__ __forceinline__ int walk_batch_item(size_t off, int n, const int32_t *next0, const fwx::PathLog &plog,
                                               int src, int dst, int32_t *out, int32_t *stack, int cap)
{
    BatchTab t;
    t.n = n;
    t.last = plog.last + off;
    t.at_col = plog.at_col + off;
    t.at_row = plog.at_row + off;
    t.next0 = next0 + off;
    return exact_walk(t, n, src, dst, out, stack, cap);
}

// The same over a traced batch (fwx_dev_exact_paths_batch): item q is (mat[q], src[q], dst[q]), matrix m of the
// batch at + m*stride in each of the four arrays, pitch n.  An item outside the batch gets FWX_ERR_INVALID, alone.
__global__ __launch_bounds__(64) void exact_paths_batch_kernel(int count, int n, long long stride,
                                                               const int32_t *next0, fwx::PathLog plog, int items,
                                                               const int32_t *mat, const int32_t *src,
                                                               const int32_t *dst, int32_t *paths, int32_t *stacks,
                                                               int cap, int32_t *len_out)
{
    const int qi = blockIdx.x * 64 + threadIdx.x;
    if (qi >= items) return;
    const int m0 = mat[qi], s0 = src[qi], d0 = dst[qi];
    if (m0 < 0 || m0 >= count || s0 < 0 || d0 < 0 || s0 >= n || d0 >= n) { len_out[qi] = FWX_ERR_INVALID; return; }
    len_out[qi] = walk_batch_item((size_t)m0 * (size_t)stride, n, next0, plog, s0, d0, paths + (size_t)qi * cap,
                                  stacks + (size_t)qi * 3 * exact_stack_triples(n), cap);
}

int launch_exact_batch(int count, int n, long long stride, const int32_t *next0, const fwx::PathLog &plog,
                       int items, const int32_t *mat, const int32_t *src, const int32_t *dst, int32_t *len_out,
                       int32_t *paths, int cap, int32_t *stacks, hipStream_t s)
{
    if (items <= 0) return FWX_OK;
    hipLaunchKernelGGL(exact_paths_batch_kernel, dim3((unsigned)(((size_t)items + 63) / 64)), dim3(64), 0, s, count,
                       n, stride, next0, plog, items, mat, src, dst, paths, stacks, cap, len_out);
    FWX_HIP(hipGetLastError());
    return FWX_OK;
}

// The same over a traced ragged batch (fwx_dev_exact_paths_ragged): matrix m has its own order n_each[m] and starts
// at offset[m].  src / dst are checked against the order of the item's OWN matrix; an order-0 matrix has no valid
// item.  The stacks are spaced by n_max, so an order above it (a plan that does not belong here) is refused too.
__global__ __launch_bounds__(64) void exact_paths_ragged_kernel(int count, const int32_t *n_each,
                                                                const int64_t *offset, int n_max,
                                                                const int32_t *next0, fwx::PathLog plog, int items,
                                                                const int32_t *mat, const int32_t *src,
                                                                const int32_t *dst, int32_t *paths, int32_t *stacks,
                                                                int cap, int32_t *len_out)
{
    const int qi = blockIdx.x * 64 + threadIdx.x;
    if (qi >= items) return;
    const int m0 = mat[qi], s0 = src[qi], d0 = dst[qi];
    if (m0 < 0 || m0 >= count) { len_out[qi] = FWX_ERR_INVALID; return; }
    const int n = n_each[m0];
    if (n > n_max || s0 < 0 || d0 < 0 || s0 >= n || d0 >= n) { len_out[qi] = FWX_ERR_INVALID; return; }
    len_out[qi] = walk_batch_item((size_t)offset[m0], n, next0, plog, s0, d0, paths + (size_t)qi * cap,
                                  stacks + (size_t)qi * 3 * exact_stack_triples(n_max), cap);
}

int launch_exact_ragged(int count, const int32_t *n_each, const int64_t *offset, int n_max, const int32_t *next0,
                        const fwx::PathLog &plog, int items, const int32_t *mat, const int32_t *src,
                        const int32_t *dst, int32_t *len_out, int32_t *paths, int cap, int32_t *stacks, hipStream_t s)
{
    if (items <= 0) return FWX_OK;
    hipLaunchKernelGGL(exact_paths_ragged_kernel, dim3((unsigned)(((size_t)items + 63) / 64)), dim3(64), 0, s, count,
                       n_each, offset, n_max, next0, plog, items, mat, src, dst, paths, stacks, cap, len_out);
    FWX_HIP(hipGetLastError());
    return FWX_OK;
}

// One query, the pair by value (checked by the caller): nothing is copied in before the launch.  `walk` holds
// the list (cap entries), then the stack (3 * exact_stack_triples(n_real) entries).
__global__ void exact_path_kernel(EntryTab t, int n_real, int src, int dst, int32_t *walk, int cap, int32_t *len_out)
{
    *len_out = exact_walk(t, n_real, src, dst, walk, walk + cap, cap);
}

// What a one-query kernel just launched on `s` leaves: the length (or error) at len_dev, which is returned,
// and that many entries at list_dev, which go to path_out.
static int read_list(hipStream_t s, const int32_t *len_dev, const int32_t *list_dev, int32_t *path_out)
{
    FWX_HIP(hipGetLastError());
    int32_t len = 0;
    FWX_HIP(hipMemcpyAsync(&len, len_dev, 4, hipMemcpyDeviceToHost, s));
    FWX_HIP(hipStreamSynchronize(s));
    if (len > 0) {
        FWX_HIP(hipMemcpyAsync(path_out, list_dev, (size_t)len * 4, hipMemcpyDeviceToHost, s));
        FWX_HIP(hipStreamSynchronize(s));
    }
    return len;
}

int run_follow(const EntryTab &tab, int n_real, hipStream_t s, int32_t *scratch, int32_t src, int32_t dst,
               int32_t *path_out, int32_t cap)
{
    const int dcap = cap < n_real ? cap : n_real;
    hipLaunchKernelGGL(follow_path_kernel, dim3(1), dim3(1), 0, s, tab, n_real, src, dst, scratch + 1, dcap,
                       scratch);
    return read_list(s, scratch, scratch + 1, path_out);
}

int run_exact_batch(const EntryTab &tab, int n_real, hipStream_t s, int32_t count, const int32_t *src,
                    const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap)
{
    // device scratch from a pooled per-call context: no hipMalloc / hipFree per query (and no hipFree
    // right behind the kernel that used the memory: drain_stream in fwx_internal.h)
    CtxLease lease;
    int rc = lease.open();
    if (rc) return rc;
    lease.c->uses_stream(s);             // the kernel below runs on the handle's stream
    const size_t c = (size_t)count;
    void *ids = nullptr, *d_paths = nullptr, *d_stacks = nullptr;
    if ((rc = lease.c->reserve(CallCtx::NEXT, c * 12, &ids)) ||
        (rc = lease.c->reserve(CallCtx::RATE, c * cap * 4, &d_paths)) ||
        (rc = lease.c->reserve(CallCtx::WS, c * exact_stack_triples(n_real) * 12, &d_stacks)))
        return rc;
    int32_t *const d_src = (int32_t *)ids, *const d_dst = d_src + c, *const d_len = d_dst + c;
    FWX_HIP(hipMemcpyAsync(d_src, src, c * 4, hipMemcpyHostToDevice, s));
    FWX_HIP(hipMemcpyAsync(d_dst, dst, c * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(exact_paths_kernel, dim3((unsigned)((c + 63) / 64)), dim3(64), 0, s, tab, n_real, count,
                       (const int32_t *)d_src, (const int32_t *)d_dst, (int32_t *)d_paths, (int32_t *)d_stacks, cap,
                       d_len);
    FWX_HIP(hipGetLastError());
    FWX_HIP(hipMemcpyAsync(len_out, d_len, c * 4, hipMemcpyDeviceToHost, s));
    FWX_HIP(hipMemcpyAsync(path_out, d_paths, c * cap * 4, hipMemcpyDeviceToHost, s));
    FWX_HIP(hipStreamSynchronize(s));
    return FWX_OK;
}

}  // namespace fwxi

namespace {
// A single-device handle as the query table: one partition of all nd rows.
EntryTab tab_of(const fwx_matrix *m)
{
    EntryTab t;
    memset(&t, 0, sizeof(t));
    t.parts = 1;
    t.nd = m->nd;
    t.row0[1] = m->nd;
    t.next[0] = m->slab.next;
    t.last[0] = m->slab.plog.last;
    t.at_col[0] = m->slab.plog.at_col;
    t.at_row[0] = m->slab.plog.at_row;
    t.next0[0] = m->slab.next0;
    return t;
}

template <typename T>
int matrix_solve_typed(fwx_matrix *m, const Opts &op, unsigned long long *upd, hipStream_t s, CallCtx *cx)
{
    const int n = m->n, nd = m->nd;      // order of the matrix; order (= pitch) of the device arrays
    const SlabData &d = m->slab;
    T *r = (T *)d.rate;
    Route route;
    bool nonneg = false;
    int *d_flag = m->flag;
    int rc;
    if (!d_flag) {                       // fwx_dev_solve: a view of caller-owned memory + a pooled context
        if (!cx) return FWX_ERR_INVALID;
        void *small = nullptr;
        if ((rc = cx->reserve(CallCtx::SMALL, (FWX_UPDATE_SHARDS + 2) * sizeof(unsigned long long), &small))) return rc;
        d_flag = (int *)((unsigned long long *)small + FWX_UPDATE_SHARDS);
    }
    m->fresh = 0;                        // whatever happens next, the arrays are no longer the upload
    if ((rc = route_solve<T>(op, n, nd, r, d.next, d.hops, upd != nullptr, d_flag, s, route, nonneg,
                             m->flag ? m : nullptr)))
        return rc;
    if (route == ROUTE_SMALL) {
        if (m->resume) { m->resume->valid_upto = 0; m->resume->state_at = -1; }
        FWX_HIP(fwx::launch_small_solve<T>(r, d.next, d.hops, nd, op.k_begin, op.k_end, upd,
                                           d.plog, s));
        return FWX_OK;
    }
    if (route == ROUTE_FUSED) {
        // a handle keeps its workspace and look-ahead stream across solves; a view borrows the
        // pooled context's
        const size_t need = fused_ws_bytes(nd, sizeof(T), d.hops != nullptr);
        void *ws = nullptr;
        SideStream *side = nullptr;
        if (m->flag) {
            if (m->ws_bytes < need) {
                if (m->ws) {
                    drain_stream(s);
                    if (m->side) m->side->drain();
                    (void)hipFree(m->ws); m->ws = nullptr; m->ws_bytes = 0;
                }
                FWX_HIP(hipMalloc(&m->ws, need));
                m->ws_bytes = need;
            }
            if (!m->side) {
                m->side = new (std::nothrow) SideStream();
                if (!m->side) return FWX_ERR_OOM;
            }
            ws = m->ws;
            side = m->side;
        } else {
            if ((rc = cx->reserve(CallCtx::WS, need, &ws))) return rc;
            side = &cx->side;
        }
        // a resumable handle records the panels of every pass and the checkpoints it walks over -- if
        // this solve continues the kept input's own solve (the arrays are that input at time k_begin)
        Resume *rec = nullptr;
        if (m->flag && m->resume) {
            Resume &R = *m->resume;
            const bool chain = m->kept_valid && R.state_at == op.k_begin && op.k_begin % FWX_FUSED_B == 0 &&
                               op.k_begin <= R.valid_upto;
            R.valid_upto = chain ? op.k_begin : 0;      // beyond k_begin: an older solve's, until this one ends
            R.state_at = -1;
            if (chain) rec = &R;
        }
        rc = fused_range<T>(r, d.next, d.hops, nd, op.k_begin, op.k_end, ws, upd, s, d.plog, nonneg, side, rec,
                            &m->slab.store);
        if (rc) return rc;
        FWX_HIP(hipStreamSynchronize(s));
        if (rec) rec->valid_upto = rec->state_at = op.k_end;
        return FWX_OK;
    }
    if (m->resume) { m->resume->valid_upto = 0; m->resume->state_at = -1; }   // nothing was recorded
    PerkRange<T> pr = PerkRange<T>::whole(r, d.next, d.hops, nd, op.k_begin, op.k_end);
    pr.serpentine = op.serpentine; pr.d_updates = upd; pr.stream = s; pr.plog = d.plog;
    return relax_range<T>(pr);
}

// Solve with the path trace (PathLog): one pass.  `last` starts at -1 everywhere; the kernels set
// it on every successful relaxation and copy its column k / row k into at_col / at_row at step k.
// resumed: the arrays AND the trace hold a restored checkpoint at time op.k_begin
// (fwx_matrix_resolve); the solve continues from there to the end.
int logged_solve(fwx_matrix *m, const Opts &op_in, hipStream_t s, bool resumed = false)
{
    if ((!resumed && op_in.k_begin != 0) || op_in.k_end != m->n)
        return FWX_ERR_UNSUPPORTED;              // the trace covers whole solves
    if (!resumed && !m->fresh) return FWX_ERR_INVALID;   // a traced solve starts from an uploaded input
    const Opts &op = op_in;                      // engines as for any matrix: single launch, fused
                                                 //   (no hops), per-k -- all three keep the trace
    const size_t nn = (size_t)m->nd * (size_t)m->nd;
    if (!resumed) {
        FWX_HIP(hipMemsetAsync(m->slab.plog.last, 0xFF, nn * 4, s));
        FWX_HIP(hipMemsetAsync(m->slab.plog.at_col, 0xFF, nn * 4, s));
        FWX_HIP(hipMemsetAsync(m->slab.plog.at_row, 0xFF, nn * 4, s));
    }
    unsigned long long *upd = op.updates_out ? m->upd : nullptr;   // counting costs registers
    if (upd) FWX_HIP(hipMemsetAsync(upd, 0, FWX_UPDATE_SHARDS * 8, s));
    m->fresh = 0;
    m->last_u = 0;
    const int rc = m->dtype == FWX_F64 ? matrix_solve_typed<double>(m, op, upd, s)
                                       : matrix_solve_typed<float>(m, op, upd, s);
    if (rc) return rc;
    if (upd) {
        uint64_t u = 0;
        const int rc2 = sum_updates(upd, &u, s);   // synchronises
        if (rc2) return rc2;
        m->last_u = u;
        *op.updates_out = u;
    } else {
        FWX_HIP(hipStreamSynchronize(s));
    }
    m->rec_ready = 1;
    return FWX_OK;
}

// ---- the data operations of a handle, once for both kinds: loops over its slabs (fwx_handle.h) --------

// The device of a single-device handle becomes current, with DeviceGuard::enter's checks; the slabs of a
// partitioned handle select theirs as they are visited.
int enter_handle(DeviceGuard &g, const fwx_matrix *m) { return m->multi ? FWX_OK : g.enter(m->device); }

// The rows of slab `d` that exist in the caller's n x n arrays (the last slab also holds the padding rows) ...
int real_rows(const fwx_matrix *m, const SlabData &d) { return d.row0 + d.rows <= m->n ? d.rows : m->n - d.row0; }
// ... to (`in`) or from the slab's array `dev` of pitch nd.  `host` is the caller's array, host or device memory
// (hipMemcpyDefault): all n rows -- or, with one partition per process, just this slab's.  One flat copy where
// nd == n on a single-device handle; partitions always take the 2-D form, as they always did, so that merging
// the two kinds changed no HIP call there.
int copy_rows(const fwx_matrix *m, const SlabData &d, void *dev, void *host, size_t es, bool in)
{
    const size_t n = (size_t)m->n, nd = (size_t)m->nd;
    const int real = real_rows(m, d);
    if (!host || real <= 0) return FWX_OK;
    if (!m->multi || multi_self(m) < 0) host = (char *)host + (size_t)d.row0 * n * es;
    void *dst = in ? dev : host;
    const void *src = in ? host : dev;
    if (nd == n && !m->multi) FWX_HIP(hipMemcpyAsync(dst, src, (size_t)real * n * es, hipMemcpyDefault, d.main));
    else FWX_HIP(hipMemcpy2DAsync(dst, (in ? nd : n) * es, src, (in ? n : nd) * es, n * es, (size_t)real,
                                  hipMemcpyDefault, d.main));
    return FWX_OK;
}

// The patched entries (indices of the caller's n x n view) into the kept input, each on the slab that owns its
// row (an entry of a row another process holds is skipped); offs, if given: per slab, their offsets in its
// arrays.
int patch_kept_entries(fwx_matrix *m, DeviceGuard &g, int32_t count, const int64_t *index, const void *rate_vals,
                     const int32_t *next_vals, const int32_t *hops_vals, std::vector<int64_t> *offs = nullptr)
{
    const size_t es = m->dtype == FWX_F64 ? 8 : 4;
    return each_slab(m, &g, [&](SlabData &d, int p) -> int {
        const Slab v = slab_of(d, m->nd, es);
        for (int32_t q = 0; q < count; ++q) {
            const int64_t row = index[q] / m->n - d.row0;
            if (row < 0 || row >= d.rows) continue;
            const size_t off = (size_t)row * (size_t)m->nd + (size_t)(index[q] % m->n);
            if (offs) offs[p].push_back((int64_t)off);
            const int rc = patch_kept(v, off, q, rate_vals, next_vals, hops_vals);
            if (rc) return rc;
        }
        return FWX_OK;
    });
}

}  // namespace

extern "C" {

int fwx_abi_version(void) { return FWX_ABI_VERSION; }

int fwx_device_count(void) { return device_count(); }

int fwx_last_hip_error(void) { return g_last_hip; }

int fwx_hip_versions(int32_t *built_against, int32_t *runtime)
{
    if (built_against) *built_against = HIP_VERSION;
    int v = 0;
    if (hipRuntimeGetVersion(&v) != hipSuccess) {
        (void)hipGetLastError();
        v = 0;
    }
    if (runtime) *runtime = v;
    // same major.minor: HIP_VERSION = major * 10^7 + minor * 10^5 + patch
    return (v / 100000 == HIP_VERSION / 100000) ? 1 : 0;
}

int fwx_test_fail_after(int32_t countdown)
{
    g_fail_countdown = countdown > 0 ? countdown : 0;
    return FWX_OK;
}

int fwx_test_kernel_forms(uint64_t *seen, int reset)
{
    if (seen) *seen = reset ? fwx::g_kernel_forms.exchange(0, std::memory_order_relaxed)
                            : fwx::g_kernel_forms.load(std::memory_order_relaxed);
    else if (reset) fwx::g_kernel_forms.store(0, std::memory_order_relaxed);
    return fwx::KF_COUNT;
}

int fwx_test_pools(uint64_t *out, int reset)
{
    static const uint64_t cap[POOL_COUNT] = {kCtxPoolMaxFree, kPerkScratchMax, kMultiPoolMaxIdle};
    for (int i = 0; i < POOL_COUNT; ++i) {
        PoolStats &st = g_pool_stats[i];
        const uint64_t leased = st.leased.load(std::memory_order_relaxed);
        const uint64_t v[4] = {cap[i],
                               reset ? st.created.exchange(0, std::memory_order_relaxed)
                                     : st.created.load(std::memory_order_relaxed),
                               reset ? st.destroyed.exchange(0, std::memory_order_relaxed)
                                     : st.destroyed.load(std::memory_order_relaxed),
                               reset ? st.peak.exchange(leased, std::memory_order_relaxed)
                                     : st.peak.load(std::memory_order_relaxed)};
        if (out)
            for (int j = 0; j < 4; ++j) out[4 * i + j] = v[j];
    }
    return POOL_COUNT;
}

const char *fwx_test_kernel_form_name(int form)
{
    static const char *const names[] = {
#define FWX_KERNEL_FORM_NAME(name) #name,
        FWX_KERNEL_FORM_LIST(FWX_KERNEL_FORM_NAME)
#undef FWX_KERNEL_FORM_NAME
    };
    return form >= 0 && form < fwx::KF_COUNT ? names[form] : nullptr;
}

const char *fwx_strerror(int status)
{
    switch (status) {
    case FWX_OK: return "ok";
    case FWX_ERR_INVALID: return "invalid argument";
    case FWX_ERR_NO_DEVICE: return "no HIP device visible (libfwx has no CPU fallback)";
    case FWX_ERR_HIP: return "HIP runtime error";
    case FWX_ERR_OOM: return "out of memory";
    case FWX_ERR_CYCLE: return "next-hop walk does not reach the destination (cycle)";
    case FWX_ERR_CAPACITY: return "output buffer too small";
    case FWX_ERR_UNSUPPORTED: return "unsupported option combination";
    case FWX_ERR_RCCL: return "RCCL could not be loaded or an RCCL call failed";
    case FWX_ERR_INTERNAL: return "internal error (an exception was stopped at the C ABI)";
    default: return "unknown status";
    }
}

int fwx_solve_f64(int32_t n, double *rate, int32_t *next, int32_t *hops, const fwx_opts *opts)
{
    return fwxi::guarded([&]() -> int { return solve_host<double>(n, rate, next, hops, opts); });
}

int fwx_solve_f32(int32_t n, float *rate, int32_t *next, int32_t *hops, const fwx_opts *opts)
{
    return fwxi::guarded([&]() -> int { return solve_host<float>(n, rate, next, hops, opts); });
}

int fwx_follow_path(int32_t n, const int32_t *next, int32_t src, int32_t dst, int32_t *out,
                    int32_t cap)
{
    return fwxi::guarded([&]() -> int {
        if (n < 0 || !next || src < 0 || dst < 0 || src >= n || dst >= n || cap < 0 ||
            (cap > 0 && !out))
            return FWX_ERR_INVALID;
        const size_t N = (size_t)n;
        if (next[(size_t)src * N + dst] < 0) return 0;
        int32_t len = 0, cur = src;
        while (cur != dst || len == 0) {
            const int32_t nx = next[(size_t)cur * N + dst];
            if (nx < 0 || nx >= n || len >= n) return FWX_ERR_CYCLE;
            if (len >= cap) return FWX_ERR_CAPACITY;
            out[len++] = nx;
            cur = nx;
        }
        return len;
    });
}

int fwx_matrix_create(fwx_matrix **out, int32_t n, int32_t dtype, int32_t with_next,
                      int32_t with_hops, int32_t device)
{
    return fwxi::guarded([&]() -> int {
        if (!out || n < 0 || (dtype != FWX_F32 && dtype != FWX_F64) || (with_hops && !with_next))
            return FWX_ERR_INVALID;
        *out = nullptr;
        DeviceGuard g;
        int rc = g.enter(device);
        if (rc) return rc;
        int dev = 0;
        FWX_HIP(hipGetDevice(&dev));
        fwx_matrix *m = new (std::nothrow) fwx_matrix();
        if (!m) return FWX_ERR_OOM;
        memset(m, 0, sizeof(*m));
        m->n = n; m->dtype = dtype; m->device = dev;
        m->with_next = with_next != 0; m->with_hops = with_hops != 0;
        const size_t es = dtype == FWX_F64 ? 8 : 4;
        // rows of 16-byte vectors for any n (fwx_matrix::nd): the arrays are nd x nd, the padding is
        // written here, once -- nothing ever stores a different value into it
        const int vw = (int)(16 / es);
        m->nd = (n + vw - 1) / vw * vw;
        SlabData &d = m->slab;               // the one slab: all rows
        d = SlabData();
        d.device = dev; d.rows = m->nd; d.ct_ld = (m->nd + 3) & ~3;
        const size_t nn = (size_t)m->nd * (size_t)m->nd;
        hipError_t e = hipMalloc(&d.rate, nn * es ? nn * es : 1);
        if (e == hipSuccess && with_next) e = hipMalloc((void **)&d.next, nn * 4 ? nn * 4 : 1);
        if (e == hipSuccess && with_hops) e = hipMalloc((void **)&d.hops, nn * 4 ? nn * 4 : 1);
        if (e == hipSuccess) e = hipMalloc((void **)&m->scratch, ((size_t)n + 2) * 4);
        if (e == hipSuccess) e = hipMalloc((void **)&m->upd, FWX_UPDATE_SHARDS * 8);
        if (e == hipSuccess) e = hipMalloc((void **)&m->flag, 16);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&d.main, hipStreamNonBlocking);
        if (e == hipSuccess && m->nd != n) {
            e = hipMemsetAsync(d.rate, 0, nn * es, d.main);                                  // +0.0
            if (e == hipSuccess && d.next) e = hipMemsetAsync(d.next, 0xFF, nn * 4, d.main);   // -1
            if (e == hipSuccess && d.hops) e = hipMemsetAsync(d.hops, 0, nn * 4, d.main);
            if (e == hipSuccess) e = hipStreamSynchronize(d.main);
        }
        if (e != hipSuccess) {
            g_last_hip = (int)e;
            (void)hipGetLastError();
            fwx_matrix_destroy(m);
            return e == hipErrorOutOfMemory ? FWX_ERR_OOM : FWX_ERR_HIP;
        }
        *out = m;
        return FWX_OK;
    });
}

int fwx_matrix_destroy(fwx_matrix *m)
{
    return fwxi::guarded([&]() -> int {
        if (!m) return FWX_OK;
        // order, on either kind: retire every command that used the arrays, then the streams and their
        // events, then the memory; a slab's own stream, arrays and store go in slab_release
        if (m->multi) {
            multi_destroy(m);
        } else {
            DeviceGuard g;
            (void)g.enter(m->device);
            drain_stream(m->slab.main);
            if (m->side) m->side->drain();
            delete m->side;
            slab_release(m->slab);
            if (m->scratch) (void)hipFree(m->scratch);
            if (m->upd) (void)hipFree(m->upd);
            if (m->walk) (void)hipFree(m->walk);
            if (m->ws) (void)hipFree(m->ws);
            if (m->flag) (void)hipFree(m->flag);
        }
        delete m->resume;
        delete m;
        return FWX_OK;
    });
}

int fwx_matrix_upload(fwx_matrix *m, const void *rate, const int32_t *next, const int32_t *hops)
{
    return fwxi::guarded([&]() -> int {
        if (!m) return FWX_ERR_INVALID;
        if (m->n == 0) return FWX_OK;
        if (!rate || (m->with_next && !next) || (m->with_hops && !hops)) return FWX_ERR_INVALID;
        DeviceGuard g;
        int rc = enter_handle(g, m);
        if (rc) return rc;
        const size_t es = m->dtype == FWX_F64 ? 8 : 4;
        m->dom_known = 0;                  // a new input: the domain check has to look at it
        if (m->resume) m->resume->valid_upto = 0;   // ... and nothing of the old solve can be resumed
        // the sources may be host arrays (what an FFI hands over) or device arrays (a caller that keeps its
        // pristine input in HBM, e.g. the benchmark)
        rc = each_slab(m, &g, [&](SlabData &d, int) -> int {
            const size_t cells = (size_t)d.rows * (size_t)m->nd;
            if (m->multi && m->nd != m->n) {      // a partitioned handle writes its padding on every upload
                FWX_HIP(hipMemsetAsync(d.rate, 0, cells * es, d.main));                   // +0.0
                if (d.next) FWX_HIP(hipMemsetAsync(d.next, 0xFF, cells * 4, d.main));     // -1
                if (d.hops) FWX_HIP(hipMemsetAsync(d.hops, 0, cells * 4, d.main));
            }
            if (real_rows(m, d) <= 0) return FWX_OK;   // (an empty partition)
            int rc2;
            if ((rc2 = copy_rows(m, d, d.rate, const_cast<void *>(rate), es, true))) return rc2;
            if (d.next && (rc2 = copy_rows(m, d, d.next, const_cast<int32_t *>(next), 4, true))) return rc2;
            if (d.hops && (rc2 = copy_rows(m, d, d.hops, const_cast<int32_t *>(hops), 4, true))) return rc2;
            // traced matrix: keep the uploaded next-hops (paths of entries never improved); kept input: all of it
            return keep_live(slab_of(d, m->nd, es));
        });
        if (rc) return rc;
        if (m->traced || (m->keep && m->with_next)) m->rec_ready = 0;   // (a next0 exists) the trace of an earlier input is stale
        if (m->keep) m->kept_valid = 1;
        if ((rc = sync_slabs(m, g))) return rc;
        m->fresh = 1;
        if (m->resume) m->resume->state_at = m->keep ? 0 : -1;
        return FWX_OK;
    });
}

int fwx_matrix_enable_path_log(fwx_matrix *m)
{
    return fwxi::guarded([&]() -> int {
        if (!m || !m->with_next || m->traced) return FWX_ERR_INVALID;
        if (m->resume) return FWX_ERR_INVALID;     // the checkpoints were sized without the trace: enable it first
        if (m->n == 0) return FWX_OK;
        DeviceGuard g;
        int rc = enter_handle(g, m);
        if (rc) return rc;
        rc = each_slab(m, &g, [&](SlabData &d, int) -> int {
            return trace_alloc(d, (size_t)d.rows * (size_t)m->nd, m->fresh);
        });
        if (rc) return rc;
        m->traced = 1;
        m->rec_ready = 0;
        return FWX_OK;
    });
}

int fwx_matrix_keep_input(fwx_matrix *m)
{
    return fwxi::guarded([&]() -> int {
        if (!m) return FWX_ERR_INVALID;
        if (m->keep || m->n == 0) return FWX_OK;
        DeviceGuard g;
        int rc = enter_handle(g, m);
        if (rc) return rc;
        const size_t es = m->dtype == FWX_F64 ? 8 : 4;
        rc = each_slab(m, &g, [&](SlabData &d, int) -> int {
            const int rc2 = kept_alloc(d, (size_t)d.rows * (size_t)m->nd, es);
            if (rc2 || !m->fresh) return rc2;
            return keep_live(slab_of(d, m->nd, es));     // an unsolved upload is in the arrays: the input to keep
        });
        if (rc) return rc;
        m->keep = 1;
        if (m->fresh) {
            if ((rc = sync_slabs(m, g))) return rc;
            m->kept_valid = 1;
        }
        return FWX_OK;
    });
}

int fwx_matrix_patch_input(fwx_matrix *m, int32_t count, const int64_t *index, const void *rate_vals,
                           const int32_t *next_vals, const int32_t *hops_vals)
{
    return fwxi::guarded([&]() -> int {
        if (!m || count < 0 || count > FWX_MAX_PATCH || (count > 0 && (!index || !rate_vals)))
            return FWX_ERR_INVALID;
        if (!m->keep || !m->kept_valid) return FWX_ERR_INVALID;
        if ((next_vals && !m->with_next) || (hops_vals && !m->with_hops)) return FWX_ERR_INVALID;
        const int64_t nn64 = (int64_t)m->n * m->n;
        for (int32_t q = 0; q < count; ++q)
            if (index[q] < 0 || index[q] >= nn64) return FWX_ERR_INVALID;
        DeviceGuard g;
        int rc = enter_handle(g, m);
        if (rc) return rc;
        const size_t es = m->dtype == FWX_F64 ? 8 : 4;
        if (m->resume) m->resume->valid_upto = 0;   // the kept input changes without a replay
        // the remembered domain answer survives a patch whose values are themselves inside the domain
        // (rate >= +0 and not NaN; a non-zero rate comes with a next-hop >= 0); anything else, or a
        // non-zero rate patched in without its next-hop, sends the next solve through the check again
        if (m->dom_known && !patch_keeps_domain(m, count, rate_vals, next_vals)) m->dom_known = 0;
        if ((rc = patch_kept_entries(m, g, count, index, rate_vals, next_vals, hops_vals))) return rc;
        if ((rc = each_slab(m, &g, [&](SlabData &d, int) -> int { return restore_kept(slab_of(d, m->nd, es)); })))
            return rc;
        if ((rc = sync_slabs(m, g))) return rc;
        m->fresh = 1;
        m->rec_ready = 0;
        if (m->resume) m->resume->state_at = 0;      // the patched kept input, unsolved
        return FWX_OK;
    });
}

int fwx_device_memory(int32_t device, uint64_t *free_bytes, uint64_t *total_bytes)
{
    return fwxi::guarded([&]() -> int {
        DeviceGuard g;
        int rc = g.enter(device);
        if (rc) return rc;
        size_t f = 0, t = 0;
        FWX_HIP(hipMemGetInfo(&f, &t));
        if (free_bytes) *free_bytes = f;
        if (total_bytes) *total_bytes = t;
        return FWX_OK;
    });
}

int fwx_matrix_resume_bytes(const fwx_matrix *m, int32_t checkpoints, uint64_t *bytes_out)
{
    return fwxi::guarded([&]() -> int {
        if (!m || !bytes_out || checkpoints < 0 || checkpoints > FWX_MAX_CHECKPOINTS) return FWX_ERR_INVALID;
        SlabCells d = {0, 0, 0};               // summed over the slabs: every partition keeps all pivot rows
        (void)each_slab(m, nullptr, [&](const SlabData &q, int) -> int {
            const SlabCells c = slab_cells(q.rows, m->nd, q.ct_ld);
            d.cells += c.cells; d.col_cells += c.col_cells; d.w_cells += c.w_cells;
            return FWX_OK;
        });
        const uint64_t es = m->dtype == FWX_F64 ? 8 : 4;
        // per checkpoint: one copy of every array; panels: w + ct (+ cnt) (+ wh + cht) for all pivots
        // (a partitioned handle: every partition keeps all pivot ROWS, its own part of the columns)
        const uint64_t per_cp = d.cells * (es + (m->with_next ? 4 : 0) + (m->with_hops ? 4 : 0) + (m->traced ? 12 : 0));
        const uint64_t panels = d.w_cells * es + d.col_cells * es + (m->with_next ? d.col_cells * 4 : 0) +
                                (m->with_hops ? d.w_cells * 4 + d.col_cells * 4 : 0);
        // ONE index buffer, although every partition of a partitioned handle allocates its own: the session's
        // memory budget (host/session.cpp) was tuned against this figure, so it stays as it is
        *bytes_out = (uint64_t)checkpoints * per_cp + panels + (uint64_t)FWX_MAX_PATCH * 8;
        return FWX_OK;
    });
}

int fwx_matrix_enable_resume(fwx_matrix *m, int32_t checkpoints)
{
    return fwxi::guarded([&]() -> int {
        if (!m || checkpoints < 1 || checkpoints > FWX_MAX_CHECKPOINTS) return FWX_ERR_INVALID;
        if (m->resume) return FWX_ERR_INVALID;
        if (!m->keep) return FWX_ERR_INVALID;                // replays start from the kept input
        // resumable = AUTO takes the fused engine for this order (fwx.h fwx_engine)
        if (m->n <= kSmallSolveAutoMax) return FWX_ERR_UNSUPPORTED;
        DeviceGuard g;
        int rc = enter_handle(g, m);
        if (rc) return rc;
        const size_t es = m->dtype == FWX_F64 ? 8 : 4;
        fail_point();
        // a failure (an allocation, or the throw above) leaves nothing behind: the handle stays usable
        struct Holder {
            fwx_matrix *m; DeviceGuard &g;
            Resume *r = new Resume();
            ~Holder()
            {
                if (!r) return;
                (void)each_slab(m, &g, [](SlabData &d, int) -> int { store_free(d.store); return FWX_OK; });
                delete r;
            }
        } hold{m, g};
        Resume *R = hold.r;
        // only block starts: a pivot block never straddles two slabs, so inside a slab blocks start at row0 + 64 t
        R->pivot = checkpoint_pivots(m->n, checkpoints, [&](int c) {
            return (c - slab_row0_of(m, c)) % FWX_FUSED_B == 0;
        });
        R->count = (int)R->pivot.size();
        rc = each_slab(m, &g, [&](SlabData &d, int) -> int {
            fail_point();         // (per slab: a failure here finds the stores of the slabs before it allocated)
            return store_alloc(d.store, slab_of(d, m->nd, es), R->count);
        });
        if (rc) return rc;
        R->state_at = (m->fresh && m->kept_valid) ? 0 : -1;
        m->resume = R;            // complete: owned by the handle from here on
        hold.r = nullptr;
        return R->count;
    });
}

int fwx_matrix_resolve(fwx_matrix *m, int32_t count, const int64_t *index, const void *rate_vals,
                       const int32_t *next_vals, const int32_t *hops_vals, const fwx_opts *opts,
                       int32_t *resumed_from)
{
    return fwxi::guarded([&]() -> int {
        if (resumed_from) *resumed_from = 0;
        if (!m || count < 0 || count > FWX_MAX_PATCH || (count > 0 && (!index || !rate_vals)))
            return FWX_ERR_INVALID;
        if (!m->keep || !m->kept_valid) return FWX_ERR_INVALID;
        if ((next_vals && !m->with_next) || (hops_vals && !m->with_hops)) return FWX_ERR_INVALID;
        const int64_t nn64 = (int64_t)m->n * m->n;
        int64_t lowest = m->n;                       // min over the patched entries' indices
        for (int32_t q = 0; q < count; ++q) {
            if (index[q] < 0 || index[q] >= nn64) return FWX_ERR_INVALID;
            const int64_t i = index[q] / m->n, j = index[q] % m->n;
            lowest = i < lowest ? i : lowest;
            lowest = j < lowest ? j : lowest;
        }
        Opts op;
        int rc = read_opts(opts, m->n, op);
        if (rc) return rc;
        // the checkpoint to resume from: the last one at or before `lowest` that still belongs to the
        // solve of the kept input -- on a handle that records them, on the reference's domain
        // (the fused engine ran and will run again), for a whole-range uncounted solve
        int c_idx = -1;
        Resume *R = m->resume;
        if (R && count > 0 && m->dom_known && !op.updates_out && !op.has_stream && op.k_begin == 0 &&
            op.k_end == m->n && op.engine != FWX_ENGINE_PERK)
            for (int q = 0; q < R->count; ++q)
                if (R->pivot[(size_t)q] <= lowest && R->pivot[(size_t)q] <= R->valid_upto) c_idx = q;
        if (c_idx >= 0) {
            // are the patched values inside the domain?  (fwx_matrix_patch_input keeps dom_known only then)
            if (!patch_keeps_domain(m, count, rate_vals, next_vals)) c_idx = -1;
        }
        if (c_idx < 0) {
            // nothing to resume from: the patched input from pivot 0 (which records anew)
            if ((rc = fwx_matrix_patch_input(m, count, index, rate_vals, next_vals, hops_vals))) return rc;
            return fwx_matrix_solve(m, opts);
        }
        DeviceGuard g;
        if ((rc = enter_handle(g, m))) return rc;
        const size_t es = m->dtype == FWX_F64 ? 8 : 4;
        const int c = R->pivot[(size_t)c_idx];
        R->valid_upto = 0;                           // until the resumed solve has finished
        // offs: per slab, the patched entries' offsets in its arrays (pitch nd).  The replay reads them with an
        // asynchronous copy, so they outlive every synchronisation below, Unwind's included
        std::vector<int64_t> offs[FWX_MAX_PARTS];
        // Any error return below leaves the handle in a state the next call can start from: nothing of this
        // call still queued on a slab's stream (the small copies read the caller's arrays), nothing resumable,
        // the live arrays no known state of the kept input (the next resolve / patch_input restores them).
        struct Unwind {
            fwx_matrix *m; DeviceGuard &g; bool armed = true;
            ~Unwind()
            {
                if (!armed) return;
                (void)sync_slabs(m, g);
                m->resume->valid_upto = 0;
                m->resume->state_at = -1;
                m->fresh = 0;
                m->rec_ready = 0;
            }
        } unwind{m, g};
        // the kept input first (the replay reads it), then on every slab the state at the start of step c, except
        // its patched entries: replayed through pivots [0, c) from the stored panels (the slab's own column
        // snapshots and the pivot rows every slab keeps)
        if ((rc = patch_kept_entries(m, g, count, index, rate_vals, next_vals, hops_vals, offs))) return rc;
        rc = each_slab(m, &g, [&](SlabData &d, int p) -> int {
            if (d.rows == 0) return FWX_OK;
            const Slab v = slab_of(d, m->nd, es);
            const int rc2 = restore_checkpoint(d.store, v, c_idx);
            if (rc2 || offs[p].empty()) return rc2;
            return m->dtype == FWX_F64 ? replay_entries<double>(d.store, v, *R, c_idx, offs[p].data(), offs[p].size())
                                       : replay_entries<float>(d.store, v, *R, c_idx, offs[p].data(), offs[p].size());
        });
        if (rc) return rc;
        m->fresh = 0;
        m->rec_ready = 0;
        R->valid_upto = c;                           // panels < c and checkpoints <= c hold for the NEW input;
                                                     // later ones are the old solve's until this one passes them
        op.k_begin = c;
        R->state_at = op.k_begin;                    // the live arrays: the NEW kept input at time c
        if (m->multi) {
            rc = multi_solve(m, op, true);
        } else if (m->traced) {
            rc = logged_solve(m, op, m->slab.main, true);
        } else {
            rc = m->dtype == FWX_F64 ? matrix_solve_typed<double>(m, op, nullptr, m->slab.main)
                                     : matrix_solve_typed<float>(m, op, nullptr, m->slab.main);
            if (!rc) FWX_HIP(hipStreamSynchronize(m->slab.main));
        }
        if (rc) return rc;
        unwind.armed = false;
        if (resumed_from) *resumed_from = op.k_begin;
        return FWX_OK;
    });
}

int fwx_matrix_path_log_count(fwx_matrix *m, uint64_t *count_out)
{
    return fwxi::guarded([&]() -> int {
        if (!m || !count_out) return FWX_ERR_INVALID;
        *count_out = (m->traced && m->rec_ready) ? m->last_u : 0;
        return FWX_OK;
    });
}

int fwx_matrix_query_exact(fwx_matrix *m, int32_t src, int32_t dst, double *rate_out,
                           int32_t *path_out, int32_t cap)
{
    return fwxi::guarded([&]() -> int {
        if (!m || src < 0 || dst < 0 || src >= m->n || dst >= m->n || cap <= 0 || !path_out)
            return FWX_ERR_INVALID;
        if (!m->traced) return FWX_ERR_INVALID;
        if (!m->rec_ready) return FWX_ERR_INVALID;             // no traced solve of this upload yet
        if (m->multi) return multi_query_exact(m, src, dst, rate_out, path_out, cap);
        DeviceGuard g;
        int rc = g.enter(m->device);
        if (rc) return rc;
        hipStream_t s = m->slab.main;
        RateRead rate;
        if ((rc = rate.queue(m->slab.rate, (size_t)src * m->nd + dst, m->dtype, s, rate_out))) return rc;
        // grow-only scratch, reused across queries: the list (cap), the walk's stack (sized by the order), the length
        const size_t stack_ints = 3 * exact_stack_triples(m->n);
        if (!m->walk || m->walk_cap < cap) {
            if (m->walk) { drain_stream(s); (void)hipFree(m->walk); m->walk = nullptr; }
            FWX_HIP(hipMalloc((void **)&m->walk, ((size_t)cap + stack_ints + 1) * 4));
            m->walk_cap = cap;
        }
        int32_t *const len_dev = m->walk + (size_t)cap + stack_ints;
        hipLaunchKernelGGL(exact_path_kernel, dim3(1), dim3(1), 0, s, tab_of(m), m->n, src, dst, m->walk, cap,
                           len_dev);
        const int len = read_list(s, len_dev, m->walk, path_out);
        rate.done();
        return len;
    });
}

int fwx_matrix_query_exact_batch(fwx_matrix *m, int32_t count, const int32_t *src, const int32_t *dst,
                                 int32_t *len_out, int32_t *path_out, int32_t cap)
{
    return fwxi::guarded([&]() -> int {
        if (!m || count < 0 || cap <= 0) return FWX_ERR_INVALID;
        if (count == 0) return FWX_OK;
        if (!src || !dst || !len_out || !path_out || !m->traced) return FWX_ERR_INVALID;
        if (!m->rec_ready) return FWX_ERR_INVALID;
        if (m->multi) return multi_query_exact_batch(m, count, src, dst, len_out, path_out, cap);
        DeviceGuard g;
        int rc = g.enter(m->device);
        if (rc) return rc;
        return run_exact_batch(tab_of(m), m->n, m->slab.main, count, src, dst, len_out, path_out, cap);
    });
}

int fwx_matrix_download(fwx_matrix *m, void *rate, int32_t *next, int32_t *hops)
{
    return fwxi::guarded([&]() -> int {
        if (!m) return FWX_ERR_INVALID;
        if (m->n == 0) return FWX_OK;
        if ((next && !m->with_next) || (hops && !m->with_hops)) return FWX_ERR_INVALID;
        DeviceGuard g;
        int rc = enter_handle(g, m);
        if (rc) return rc;
        const size_t es = m->dtype == FWX_F64 ? 8 : 4;
        rc = each_slab(m, &g, [&](SlabData &d, int) -> int {
            int rc2;
            if ((rc2 = copy_rows(m, d, d.rate, rate, es, false)) || (rc2 = copy_rows(m, d, d.next, next, 4, false)) ||
                (rc2 = copy_rows(m, d, d.hops, hops, 4, false)))
                return rc2;
            return FWX_OK;
        });
        return rc ? rc : sync_slabs(m, g);
    });
}

int fwx_matrix_solve(fwx_matrix *m, const fwx_opts *opts)
{
    return fwxi::guarded([&]() -> int {
        if (!m) return FWX_ERR_INVALID;
        if (m->n == 0) return FWX_OK;
        Opts op;
        int rc = read_opts(opts, m->n, op);
        if (rc) return rc;
        if (m->multi) return multi_solve(m, op);
        DeviceGuard g;
        if ((rc = g.enter(m->device))) return rc;
        hipStream_t s = op.has_stream ? op.stream : m->slab.main;
        if (m->traced) return logged_solve(m, op, s);
        unsigned long long *upd = op.updates_out ? m->upd : nullptr;
        if (upd) FWX_HIP(hipMemsetAsync(upd, 0, FWX_UPDATE_SHARDS * 8, s));
        if (m->dtype == FWX_F64)
            rc = matrix_solve_typed<double>(m, op, upd, s);
        else
            rc = matrix_solve_typed<float>(m, op, upd, s);
        if (rc) return rc;
        FWX_HIP(hipStreamSynchronize(s));
        if (op.has_stream) drain_stream(s);   // the caller may destroy the handle next: nothing of this
                                              // solve is left un-retired on a stream the handle does not own
        if (upd) return sum_updates(upd, op.updates_out, s);
        return FWX_OK;
    });
}

int fwx_matrix_query(fwx_matrix *m, int32_t src, int32_t dst, double *rate_out, int32_t *path_out,
                     int32_t cap)
{
    return fwxi::guarded([&]() -> int {
        if (!m || src < 0 || dst < 0 || src >= m->n || dst >= m->n || cap < 0 || (cap > 0 && !path_out))
            return FWX_ERR_INVALID;
        if (m->multi) return multi_query(m, src, dst, rate_out, path_out, cap);
        DeviceGuard g;
        int rc = g.enter(m->device);
        if (rc) return rc;
        RateRead rate;
        if ((rc = rate.queue(m->slab.rate, (size_t)src * m->nd + dst, m->dtype, m->slab.main, rate_out))) return rc;
        if (!m->with_next) {
            FWX_HIP(hipStreamSynchronize(m->slab.main));
            rate.done();
            return FWX_ERR_INVALID;
        }
        const int len = run_follow(tab_of(m), m->n, m->slab.main, m->scratch, src, dst, path_out, cap);
        rate.done();
        return len;
    });
}

int fwx_dev_relax(const fwx_slab *slab, const fwx_pivots *piv, int32_t serpentine,
                  unsigned long long *d_updates, void *stream)
{
    return fwxi::guarded([&]() -> int {
        return fwx_dev_relax_skip(slab, piv, serpentine, d_updates, 0, 0, stream);
    });
}

int fwx_dev_relax_skip(const fwx_slab *slab, const fwx_pivots *piv, int32_t serpentine,
                       unsigned long long *d_updates, int32_t skip_lo, int32_t skip_hi, void *stream)
{
    return fwxi::guarded([&]() -> int {
        int rc = check_slab(slab);
        if (rc) return rc;
        if (!piv || piv->k_begin < 0 || piv->k_end < piv->k_begin || piv->k_end > slab->n)
            return FWX_ERR_INVALID;
        if (slab->rows == 0 || slab->n == 0 || piv->k_end == piv->k_begin) return FWX_OK;
        if (!piv->rate || (slab->hops && !piv->hops)) return FWX_ERR_INVALID;
        if (device_count() <= 0) return FWX_ERR_NO_DEVICE;
        hipStream_t s = (hipStream_t)stream;
        if (skip_lo < 0 || skip_hi < skip_lo || skip_hi > slab->rows ||
            (skip_hi > skip_lo && (skip_lo % 4 || skip_hi % 4)))
            return FWX_ERR_INVALID;
        auto run = [&](auto elem) -> int {
            using T = decltype(elem);
            PerkRange<T> pr;
            pr.rate = (T *)slab->rate; pr.next = slab->next; pr.hops = slab->hops;
            pr.rows = slab->rows; pr.n = slab->n; pr.row0 = slab->row0;
            pr.prow0 = (const T *)piv->rate; pr.phops0 = piv->hops; pr.pnext0 = slab->next ? piv->next : nullptr;
            pr.stride = piv->stride; pr.k_begin = piv->k_begin; pr.k_end = piv->k_end; pr.serpentine = serpentine;
            pr.d_updates = d_updates; pr.stream = s; pr.skip_lo = skip_lo; pr.skip_hi = skip_hi;
            return relax_range<T>(pr);
        };
        return slab->dtype == FWX_F64 ? run(double()) : run(float());
    });
}

int fwx_dev_panel(const fwx_slab *block, void *w_rate, int32_t *w_hops,
                  unsigned long long *d_updates, void *stream)
{
    return fwxi::guarded([&]() -> int {
        int rc = check_slab(block);
        if (rc) return rc;
        if (block->rows == 0 || block->n == 0) return FWX_OK;
        if (!w_rate || (block->hops && !w_hops)) return FWX_ERR_INVALID;
        if (device_count() <= 0) return FWX_ERR_NO_DEVICE;
        hipStream_t s = (hipStream_t)stream;
        if (block->dtype == FWX_F64)
            return panel_impl<double>(block, (double *)w_rate, w_hops, d_updates, s);
        return panel_impl<float>(block, (float *)w_rate, w_hops, d_updates, s);
    });
}

int fwx_dev_solve(const fwx_slab *full, const fwx_opts *opts)
{
    return fwxi::guarded([&]() -> int {
        int rc = check_slab(full);
        if (rc) return rc;
        if (full->row0 != 0 || full->rows != full->n) return FWX_ERR_INVALID;
        if (full->n == 0) return FWX_OK;
        Opts op;
        if ((rc = read_opts(opts, full->n, op))) return rc;
        if (device_count() <= 0) return FWX_ERR_NO_DEVICE;
        fwx_matrix m;
        memset(&m, 0, sizeof(m));
        m.n = m.nd = full->n; m.dtype = full->dtype;      // caller-owned memory: pitch n, no padding
        m.with_next = full->next != nullptr; m.with_hops = full->hops != nullptr;
        m.slab.rate = full->rate; m.slab.next = full->next; m.slab.hops = full->hops;
        m.slab.rows = m.nd; m.slab.ct_ld = (m.nd + 3) & ~3;
        DeviceGuard g;                       // the context belongs to the device the call runs on
        if ((rc = g.enter(op.device))) return rc;
        CtxLease lease;
        if ((rc = lease.open())) return rc;
        hipStream_t s = op.has_stream ? op.stream : lease.c->s;
        if (op.has_stream) lease.c->uses_stream(op.stream);
        struct { void *p = nullptr; } upd;
        if (op.updates_out) {
            void *small = nullptr;
            if ((rc = lease.c->reserve(CallCtx::SMALL, (FWX_UPDATE_SHARDS + 2) * sizeof(unsigned long long), &small))) return rc;
            upd.p = small;
            FWX_HIP(hipMemsetAsync(upd.p, 0, FWX_UPDATE_SHARDS * 8, s));
        }
        rc = full->dtype == FWX_F64
                 ? matrix_solve_typed<double>(&m, op, (unsigned long long *)upd.p, s, lease.c)
                 : matrix_solve_typed<float>(&m, op, (unsigned long long *)upd.p, s, lease.c);
        if (rc) return rc;
        FWX_HIP(hipStreamSynchronize(s));
        if (op.updates_out) return sum_updates((unsigned long long *)upd.p, op.updates_out, s);
        return FWX_OK;
    });
}

int fwx_dev_follow_paths(int32_t n, const int32_t *next, int32_t count, const int32_t *src,
                         const int32_t *dst, int32_t *len_out, const void *edge_rate,
                         int32_t dtype, double *prod_out, int32_t *path_out, int32_t cap,
                         void *stream)
{
    return fwxi::guarded([&]() -> int {
        if (n < 0 || count < 0 || cap < 0 || (dtype != FWX_F32 && dtype != FWX_F64))
            return FWX_ERR_INVALID;
        if (count == 0) return FWX_OK;
        if (!next || !src || !dst || !len_out || (prod_out && !edge_rate) || (path_out && cap == 0))
            return FWX_ERR_INVALID;
        if (device_count() <= 0) return FWX_ERR_NO_DEVICE;
        hipStream_t s = (hipStream_t)stream;
        const dim3 grid((unsigned)((count + 255) / 256)), block(256);
        if (dtype == FWX_F64)
            hipLaunchKernelGGL(follow_paths_kernel<double>, grid, block, 0, s, next, n, count, src,
                               dst, len_out, (const double *)edge_rate, prod_out, path_out, cap);
        else
            hipLaunchKernelGGL(follow_paths_kernel<float>, grid, block, 0, s, next, n, count, src, dst,
                               len_out, (const float *)edge_rate, prod_out, path_out, cap);
        FWX_HIP(hipGetLastError());
        return FWX_OK;
    });
}

int fwx_dev_panel_snap(const fwx_slab *block, void *w_rate, int32_t *w_hops, const fwx_trace *trace,
                       void *stream)
{
    return fwxi::guarded([&]() -> int {
        int rc = check_slab(block);
        if (rc) return rc;
        if (block->rows == 0 || block->n == 0) return FWX_OK;
        if (!w_rate || block->rows > FWX_FUSED_B || (block->hops && !w_hops)) return FWX_ERR_INVALID;
        if (trace && (!trace->last || !trace->at_row || !block->next)) return FWX_ERR_INVALID;
        if (device_count() <= 0) return FWX_ERR_NO_DEVICE;
        hipStream_t s = (hipStream_t)stream;
        fwx::PathLog pl = fwx::PathLog();
        if (trace) { pl.last = trace->last; pl.at_col = trace->at_col; pl.at_row = trace->at_row; }
        if (block->dtype == FWX_F64)
            FWX_HIP(fwx::launch_fused_panel<double>((const double *)block->rate, block->n, block->row0,
                                                    block->rows, (double *)w_rate, s, pl, block->hops, w_hops));
        else
            FWX_HIP(fwx::launch_fused_panel<float>((const float *)block->rate, block->n, block->row0,
                                                   block->rows, (float *)w_rate, s, pl, block->hops, w_hops));
        return FWX_OK;
    });
}

int fwx_dev_check_nonneg(const fwx_slab *slab, int32_t *d_flag, void *stream)
{
    return fwxi::guarded([&]() -> int {
        int rc = check_slab(slab);
        if (rc) return rc;
        if (!d_flag) return FWX_ERR_INVALID;
        if (device_count() <= 0) return FWX_ERR_NO_DEVICE;
        hipStream_t s = (hipStream_t)stream;
        if (slab->dtype == FWX_F64)
            FWX_HIP(fwx::launch_nonneg_check((const double *)slab->rate, slab->next,
                                             (size_t)slab->rows * slab->n, (int *)d_flag, s));
        else
            FWX_HIP(fwx::launch_nonneg_check((const float *)slab->rate, slab->next,
                                             (size_t)slab->rows * slab->n, (int *)d_flag, s));
        return FWX_OK;
    });
}

int fwx_dev_relax_fused(const fwx_slab *slab, const fwx_pivots *piv, const fwx_fused_scratch *scratch,
                        const fwx_trace *trace, unsigned long long *d_updates, int32_t flags,
                        void *stream)
{
    return fwxi::guarded([&]() -> int {
        return fwx_dev_relax_fused_skip(slab, piv, scratch, trace, d_updates, flags, 0, 0, stream);
    });
}

int fwx_dev_relax_fused_skip(const fwx_slab *slab, const fwx_pivots *piv,
                             const fwx_fused_scratch *scratch, const fwx_trace *trace,
                             unsigned long long *d_updates, int32_t flags, int32_t skip_lo,
                             int32_t skip_hi, void *stream)
{
    return fwxi::guarded([&]() -> int {
        int rc = check_slab(slab);
        if (rc) return rc;
        if (!piv || piv->k_begin < 0 || piv->k_end < piv->k_begin || piv->k_end > slab->n ||
            piv->k_end - piv->k_begin > FWX_FUSED_B)
            return FWX_ERR_INVALID;
        if (slab->rows == 0 || slab->n == 0 || piv->k_end == piv->k_begin) return FWX_OK;
        if (!piv->rate || piv->stride != slab->n || !scratch || !scratch->col_rate ||
            (slab->next && !scratch->col_next) || (slab->hops && (!scratch->col_hops || !piv->hops)))
            return FWX_ERR_INVALID;
        if (trace && (!slab->next || !trace->last || !trace->at_col)) return FWX_ERR_INVALID;
        if (skip_lo < 0 || skip_hi < skip_lo || skip_hi > slab->rows ||
            (skip_hi > skip_lo && (skip_lo % 8 || skip_hi % 8)))
            return FWX_ERR_INVALID;
        if (device_count() <= 0) return FWX_ERR_NO_DEVICE;
        hipStream_t s = (hipStream_t)stream;
        const bool nonneg = (flags & FWX_FLAG_NONNEG) != 0;
        if (slab->dtype == FWX_F64)
            return fused_block<double>(slab, piv->k_begin, piv->k_end - piv->k_begin, (const double *)piv->rate,
                                       piv->hops, scratch, trace, d_updates, nonneg, s, skip_lo, skip_hi);
        return fused_block<float>(slab, piv->k_begin, piv->k_end - piv->k_begin, (const float *)piv->rate,
                                  piv->hops, scratch, trace, d_updates, nonneg, s, skip_lo, skip_hi);
    });
}

}  // extern "C"
