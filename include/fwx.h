/*
 * fwx.h -- C ABI of libfwx, the MI355X (gfx950) max-product Floyd-Warshall engine.
 *
 * Drop-in boundary.  The reference has no FFI; its seam is the pure function
 *     floydWarshall :: Map (Vertex,Vertex) Double -> Matrix RateEntry
 *         /root/reference/src/lib/Algorithms.hs:19-20   (= runAlgo 0 . buildMatrix)
 * whose replaceable core is
 *     runAlgo :: Int -> Matrix RateEntry -> Matrix RateEntry
 *         /root/reference/src/lib/Algorithms.hs:42-61
 * The host keeps buildMatrix (:26-40) and optimum (:65-78); this library replaces runAlgo on the
 * dense structure-of-arrays form of `Matrix RateEntry` (Types.hs:24-29, :39):
 *
 *     rate[n*n]  row-major, T = double (the reference's precision, Types.hs:26) or float
 *     next[n*n]  int32: index of `head _path`, -1 for the empty path        (optional)
 *     hops[n*n]  int32: `length _path`                                      (optional)
 *
 * `_start` of row i is implicit (vertex i).  "No route" is rate 0.0 / next -1 / hops 0
 * (isolatedEntry, Utils.hs:13-14).
 *
 * Semantics preserved exactly: k ascending (:44); row k copied (:50);
 * entries j==i or j==k untouched (:54); operands from the state at the start of step k (:58-60);
 * one IEEE multiply (:61) and one strict ordered compare (:55) per relaxation -- no fast-math, no
 * FMA, denormals kept, NaN compares false.  Results are bit-identical to the reference loop.
 *
 * Errors: every entry point returns FWX_OK (0) or a negative fwx_status; no C++ exception or
 * abort crosses this boundary.  n == 0 is success and touches nothing (the reference returns the
 * empty matrix: src/test/AlgorithmsTest.hs:45-47, :62-64).  There is NO CPU fallback: without a
 * HIP device the solve entry points return FWX_ERR_NO_DEVICE.
 *
 * Domain.  The reference's parser only admits rates > 0 (Parsers.hs:40) and buildMatrix gives every
 * entry it fills a one-vertex path (Algorithms.hs:35-37), so in the reference every matrix obeys
 *     (D1) every rate is >= +0.0 and not NaN          (D2) rate != 0  =>  next >= 0  (path non-empty)
 * On that domain a winning product has two positive factors, hence a non-empty ikPath, and
 * head (ikPath ++ kjPath) = next[i][k].  The engine does NOT assume the domain: it checks it on the
 * device (one read of the matrix) before a fused solve, and a matrix outside it -- negative or NaN
 * rates, or a positive rate with next == -1 -- is solved by the per-k engine, which implements the
 * list rule in full (head = next[i][k] if that is >= 0, else next[k][j]).  Either way rates, next,
 * hops and U equal the reference's loop bit for bit.  Only the slab entry points (fwx_dev_relax*,
 * which see one slab and not the matrix) leave the check to the caller: see fwx_pivots.next and
 * fwx_dev_check_nonneg.
 *
 * Threading / streams: calls are blocking unless a stream is passed explicitly (fwx_dev_*, or
 * fwx_opts.stream), may come from any OS thread, keep no global mutable state besides a
 * mutex-protected pool of per-call contexts, and restore the
 * caller's current HIP device.  No entry point uses the legacy null stream: one-shot calls run on
 * a non-blocking stream of their own (taken, with the device buffers and workspace the call needs,
 * from a process-wide pool of per-call contexts: a call creates and frees nothing on the device
 * once the pool is warm), a handle on the handle's own non-blocking stream, so solves
 * on different host threads overlap on the device and nothing synchronises implicitly with the
 * streams of other libraries in the process (torch's included).
 * What is NOT promised: one handle must not be used by two threads at once (calls on different handles
 * are independent).  Two host threads must not have step-API calls (fwx_dev_relax*) in flight on the
 * same stream at once, the null stream included: the snapshot panels are one buffer per stream.  If
 * more callers come at once than a pool keeps -- contexts, per-stream panels, parked multi-partition
 * handles -- the pool grows for the moment and shrinks again: what is in use by a call that has not
 * returned is never freed under it, and the surplus is released (which synchronises the device) as the
 * calls return or by a later call.
 */
#ifndef FWX_H
#define FWX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FWX_ABI_VERSION 3

typedef enum fwx_status {
    FWX_OK = 0,
    FWX_ERR_INVALID = -1,     /* bad argument (null pointer, negative size, bad range, misaligned) */
    FWX_ERR_NO_DEVICE = -2,   /* no HIP device visible: the engine has no CPU fallback            */
    FWX_ERR_HIP = -3,         /* a HIP runtime call failed (fwx_last_hip_error gives the code)    */
    FWX_ERR_OOM = -4,         /* device or host allocation failed                                 */
    FWX_ERR_CYCLE = -5,       /* fwx_follow_path: next-hops do not reach dst within n hops        */
    FWX_ERR_CAPACITY = -6,    /* fwx_follow_path: output buffer too small                         */
    FWX_ERR_UNSUPPORTED = -7, /* option combination not implemented                               */
    FWX_ERR_RCCL = -8,        /* librccl.so.1 could not be loaded, or an RCCL call failed         */
    FWX_ERR_INTERNAL = -9     /* an unexpected C++ exception was stopped at the boundary          */
} fwx_status;

typedef enum fwx_dtype { FWX_F32 = 0, FWX_F64 = 1 } fwx_dtype;

/* Which relaxation engine runs the pivots.  All are bit-exact with the reference loop.
 * AUTO: n <= 64 -> the whole solve in one single-workgroup launch; above -> FUSED (two launches
 * per 64 pivots).  The fused kernels read rows in 16-byte vectors; buildMatrix (Algorithms.hs:29)
 * produces any n, so every entry point that OWNS its device memory -- fwx_solve_f32/f64, the handles
 * of fwx_matrix_create and fwx_matrix_create_multi -- keeps the matrix at a device order rounded up
 * to 4 (f32) / 2 (f64) with inert padding (rate +0.0, next -1: a padding index is never a pivot and
 * a +0.0 target never improves) and runs any engine on any n.  Where FUSED does not apply -- an
 * input outside the domain below, or caller-owned device memory (fwx_dev_*) whose rows are not a
 * multiple of 16 bytes -- AUTO takes the single-launch kernel up to n = 128 and PERK above; an
 * explicit FUSED on such caller-owned memory is refused (FWX_ERR_UNSUPPORTED).                     */
typedef enum fwx_engine {
    FWX_ENGINE_AUTO = 0,
    FWX_ENGINE_PERK = 1,  /* one N x N launch per pivot k (HBM-bound streaming kernel)            */
    FWX_ENGINE_FUSED = 2  /* B pivots per launch from time-k snapshots of the pivot panels         */
} fwx_engine;

/* Options; zero-initialise and set struct_size = sizeof(fwx_opts).  NULL means all defaults. */
typedef struct fwx_opts {
    uint32_t struct_size;
    int32_t device;        /* HIP device ordinal; -1 = the caller's current device                 */
    int32_t engine;        /* fwx_engine                                                           */
    int32_t k_begin;       /* first pivot (default 0): a solve over [k_begin,k_end) is resumable   */
    int32_t k_end;         /* one past the last pivot; <= 0 means n                                */
    int32_t block;         /* reserved, must be 0 (the fused engine works in FWX_FUSED_BLOCK pivots)*/
    int32_t serpentine;    /* 0 = default (on): alternate sweep direction per pivot so the tail of */
                           /* one launch is re-read from the Infinity Cache; 1 = off               */
    uint64_t *updates_out; /* host pointer, optional: receives U = number of successful updates    */
    void *stream;          /* hipStream_t to run on, honoured iff use_stream != 0 (fwx_matrix_solve,  */
    int32_t use_stream;    /* fwx_dev_solve, fwx_solve_*); the call still blocks until it is done.    */
    int32_t reserved0;     /* 0: a library-owned non-blocking stream (per call / per handle)          */
} fwx_opts;

int fwx_abi_version(void);
int fwx_device_count(void);              /* number of HIP devices, 0 if none (never an error)      */
const char *fwx_strerror(int status);
int fwx_last_hip_error(void);            /* hipError_t of the last FWX_ERR_HIP on this thread      */
/* HIP_VERSION libfwx was compiled against and the version of the HIP runtime it is bound to in this
 * process (hipRuntimeGetVersion; 0 if that fails).  Returns 1 if major.minor agree, else 0.  They
 * differ when another library mapped its own libamdhip64 first -- a torch wheel bundles one -- and
 * libfwx's DT_NEEDED resolved to that copy: it works, but it is not the pairing the library was
 * built and fuzzed on, so hosts should load libfwx before such a library or
 * at least log the mismatch (floydwarshall_amd/_lib.py does both).                                  */
int fwx_hip_versions(int32_t *built_against, int32_t *runtime);
/* TEST HOOK for the exception barrier: arms a countdown on the calling thread; the countdown-th
 * internal allocation point reached by later calls on this thread throws std::bad_alloc, which the
 * boundary must turn into FWX_ERR_OOM with nothing leaked.  0 disarms.  Not for production use.     */
int fwx_test_fail_after(int32_t countdown);
/* TEST HOOK for dispatch coverage: every kernel launch of the solvers ORs a bit for its form (kernel and
 * the instantiation a size threshold picks) into one process-wide word.  Stores that word into *seen
 * (if not NULL) and clears it if reset; returns the number of forms.  fwx_test_kernel_form_name gives
 * the name of bit `form`, NULL past the last.  Not for production use.                                */
int fwx_test_kernel_forms(uint64_t *seen, int reset);
const char *fwx_test_kernel_form_name(int form);
/* TEST HOOK for the per-k engine's multi-pivot schedule: returns what FWX_PERK_PIVOTS parses to right now
 * (1, 2, 4 or 8; the default on anything else).  launches (if not NULL) receives five counters of the
 * launches that schedule has made in this process -- single-pivot, 2-, 4- and 8-pivot sweeps, panel
 * launches -- which are cleared if reset.  A 16-pivot sweep of the wide pass (FWX_PERK_WIDE, below) applies two
 * 8-pivot groups and adds 2 to the 8-pivot counter, so the five read the same with the wide pass on and off.
 * Needs no device.  Not for production use.                                                             */
int fwx_test_perk_pivots(uint64_t *launches, int reset);
/* TEST HOOK for the wide pass of that schedule: returns what FWX_PERK_WIDE parses to right now: 0 = off (the value
 * `0`, exactly), 1 = on (anything else, or unset).  *wide_launches (if not NULL) receives the number of 16-pivot
 * sweeps launched in this process -- each of them also counted as 2 by fwx_test_perk_pivots -- which is cleared if
 * reset.  Needs no device.  Not for production use.                                                     */
int fwx_test_perk_wide(uint64_t *wide_launches, int reset);
/* TEST HOOK: what FWX_PERK_FOLD parses to right now: 1 = compare (the value `compare`, exactly), 0 = automatic
 * (anything else, or unset).  Needs no device.  Not for production use.                              */
int fwx_test_perk_fold(void);
/* TEST HOOK: what FWX_PERK_WALK parses to right now: 0 = round 19's kernel sweeps the 16-pivot launches (the value
 * `0`, exactly), 1 = round 23's does (anything else, or unset).  Launches are counted by the two hooks above, the
 * same either way.  Needs no device.  Not for production use.                                        */
int fwx_test_perk_walk(void);
/* TEST HOOK for the deep pass of that schedule (FWX_PERK_DEEP): returns what the variable parses to right now: 0 = off
 * (the value `0`, exactly: the ladder starts at 16, the schedule before the 32-pivot sweep launch for launch), 1 = on
 * (anything else, or unset: where the ladder would start at 16 with the walk on, it starts at 32).  *deep_launches
 * (if not NULL) receives the number of 32-pivot sweeps launched in this process -- each of them also counted as 4 by
 * fwx_test_perk_pivots and as 2 by fwx_test_perk_wide -- which is cleared if reset.  Needs no device.  Not for
 * production use.                                                                                        */
int fwx_test_perk_deep(uint64_t *deep_launches, int reset);
/* TEST HOOK for the tile sweep of that schedule (FWX_PERK_TILE_MIN_N): returns what the variable parses to right now:
 * 0 = never, otherwise the smallest order n whose full 64-pivot blocks take ONE tile sweep where the deep pass would
 * issue two 32-pivot sweeps (digits only; any other text, or unset: the default).  *launches (if not NULL) receives
 * the number of tile sweeps launched in this process -- each of them also counted as 8 by fwx_test_perk_pivots, as 4
 * by fwx_test_perk_wide and as 2 by fwx_test_perk_deep -- which is cleared if reset.  Needs no device.  Not for
 * production use.                                                                                        */
int fwx_test_perk_tile(uint64_t *launches, int reset);
/* TEST HOOK for the pair schedule (FWX_PERK_PAIR_MIN_N): returns what the variable parses to right now: 0 = never,
 * otherwise the smallest order n at which a call that takes the tile sweep applies its full blocks two at a time, one
 * 128-pivot launch per pair with the next pair's panels made beside it on a look-ahead stream (digits only; any other
 * text, or unset: the default).  *launches (if not NULL) receives the number of 128-pivot main launches in this
 * process -- each of them also counted as 16 by fwx_test_perk_pivots, as 8 by fwx_test_perk_wide, as 4 by
 * fwx_test_perk_deep and as 2 by fwx_test_perk_tile -- which is cleared if reset.  Needs no device.  Not for
 * production use.                                                                                        */
int fwx_test_perk_pair(uint64_t *launches, int reset);
/* TEST HOOK for the group schedule (FWX_PERK_GROUP_MAX): returns what the variable parses to right now: 2, 4, 6 or 8,
 * the most blocks a main launch of a call that takes the pair schedule applies (digits only, 2 to 8, an odd value
 * counting as the even one below it), or 0 for any other text or unset: the default, which goes by the order of the
 * matrix.  launches (if not NULL) receives four counters: the main launches of 2, 4, 6 and 8 blocks in this process
 * (the pair schedule's own 128-pivot launches are the first) -- a launch of G blocks also counted as G / 2 by
 * fwx_test_perk_pair and in proportion by the four hooks above it -- which are cleared if reset.  Needs no device.
 * Not for production use.                                                                                */
int fwx_test_perk_group(uint64_t *launches, int reset);
/* TEST HOOK: the group sizes of a call of that schedule with nfull full blocks from its first tile boundary, at most
 * gmax blocks per group (0: what a call on a matrix of order n would take: the variable, or the default for n).
 * Writes up to cap sizes, in order, to size[] and the index of the first panel set of each group to set[] (either
 * may be NULL; a group's panels take `size` sets from there and the call keeps 2 * gmax sets); an odd last block is a
 * group of 1.  Returns the number of groups, or -1 for arguments out of range.  Needs no device.  Not for production
 * use.                                                                                                   */
int fwx_test_perk_group_plan(int n, int nfull, int gmax, int *size, int *set, int cap);
/* TEST HOOK for the three process-wide pools: the per-call contexts of the one-shot entry points, the per-stream
 * snapshot panels of fwx_dev_relax* (below) and the parked handles of fwx_solve_multi_*.  out (if not NULL) receives
 * twelve numbers, four per pool in that order: how many entries the pool keeps (its capacity), the entries created
 * in this process, the entries destroyed or evicted, and the most that were leased -- in a call -- at one time.
 * reset clears created and destroyed and sets the peak to what is leased right now.  Returns the number of pools, 3.
 * Needs no device.  Not for production use.                                                               */
int fwx_test_pools(uint64_t *out, int reset);
/* TEST HOOK: the rule by which the pool of snapshot panels picks the entry it evicts, over `count` entries with the
 * stamps used[] (larger = more recently used) and the marks busy[] (non-zero: a call that has not returned holds the
 * entry) in a pool that keeps `cap`: the index of the least recently used idle entry; -1 below capacity
 * (count < cap: nothing is evicted) and when every entry is busy (the pool grows for the moment); -2 for arguments
 * out of range.  Needs no device.  Not for production use.                                                 */
int fwx_test_perk_scratch_victim(const uint64_t *used, const int *busy, int count, int cap);

/* ---- one-shot host-buffer entry points: what the reference-side FFI binds --------------------
 * Replace runAlgo (Algorithms.hs:42-61) for a matrix produced by buildMatrix (:26-40).
 * rate/next/hops are n*n row-major HOST arrays, updated IN PLACE; next and hops may be NULL
 * (rates only).  The caller owns all buffers; no pointer is retained after return.            */
int fwx_solve_f64(int32_t n, double *rate, int32_t *next, int32_t *hops, const fwx_opts *opts);
int fwx_solve_f32(int32_t n, float *rate, int32_t *next, int32_t *hops, const fwx_opts *opts);

/* ---- batched small solves: many matrices of one order n <= FWX_BATCH_MAX_N in ONE launch ---------
 * The reference's own regime is small (its tests stop at 4 x 4); a host with many independent small
 * matrices -- one per timestamp of a price history, one per venue group, a what-if sweep over quotes --
 * solves them all in one call instead of looping over fwx_solve_*: one workgroup (n <= 16: one wave) per
 * matrix, so the batch spreads over the whole chip where the loop keeps one CU busy.  Every matrix gets
 * the full semantics above, the list rule included (head = next[i][k] if that is >= 0, else next[k][j]);
 * there is no domain check and no routing: a batch may mix matrices inside and outside the domain, and
 * each comes back bit-identical to the reference loop on that matrix alone.
 *
 * count matrices of order n, matrix b at rate + b*n*n (next / hops alike, both optional, hops needs next);
 * HOST arrays, solved in place.  updates_each: optional, count entries, U of each matrix.
 * count == 0 or n == 0: FWX_OK, nothing is touched.  FWX_ERR_INVALID: count < 0, n < 0, rate NULL, hops
 * without next, a bad struct_size or pivot range.  FWX_ERR_UNSUPPORTED: n > FWX_BATCH_MAX_N, or
 * opts->engine other than FWX_ENGINE_AUTO (the batch kernels are the only engine here).  All of these are
 * decided before any device call; then FWX_ERR_NO_DEVICE without a device, the arrays untouched.
 * opts: device, k_begin / k_end (one range for every matrix), stream / use_stream and updates_out (the SUM of
 * U over the batch) are honoured; serpentine is ignored.
 * Tier choice: FWX_BATCH_WAVE_MAX_N (environment, read per call; an integer 0 ... 16, default 16, anything
 * else means the default): n at or below it runs one wave per matrix with the matrix in registers, larger n
 * one workgroup per matrix; 0 turns the wave tier off.  No result bit depends on it.                   */
#define FWX_BATCH_MAX_N 128
int fwx_solve_batch_f64(int32_t count, int32_t n, double *rate, int32_t *next, int32_t *hops,
                        uint64_t *updates_each, const fwx_opts *opts);
int fwx_solve_batch_f32(int32_t count, int32_t n, float *rate, int32_t *next, int32_t *hops,
                        uint64_t *updates_each, const fwx_opts *opts);
/* The same on caller-owned DEVICE memory, asynchronous on `stream`, nothing allocated or synchronised;
 * stride = elements between consecutive matrices (>= n*n, else FWX_ERR_INVALID; the gap is never read or
 * written); pivots [k_begin, k_end) of every matrix, k_end <= 0 means n; dtype: fwx_dtype;
 * d_updates_each: optional device array of count uint64, INCREMENTED by each matrix's U.  Statuses as above
 * (n > FWX_BATCH_MAX_N: FWX_ERR_UNSUPPORTED).                                                          */
int fwx_dev_solve_batch(int32_t count, int32_t n, int32_t dtype, void *rate, int32_t *next, int32_t *hops,
                        int64_t stride, int32_t k_begin, int32_t k_end,
                        unsigned long long *d_updates_each, void *stream);
/* TEST HOOK: what FWX_BATCH_WAVE_MAX_N parses to right now.  Needs no device.  Not for production use. */
int fwx_test_batch_wave_max_n(void);

/* ---- batched mid-size solves: many matrices of one order n <= FWX_BATCH_MID_MAX_N in ONE launch ------------
 * The calls above stop at n = 128, where a matrix with next and hops still fits the registers and LDS of one
 * workgroup.  A market of 20 exchanges x 12 currencies has 240 vertices; a price history or a what-if sweep over
 * such a market is a batch of mid-size matrices.  These entry points take the batch up to n = 256: one workgroup per
 * matrix, the matrix resident in device memory, 16 pivots per pass from time-k snapshots held in LDS.  Every matrix
 * gets the full semantics above, the list rule included; there is no domain check and no routing by content, and
 * each matrix comes back bit-identical to the reference loop on that matrix alone -- rate, next, hops and U.
 *
 * The contract is that of fwx_solve_batch_* / fwx_dev_solve_batch, with the limit at FWX_BATCH_MID_MAX_N:
 * count matrices of order n, matrix b at rate + b*n*n (next / hops alike, both optional, hops needs next);
 * HOST arrays, solved in place.  updates_each: optional, count entries, U of each matrix.
 * count == 0 or n == 0: FWX_OK, nothing is touched.  FWX_ERR_INVALID: count < 0, n < 0, rate NULL, hops
 * without next, a bad struct_size or pivot range.  FWX_ERR_UNSUPPORTED: n > FWX_BATCH_MID_MAX_N, or
 * opts->engine other than FWX_ENGINE_AUTO.  All of these are decided before any device call; then
 * FWX_ERR_NO_DEVICE without a device, the arrays untouched.  opts: device, k_begin / k_end (one range for every
 * matrix), stream / use_stream and updates_out (the SUM of U over the batch) are honoured; serpentine is ignored.
 * Routing: FWX_BATCH_MID_MIN_N (environment, read per call; an integer 1 ... 129, default 129, anything else
 * means the default): orders below it are forwarded to fwx_solve_batch_* / fwx_dev_solve_batch (tier choice by
 * FWX_BATCH_WAVE_MAX_N as above), orders from it up to 256 run the mid tier.  No result bit depends on it; it
 * exists so that tests and A/B runs can put n <= 128 through the mid tier.
 * When to use it: see the measurements beside the device form below.                                       */
#define FWX_BATCH_MID_MAX_N 256
int fwx_solve_batch_mid_f64(int32_t count, int32_t n, double *rate, int32_t *next, int32_t *hops,
                            uint64_t *updates_each, const fwx_opts *opts);
int fwx_solve_batch_mid_f32(int32_t count, int32_t n, float *rate, int32_t *next, int32_t *hops,
                            uint64_t *updates_each, const fwx_opts *opts);
/* The same on caller-owned DEVICE memory, asynchronous on `stream`, nothing allocated or synchronised;
 * stride = elements between consecutive matrices (>= n*n, else FWX_ERR_INVALID; the gap is never read or
 * written; no alignment beyond the element is assumed); pivots [k_begin, k_end) of every matrix, k_end <= 0
 * means n; dtype: fwx_dtype; d_updates_each: optional device array of count uint64, INCREMENTED by each
 * matrix's U.  Statuses as above (n > FWX_BATCH_MID_MAX_N: FWX_ERR_UNSUPPORTED).
 * When it pays (MI355X, f64 + next + hops, profiles/r20_batch_mid.txt): one call against `count` blocking
 * fwx_dev_solve calls.  A workgroup solves its matrix alone on one CU -- 0.33 ms at n = 129, 0.62 ms at 192,
 * 1.28 ms at 256, and no longer for up to 256 matrices -- where one fwx_dev_solve call takes 0.26 - 0.48 ms.  The
 * batch call overtakes the loop at count = 1 for n = 129, between 2 and 4 matrices for n = 192 and n = 256 (at
 * count = 4: 2.1x and 1.3x), and is 68 - 286x faster at count = 256.  For one or two matrices of order 192 and
 * up, call fwx_dev_solve: this entry point does not route them there, because it may not block or allocate.      */
int fwx_dev_solve_batch_mid(int32_t count, int32_t n, int32_t dtype, void *rate, int32_t *next, int32_t *hops,
                            int64_t stride, int32_t k_begin, int32_t k_end,
                            unsigned long long *d_updates_each, void *stream);
/* TEST HOOK: what FWX_BATCH_MID_MIN_N parses to right now.  Needs no device.  Not for production use. */
int fwx_test_batch_mid_min_n(void);
/* TEST HOOK: the pivots per pass of the mid tier (B).  Needs no device.  Not for production use. */
int fwx_test_batch_mid_block(void);

/* ---- batched large solves: many matrices of one order n <= FWX_BATCH_LARGE_MAX_N, several workgroups each ----
 * The calls above stop at n = 256, where one workgroup still solves its matrix alone.  A price history of a 30 x 20
 * market (600 vertices) or a what-if sweep over a 1000-vertex book is a batch of larger matrices, and one such solve
 * does not fill the chip.  These entry points take the batch up to n = 1024: the mid tier's scheme -- 16 pivots per
 * pass from time-k snapshot panels -- with the two phases of a pass as two launches over the whole batch, the
 * panels in device scratch between them, column strips (panel) and tiles (sweep) of every matrix on workgroups of
 * their own.  Every matrix gets the full semantics above, the list rule included; there is no domain check and no
 * routing by content, and each matrix comes back bit-identical to the reference loop on that matrix alone -- rate,
 * next, hops (diagonals included) and U.  The exact `_path` lists: fwx_solve_batch_large_lists_* below.  Matrices
 * of different orders up to 1024 in one call: "ragged batches up to order FWX_BATCH_LARGE_MAX_N" below.
 *
 * The contract is that of fwx_solve_batch_mid_* / fwx_dev_solve_batch_mid, with the limit at
 * FWX_BATCH_LARGE_MAX_N: count matrices of order n, matrix b at rate + b*n*n (next / hops alike, both optional, hops
 * needs next); HOST arrays, solved in place.  updates_each: optional, count entries, U of each matrix.
 * count == 0 or n == 0: FWX_OK, nothing is touched.  FWX_ERR_INVALID: count < 0, n < 0, rate NULL, hops without
 * next, a bad struct_size or pivot range.  FWX_ERR_UNSUPPORTED: n > FWX_BATCH_LARGE_MAX_N, or opts->engine other
 * than FWX_ENGINE_AUTO.  All of these are decided before any device call; then FWX_ERR_NO_DEVICE without a device,
 * the arrays untouched.  opts: device, k_begin / k_end (one range for every matrix), stream / use_stream and
 * updates_out (the SUM of U over the batch) are honoured; serpentine is ignored.  The host forms take the scratch
 * panels from the pooled per-call context, at most 256 MiB: larger batches run in groups on the one stream.
 * Routing: FWX_BATCH_LARGE_MIN_N (environment, read per call; an integer 1 ... 257, default 257, anything else
 * means the default): orders below it are forwarded to fwx_solve_batch_mid_* / fwx_dev_solve_batch_mid (which
 * forward further by FWX_BATCH_MID_MIN_N), orders from it up to 1024 run the large tier.  No result bit depends on
 * it; it exists so that tests and A/B runs can put n <= 256 through the large tier.
 * When to use it: see the measurements beside the device form below.                                        */
#define FWX_BATCH_LARGE_MAX_N 1024
/* Device scratch ONE matrix of order n needs in fwx_dev_solve_batch_large, in bytes: the snapshot panels of 16
 * pivots, 2 panels x 16 rows x n columns x 16 bytes (rate + next + hops in f64; an upper bound for every dtype and
 * field set).                                                                                                 */
#define FWX_BATCH_LARGE_SCRATCH_BYTES(n) ((size_t)(n) * 512)
int fwx_solve_batch_large_f64(int32_t count, int32_t n, double *rate, int32_t *next, int32_t *hops,
                              uint64_t *updates_each, const fwx_opts *opts);
int fwx_solve_batch_large_f32(int32_t count, int32_t n, float *rate, int32_t *next, int32_t *hops,
                              uint64_t *updates_each, const fwx_opts *opts);
/* The same on caller-owned DEVICE memory, asynchronous on `stream`, nothing allocated or synchronised; stride,
 * pivots, dtype and d_updates_each (INCREMENTED) as fwx_dev_solve_batch_mid.  scratch: device memory for the
 * snapshot panels, 16-byte aligned, scratch_bytes >= FWX_BATCH_LARGE_SCRATCH_BYTES(n); the batch is solved in groups
 * of floor(scratch_bytes / FWX_BATCH_LARGE_SCRATCH_BYTES(n)) matrices, one group after the other on `stream`, and
 * nothing past group x FWX_BATCH_LARGE_SCRATCH_BYTES(n) bytes of it is touched.  FWX_ERR_INVALID for scratch that is
 * NULL, misaligned or too small for one matrix -- only when n is routed to the large tier and the pivot range is not
 * empty; below FWX_BATCH_LARGE_MIN_N scratch is ignored.  Statuses otherwise as above (n > FWX_BATCH_LARGE_MAX_N:
 * FWX_ERR_UNSUPPORTED).  A solve is 2 * ceil(pivots / 16) launches per group.
 * When it pays (MI355X, f64 + next + hops, profiles/r24_batch_large.txt): one call against `count` blocking
 * fwx_dev_solve calls.  One matrix takes the call 0.42 ms at n = 257, 0.59 at 384, 0.78 at 512, 1.20 at 768 and
 * 1.60 ms at 1024 -- 64 pivot blocks of a 7.7 us panel launch and a 17.3 us sweep launch, back to back -- where
 * fwx_dev_solve takes 1.03, 0.45, 0.55, 0.82 and 1.07 ms.  The call overtakes the loop at count = 1 for n = 257 and at
 * count = 2 for n = 384 ... 1024 (1.5x ... 1.1x); at count = 16 it is 26x, 14x, 9.7x, 7.4x and 4.7x faster, at
 * count = 256 66x, 21x, 15x, 7.5x and 4.4x (0.048 ms per matrix at n = 512, 0.33 ms at n = 1024).  For ONE matrix of
 * order 384 and up call fwx_dev_solve: this entry point does not route it there, because it may not block or
 * allocate.  Around n = 256 fwx_dev_solve_batch_mid is the better call somewhere between 64 and 256 matrices
 * (64: 1.31 ms at n = 256 against 1.05 ms at n = 257 here; 256: 1.37 against 3.21 ms); for fewer matrices this
 * tier is the faster one, 0.42 against 1.26 ms up to 4 matrices (FWX_BATCH_LARGE_MIN_N routes them here).     */
int fwx_dev_solve_batch_large(int32_t count, int32_t n, int32_t dtype, void *rate, int32_t *next, int32_t *hops,
                              int64_t stride, int32_t k_begin, int32_t k_end,
                              unsigned long long *d_updates_each,
                              void *scratch, size_t scratch_bytes, void *stream);
/* TEST HOOK: what FWX_BATCH_LARGE_MIN_N parses to right now.  Needs no device.  Not for production use. */
int fwx_test_batch_large_min_n(void);
/* TEST HOOK: the geometry of the large tier: out[0] = pivots per pass (B), out[1] = width of a panel strip (S),
 * out[2] / out[3] = rows / columns of a sweep tile.  Needs no device.  Not for production use. */
int fwx_test_batch_large_geometry(int32_t out[4]);

/* ---- batched small solves with the exact `_path` lists ----------------------------------------------------
 * The reference returns, per entry, the list it concatenated when the entry last improved (`_path`,
 * Algorithms.hs:55; see "Exact `_path` lists" below): under exact ties -- its 1.0 edges between the same currency
 * on two exchanges make them the normal case -- that is not the walk of the final next-hops.  The traced batch
 * solve keeps, per matrix, the three int32 arrays of the path trace (fwx_trace: last, at_col, at_row), laid out
 * like next: matrix b at + b*stride, pitch n.  The solve writes every cell of the n x n part of each array (the
 * caller need not initialise them) and never the gap.  Whole pivot range only; next is required, hops optional.
 * fwx_dev_exact_paths_batch then rebuilds the lists of `items` triples (mat[q], src[q], dst[q]) from the trace and
 * from next0, the caller's copy of the UNSOLVED next-hop array of the batch (same layout; fwx_dev_follow_paths
 * takes the unsolved edge rates in the same way): one thread per item.  len_out[q] is the length of list q,
 * FWX_ERR_CAPACITY when that list is longer than cap, FWX_ERR_INVALID for an item with mat outside [0, count) or
 * src / dst outside [0, n) -- item by item, the other items are answered; path_out + q*cap receives list q.
 * Capacity, as for fwx_matrix_query_exact: a list of L entries is returned whenever cap >= L, and
 * FWX_ERR_CAPACITY exactly when L > cap.  An empty list (length 0) fits any cap >= 1.  The walk's stack is sized by
 * n and never by cap: scratch holds items * FWX_EXACT_SCRATCH_INTS(n) int32.
 * Domain: there is no domain check and no routing: a batch may mix matrices inside and outside the domain, and
 * every list equals the reference's.
 * Both device forms run on caller-owned DEVICE memory (the item arrays and outputs included), asynchronously on
 * `stream`; they allocate nothing and synchronise nothing.  Tier choice by FWX_BATCH_WAVE_MAX_N as above.
 *
 * fwx_solve_batch_lists_f64 / _f32: HOST arrays.  What fwx_solve_batch_* does over the whole pivot range -- the
 * arrays solved in place, updates_each, opts->updates_out -- and in the same call the lists of `items` triples
 * (host arrays; len_out and path_out as above).  items == 0 is a plain whole-range batch solve.  The unsolved
 * next-hops and the trace stay on the device in the pooled per-call context; the items are walked in chunks so that
 * the lists, stacks and item arrays of one launch stay within 64 MiB of device memory.
 * FWX_BATCH_LISTS_CHUNK (environment, read per call; digits only, >= 1, anything else means the default): items per
 * launch, where that is fewer than the budget allows -- for tests and A/B runs.  No result depends on it.
 *
 * Statuses, all decided before any device call.  FWX_ERR_INVALID: count, n or items negative; rate, next or
 * trace (or one of its three pointers; device forms) NULL; hops without next; stride < n*n; cap < 1 with
 * items > 0; a NULL item array, output or scratch with items > 0; a bad struct_size; a pivot range in opts other
 * than the whole one.  FWX_ERR_UNSUPPORTED: n > FWX_BATCH_MAX_N, or an engine other than FWX_ENGINE_AUTO.
 * count == 0 or n == 0: FWX_OK, nothing is touched.  Then FWX_ERR_NO_DEVICE without a device, the arrays
 * untouched.                                                                                              */
struct fwx_trace;
int fwx_dev_solve_batch_traced(int32_t count, int32_t n, int32_t dtype, void *rate, int32_t *next, int32_t *hops,
                               int64_t stride, const struct fwx_trace *trace,
                               unsigned long long *d_updates_each, void *stream);
#define FWX_EXACT_SCRATCH_INTS(n) (3 * ((n) + 2))        /* per item */
int fwx_dev_exact_paths_batch(int32_t count, int32_t n, int64_t stride, const int32_t *next0,
                              const struct fwx_trace *trace, int32_t items, const int32_t *mat,
                              const int32_t *src, const int32_t *dst, int32_t *len_out, int32_t *path_out,
                              int32_t cap, int32_t *scratch, void *stream);
int fwx_solve_batch_lists_f64(int32_t count, int32_t n, double *rate, int32_t *next, int32_t *hops,
                              uint64_t *updates_each, int32_t items, const int32_t *mat, const int32_t *src,
                              const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap,
                              const fwx_opts *opts);
int fwx_solve_batch_lists_f32(int32_t count, int32_t n, float *rate, int32_t *next, int32_t *hops,
                              uint64_t *updates_each, int32_t items, const int32_t *mat, const int32_t *src,
                              const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap,
                              const fwx_opts *opts);
/* TEST HOOK: items per launch of fwx_solve_batch_lists_* for order n and capacity cap, as FWX_BATCH_LISTS_CHUNK and
 * the budget give it right now (FWX_ERR_INVALID for n < 0 or cap < 1).  Needs no device.  Not for production use. */
int64_t fwx_test_batch_lists_chunk(int32_t n, int32_t cap);

/* ---- batched mid-size solves with the exact `_path` lists -------------------------------------------------
 * The three families above with the limit at FWX_BATCH_MID_MAX_N (256): a batch of 20 x 12 markets gets the lists
 * the reference would print, not only rate, next and hops.  The contracts are those of fwx_dev_solve_batch_traced,
 * fwx_dev_exact_paths_batch and fwx_solve_batch_lists_*, word for word -- the statuses decided before any device
 * call (FWX_ERR_UNSUPPORTED: n > FWX_BATCH_MID_MAX_N), whole pivot range only, next required, hops optional, every
 * cell of the n x n part of the three trace arrays written by the solve and the gap never, the capacity rule, items
 * judged one by one, scratch of items * FWX_EXACT_SCRATCH_INTS(n) int32, chunks by FWX_BATCH_LISTS_CHUNK.
 * Routing by FWX_BATCH_MID_MIN_N as for fwx_solve_batch_mid_*: orders below it run the traced tiers above, orders
 * from it up the mid tier, which keeps the trace in device memory beside the matrix (no LDS copy: the f64 + next +
 * hops form already fills the CU's LDS).  No cell of any output, the trace arrays included, depends on it.  The
 * entry points above keep refusing n > FWX_BATCH_MAX_N.
 * Cost (MI355X, f64 + next + hops on market inputs): profiles/r21_batch_mid_lists.txt.                        */
int fwx_dev_solve_batch_mid_traced(int32_t count, int32_t n, int32_t dtype, void *rate, int32_t *next,
                                   int32_t *hops, int64_t stride, const struct fwx_trace *trace,
                                   unsigned long long *d_updates_each, void *stream);
int fwx_dev_exact_paths_batch_mid(int32_t count, int32_t n, int64_t stride, const int32_t *next0,
                                  const struct fwx_trace *trace, int32_t items, const int32_t *mat,
                                  const int32_t *src, const int32_t *dst, int32_t *len_out, int32_t *path_out,
                                  int32_t cap, int32_t *scratch, void *stream);
int fwx_solve_batch_mid_lists_f64(int32_t count, int32_t n, double *rate, int32_t *next, int32_t *hops,
                                  uint64_t *updates_each, int32_t items, const int32_t *mat, const int32_t *src,
                                  const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap,
                                  const fwx_opts *opts);
int fwx_solve_batch_mid_lists_f32(int32_t count, int32_t n, float *rate, int32_t *next, int32_t *hops,
                                  uint64_t *updates_each, int32_t items, const int32_t *mat, const int32_t *src,
                                  const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap,
                                  const fwx_opts *opts);

/* ---- batched large solves with the exact `_path` lists ----------------------------------------------------
 * The three families above with the limit at FWX_BATCH_LARGE_MAX_N (1024): a price history of a 30 x 20 market gets
 * the lists the reference would print, not only rate, next and hops.  The contracts are those of
 * fwx_dev_solve_batch_mid_traced, fwx_dev_exact_paths_batch_mid and fwx_solve_batch_mid_lists_*, word for word -- the
 * statuses decided before any device call (FWX_ERR_UNSUPPORTED: n > FWX_BATCH_LARGE_MAX_N), whole pivot range only,
 * next required, hops optional, every cell of the n x n part of the three trace arrays written by the solve (the
 * diagonal included; the caller initialises nothing) and the gap never, the capacity rule, items judged one by one,
 * scratch of the walk items * FWX_EXACT_SCRATCH_INTS(n) int32, chunks by FWX_BATCH_LISTS_CHUNK.
 * scratch / scratch_bytes of the traced solve: the snapshot panels, by the rules of fwx_dev_solve_batch_large --
 * 16-byte aligned, at least FWX_BATCH_LARGE_SCRATCH_BYTES(n) (the trace needs none of it: the value is the untraced
 * call's), the batch solved in groups of what it holds; FWX_ERR_INVALID for scratch that is NULL, misaligned or too
 * small, only when n is routed to the large tier.  The host forms take the panels and the lists' memory from the
 * pooled per-call context in one piece, the panels capped at 256 MiB as for fwx_solve_batch_large_*.
 * Routing by FWX_BATCH_LARGE_MIN_N as for fwx_solve_batch_large_*: orders below it go to
 * fwx_dev_solve_batch_mid_traced / the mid lists path (which forward further), orders from it up run the large tier:
 * `last` is filled by a launch of its own before the first pivot block, the panel launch carries `last` of its strip
 * through the panel phase in two more LDS panels and writes every cell of at_row / at_col from exactly one workgroup,
 * the sweep stores `last` with next and hops.  No cell of any output, the trace arrays included, depends on the
 * routing.  The entry points above keep refusing n > FWX_BATCH_MID_MAX_N.
 * When it pays (MI355X, f64 + next + hops on market inputs, profiles/r27_batch_large_lists.txt).  The trace costs the
 * solve 6 - 8 % for one matrix, 5.5 - 15 % for 16 and 15 - 18 % for 256 (n = 512, 16 matrices: 1.23 against 1.16 ms;
 * n = 1024, 256 matrices: 91.4 against 79.4 ms); the walk of 65536 lists takes 0.10 - 0.13 ms at every order.  Against
 * what a host had before -- one traced handle per matrix: upload, solve, fwx_matrix_query_exact_batch -- solve plus
 * walk per matrix is 11.6x / 11.2x / 9.5x / 7.2x / 4.8x faster at n = 257 / 384 / 512 / 768 / 1024 with 16 matrices
 * (0.042 ... 0.40 ms against 0.49 ... 1.9 ms), 29x ... 4.1x with 256, and 1.2 - 1.6x with one.  The HOST form copies the
 * whole batch to the device and back through the caller's arrays and is bound by that: with 16 matrices it is 3.6x and
 * 2.4x faster than the handle loop at n = 257 and 512 but 2 - 3x slower at n = 384, 768 and 1024, and 1.5 - 1.7x slower
 * for one matrix at every order -- a host that can keep the batch on the device calls the device forms.           */
int fwx_dev_solve_batch_large_traced(int32_t count, int32_t n, int32_t dtype, void *rate, int32_t *next,
                                     int32_t *hops, int64_t stride, const struct fwx_trace *trace,
                                     unsigned long long *d_updates_each,
                                     void *scratch, size_t scratch_bytes, void *stream);
int fwx_dev_exact_paths_batch_large(int32_t count, int32_t n, int64_t stride, const int32_t *next0,
                                    const struct fwx_trace *trace, int32_t items, const int32_t *mat,
                                    const int32_t *src, const int32_t *dst, int32_t *len_out, int32_t *path_out,
                                    int32_t cap, int32_t *scratch, void *stream);
int fwx_solve_batch_large_lists_f64(int32_t count, int32_t n, double *rate, int32_t *next, int32_t *hops,
                                    uint64_t *updates_each, int32_t items, const int32_t *mat, const int32_t *src,
                                    const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap,
                                    const fwx_opts *opts);
int fwx_solve_batch_large_lists_f32(int32_t count, int32_t n, float *rate, int32_t *next, int32_t *hops,
                                    uint64_t *updates_each, int32_t items, const int32_t *mat, const int32_t *src,
                                    const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap,
                                    const fwx_opts *opts);

/* ---- ragged batched small solves: matrices of DIFFERENT orders in one call --------------------------------
 * A price history does not have one order: the vertex set grows as exchanges and currencies first appear, and venue
 * groups differ in size.  A ragged batch is `count` matrices; matrix b has order n_each[b], 0 <= n_each[b] <=
 * FWX_BATCH_MAX_N, pitch n_each[b], and starts at element offset[b] of rate; next, hops and the three trace arrays
 * use the same offsets.  These are the semantics of the uniform batch above applied per matrix: the full list rule,
 * no domain check and no routing, every matrix bit-identical to the reference loop on that matrix alone, and no
 * matrix pays for the largest order of the batch.  Only the whole pivot range is supported.
 *
 * fwx_ragged_plan: the schedule, from the orders alone; needs no device.  offset_out (count + 1 entries) receives the
 * PACKED offsets, offset[b] = sum of n_a * n_a over a < b, and the total at [count].  order_out (count entries)
 * receives the indices of the matrices with n_b >= 1 grouped by tier -- the wave tier (n_b <= FWX_BATCH_WAVE_MAX_N,
 * the setting above, read by the plan and only by the plan), then the 64-wide workgroup tier (n_b <= 64), then the
 * 128-wide one -- and within a tier sorted by descending order, ties by ascending index, so that the longest
 * workgroups start first; the entries past the three counts are -1.  tier_count_out: matrices per tier.  Matrices of
 * order 0 appear in no tier.  Any of the three outputs may be NULL.  FWX_ERR_INVALID: count < 0, n_each NULL with
 * count > 0, a negative order.  FWX_ERR_UNSUPPORTED: an order above FWX_BATCH_MAX_N.  No result bit of a solve
 * depends on the split.
 *
 * fwx_solve_ragged_f64 / _f32: HOST arrays, the batch packed (the offsets of fwx_ragged_plan), solved in place with
 * up to three launches -- one per non-empty tier, the 128-wide tier first -- on one stream.  updates_each: optional,
 * count entries, U of each matrix (0 for order 0).  opts as for fwx_solve_batch_*, except that a pivot range other
 * than the whole one (k_begin != 0 or k_end > 0) is FWX_ERR_INVALID.
 * fwx_solve_ragged_lists_f64 / _f32: the same and, in the same call, the exact `_path` lists of `items` triples, as
 * fwx_solve_batch_lists_*; the items are walked in chunks sized by the largest order present.
 *
 * fwx_dev_solve_ragged: caller-owned DEVICE memory -- the three index arrays d_n_each, d_offset (count entries each)
 * and d_order included -- asynchronous on `stream`, nothing allocated or synchronised.  The offsets need not be
 * packed: nothing outside the n_b x n_b cells of a matrix is read or written, so the caller may leave gaps between
 * matrices and place them in any order (they must not overlap).  d_order / tier_count (HOST, three entries) are a
 * plan as fwx_ragged_plan gives it for these orders; a matrix listed in a tier whose tile does not hold its order is
 * left untouched.  trace (or NULL): the path trace as in fwx_dev_solve_batch_traced, at the same offsets; next is
 * then required and every cell of every n_b x n_b part of the three arrays is written.  d_updates_each: optional,
 * count uint64, entry b INCREMENTED by U of matrix b.
 * fwx_dev_exact_paths_ragged: the lists of `items` triples from such a trace and from next0, the caller's copy of the
 * unsolved next-hops (same offsets), one thread per item, as fwx_dev_exact_paths_batch.  An item with mat outside
 * [0, count), or with src / dst outside [0, n_mat) -- n_mat the order of THAT item's matrix, not n_max; no item of an
 * order-0 matrix is valid -- gets FWX_ERR_INVALID alone.  Capacity rule and stack bound as above; n_max is at least
 * the largest order of the batch and scratch holds items * FWX_EXACT_SCRATCH_INTS(n_max) int32.
 *
 * Statuses, all decided before any device call.  FWX_ERR_INVALID: a negative count, items or order; n_each NULL; rate
 * NULL when some order is positive; hops without next; the lists arguments as in fwx_solve_batch_lists_*; a bad
 * struct_size; a pivot range; in the device forms a bad dtype, a NULL tier_count, a negative tier count or a sum of
 * the three above count, a NULL index array, a trace without next or with a NULL pointer.  FWX_ERR_UNSUPPORTED: an
 * order (n_max in the walk) above FWX_BATCH_MAX_N, or an engine other than FWX_ENGINE_AUTO.  count == 0, or every
 * order 0 (device form: all three tier counts 0; walk: n_max == 0 or items == 0): FWX_OK, nothing is touched.  Then
 * FWX_ERR_NO_DEVICE without a device, the arrays untouched.                                                   */
int fwx_ragged_plan(int32_t count, const int32_t *n_each, int64_t *offset_out, int32_t *order_out,
                    int32_t tier_count_out[3]);
int fwx_solve_ragged_f64(int32_t count, const int32_t *n_each, double *rate, int32_t *next, int32_t *hops,
                         uint64_t *updates_each, const fwx_opts *opts);
int fwx_solve_ragged_f32(int32_t count, const int32_t *n_each, float *rate, int32_t *next, int32_t *hops,
                         uint64_t *updates_each, const fwx_opts *opts);
int fwx_dev_solve_ragged(int32_t count, int32_t dtype, void *rate, int32_t *next, int32_t *hops,
                         const int32_t *d_n_each, const int64_t *d_offset, const int32_t *d_order,
                         const int32_t tier_count[3], const struct fwx_trace *trace,
                         unsigned long long *d_updates_each, void *stream);
int fwx_dev_exact_paths_ragged(int32_t count, const int32_t *d_n_each, const int64_t *d_offset, int32_t n_max,
                               const int32_t *next0, const struct fwx_trace *trace, int32_t items,
                               const int32_t *mat, const int32_t *src, const int32_t *dst, int32_t *len_out,
                               int32_t *path_out, int32_t cap, int32_t *scratch, void *stream);
int fwx_solve_ragged_lists_f64(int32_t count, const int32_t *n_each, double *rate, int32_t *next, int32_t *hops,
                               uint64_t *updates_each, int32_t items, const int32_t *mat, const int32_t *src,
                               const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap,
                               const fwx_opts *opts);
int fwx_solve_ragged_lists_f32(int32_t count, const int32_t *n_each, float *rate, int32_t *next, int32_t *hops,
                               uint64_t *updates_each, int32_t items, const int32_t *mat, const int32_t *src,
                               const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap,
                               const fwx_opts *opts);

/* ---- ragged batches up to order FWX_BATCH_MID_MAX_N: a fourth tier in the same call ------------------------
 * A history of the 20 x 12 market above (240 vertices) is ragged AND crosses 128.  These entry points are the
 * ragged family above, word for word, with the limit at FWX_BATCH_MID_MAX_N (256) and a plan of FOUR tiers: the
 * three above and the mid tier (one workgroup per matrix, the matrix resident in device memory, as
 * fwx_dev_solve_batch_mid runs it).  Every matrix comes back bit-identical to the reference loop on that matrix alone
 * -- rate, next, hops, U, the trace and the lists -- and no matrix pays for the largest order of the batch.  The
 * entry points above keep refusing orders above FWX_BATCH_MAX_N, and fwx_ragged_plan keeps its three tiers.
 *
 * fwx_ragged_mid_plan: as fwx_ragged_plan, needs no device; order_out groups the matrices with n_b >= 1 into the
 * wave tier, the 64-wide tier, the 128-wide tier and the mid tier, in this order, each sorted by descending order,
 * ties by ascending index, the rest -1; tier_count_out has four entries.  Tier boundaries: FWX_BATCH_WAVE_MAX_N as
 * above, and FWX_BATCH_MID_MIN_N (1 ... 129, default 129, as for fwx_solve_batch_mid_*) sends every order from it
 * upward to the mid tier.  Both are read by the plan and only by the plan.  Where both settings claim an order
 * (FWX_BATCH_MID_MIN_N <= n_b <= FWX_BATCH_WAVE_MAX_N) the MID tier wins.  With FWX_BATCH_MID_MIN_N at its default
 * and every order <= FWX_BATCH_MAX_N the first three counts and the order list are fwx_ragged_plan's.
 * FWX_ERR_INVALID as fwx_ragged_plan; FWX_ERR_UNSUPPORTED: an order above FWX_BATCH_MID_MAX_N.  No result bit of a
 * solve depends on the split.
 *
 * fwx_solve_ragged_mid_f64 / _f32 and fwx_solve_ragged_mid_lists_f64 / _f32: HOST arrays, packed, whole pivot range
 * only; up to four launches on one stream, the mid tier first because its workgroups run longest.  updates_each,
 * opts->updates_out, the lists arguments, the chunks (FWX_BATCH_LISTS_CHUNK, sized by the largest order present) and
 * the capacity rule as in fwx_solve_ragged_* / fwx_solve_ragged_lists_*.
 *
 * fwx_dev_solve_ragged_mid / fwx_dev_exact_paths_ragged_mid: caller-owned DEVICE memory, asynchronous on `stream`,
 * nothing allocated or synchronised; the offsets need not be packed and nothing outside the n_b x n_b cells of a
 * matrix is read or written.  tier_count (HOST) has four entries.  In the three small tiers a matrix listed in a
 * tier whose tile does not hold its order is left untouched, as above; the mid tier's tile holds every order 1 ...
 * 256, so a matrix of ANY such order listed there is solved.  An id outside [0, count) in d_order leaves its
 * workgroup idle.  The walk: n_max <= FWX_BATCH_MID_MAX_N, scratch holds items * FWX_EXACT_SCRATCH_INTS(n_max) int32.
 *
 * Statuses, all decided before any device call, as in the ragged family above with: FWX_ERR_UNSUPPORTED for an order
 * (n_max in the walk) above FWX_BATCH_MID_MAX_N; FWX_ERR_INVALID for a sum of the FOUR tier counts above count.
 * Then FWX_ERR_NO_DEVICE without a device, the arrays untouched.
 * When it pays (MI355X, f64 + next + hops, profiles/r22_ragged_mid.txt): 4096 matrices whose orders ramp from 4 to 256
 * take 8.3 ms in one fwx_dev_solve_ragged_mid call, 19.7 ms NaN-padded to 256 in one fwx_dev_solve_batch_mid launch
 * and 12.5 ms split by hand into fwx_dev_solve_ragged plus one padded mid launch.  With all orders equal the call is
 * 0.4 - 1.5 % slower than fwx_dev_solve_batch_mid (most at n = 129): use that one for a uniform batch.          */
int fwx_ragged_mid_plan(int32_t count, const int32_t *n_each, int64_t *offset_out, int32_t *order_out,
                        int32_t tier_count_out[4]);
int fwx_solve_ragged_mid_f64(int32_t count, const int32_t *n_each, double *rate, int32_t *next, int32_t *hops,
                             uint64_t *updates_each, const fwx_opts *opts);
int fwx_solve_ragged_mid_f32(int32_t count, const int32_t *n_each, float *rate, int32_t *next, int32_t *hops,
                             uint64_t *updates_each, const fwx_opts *opts);
int fwx_dev_solve_ragged_mid(int32_t count, int32_t dtype, void *rate, int32_t *next, int32_t *hops,
                             const int32_t *d_n_each, const int64_t *d_offset, const int32_t *d_order,
                             const int32_t tier_count[4], const struct fwx_trace *trace,
                             unsigned long long *d_updates_each, void *stream);
int fwx_dev_exact_paths_ragged_mid(int32_t count, const int32_t *d_n_each, const int64_t *d_offset, int32_t n_max,
                                   const int32_t *next0, const struct fwx_trace *trace, int32_t items,
                                   const int32_t *mat, const int32_t *src, const int32_t *dst, int32_t *len_out,
                                   int32_t *path_out, int32_t cap, int32_t *scratch, void *stream);
int fwx_solve_ragged_mid_lists_f64(int32_t count, const int32_t *n_each, double *rate, int32_t *next, int32_t *hops,
                                   uint64_t *updates_each, int32_t items, const int32_t *mat, const int32_t *src,
                                   const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap,
                                   const fwx_opts *opts);
int fwx_solve_ragged_mid_lists_f32(int32_t count, const int32_t *n_each, float *rate, int32_t *next, int32_t *hops,
                                   uint64_t *updates_each, int32_t items, const int32_t *mat, const int32_t *src,
                                   const int32_t *dst, int32_t *len_out, int32_t *path_out, int32_t cap,
                                   const fwx_opts *opts);

/* ---- ragged batches up to order FWX_BATCH_LARGE_MAX_N: a fifth tier in the same call ----------------------
 * A price history of the 30 x 20 market above (600 vertices) is ragged AND crosses 256.  These entry points are the
 * ragged-mid family above, entry for entry and word for word, with the limit at FWX_BATCH_LARGE_MAX_N (1024) and a
 * plan of FIVE tiers: the four above and the large tier (several workgroups per matrix over two launches per block of
 * 16 pivots, as fwx_dev_solve_batch_large runs it).  Every matrix comes back bit-identical to the reference loop on
 * that matrix alone -- rate, next, hops (diagonals included), U, the trace and the lists; the full list rule, no
 * domain check, no routing by content, whole pivot range only -- and no matrix pays for the largest order of the
 * batch: a matrix of order n_b takes part in ceil(n_b / 16) blocks of pivots and costs nothing afterwards.  The entry
 * points above keep their limits and their outputs; fwx_ragged_plan and fwx_ragged_mid_plan are unchanged.
 *
 * fwx_ragged_large_plan: as fwx_ragged_mid_plan, needs no device; order_out groups the matrices with n_b >= 1 into
 * the wave, 64-wide, 128-wide, mid and large tier, in this order, each sorted by descending order, ties by ascending
 * index, the rest -1; tier_count_out has five entries.  Tier boundaries: FWX_BATCH_WAVE_MAX_N and FWX_BATCH_MID_MIN_N
 * as above, and FWX_BATCH_LARGE_MIN_N (1 ... 257, default 257, as for fwx_solve_batch_large_*) sends every order from
 * it upward to the large tier.  All three are read by the plan and only by the plan.  Where several settings claim an
 * order the LARGE tier wins over the mid tier, and the mid tier over the wave tier.  At default settings with every
 * order <= FWX_BATCH_MID_MAX_N the first four counts and the order list are fwx_ragged_mid_plan's.
 * work_out (optional like the others; FWX_RAGGED_LARGE_WORK_ENTRIES(count) int64): the large tier's work table, three
 * rows of count + 1 entries.  With L matrices in the large tier and slot m the m-th of its list, for every m <= L
 *   row 0, panel_base[m] = sum of n_a over the slots a < m: the scratch panels of slot m start 512 * (panel_base[m] -
 *          panel_base[first slot of its group]) bytes into the scratch;
 *   row 1, strip_base[m] = sum of ceil(n_a / S): the panel workgroups before slot m;
 *   row 2, tile_base[m]  = sum of ceil(n_a / TC) * ceil(n_a / TR): the sweep workgroups before slot m,
 * (S, TR, TC) those of fwx_test_batch_large_geometry; the entries past L repeat entry L.  The sort is what the
 * kernels rely on: at the block of pivots that starts at k0 the matrices still active, n_b > k0, are a prefix of the
 * list.  FWX_ERR_INVALID as fwx_ragged_plan; FWX_ERR_UNSUPPORTED: an order above FWX_BATCH_LARGE_MAX_N.  No result
 * bit of a solve depends on the split.
 *
 * fwx_solve_ragged_large_f64 / _f32 and fwx_solve_ragged_large_lists_f64 / _f32: HOST arrays, packed, whole pivot
 * range only; the four small tiers' launches as in fwx_solve_ragged_mid_*, then the large tier's on the same stream.
 * The plan, the work table and the scratch panels come from the pooled per-call context, the panels capped at
 * 256 MiB as for fwx_solve_batch_large_*: larger batches run in groups.  updates_each, opts->updates_out, the lists
 * arguments, the chunks and the capacity rule as in fwx_solve_ragged_mid_* / fwx_solve_ragged_mid_lists_*.
 *
 * fwx_dev_solve_ragged_large / fwx_dev_exact_paths_ragged_large: caller-owned DEVICE memory, asynchronous on
 * `stream`, nothing allocated or synchronised; offsets, trace and counters (by matrix id) as in
 * fwx_dev_solve_ragged_mid.  tier_count (HOST) has five entries.  work (HOST) and d_work (DEVICE, the same contents)
 * are the plan's work table; scratch is device memory for the panels, 16-byte aligned, scratch_bytes at least
 * FWX_BATCH_LARGE_SCRATCH_BYTES(the largest order of the large tier).  A GROUP is a maximal run of consecutive slots
 * whose panels fit scratch_bytes (and whose tiles number less than 2^31); the groups run one after the other on
 * `stream`, each 2 * ceil(n_first / 16) launches, n_first its largest order: per block of pivots one panel and one
 * sweep launch over the group's active prefix, in which every workgroup finds its slot by binary search in d_work.
 * With a trace one more launch, before the first group, writes -1 to exactly the n_b x n_b cells of `last`.  A
 * workgroup whose matrix id lies outside [0, count), whose order lies outside 1 ... 1024 or whose panels would end
 * past scratch_bytes stays idle; whatever the device tables hold, nothing outside the n_b x n_b cells of a matrix
 * and the scratch_bytes given is read or written.  With tier_count[4] == 0 the table and the scratch are ignored and
 * may be NULL.  The walk: n_max <= FWX_BATCH_LARGE_MAX_N, scratch holds items * FWX_EXACT_SCRATCH_INTS(n_max) int32.
 *
 * Statuses, all decided before any device call, as in the ragged-mid family with: FWX_ERR_UNSUPPORTED for an order
 * (n_max in the walk) above FWX_BATCH_LARGE_MAX_N; FWX_ERR_INVALID for a sum of the FIVE tier counts above count
 * and, with tier_count[4] > 0, for a NULL work or d_work, a host table whose rows are not non-decreasing, whose
 * orders (the differences of row 0) lie outside 1 ... 1024 or do not descend, or whose strip and tile rows are not
 * those of these orders, and for scratch that is NULL, misaligned or too small.  Then FWX_ERR_NO_DEVICE without a
 * device, the arrays untouched.
 * When it pays (MI355X, f64 + next + hops, profiles/r31_ragged_large.txt): 512 matrices whose orders ramp from 4 to
 * 1024 take 56.1 ms in one fwx_dev_solve_ragged_large call (one group, 128 launches), 144.3 ms NaN-padded to 1024 in
 * one fwx_dev_solve_batch_large call and 113.6 ms split by hand into fwx_dev_solve_ragged_mid plus one padded large
 * call; the host form takes 158.1 ms against 451.4 ms padded.  With all orders equal the call is SLOWER than
 * fwx_dev_solve_batch_large by more than twice that call's spread in every cell measured -- 6.7 / 7.4 % at n = 257
 * (16 / 256 matrices), 6.0 / 4.9 % at 512, 3.5 / 3.8 % at 1024, the cost of the slot search: use that one for a
 * uniform batch.                                                                                               */
#define FWX_RAGGED_LARGE_WORK_ENTRIES(count) (3 * ((size_t)(count) + 1))
int fwx_ragged_large_plan(int32_t count, const int32_t *n_each, int64_t *offset_out, int32_t *order_out,
                          int32_t tier_count_out[5], int64_t *work_out);
int fwx_solve_ragged_large_f64(int32_t count, const int32_t *n_each, double *rate, int32_t *next, int32_t *hops,
                               uint64_t *updates_each, const fwx_opts *opts);
int fwx_solve_ragged_large_f32(int32_t count, const int32_t *n_each, float *rate, int32_t *next, int32_t *hops,
                               uint64_t *updates_each, const fwx_opts *opts);
int fwx_dev_solve_ragged_large(int32_t count, int32_t dtype, void *rate, int32_t *next, int32_t *hops,
                               const int32_t *d_n_each, const int64_t *d_offset, const int32_t *d_order,
                               const int32_t tier_count[5], const int64_t *work, const int64_t *d_work,
                               const struct fwx_trace *trace, unsigned long long *d_updates_each, void *scratch,
                               size_t scratch_bytes, void *stream);
int fwx_dev_exact_paths_ragged_large(int32_t count, const int32_t *d_n_each, const int64_t *d_offset, int32_t n_max,
                                     const int32_t *next0, const struct fwx_trace *trace, int32_t items,
                                     const int32_t *mat, const int32_t *src, const int32_t *dst, int32_t *len_out,
                                     int32_t *path_out, int32_t cap, int32_t *scratch, void *stream);
int fwx_solve_ragged_large_lists_f64(int32_t count, const int32_t *n_each, double *rate, int32_t *next,
                                     int32_t *hops, uint64_t *updates_each, int32_t items, const int32_t *mat,
                                     const int32_t *src, const int32_t *dst, int32_t *len_out, int32_t *path_out,
                                     int32_t cap, const fwx_opts *opts);
int fwx_solve_ragged_large_lists_f32(int32_t count, const int32_t *n_each, float *rate, int32_t *next,
                                     int32_t *hops, uint64_t *updates_each, int32_t items, const int32_t *mat,
                                     const int32_t *src, const int32_t *dst, int32_t *len_out, int32_t *path_out,
                                     int32_t cap, const fwx_opts *opts);
/* TEST HOOK: the schedule fwx_dev_solve_ragged_large makes of a host work table (count + 1 entries to a row) whose
 * first large_count slots are listed, with scratch_bytes of scratch: returns the number of groups and writes the first
 * slot of each, up to cap, to group_first; totals[0] = launches, totals[1] = panel workgroups, totals[2] = sweep
 * workgroups over the whole call (no trace).  FWX_ERR_INVALID as the device form.  Needs no device.  Not for
 * production use. */
int fwx_test_ragged_large_schedule(int32_t count, int32_t large_count, const int64_t *work, size_t scratch_bytes,
                                   int32_t *group_first, int32_t cap, int64_t totals[3]);

/* ---- batched what-if sweeps: variants of ONE base matrix of order n <= FWX_SWEEP_MAX_N solved in one call ----
 * A what-if sweep is `count` variants of one matrix that differ from it in a handful of entries -- a candidate quote
 * changes two entries of buildMatrix's output -- and the host wants a few entries of each solved variant, say the best
 * rate A -> B under each quote.  fwx_solve_batch_* serves it only from `count` materialised copies, count * n * n
 * entries per field each way; here the base goes up once, the device builds variant b in the registers of the batch
 * tiers, and only the queried entries come back.  No count * n * n array exists unless the caller asks for one.
 *
 * Variant b is M_b = the base with the patches [patches->ptr[b], patches->ptr[b+1]) applied in list order: patch q
 * puts rate[q] at cell index[q] = i*n + j, and next[q] / hops[q] there if those arrays are given (NULL: that field
 * of the cell keeps the base's value, as fwx_matrix_patch_input); a later patch of the same cell wins; the diagonal
 * may be patched.  Item q of [items->ptr[b], items->ptr[b+1]) receives entry (src[q], dst[q]) of the SOLVED M_b:
 * rate_out[q], and next_out[q] (the first hop) / hops_out[q] (the length) if given.  Every output is bit for bit what
 * fwx_solve_batch_* returns for M_b, and so what the reference loop returns for it: rate, next, hops (diagonals
 * included) and U; the full list rule applies, there is no domain check and no routing by content.  Whole pivot range
 * only, no path trace.  Tier choice by FWX_BATCH_WAVE_MAX_N as above; no result bit depends on it.  Inputs and
 * outputs must not overlap.
 *
 * Device form: every pointer, those inside the structs included, is DEVICE memory; asynchronous on `stream`, nothing
 * allocated or synchronised; the base is never written.  patches NULL: every variant is the base.  items NULL: no
 * items.  full NULL, or any of its three pointers NULL: that output is not wanted; otherwise the whole n x n part of
 * the solved M_b goes to full->rate + b*stride (next, hops alike), diagonal included, the gap never written.
 * d_updates_each: optional, count uint64, INCREMENTED by each variant's U.  The device form cannot read the tables:
 * each [ptr[b], ptr[b+1]) is clamped into [0, total] (a descending pair is empty), a patch whose index is outside
 * [0, n*n) is ignored and an item whose src or dst is outside [0, n) leaves its outputs untouched -- whatever the
 * tables hold, nothing outside the arrays' stated extents is read or written.
 *
 * Host form: HOST arrays throughout.  The base, the patch arrays and the item arrays go up once, the item outputs
 * and updates_each (optional, count entries) come down; there are no full outputs -- a host that wants every solved
 * matrix calls fwx_solve_batch_*.  Device memory comes from the pooled per-call context.  opts: device, stream /
 * use_stream and updates_out (the SUM of U) are honoured; a pivot range other than the whole one is FWX_ERR_INVALID,
 * an engine other than FWX_ENGINE_AUTO FWX_ERR_UNSUPPORTED.
 *
 * Statuses, all decided before any device call.  FWX_ERR_INVALID: count < 0 or n < 0; a bad dtype; base_rate NULL;
 * base_hops without base_next; patches->next, items->next_out or full->next without base_next; patches->hops,
 * items->hops_out or full->hops without base_hops; a negative total; a NULL ptr, index, rate, src, dst or rate_out
 * with total > 0; full->stride < n*n with a non-NULL full pointer; a bad struct_size.  Host form only, which can read
 * the tables: ptr[0] != 0, a descending ptr, ptr[count] != total, a patch index outside [0, n*n), an item src or dst
 * outside [0, n).  FWX_ERR_UNSUPPORTED: n > FWX_SWEEP_MAX_N.  count == 0 or n == 0: FWX_OK, nothing is touched.  Then
 * FWX_ERR_NO_DEVICE without a device, every output untouched.
 *
 * When it pays (MI355X, f64 + next + hops, two patches and four items a variant; profiles/r34_sweep.txt).  Host form
 * against numpy building the copies, fwx_solve_batch_f64 and indexing the answers: 15.2x at n = 128, count = 4096 (6.3
 * against 96.0 ms; 0.9 MB moved instead of 2 x 1.07 GB), 17.6x at n = 64, count = 4096, 11.7x / 7.6x at count = 256,
 * 10.6x at n = 16, count = 4096; at n = 4 and at n = 16, count = 256 1.2 ... 2.3x -- use whichever is at hand.  Device
 * form against fwx_dev_solve_batch on variants already materialised on the device: equal at n = 128 and at n = 64,
 * count = 256, 1.39x SLOWER at n = 64, count = 4096 and 1.7 ... 2x slower at n = 4 (3 us): a caller whose variants
 * already lie on the device gains nothing from it; it pays where the copies would have to be built or moved.       */
#define FWX_SWEEP_MAX_N FWX_BATCH_MAX_N
typedef struct fwx_sweep_patches {   /* variant b: entries [ptr[b], ptr[b+1]) */
    const int64_t *ptr;              /* count + 1, ptr[0] = 0, non-decreasing */
    int64_t total;                   /* = ptr[count]; entries in the arrays below */
    const int64_t *index;            /* i*n + j */
    const void *rate;                /* dtype */
    const int32_t *next, *hops;      /* optional: NULL = that field keeps the base's value */
} fwx_sweep_patches;
typedef struct fwx_sweep_items {     /* variant b: items [ptr[b], ptr[b+1]) */
    const int64_t *ptr;              /* count + 1, ptr[0] = 0, non-decreasing */
    int64_t total;                   /* = ptr[count] */
    const int32_t *src, *dst;
    void *rate_out;                  /* dtype, total entries */
    int32_t *next_out, *hops_out;    /* optional */
} fwx_sweep_items;
typedef struct fwx_sweep_full {      /* the solved variants whole, variant b at + b*stride */
    void *rate;                      /* dtype; optional like the two below */
    int32_t *next, *hops;
    int64_t stride;                  /* elements, >= n*n */
} fwx_sweep_full;
int fwx_dev_solve_sweep(int32_t count, int32_t n, int32_t dtype, const void *base_rate, const int32_t *base_next,
                        const int32_t *base_hops, const fwx_sweep_patches *patches, const fwx_sweep_items *items,
                        const fwx_sweep_full *full, unsigned long long *d_updates_each, void *stream);
int fwx_solve_sweep_f64(int32_t count, int32_t n, const double *base_rate, const int32_t *base_next,
                        const int32_t *base_hops, const fwx_sweep_patches *patches, const fwx_sweep_items *items,
                        uint64_t *updates_each, const fwx_opts *opts);
int fwx_solve_sweep_f32(int32_t count, int32_t n, const float *base_rate, const int32_t *base_next,
                        const int32_t *base_hops, const fwx_sweep_patches *patches, const fwx_sweep_items *items,
                        uint64_t *updates_each, const fwx_opts *opts);

/* ---- what-if sweeps up to order FWX_SWEEP_MID_MAX_N (256): variants built in per-workgroup slots -----------------
 * The sweep above builds a variant in the registers and LDS of the two small batch tiers and stops at n = 128; the
 * market of 20 exchanges x 12 currencies (240 vertices) needs the mid tier, whose matrix is resident in GLOBAL memory.
 * Here a fixed number of workgroups (`slots`) is launched, each owning one workspace slot of n*n entries per field:
 * a workgroup walks the variants b = s, s + slots, ... and per variant copies the base into its slot, applies the
 * patches, runs the mid tier's solve on the slot, answers the items from it and goes on.  Device memory is slots x n*n
 * entries per field whatever `count` is (materialised copies for fwx_dev_solve_batch_mid: count x n*n), the base stays
 * in L2, and nothing but the queried entries comes back.
 *
 * The contract is that of fwx_dev_solve_sweep / fwx_solve_sweep_*, word for word, with the limit at
 * FWX_SWEEP_MID_MAX_N: the same structs, the same clamping of the tables in the device form, the same table checks in
 * the host form, the same statuses in the same order (FWX_ERR_UNSUPPORTED: n > FWX_SWEEP_MID_MAX_N; the entry points
 * above keep refusing n > FWX_SWEEP_MAX_N), every output bit for bit what fwx_solve_batch_mid_* returns for M_b.
 * Whole pivot range only, no path trace.  Routing by FWX_BATCH_MID_MIN_N as fwx_solve_batch_mid_*: orders below it are
 * forwarded to fwx_dev_solve_sweep / the path of fwx_solve_sweep_* (scratch is ignored and may be NULL), orders from it
 * up run the slots.  No result bit depends on the routing or on the number of slots.
 *
 * scratch (device form): device memory, 16-byte aligned, at least FWX_SWEEP_MID_SCRATCH_BYTES(n) -- one slot, an upper
 * bound for every dtype and field set: the rates, then next, then hops, each n*n elements at pitch n.  The call
 * launches slots = min(count, scratch_bytes / FWX_SWEEP_MID_SCRATCH_BYTES(n), FWX_SWEEP_MID_SLOTS) workgroups and
 * touches nothing past slots x FWX_SWEEP_MID_SCRATCH_BYTES(n) bytes of it.  FWX_SWEEP_MID_SLOTS: environment, read
 * once per call, digits only, >= 1, anything else means the default of 512 -- two 1024-thread workgroups on each of
 * the 256 CUs, the most that can be resident (f64 + next + hops holds 133 KB of LDS and fits one per CU: 256 slots
 * fill the chip there); more slots than can be resident queue, nothing waits on another workgroup.  Scratch that is
 * NULL, misaligned or smaller than one slot is FWX_ERR_INVALID -- only where n is routed to the slots and count > 0 and
 * n > 0; decided after the statuses above and before any device call.  The device form allocates nothing and
 * synchronises nothing; the scratch must stay alive until the stream has run the call and may then hold anything.
 * The host form takes its slots from the pooled per-call context, as many as fit under 256 MiB, capped by the rule
 * above.
 *
 * When it pays (MI355X, f64 + next + hops, two patches and four items a variant; profiles/r35_sweep_mid.txt).  Host
 * form against numpy building the copies, fwx_solve_batch_mid_f64 and indexing the answers: 13.6x at n = 256, count =
 * 2048 (14.3 against 195.2 ms; 1.4 MB moved instead of 2 x 2.15 GB), 14.8x at n = 192, 13.9x at n = 129; 12.3 ... 13.5x
 * at count = 256.  Device form against fwx_dev_solve_batch_mid on variants already materialised on the device: 1.06 ...
 * 1.15x SLOWER (one more read and one more write of the matrix per variant), in a quarter of the device memory at
 * count = 2048 and less with every further variant: it pays where the copies would have to be built, moved or held. */
#define FWX_SWEEP_MID_MAX_N FWX_BATCH_MID_MAX_N
#define FWX_SWEEP_MID_SCRATCH_BYTES(n) ((size_t)(n) * (n) * 16)
int fwx_dev_solve_sweep_mid(int32_t count, int32_t n, int32_t dtype, const void *base_rate, const int32_t *base_next,
                            const int32_t *base_hops, const fwx_sweep_patches *patches, const fwx_sweep_items *items,
                            const fwx_sweep_full *full, unsigned long long *d_updates_each, void *scratch,
                            size_t scratch_bytes, void *stream);
int fwx_solve_sweep_mid_f64(int32_t count, int32_t n, const double *base_rate, const int32_t *base_next,
                            const int32_t *base_hops, const fwx_sweep_patches *patches, const fwx_sweep_items *items,
                            uint64_t *updates_each, const fwx_opts *opts);
int fwx_solve_sweep_mid_f32(int32_t count, int32_t n, const float *base_rate, const int32_t *base_next,
                            const int32_t *base_hops, const fwx_sweep_patches *patches, const fwx_sweep_items *items,
                            uint64_t *updates_each, const fwx_opts *opts);
/* TEST HOOK: the grid (= the slots) a fwx_dev_solve_sweep_mid call of `count` variants of order n with this much
 * scratch would launch right now: min(count, scratch_bytes / FWX_SWEEP_MID_SCRATCH_BYTES(n), FWX_SWEEP_MID_SLOTS);
 * 0 where count or n is 0; FWX_ERR_INVALID for a negative count or n, FWX_ERR_UNSUPPORTED for n >
 * FWX_SWEEP_MID_MAX_N.  Needs no device.  Not for production use. */
int fwx_test_sweep_mid_slots(int32_t count, int32_t n, size_t scratch_bytes);

/* Index form of the `_path` list that optimum returns (Algorithms.hs:74-75): follow next-hops
 * from src until dst.  Returns the number of vertices written to out (dst included, src not), 0 if
 * next[src][dst] == -1 (empty path, "no exchange"), or a negative fwx_status.  Host arrays.      */
int fwx_follow_path(int32_t n, const int32_t *next, int32_t src, int32_t dst, int32_t *out,
                    int32_t cap);

/* ---- device-resident handle: keeps the solved matrix in HBM across queries --------------------
 * Host counterpart of `InSync exRates matrix` (Types.hs:35-37): upload once per rate change,
 * solve once, then answer any number of (src,dst) queries without re-solving.                   */
typedef struct fwx_matrix fwx_matrix;

int fwx_matrix_create(fwx_matrix **out, int32_t n, int32_t dtype, int32_t with_next,
                      int32_t with_hops, int32_t device);
/* upload: rate / next / hops may be HOST or DEVICE arrays (hipMemcpyDefault); download likewise. */
int fwx_matrix_upload(fwx_matrix *m, const void *rate, const int32_t *next, const int32_t *hops);
int fwx_matrix_solve(fwx_matrix *m, const fwx_opts *opts);
int fwx_matrix_download(fwx_matrix *m, void *rate, int32_t *next, int32_t *hops);
/* One entry + its path, read back from the device (8 + 4*len bytes instead of the matrix).      */
int fwx_matrix_query(fwx_matrix *m, int32_t src, int32_t dst, double *rate_out, int32_t *path_out,
                     int32_t cap);
int fwx_matrix_destroy(fwx_matrix *m);

/* Incremental re-marshalling (SURVEY.md section 8f, row f3 -- the exact part of it).  The reference
 * rebuilds and re-solves the whole matrix after every accepted rate update
 * (ProcessRequests.hs:82-85, :99-102), although such an update changes TWO entries of
 * buildMatrix's output.  With the input KEPT on the device (one more copy of each array), the host
 * sends only the changed entries: fwx_matrix_patch_input replaces `count` entries of the kept input
 * (index[q] = i*n + j; rate_vals in the handle's dtype; next_vals / hops_vals may be NULL =
 * unchanged) and makes the patched input the handle's unsolved matrix again (device-to-device
 * restore), ready for fwx_matrix_solve -- a FULL solve, so every result stays bit-identical to the
 * reference; what is saved is buildMatrix over n^2 entries and the PCIe upload.
 * keep_input: call once after create (before or after an upload).  patch_input needs a kept
 * upload (FWX_ERR_INVALID otherwise); count <= FWX_MAX_PATCH.  Works on partitioned handles.     */
#define FWX_MAX_PATCH 4096
int fwx_matrix_keep_input(fwx_matrix *m);
int fwx_matrix_patch_input(fwx_matrix *m, int32_t count, const int64_t *index, const void *rate_vals,
                           const int32_t *next_vals, const int32_t *hops_vals);

/* Resume instead of re-solve (row f3, exactly).  An input entry (i,j) is an OPERAND of runAlgo only in
 * steps i and j (Algorithms.hs:58-60: step k reads r[i][k] and r[k][j]), so changing entries cannot
 * influence any OTHER entry before step m = the smallest index among them: up to there the old solve
 * and the new one differ in the changed entries alone.  A resumable handle therefore keeps, from its
 * last solve, (a) the state (rate, next, hops, path trace) at a few CHECKPOINT pivots and (b) the
 * time-k snapshots of every pivot row and column -- the panels the fused engine produces anyway.
 * fwx_matrix_resolve(changed entries) restores the last checkpoint c <= m, replays just the changed
 * entries through pivots [0, c) from the stored panels (their operands there are unchanged entries),
 * and runs pivots [c, n) only.  Every operand, product and compare is the one a from-scratch solve
 * performs: results are bit-identical (rates, next, hops, exact `_path` lists); the saving is c / n of
 * the solve.  The checkpoints and panels are refreshed as the resumed solve passes them.
 *
 * enable_resume: after create, enable_path_log (if the trace is wanted: afterwards it is refused) and
 *   keep_input, before the upload whose solve is to be resumable; `checkpoints` in 1..FWX_MAX_CHECKPOINTS, spread evenly over the pivots on multiples
 *   of 64; returns the number placed (n < 128 leaves room for none: 0), or FWX_ERR_UNSUPPORTED where
 *   AUTO does not take the fused engine (n <= 64).  Any other n works (the handle pads its rows), on one
 *   device and on partitioned handles alike -- there every partition keeps the checkpoints of its slab, its
 *   own part of the pivot-column snapshots and ALL pivot rows (it receives them anyway), a changed entry is
 *   replayed on the partition that owns its row, and a checkpoint must be a block start: with partitions
 *   that do not start on a multiple of 64 fewer are placed.  Memory: one copy of every array per checkpoint
 *   + ~2.5 more for the panels (fwx_matrix_resume_bytes gives the figure).
 * resolve: fwx_matrix_patch_input + fwx_matrix_solve in one call, resuming where it can.  Falls back
 *   to exactly that pair (a full solve from the patched kept input, which records afresh) when there
 *   is nothing to resume from: no checkpoint at or below m, the previous solve did not record (other
 *   engine, input outside the reference's domain, a pivot range), a patch value outside the domain,
 *   or opts asking for U, a stream, a pivot range or the per-k engine.  *resumed_from (optional)
 *   receives the pivot the solve started at (0 = full solve).                                       */
#define FWX_MAX_CHECKPOINTS 16
int fwx_matrix_enable_resume(fwx_matrix *m, int32_t checkpoints);
/* What enable_resume(checkpoints) would allocate on the device(s) for this handle, in bytes (call it
 * after enable_path_log, like enable_resume itself), and the free / total memory of a device
 * (hipMemGetInfo; device -1 = the caller's current one): a host sizes its checkpoint count with these
 * -- the Session mirror keeps the resume memory below half of what is free and carries on WITHOUT
 * resuming when even one checkpoint does not fit or the allocation fails.                          */
int fwx_matrix_resume_bytes(const fwx_matrix *m, int32_t checkpoints, uint64_t *bytes_out);
int fwx_device_memory(int32_t device, uint64_t *free_bytes, uint64_t *total_bytes);
int fwx_matrix_resolve(fwx_matrix *m, int32_t count, const int64_t *index, const void *rate_vals,
                       const int32_t *next_vals, const int32_t *hops_vals, const fwx_opts *opts,
                       int32_t *resumed_from);

/* Exact `_path` lists.  Following next-hops (fwx_matrix_query) yields A best path; the reference
 * keeps, per entry, the list it concatenated when the entry was last improved
 * (`_path = ikPath ++ kjPath`, Algorithms.hs:55), and under exact ties (its built-in 1.0 edges
 * between the same currency on two exchanges make them common) that list can be a different,
 * longer route of equal rate.  With the PATH TRACE enabled the solve keeps three more n x n int32
 * matrices on the device -- for every entry the pivot of its newest successful relaxation, at the
 * end of the solve, at the start of the step named by its column index and at the start of the
 * step named by its row index -- from which fwx_matrix_query_exact rebuilds the reference's list
 * exactly: path(i,j) = path_q(i,q) ++ path_q(q,j) with q the newest pivot of (i,j), and a
 * sub-entry is only ever needed "as of the step named by one of its own indices".  No lists, no
 * update records, one pass; any n.  Enable after create; needs the next-hop matrix; every engine
 * keeps it (engine choice as for any matrix); whole pivot range only, and the solve starts from an
 * uploaded input (fwx_matrix_solve on an already solved traced matrix: FWX_ERR_INVALID).
 * query_exact before a completed traced solve of the current upload: FWX_ERR_INVALID.
 * fwx_matrix_path_log_count: U of that solve if it was asked to count (fwx_opts.updates_out),
 * else 0.  path_out receives the vertices after src up to dst; returns the length.
 * Capacity, for every input (inside the domain or not): a list of L entries is returned whenever
 * cap >= L, and FWX_ERR_CAPACITY exactly when L > cap -- cap bounds the list and nothing else.  The
 * walk's own stack is sized by n (its depth is at most n: the pivots along a descent of the
 * concatenation tree strictly decrease), so a list whose tree has halves that contribute nothing (an
 * empty ikPath, a leaf without an edge: possible only outside the domain) needs no more cap than its
 * length.  An empty list (length 0) fits any cap >= 1.                                            */
int fwx_matrix_enable_path_log(fwx_matrix *m);
int fwx_matrix_path_log_count(fwx_matrix *m, uint64_t *count_out);
int fwx_matrix_query_exact(fwx_matrix *m, int32_t src, int32_t dst, double *rate_out,
                           int32_t *path_out, int32_t cap);
/* Batch form: count (src, dst) pairs in one launch (one thread per pair).  len_out[q] = length of
 * list q or a negative fwx_status (FWX_ERR_CAPACITY: list q is longer than cap, the rule above, item
 * by item: the other items of the batch are answered); path_out + q*cap receives it.  Host arrays in
 * and out.  Device scratch: cap + 3 (n + 2) int32 per pair.                                        */
int fwx_matrix_query_exact_batch(fwx_matrix *m, int32_t count, const int32_t *src, const int32_t *dst,
                                 int32_t *len_out, int32_t *path_out, int32_t cap);

/* ---- row-partitioned solve behind the same call: ONE process, several devices ------------------
 * The reference has one call site, ProcessRequests.hs:82-84 -> floydWarshall (Algorithms.hs:19-20);
 * a host bound to that one call gets the whole node through these entry points.  The matrix is cut
 * into n_parts contiguous row blocks (partition p holds rows [n*p/P, n*(p+1)/P) of rate / next and
 * of the path trace -- the bounds rounded down to multiples of 64 for n >= 128 P, fwx_matrix_part_rows); step k needs, besides local values, only pivot row k AS IT STANDS AT THE
 * START OF STEP k, so pivots travel FWX_FUSED_BLOCK at a time as one snapshot panel per block,
 * produced by the partition that owns those rows and sent to all others, with look-ahead (the
 * owner of the next block relaxes those rows first and runs their panel + the exchange on a side
 * stream while every partition sweeps the rest of its slab).  No operand and no order changes:
 * results are bit-identical to the single-device solve and to the reference loop.
 *
 * devices[p] = HIP ordinal of partition p (-1 = the caller's current device).  A device may be listed MORE THAN ONCE (logical
 * partitions on one GPU: how the partitioned schedule is tested where only one GPU exists).
 * exchange:
 *   FWX_XCHG_RCCL  ncclBroadcast of each panel on RCCL (ncclCommInitAll over the devices, one
 *                  communicator per partition, calls grouped; librccl.so.1 is loaded on first use,
 *                  libfwx does not link it).  Needs pairwise distinct devices.  On this pool RCCL needs
 *                  HSA_ENABLE_IPC_MODE_LEGACY=0 in the environment BEFORE the first HIP call of the
 *                  process (the host driver only supports dmabuf IPC; otherwise ncclCommInitAll fails
 *                  in hipIpcGetMemHandle and create_multi returns FWX_ERR_RCCL): a host exports it or
 *                  falls back to FWX_XCHG_PEER, which needs no IPC inside one process.
 *   FWX_XCHG_PEER  hipMemcpyPeerAsync from the owner's panel into every other partition's panel
 *                  buffer (plain device-to-device copies when the device is the same).
 *   FWX_XCHG_AUTO  RCCL when there are >= 2 partitions on pairwise distinct devices, else PEER.
 * Distinct devices get peer access enabled pairwise where the hardware allows; it is needed by the
 * QUERIES only (they walk the slabs from one device: without it fwx_matrix_query walks from the host
 * and query_exact[_batch] returns FWX_ERR_UNSUPPORTED), never by the exchange.
 *
 * A multi handle is an fwx_matrix: upload / solve / download / query / enable_path_log /
 * query_exact[_batch] / path_log_count / destroy work on it unchanged (pivot ranges as on one device:
 * any [k_begin, k_end) without the path trace, the whole range with it;
 * fwx_opts.engine AUTO / FUSED, or PERK = one launch per pivot and partition with the pivot rows
 * read from the exchanged panel -- rate / next / hops, no path trace; fwx_opts.device / stream are
 * ignored).  Any n: rows are padded on
 * the device to a multiple of 16 bytes.  rate, next, hops and the path trace are all carried
 * through the slabs (the hops of the pivot rows travel with their rates).  Not carried: matrices
 * outside the reference's domain WITH next-hops (see "Domain": the slab kernels take next[i][k];
 * such a matrix returns FWX_ERR_UNSUPPORTED from solve and is solved on one device by
 * fwx_solve_* / fwx_matrix_create).                                                               */
#define FWX_XCHG_AUTO 0
#define FWX_XCHG_PEER 1
#define FWX_XCHG_RCCL 2
#define FWX_XCHG_CALLBACK 3   /* fwx_matrix_create_part only */
#define FWX_MAX_PARTS 32
int fwx_matrix_create_multi(fwx_matrix **out, int32_t n, int32_t dtype, int32_t with_next,
                            int32_t with_hops, int32_t n_parts, const int32_t *devices,
                            int32_t exchange);
/* ---- the same partitioned solve, ONE PARTITION PER PROCESS (one process per GPU) -----------------
 * fwx_matrix_create_part builds the handle of partition `rank` of `world` row blocks: only that slab
 * lives in this process, and the one exchange of the algorithm -- the 64-pivot snapshot panel, from the
 * rank that owns those rows to every other -- is the host's: `exchange` is called on the solving thread
 * once per panel, in the same order on every rank, and must make `w` (count elements of the handle's
 * dtype) and, if not NULL, `wh` (count int32: the hops of the pivot rows) hold rank `owner`'s copy ON
 * EVERY RANK, ordered on `stream` (a hipStream_t: enqueue a broadcast on it -- RCCL, or MPI with the
 * stream synchronised around it; floydwarshall_amd/dist.py uses torch.distributed).  Return 0, or non-zero
 * to fail the solve (FWX_ERR_RCCL).  Everything else is the code the one-process handle runs -- same
 * schedules (single pass, the 128-pivot pair schedule, the per-k engine), same kernels, path trace, kept
 * input, resume -- and so the same bits.  What differs for the caller:
 *   upload / download  take THIS RANK'S row block (fwx_matrix_part_rows(m, rank, &row0, &rows)): rows x n
 *   the domain check   is per slab; the host combines the ranks' answers: fwx_matrix_domain_bits (local
 *                      bits: 1 = every rate >= +0 and not NaN, 2 = no positive rate without a path), an
 *                      all-reduce AND among the ranks, fwx_matrix_set_domain -- before the first solve of
 *                      every upload (a solve without it: FWX_ERR_INVALID)
 *   updates_out        receives this rank's share of U
 *   patch / resolve    take the caller's n x n entry indices on every rank; each rank applies its rows'
 *   queries            walk other ranks' slabs: FWX_ERR_UNSUPPORTED (download the slab instead)
 * Every rank must issue the same calls with the same options (the schedule is a function of n, world,
 * the options and the FWX_* environment), or the exchanges do not pair up.                           */
typedef int (*fwx_exchange_fn)(void *ctx, int32_t k0, int32_t bt, int32_t owner, void *w, int32_t *wh,
                               int64_t count, void *stream);
int fwx_matrix_create_part(fwx_matrix **out, int32_t n, int32_t dtype, int32_t with_next, int32_t with_hops,
                           int32_t rank, int32_t world, int32_t device, fwx_exchange_fn exchange, void *ctx);
int fwx_matrix_domain_bits(fwx_matrix *m, int32_t *bits_out);
int fwx_matrix_set_domain(fwx_matrix *m, int32_t bits);

/* Per-step timings of the last solve of a partitioned handle, from HIP events on the streams the work
 * ran on (a diagnostic: each span costs two event records; off by default).  A step is one block of 64
 * pivots, or a PAIR of blocks where the solve ran two passes per main launch (pivots_per_step = 128).
 *   bulk_us       what a step costs when nothing else limits it: the slab sweep (column panel + main
 *                 kernel / the 64 per-k launches) on a partition's main stream -- mean over steps of the
 *                 MAX over partitions; bulk_mean_us: the plain mean
 *   lookahead_us  the owner bringing the next block's rows up to date (single pass; main stream)
 *   panel_us      the owner's snapshot panel kernel (side stream)
 *   exchange_us   the panel's way to the other partitions: peer copy on each receiver / the RCCL
 *                 broadcast call on every partition's side stream -- mean over steps of the max
 *   chain_us      everything the NEXT step waits for besides the sweep.  Single pass: lookahead + panel
 *                 + exchange.  Double pass: measured whole on each partition's side stream, from the end
 *                 of the previous main launch to the last column panel of the next pair (cross launches,
 *                 both panels, both exchanges) -- mean over steps of the max over partitions
 *   chain_over_bulk > 1: the solve is bound by the panel chain, not by the sweep */
typedef struct fwx_multi_timing {
    uint32_t struct_size;
    int32_t steps, pivots_per_step, partitions;
    float bulk_us, bulk_mean_us, lookahead_us, panel_us, exchange_us, chain_us, chain_over_bulk;
} fwx_multi_timing;
int fwx_matrix_set_timing(fwx_matrix *m, int32_t on);      /* FWX_ERR_UNSUPPORTED on a single-device handle */
int fwx_matrix_get_timing(const fwx_matrix *m, fwx_multi_timing *out);   /* out->struct_size = sizeof(*out) */
/* Rows partition `part` holds: [*row0_out, *row0_out + *rows_out).  Balanced row blocks, n * p / P, rounded
 * down to a multiple of 64 once every partition holds two pivot blocks (n >= 128 P): blocks of 64 pivots never
 * straddle two partitions, so aligned partitions make every block full and aligned for ANY n, which is what
 * the 128-pivot pair schedule and the checkpoints of resumable solves need.  A host that feeds slabs
 * (fwx_matrix_create_part) asks here instead of computing the bounds itself.                        */
int fwx_matrix_part_rows(const fwx_matrix *m, int32_t part, int32_t *row0_out, int32_t *rows_out);
/* Partitions of a handle (1 for a single-device handle); exchange_out (optional) receives the
 * transport in use (FWX_XCHG_PEER / FWX_XCHG_RCCL).                                              */
int fwx_matrix_parts(const fwx_matrix *m, int32_t *exchange_out);
/* Ranks of the RCCL communicator the handle exchanges panels on (ncclCommCount), 0 when the
 * exchange is not RCCL (single device, FWX_XCHG_PEER).                                            */
int fwx_matrix_comm_ranks(const fwx_matrix *m);
/* One-shot host-buffer form, same contract as fwx_solve_f64 / _f32 (in place, caller owns the
 * arrays): create_multi + upload + solve + download.  Like the per-call contexts of fwx_solve_*,
 * the handle (slabs, streams, events, RCCL communicator) is parked in a process-wide pool keyed by
 * (n, dtype, fields, device list, exchange) and reused by the next call with the same key; handles
 * whose rate slabs exceed 256 MiB in total are destroyed on return.  opts: engine and updates_out are honoured.     */
int fwx_solve_multi_f64(int32_t n, double *rate, int32_t *next, int32_t *hops, int32_t n_parts,
                        const int32_t *devices, int32_t exchange, const fwx_opts *opts);
int fwx_solve_multi_f32(int32_t n, float *rate, int32_t *next, int32_t *hops, int32_t n_parts,
                        const int32_t *devices, int32_t exchange, const fwx_opts *opts);

/* ---- device-pointer step API (caller-owned DEVICE memory, caller's stream) --------------------
 * Used by the benchmark and by the row-partitioned multi-GPU driver, which own their buffers
 * through torch / torch.distributed.  All launches are asynchronous on `stream` (a hipStream_t,
 * NULL = default stream); nothing is synchronised.                                              */

/* `rows` consecutive rows [row0, row0+rows) of the global n x n matrix, rows*n elements each. */
typedef struct fwx_slab {
    int32_t n;       /* order of the global matrix = row length                                   */
    int32_t row0;    /* global index of the slab's first row                                      */
    int32_t rows;    /* rows held in this slab                                                    */
    int32_t dtype;   /* fwx_dtype                                                                 */
    void *rate;      /* device, rows*n                                                            */
    int32_t *next;   /* device, rows*n, or NULL                                                   */
    int32_t *hops;   /* device, rows*n, or NULL                                                   */
} fwx_slab;

/* Pivot rows for steps [k_begin, k_end): row k AS IT STANDS AT THE START OF STEP k is at
 * rate + (k - k_begin) * stride (elements).  For a single-GPU solve this is the matrix itself
 * (rate = matrix + k_begin*n, stride = n: row k is not modified by step k).  For a partitioned
 * solve it is the panel of time-k snapshots produced by fwx_dev_panel on the owner.             */
typedef struct fwx_pivots {
    int32_t k_begin;
    int32_t k_end;
    const void *rate;
    const int32_t *hops; /* same layout; required iff slab.hops != NULL                            */
    int64_t stride;
    const int32_t *next; /* same layout, optional: next-hop rows of the pivots at time k.  Given, an  */
                         /* update whose ikPath is empty (next[i][k] < 0) takes next[k][j], as the    */
                         /* reference's list concatenation does; NULL = the caller vouches for the    */
                         /* domain (see "Domain"), where that case cannot arise                        */
} fwx_pivots;

/* Apply pivots [k_begin,k_end) in order to every row of the slab, asynchronously on `stream`.
 * In general one launch per pivot, each reading the slab once.  A rates-only call (no next, no hops) on
 * the WHOLE matrix in place -- row0 = 0, rows = n, the pivots its own rows (piv->rate = rate +
 * k_begin*n, stride n), n a multiple of 16 bytes of elements, rate 16-byte aligned, no skip range --
 * applies FWX_PERK_PIVOTS pivots per launch instead (environment, 1 | 2 | 4 | 8, read per call, default
 * 8; 1 = one launch per pivot): per block of 64 pivots one panel launch takes the time-k snapshots of
 * the block's rows and columns, then every launch folds 2, 4 or 8 neighbouring pivots from those
 * snapshots into each entry it streams, so the matrix is read once per launch, not once per pivot.
 * At the width 8 an f32 call without d_updates folds 16 pivots per launch wherever two 8-pivot launches of one
 * block would follow each other (FWX_PERK_WIDE, environment, read per call: `0` turns that off, anything else, or
 * unset, leaves it on; FWX_PERK_PIVOTS itself takes 1 | 2 | 4 | 8 only, and a counted or f64 call stays 8 wide).
 * The result is bit for bit the same.  FWX_PERK_FOLD (environment, read per call): `compare` makes every
 * such f32 launch fold with a compare and a select per pivot, as every counting and every f64 launch does;
 * anything else, or unset, is automatic -- a wave whose loaded pivot operands are all NaN or sign-clear takes
 * the maximum of its candidates first and compares once, which gives the same bits for every entry.  For
 * tests and A/B runs; no result bit depends on it.  The snapshots live in library-owned device scratch on the stream's
 * device, one buffer of 128 * n elements per stream (at most 16 are kept, the least recently used that no call still
 * inside the library holds goes; with more than 16 callers inside at once the pool grows for the moment):
 * the FIRST such call on a stream calls hipMalloc, and a call with a larger n than the stream has seen
 * waits for the stream before it frees and allocates again -- so such a call cannot be captured into a
 * graph; set FWX_PERK_PIVOTS=1 for that.  Every later call allocates nothing, synchronises nothing and
 * returns with its launches queued.
 * d_updates: optional device array of FWX_UPDATE_SHARDS uint64 counters, incremented by U.      */
#define FWX_UPDATE_SHARDS 256
int fwx_dev_relax(const fwx_slab *slab, const fwx_pivots *piv, int32_t serpentine,
                  unsigned long long *d_updates, void *stream);
/* Same, leaving the slab rows [skip_lo, skip_hi) (relative to the slab, multiples of 4) alone: the
 * rows of the NEXT pivot panel, which a look-ahead step has already relaxed -- one launch per
 * pivot instead of one above and one below those rows.                                          */
int fwx_dev_relax_skip(const fwx_slab *slab, const fwx_pivots *piv, int32_t serpentine,
                       unsigned long long *d_updates, int32_t skip_lo, int32_t skip_hi, void *stream);

/* Owner-side panel phase for a partitioned solve.  `block` holds the pivot rows
 * [block->row0, block->row0 + block->rows) at time k = block->row0.  Evolves them in place through
 * those pivots and writes the time-k snapshot of each pivot row to w_rate (rows x n) (and its hops
 * row to w_hops if the slab carries hops).  Afterwards the block rows are at time row0+rows and
 * every other row of the matrix must be relaxed with fwx_dev_relax(pivots = w_rate).  Inside the
 * block the list rule holds in full, outside the domain too: an update with an empty ikPath takes
 * next[k][j] from the block's own row k, which step k leaves alone.                              */
int fwx_dev_panel(const fwx_slab *block, void *w_rate, int32_t *w_hops,
                  unsigned long long *d_updates, void *stream);

/* Whole solve on caller-owned DEVICE memory: `full` must hold the entire matrix (row0 = 0,
 * rows = n).  Same engines and options as fwx_matrix_solve (opts->device is ignored: the memory
 * decides); scratch is allocated and released internally; BLOCKING (returns after the solve has
 * completed on the device).  The fused engine overlaps each snapshot panel with the previous
 * pass on an internal side stream (look-ahead).                                                 */
int fwx_dev_solve(const fwx_slab *full, const fwx_opts *opts);

/* Batch form of `optimum`'s path reconstruction (Algorithms.hs:74-75) on the device: for each
 * pair q, walk next-hops from src[q] until dst[q].  All pointers are DEVICE pointers; `next` is
 * the full n x n matrix.  len_out[q] = path length (0 = no route, FWX_ERR_CYCLE if dst is not
 * reached within n hops).  Optional outputs (NULL to skip): prod_out[q] = product, accumulated in
 * double left to right, of edge_rate[u][v] along the path (edge_rate = the UNSOLVED input matrix,
 * dtype given) -- the solved rate must equal it up to rounding; path_out + q*cap receives up to
 * cap vertices (longer paths are truncated there but still walked and counted).                */
int fwx_dev_follow_paths(int32_t n, const int32_t *next, int32_t count, const int32_t *src,
                         const int32_t *dst, int32_t *len_out, const void *edge_rate,
                         int32_t dtype, double *prod_out, int32_t *path_out, int32_t cap,
                         void *stream);

/* ---- fused engine (FWX_FUSED_BLOCK pivots per pass; bit-identical to the per-k engine) --------
 * fwx_dev_panel_snap: snapshot panel of the pivot rows in `block` (rows [row0,row0+rows), rows <=
 *   FWX_FUSED_BLOCK, at time row0): writes the time-k snapshot of each pivot row to w_rate
 *   (rows x n) and, if the block carries hops, of its hops row to w_hops.  UNLIKE fwx_dev_panel THE
 *   MATRIX IS NOT MODIFIED: the pivot rows are then relaxed like any other row.  trace (optional):
 *   the path trace OF THE SAME ROWS (views of rows [row0, row0+rows) of the trace arrays); its
 *   at_row rows are written.
 * fwx_dev_relax_fused: applies the pivots [piv->k_begin, piv->k_end) (at most FWX_FUSED_BLOCK,
 *   piv->rate = snapshot panel, piv->hops = hops panel, stride n) to EVERY row of the slab in one
 *   pass.  scratch: device scratch of FWX_FUSED_BLOCK * ((slab->rows + 3) & ~3) elements per array
 *   (col_next only if the slab carries next, col_hops only if it carries hops).  trace
 *   (optional): the slab's path trace, rows x n like rate / next (LOCAL rows).  n must be a
 *   multiple of 16 bytes worth of elements.
 * The snapshot panel also feeds fwx_dev_relax (per-k engine), so fwx_dev_panel_snap +
 * fwx_dev_relax over all rows is a valid (slower) combination.
 *
 * flags: FWX_FLAG_NONNEG = the caller has verified (fwx_dev_check_nonneg on EVERY slab of the
 *   matrix, all ranks) that every entry is >= +0.0 and not NaN -- what the reference's parser
 *   guarantees (rates > 0, Parsers.hs:40; "no route" = +0.0) -- and, if next is carried, that no
 *   non-zero rate lacks a path (both bits).  On that domain the strict fold equals max() bit for
 *   bit, and f32 slabs take the kernels that fold two pivots per v_max3_f32 (rates only, or
 *   rates + next + trace + hops through the arg re-scan).  Without the flag nothing is assumed
 *   about the rates.
 *   A slab WITH next must be inside the domain in any case (D1 and D2 on every slab): the fused
 *   kernels take next[i][k] as the head of the concatenated path.  The whole-matrix entry points
 *   check this themselves; here it is the caller's duty.                                        */
#define FWX_FUSED_BLOCK 64
#define FWX_FLAG_NONNEG 1
typedef struct fwx_trace {      /* path trace of a slab (or of a block of pivot rows): rows x n each */
    int32_t *last, *at_col, *at_row;
} fwx_trace;
typedef struct fwx_fused_scratch {
    void *col_rate;             /* pivot-column snapshots of the slab's rows                       */
    int32_t *col_next;          /* ... their next-hops (iff slab->next)                            */
    int32_t *col_hops;          /* ... their hops      (iff slab->hops)                            */
} fwx_fused_scratch;
int fwx_dev_panel_snap(const fwx_slab *block, void *w_rate, int32_t *w_hops, const fwx_trace *trace,
                       void *stream);
int fwx_dev_relax_fused(const fwx_slab *slab, const fwx_pivots *piv, const fwx_fused_scratch *scratch,
                        const fwx_trace *trace, unsigned long long *d_updates, int32_t flags,
                        void *stream);
/* Same, leaving the slab rows [skip_lo, skip_hi) (multiples of 8) to an earlier look-ahead step:
 * nothing of those rows is read or written -- rate, next, hops and their rows of the trace (at_col
 * included) stay as that step left them.                                                         */
int fwx_dev_relax_fused_skip(const fwx_slab *slab, const fwx_pivots *piv,
                             const fwx_fused_scratch *scratch, const fwx_trace *trace,
                             unsigned long long *d_updates, int32_t flags, int32_t skip_lo,
                             int32_t skip_hi, void *stream);
/* Domain check of one slab (see "Domain").  *d_flag is a device int32 the caller has set to 3 (or
 * to 1 for a rates-only slab): bit 0 is cleared if any rate of the slab is negative, -0.0 or NaN,
 * bit 1 if the slab carries next and some entry has a non-zero rate with next < 0.  A partitioned
 * solve ANDs the flags of all slabs.                                                            */
int fwx_dev_check_nonneg(const fwx_slab *slab, int32_t *d_flag, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FWX_H */
