// fwx_internal.h -- pieces shared by the translation units behind the C ABI (fwx_api.hip: one
// device; fwx_batch.hip: the batched solves; fwx_multi.hip: the row-partitioned multi-device handle; fwx_perk.hip:
// the per-k engine's host side, declared in fwx_perk.h).  Not installed, not part of the ABI.
#ifndef FWX_INTERNAL_H
#define FWX_INTERNAL_H

#include <hip/hip_runtime.h>
#include <mutex>
#include <new>
#include <vector>
#include <stddef.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>

#include "fwx.h"
#include "fwx_kernels.h"

static_assert(FWX_UPDATE_SHARDS == FWX_UPDATE_SHARDS_K, "shard count mismatch");

namespace fwxi {

inline thread_local int g_last_hip = 0;

#define FWX_HIP(call)                                                                              \
    do {                                                                                           \
        hipError_t e__ = (call);                                                                   \
        if (e__ != hipSuccess) {                                                                   \
            g_last_hip = (int)e__;                                                                 \
            (void)hipGetLastError();                                                               \
            return e__ == hipErrorOutOfMemory ? FWX_ERR_OOM : FWX_ERR_HIP;                         \
        }                                                                                          \
    } while (0)

inline int device_count()
{
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return c;
}

// The current device for the scope of one ABI call; the caller's is restored on the way out.  enter() is the
// checked form of the single-device entry points; set() is what the loops over a partitioned handle's slabs
// call.  Neither issues hipSetDevice for a device that is current already; set() asks the runtime what is
// current, so code that is not the library's (RCCL, the host's exchange callback) cannot leave it mistaken.
struct DeviceGuard {
    int prev = -1;
    bool changed = false;
    int enter(int device)
    {
        const int cnt = device_count();
        if (cnt <= 0) return FWX_ERR_NO_DEVICE;
        if (hipGetDevice(&prev) != hipSuccess) return FWX_ERR_HIP;
        if (device < 0) return FWX_OK;
        if (device >= cnt) return FWX_ERR_INVALID;
        if (device != prev) {
            FWX_HIP(hipSetDevice(device));
            changed = true;
        }
        return FWX_OK;
    }
    int set(int device)
    {
        int now = -1;
        FWX_HIP(hipGetDevice(&now));
        if (prev < 0) prev = now;
        if (device != now) {
            FWX_HIP(hipSetDevice(device));
            changed = true;
        }
        return FWX_OK;
    }
    void keep() { changed = false; }   // (a thread of the library's own: nothing to restore)
    ~DeviceGuard()
    {
        if (changed) (void)hipSetDevice(prev);
    }
};

struct Opts {
    int device = -1, engine = FWX_ENGINE_AUTO, k_begin = 0, k_end = 0, block = 0, serpentine = 1;
    uint64_t *updates_out = nullptr;
    hipStream_t stream = nullptr;      // caller's stream (fwx_opts.stream), nullptr = library-owned
    bool has_stream = false;
};

// The stream one blocking ABI call runs on: the caller's (fwx_opts.stream) or a non-blocking stream
// of its own -- never the legacy null stream, which would serialise the call against every other
// blocking stream of the process (torch's included) and against solves on other host threads.
// Bounds the number of launches in flight on a stream: every EVERY launches an event is recorded
// and the host waits for the event recorded 2*EVERY launches earlier.  The GPU never idles (at
// least EVERY launches are queued behind the one being waited for), but a solve of N = 16384
// pivots no longer parks 16384 dispatches in the queue: rocprofv3's counter collection, which
// intercepts every AQL packet, crashed on exactly that.
// Its events come from a process-wide pool per device and go back there, recorded or not: an event is
// never destroyed while a command may still reference it (round 3 waited for armed events in the
// destructor instead, which made the asynchronous entry points -- fwx_dev_relax with 256 or more pivots
// -- block the host until their last recorded event had completed; fwx.h promises "nothing is
// synchronised"), and a call creates no event once the pool is warm.  Re-recording a pooled event whose
// earlier record is still pending is legal HIP; a Throttle only ever waits for records it made itself.
class ThrottleEvents {
public:
    static hipEvent_t take(int dev)
    {
        Pool &p = pool();
        {
            std::lock_guard<std::mutex> lk(p.mu);
            if (dev >= 0 && dev < kMaxDev && !p.idle[dev].empty()) {
                hipEvent_t e = p.idle[dev].back();
                p.idle[dev].pop_back();
                return e;
            }
        }
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
            g_last_hip = (int)hipGetLastError();
            return nullptr;
        }
        return e;
    }
    static void give(int dev, hipEvent_t e)
    {
        if (!e) return;
        Pool &p = pool();
        std::lock_guard<std::mutex> lk(p.mu);
        if (dev >= 0 && dev < kMaxDev) p.idle[dev].push_back(e);     // (else: leaked, never destroyed pending)
    }

private:
    static constexpr int kMaxDev = 64;
    struct Pool { std::mutex mu; std::vector<hipEvent_t> idle[kMaxDev]; };
    static Pool &pool() { static Pool *p = new Pool(); return *p; }   // leaked on purpose
};

struct Throttle {
    static constexpr int EVERY = 256;
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool armed[2] = {false, false};
    int count = 0, slot = 0, dev = -1;
    ~Throttle()
    {
        for (int i = 0; i < 2; ++i) ThrottleEvents::give(dev, ev[i]);
    }
    // the stream's device must be current
    int tick(hipStream_t s, int launches = 1)
    {
        count += launches;
        if (count < EVERY) return FWX_OK;
        count = 0;
        if (!ev[slot]) {
            if (dev < 0) FWX_HIP(hipGetDevice(&dev));
            if (!(ev[slot] = ThrottleEvents::take(dev))) return FWX_ERR_HIP;
        }
        if (armed[slot]) FWX_HIP(hipEventSynchronize(ev[slot]));
        FWX_HIP(hipEventRecord(ev[slot], s));
        armed[slot] = true;
        slot ^= 1;
        return FWX_OK;
    }
};

inline int read_opts(const fwx_opts *o, int n, Opts &out)
{
    if (o) {
        // v1 callers pass the struct up to and including updates_out; later fields are optional
        if (o->struct_size < offsetof(fwx_opts, stream)) return FWX_ERR_INVALID;
        out.device = o->device;
        out.engine = o->engine;
        out.k_begin = o->k_begin;
        out.k_end = o->k_end;
        out.block = o->block;
        out.serpentine = o->serpentine == 0 ? 1 : 0;
        out.updates_out = o->updates_out;
        if (o->struct_size >= offsetof(fwx_opts, use_stream) + sizeof(int32_t) && o->use_stream) {
            out.stream = (hipStream_t)o->stream;
            out.has_stream = true;
        }
    }
    if (out.k_end <= 0) out.k_end = n;
    if (out.k_begin < 0 || out.k_begin > out.k_end || out.k_end > n) return FWX_ERR_INVALID;
    if (out.engine != FWX_ENGINE_AUTO && out.engine != FWX_ENGINE_PERK &&
        out.engine != FWX_ENGINE_FUSED)
        return FWX_ERR_INVALID;
    return FWX_OK;
}

inline int sum_updates(unsigned long long *d_updates, uint64_t *out, hipStream_t s)
{
    unsigned long long h[FWX_UPDATE_SHARDS];
    FWX_HIP(hipMemcpyAsync(h, d_updates, sizeof(h), hipMemcpyDeviceToHost, s));
    FWX_HIP(hipStreamSynchronize(s));
    uint64_t u = 0;
    for (int i = 0; i < FWX_UPDATE_SHARDS; ++i) u += h[i];
    *out = u;
    return FWX_OK;
}

// Retire barrier.  hipStreamSynchronize returns when the awaited command's status is set; the HIP
// runtime's signal-handler thread may still be RETIRING that command (releasing its references to the
// memory objects behind the kernel's pointer arguments).  The handler retires the commands of a queue
// strictly in order, so one more trivial command on the stream, waited for, proves that everything
// before it has been retired; its own retirement only touches a buffer that is never freed.  libfwx
// runs this before it releases anything a stream's commands used (buffers, events, the stream).
//
// Why it exists: tools/fuzz_domain.py died with a SIGSEGV in that handler thread (round 2, only under
// the HIP runtime bundled with the torch wheel, ROCm 7.0, not the /opt/rocm 7.2 one libfwx is built
// against): amd::KernelParameters::release -> amd::ReferenceCountedObject::release on the memory
// object of a kernel's pointer argument (DESIGN.md section 7 has the disassembly-level record).  This
// barrier made the crash rarer but did NOT remove it under that runtime, so the cause is not proven
// to be a hipFree racing the handler; it is kept as lifetime hygiene, not as the fix.
inline void drain_stream(hipStream_t s)
{
    static std::mutex mu;
    static void *pad[64] = {nullptr};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return;
    void *p = nullptr;
    {
        std::lock_guard<std::mutex> lk(mu);
        if (!pad[dev] && hipMalloc(&pad[dev], 256) != hipSuccess) { (void)hipGetLastError(); pad[dev] = nullptr; }
        p = pad[dev];
    }
    if (s) (void)hipStreamSynchronize(s);
    if (p && s) {
        (void)hipMemsetAsync(p, 0, 4, s);
        (void)hipStreamSynchronize(s);
    }
}

struct SideStream {
    hipStream_t s = nullptr;
    hipEvent_t rows_done = nullptr, panel_done = nullptr, main_done = nullptr;
    ~SideStream()
    {
        if (main_done) (void)hipEventDestroy(main_done);
        if (rows_done) (void)hipEventDestroy(rows_done);
        if (panel_done) (void)hipEventDestroy(panel_done);
        if (s) (void)hipStreamDestroy(s);
    }
    void drain() { if (s) drain_stream(s); }
    int init()
    {
        FWX_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        FWX_HIP(hipEventCreateWithFlags(&rows_done, hipEventDisableTiming));
        FWX_HIP(hipEventCreateWithFlags(&panel_done, hipEventDisableTiming));
        FWX_HIP(hipEventCreateWithFlags(&main_done, hipEventDisableTiming));
        return FWX_OK;
    }
};

// What the three process-wide pools have done in this process (test hook fwx_test_pools, fwx.h): entries created,
// entries destroyed or evicted, and the most that were leased -- in a call -- at one time.  Relaxed host atomics.
struct PoolStats {
    std::atomic<uint64_t> created{0}, destroyed{0}, leased{0}, peak{0};
    void lease()
    {
        const uint64_t now = leased.fetch_add(1, std::memory_order_relaxed) + 1;
        uint64_t p = peak.load(std::memory_order_relaxed);
        while (p < now && !peak.compare_exchange_weak(p, now, std::memory_order_relaxed)) {}
    }
    void unlease() { leased.fetch_sub(1, std::memory_order_relaxed); }
};
enum { POOL_CTX, POOL_PERK, POOL_MULTI, POOL_COUNT };
inline PoolStats g_pool_stats[POOL_COUNT];
constexpr size_t kCtxPoolMaxFree = 8;          // CtxPool keeps this many idle contexts (POOL_PERK's: fwx_perk.h)
constexpr size_t kMultiPoolMaxIdle = 2;        // MultiPool (fwx_multi.hip) parks this many handles

// ------------------------------------------------------------------------------------------------
// Per-call context.  fwx_solve_f64 / _f32 / fwx_dev_solve are stateless for the caller, but what a
// call needs on the device -- a stream, the look-ahead stream and its events, device buffers for the
// caller's arrays, the fused engine's workspace -- is expensive to create and, above all, to
// release (hipFree and hipStreamDestroy synchronise the device): 5-12 ms per call whatever the
// matrix order, for a 4 x 4 solve that takes 20 us.  Contexts are therefore kept in a
// process-wide pool, one per concurrent call and device; a call takes one, grows its buffers if it
// must, and puts it back.  Buffers above kKeepBytes are released on the way back, so a one-off
// N = 16384 solve does not pin gigabytes; the pool itself is never torn down (no HIP calls from
// static destructors).
// ------------------------------------------------------------------------------------------------
struct CallCtx {
    enum { RATE, NEXT, HOPS, WS, SMALL, NBUF };            // SMALL: update shards + domain flag; in
                                                           // fwx_solve_batch_lists_*: next0, the trace, the walk's chunk;
                                                           // fwx_solve_batch_large_* / ragged_large: the scratch panels in
                                                           // front (up to 256 MiB); fwx_solve_sweep_mid_*: the workspace
                                                           // slots of the mid tier's sweep (up to 256 MiB)
    static constexpr size_t kKeepBytes = (size_t)256 << 20;
    int device = -1;
    hipStream_t s = nullptr;
    SideStream side;
    void *buf[NBUF] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t cap[NBUF] = {0, 0, 0, 0, 0};

    void *pin = nullptr;               // pinned host staging for small host <-> device transfers
    size_t pin_cap = 0;
    // solves whose arrays sum to more than this go straight from / to the caller's memory (measured,
    // fwx_solve_f64 + next + hops: staged wins up to n = 256 = 1 MiB, 0.92 against 1.04 ms, and loses
    // at n = 512 = 4 MiB, 2.07 against 1.91 ms; gpurun_out/r02_call_latency_staged.txt)
    static constexpr size_t kStageBytes = (size_t)3 << 19;
    int reserve_pinned(size_t bytes, void **out)
    {
        if (pin_cap < bytes) {
            if (pin) { drain(); (void)hipHostFree(pin); pin = nullptr; pin_cap = 0; }
            const size_t want = bytes < ((size_t)1 << 20) ? ((size_t)1 << 20) : bytes;
            FWX_HIP(hipHostMalloc(&pin, want, hipHostMallocDefault));
            pin_cap = want;
        }
        *out = pin;
        return FWX_OK;
    }
    // Streams that are not the context's own but ran commands on its buffers during the current
    // lease: the caller's stream (fwx_opts.stream) or a handle's stream (the batch queries borrow
    // scratch from a context).  They are drained with the context's streams before any buffer is
    // released, regrown or handed to the next lease.
    hipStream_t foreign[2] = {nullptr, nullptr};
    void uses_stream(hipStream_t st)
    {
        if (!st || st == s || st == side.s || st == foreign[0] || st == foreign[1]) return;
        if (!foreign[0]) foreign[0] = st;
        else if (!foreign[1]) foreign[1] = st;
        else { drain_stream(foreign[0]); foreign[0] = st; }
    }
    void drain()
    {
        drain_stream(s);
        side.drain();
        for (hipStream_t &f : foreign)
            if (f) drain_stream(f);
    }
    int reserve(int which, size_t bytes, void **out)
    {
        if (cap[which] < bytes) {
            if (buf[which]) { drain(); (void)hipFree(buf[which]); buf[which] = nullptr; cap[which] = 0; }
            const size_t want = bytes < 4096 ? 4096 : bytes + bytes / 8;      // a little head room
            if (hipMalloc(&buf[which], want) != hipSuccess) {
                (void)hipGetLastError();
                FWX_HIP(hipMalloc(&buf[which], bytes));                       // exactly, then
                cap[which] = bytes;
            } else {
                cap[which] = want;
            }
        }
        *out = buf[which];
        return FWX_OK;
    }
    void trim()
    {
        bool any = false;
        for (int i = 0; i < NBUF; ++i) any = any || cap[i] > kKeepBytes;
        if (any) drain();
        for (int i = 0; i < NBUF; ++i)
            if (cap[i] > kKeepBytes) { (void)hipFree(buf[i]); buf[i] = nullptr; cap[i] = 0; }
    }
    void destroy()
    {
        drain();
        if (pin) (void)hipHostFree(pin);
        for (int i = 0; i < NBUF; ++i)
            if (buf[i]) (void)hipFree(buf[i]);
        if (s) (void)hipStreamDestroy(s);
    }
};

class CtxPool {
public:
    // The current device must already be the call's device (DeviceGuard).
    static int acquire(CallCtx **out)
    {
        int dev = 0;
        FWX_HIP(hipGetDevice(&dev));
        Pool &p = pool();
        {
            std::lock_guard<std::mutex> lk(p.mu);
            for (size_t i = 0; i < p.free_.size(); ++i)
                if (p.free_[i]->device == dev) {
                    *out = p.free_[i];
                    p.free_.erase(p.free_.begin() + (long)i);
                    g_pool_stats[POOL_CTX].lease();
                    return FWX_OK;
                }
        }
        CallCtx *c = new (std::nothrow) CallCtx();
        if (!c) return FWX_ERR_OOM;
        c->device = dev;
        if (hipStreamCreateWithFlags(&c->s, hipStreamNonBlocking) != hipSuccess) {
            g_last_hip = (int)hipGetLastError();
            delete c;
            return FWX_ERR_HIP;
        }
        g_pool_stats[POOL_CTX].created.fetch_add(1, std::memory_order_relaxed);
        g_pool_stats[POOL_CTX].lease();
        *out = c;
        return FWX_OK;
    }
    static void release(CallCtx *c)
    {
        if (!c) return;
        g_pool_stats[POOL_CTX].unlease();
        c->trim();
        Pool &p = pool();
        {
            std::lock_guard<std::mutex> lk(p.mu);
            if (p.free_.size() < kMaxFree) { p.free_.push_back(c); return; }
        }
        c->destroy();          // more concurrent callers than the pool keeps: this one goes
        delete c;
        g_pool_stats[POOL_CTX].destroyed.fetch_add(1, std::memory_order_relaxed);
    }

private:
    static constexpr size_t kMaxFree = kCtxPoolMaxFree;
    struct Pool { std::mutex mu; std::vector<CallCtx *> free_; };
    static Pool &pool() { static Pool *p = new Pool(); return *p; }   // leaked on purpose
};

// A context for the duration of one call.
struct CtxLease {
    CallCtx *c = nullptr;
    int open() { return CtxPool::acquire(&c); }
    ~CtxLease()
    {
        if (c) {       // an error return may leave work queued: the context goes back idle
            (void)hipStreamSynchronize(c->s);
            if (c->side.s) (void)hipStreamSynchronize(c->side.s);
            for (hipStream_t &f : c->foreign)
                if (f) { drain_stream(f); f = nullptr; }   // the stream belongs to someone else: forget it
        }
        CtxPool::release(c);
    }
};

inline size_t fused_ws_bytes(int n, size_t es, bool with_hops)
{
    const size_t ld = ((size_t)n + 3) & ~(size_t)3;
    // FOUR panel sets -- W, Ct, CNt, and with hops WH, CHt -- of 64 pivots each: the double-pass
    // schedule (fused_range) applies two passes per main launch while the next two are produced; the
    // single-pass schedules use the first two sets
    size_t b = (size_t)4 * FWX_FUSED_B * ((size_t)n * es + ld * (es + 4)) + 256;
    if (with_hops) b += (size_t)4 * FWX_FUSED_B * ((size_t)n * 4 + ld * 4);
    return b;
}

// One read of the matrix (fwx.h "Domain"): bit 0 = every rate is >= +0.0 and not NaN; bit 1 = no
// entry has a non-zero rate and next < 0.  d_flag: a device int the caller owns.
template <typename T>
int domain_bits(const T *rate, const int32_t *next, size_t count, int *d_flag, hipStream_t s, int &bits)
{
    int h = 3;
    FWX_HIP(hipMemcpyAsync(d_flag, &h, sizeof(int), hipMemcpyHostToDevice, s));
    FWX_HIP(fwx::launch_nonneg_check(rate, next, count, d_flag, s));
    FWX_HIP(hipMemcpyAsync(&h, d_flag, sizeof(int), hipMemcpyDeviceToHost, s));
    FWX_HIP(hipStreamSynchronize(s));
    bits = h;
    return FWX_OK;
}

// The digits-only environment switches, read on every call: the first character is a digit (no sign, no blank), the
// whole string is consumed and the value lies in [lo, hi]; anything else, or unset, gives dflt.  A value too large
// for strtoll saturates and fails the range.
inline long long env_digits(const char *name, long long lo, long long hi, long long dflt)
{
    const char *e = getenv(name);
    if (!e || *e < '0' || *e > '9') return dflt;
    char *end = nullptr;
    const long long v = strtoll(e, &end, 10);
    return *end == '\0' && v >= lo && v <= hi ? v : dflt;
}

// The path trace `off` elements further on (e.g. at pivot row k0: off = k0 * n); null stays null.
inline fwx::PathLog plog_rows(fwx::PathLog p, size_t off)
{
    if (p.last) { p.last += off; p.at_col += off; p.at_row += off; }
    return p;
}

// crossover (single / double pass, ms; profiles/r03_double_pass_crossover.txt): f32 4096: 4.10 / 4.74,
// 6144: 10.47 / 10.18, 8192: 21.2 / 20.0, 12288: 68.1 / 61.0, 16384: 152.0 / 135.3; f64 6144: 23.1 / 22.1,
// 16384: 355 / 324 -- below ~6000 the side chain (five launches per 128 pivots) is the critical path
constexpr int kDoublePassMinN = 6144;    // FWX_DOUBLE_PASS_MIN_N overrides
// ... and with next-hops (the arg kernels; + trace, + hops), f32 only: FWX_DOUBLE_PASS_NEXT_MIN_N overrides.
// (f64: the two-pass fused_main_arg_f64 is SLOWER than two launches, N = 16384 + next 486 -> 499 ms on
// one box -- tools/runs/r03_run33.sh --, so f64 stays on the single pass unless the variable asks)
// (round 4, after the panel flags and the 32-row column panels: tools/runs/r04_run42.sh, single / double pass, ms:
//  + next 4096 5.8 / 6.0, 5120 9.9 / 9.7, 6144 16.2 / 16.0, 7168 24.3 / 23.8; + trace 4096 6.3 / 6.8, 6144 21.0 /
//  17.9, 7168 32.0 / 26.1 -- the threshold was 8192)
constexpr int kDoublePassNextMinN = 5120;
// The partitioned handle's crossover with next-hops lags the single-device value on purpose: round 4 measured
// one device only, and nobody has measured partitions in [5120, 8192) yet.
constexpr int kMultiDoublePassNextMinN = 8192;
// FWX_LOOKAHEAD_MIN_N / FWX_SYMMETRIC_MIN_N / FWX_DOUBLE_PASS_* override the thresholds (tests force each
// schedule at small sizes, tuning runs switch one off with a huge value); read on every solve.
inline int env_threshold(const char *name, int dflt)
{
    const char *e = getenv(name);
    if (e && *e) {
        char *end = nullptr;
        const long v = strtol(e, &end, 10);
        if (end != e && v >= 0 && v <= INT32_MAX) return (int)v;
    }
    return dflt;
}

}  // namespace fwxi

#endif
