// fwx_internal.h -- pieces shared by the translation units behind the C ABI (fwx_api.hip: one
// device; fwx_batch.hip: the batched solves; fwx_multi.hip: the row-partitioned multi-device handle).  Not
// installed, not part of the ABI.
#ifndef FWX_INTERNAL_H
#define FWX_INTERNAL_H

#include <hip/hip_runtime.h>
#include <algorithm>
#include <mutex>
#include <new>
#include <type_traits>
#include <vector>
#include <limits.h>
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
constexpr size_t kCtxPoolMaxFree = 8;          // CtxPool keeps this many idle contexts
constexpr size_t kPerkScratchMax = 16;         // PerkScratch keeps this many streams' buffers
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
                                                           // fwx_solve_batch_lists_*: next0, the trace, the walk's chunk
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


// Temporal-tail budget of the per-k engine (fwx::RelaxArgs::temporal_bytes): the bytes of a slab's last
// rows that are loaded with the default cache policy in every launch; the rest of a larger slab is
// streamed non-temporally (presumably not allocating in the 256 MiB Infinity Cache, so the tail stays
// resident there).  Default from profiles/r05_tune_relax_policy.txt; FWX_PERK_TEMPORAL_MIB=<MiB> overrides it
// (may be fractional; 0: the whole slab non-temporal, a huge value: all default policy), read on
// every call.
#define FWX_PERK_TEMPORAL_MIB_DEFAULT 256
// Build switch for A/B runs (`python -m floydwarshall_amd.build --variant NAME -DFWX_XCD_SERPENTINE=0`): 0 =
// the serpentine sweep reverses tile by tile even where the split applies.
#ifndef FWX_XCD_SERPENTINE
#define FWX_XCD_SERPENTINE 1
#endif
inline long long perk_temporal_bytes(size_t slab_bytes)
{
    double mib = FWX_PERK_TEMPORAL_MIB_DEFAULT;
    if (const char *e = getenv("FWX_PERK_TEMPORAL_MIB"))
        if (*e) mib = std::max(0.0, strtod(e, nullptr));
    const double b = mib * (1 << 20);
    if (!(b < (double)slab_bytes)) return -1;          // the slab fits (or NaN): all default policy
    return (long long)b;
}

// Store granularity of relax_k's rates-only path (fwx::RelaxArgs::store_bytes): FWX_PERK_STORE_BYTES=<16|32|64|128>
// overrides FWX_PERK_STORE_BYTES_DEFAULT, read on every call; any other value: the default.  No result bit
// depends on it.
inline int perk_store_bytes()
{
    if (const char *e = getenv("FWX_PERK_STORE_BYTES")) {
        const int b = atoi(e);
        if (b == 16 || b == 32 || b == 64 || b == 128) return b;
    }
    return FWX_PERK_STORE_BYTES_DEFAULT;
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

// Pivots per streaming pass of the per-k engine's rates-only whole-matrix solves (relax_kt):
// FWX_PERK_PIVOTS=<1|2|4|8> overrides FWX_PERK_PIVOTS_DEFAULT, read on every call; any other value: the
// default.  1 = one relax_k launch per pivot, launch for launch the engine before relax_kt existed.  No
// result bit depends on it.
#define FWX_PERK_PIVOTS_DEFAULT 8
inline int perk_pivots()
{
    if (const char *e = getenv("FWX_PERK_PIVOTS")) {
        char *end = nullptr;
        const long v = strtol(e, &end, 10);
        if (end != e && *end == '\0' && (v == 1 || v == 2 || v == 4 || v == 8)) return (int)v;
    }
    return FWX_PERK_PIVOTS_DEFAULT;
}

// The wide pass of the multi-pivot schedule (round 19): where it would issue two consecutive 8-pivot sweeps inside a
// block, an uncounted f32 solve at the width 8 issues one 16-pivot sweep.  FWX_PERK_WIDE=0 turns it off -- launch
// for launch the schedule before it -- and anything else, or unset, leaves it on; read on every call.  It has no
// effect at any other width (FWX_PERK_PIVOTS keeps its parse: 16 is no width), on a counted call or on f64.  For
// tests and A/B runs in one binary.  No result bit depends on it.
inline bool perk_wide()
{
    const char *e = getenv("FWX_PERK_WIDE");
    return !(e && !strcmp(e, "0"));
}

// The kernel of the 16-pivot sweep (round 23): relax_walk -- one body for every tile, three waves per SIMD
// (fwx_kernels.hip; the geometry: FWX_PERK_WALK_* in fwx_kernels.h).  FWX_PERK_WALK=0 gives round 19's relax_kt instead,
// launch for launch; anything else, or unset, leaves relax_walk on; read on every call.  The schedule, its launch
// counts and both hooks' counters are the same either way.  For tests and A/B runs in one binary, and the remedy
// should the new kernel misbehave.  No result bit depends on it.
inline bool perk_walk()
{
    const char *e = getenv("FWX_PERK_WALK");
    return !(e && !strcmp(e, "0"));
}

// The deep pass (round 25): where the ladder of the multi-pivot schedule starts at 16 -- an uncounted f32 call at the
// width 8 with the wide pass and the walk on -- it starts at 32: relax_walk with 8 bytes of a row per lane and 32
// pivots per streaming pass, so a 64-pivot block is one panel launch and two sweeps.  FWX_PERK_DEEP=0 gives the
// schedule before it, launch for launch; anything else, or unset, leaves the 32-pivot pass on; read on every call.
// Both hooks' counters read the same either way (a 32-pivot launch is four 8-pivot groups and two wide ones); the
// 32-pivot launches themselves are g_perk_deep_launches.  For tests and A/B runs in one binary, and the remedy for
// inputs with sparse sign-set operands.  No result bit depends on it.
inline bool perk_deep()
{
    const char *e = getenv("FWX_PERK_DEEP");
    return !(e && !strcmp(e, "0"));
}

// The tile sweep (round 26): where the deep pass would issue two 32-pivot sweeps for a FULL 64-pivot block, a matrix
// of order n >= FWX_PERK_TILE_MIN_N takes one relax_tile launch (fwx_fused.hip: the block's 64 pivots in one pass on
// register tiles).  Digits only, read on every call: 0 = never, otherwise the smallest order that takes it; any
// other text means the default.  Ragged blocks, counted calls, f64 and every switch above at `0` keep the ladder.  The
// three older hooks' counters read the same either way (a tile launch is eight 8-pivot groups, four wide ones and
// two deep ones); the tile launches themselves are g_perk_tile_launches.  For tests and A/B runs in one binary, and
// the remedy for inputs whose operands carry sign bits everywhere.  No result bit
// depends on it.
#define FWX_PERK_TILE_MIN_N_DEFAULT 1024
inline int perk_tile_min_n() { return (int)env_digits("FWX_PERK_TILE_MIN_N", 0, INT_MAX, FWX_PERK_TILE_MIN_N_DEFAULT); }

// The pair schedule (round 29): a call that takes the tile sweep, starts on a multiple of 64, has at least four full
// blocks from its first pivot that is a multiple of 128, runs on the stream's own scratch entry and on a stream that
// is not capturing, at n >= FWX_PERK_PAIR_MIN_N, applies its full blocks two at a time: one 128-pivot relax_tile
// launch per pair on the caller's stream, the panels of the next pair made beside it on a look-ahead stream
// (relax_range_kt).  Digits only, read on every call: 0 = never, otherwise the smallest order that takes it; any other
// text means the default.  Every older hook's counters read the same either way (a 128-pivot launch is sixteen 8-pivot
// groups, eight wide, four deep and two tile launches); the 128-pivot launches themselves are g_perk_pair_launches.
// No result bit depends on it.  Since round 30 it is the threshold of the group
// schedule as well: how many blocks a main launch applies is FWX_PERK_GROUP_MAX's matter (below), whether the call takes
// a look-ahead schedule at all is this variable's, and 0 still gives the serial schedule whatever the other says.
// The default: serial / pair, ms per whole solve (profiles/r29_pair_crossover.txt): 2048 1.27 / 1.76, 3072 2.58 / 2.75,
// 4096 4.23 / 4.58, 5120 6.90 / 6.09, 6144 10.12 / 9.19, 8192 20.7 / 18.9, 12288 69.5 / 62.1, 16384 158.5 / 142.9 -- up
// to 4096 the look-ahead chain (four launches per 128 pivots) is the critical path, as it is for the fused engine's
// double pass below its own crossover.
#define FWX_PERK_PAIR_MIN_N_DEFAULT 5120
inline int perk_pair_min_n() { return (int)env_digits("FWX_PERK_PAIR_MIN_N", 0, INT_MAX, FWX_PERK_PAIR_MIN_N_DEFAULT); }

// The group schedule (round 30): a call that takes the pair schedule applies its full blocks in groups of up to
// FWX_PERK_GROUP_MAX blocks per main launch, the groups growing inside the call (perk_group_size).  Digits only, read on
// every call: 2 ... FWX_PERK_GROUP_CAP, an odd value rounded down to the even one below it; 2 is the pair schedule of
// round 29, launch for launch.  Any other text, or unset, means the default, which goes by the order of the matrix
// (perk_group_max(n)); a value that is set holds at every order.  FWX_PERK_PAIR_MIN_N=0 still gives the serial
// schedule.  Every older hook's counters read the same for every value (a 512-pivot launch is four 128-pivot ones, and
// so on down); the main launches by group size are g_perk_group_launches.  No result bit depends on it (DESIGN.md
// section 4.1, round 30).
// The default: serial / 2 / 4 / 8, ms per whole solve in one call (profiles/r30_group_crossover.txt): 5120 6.92 / 6.15 /
// 6.41 / 6.73, 6144 10.18 / 9.15 / 9.18 / 9.00, 8192 20.8 / 19.1 / 18.0 / 17.8, 12288 70.2 / 62.1 / 57.5 / 56.8, 16384
// 158.9 / 143.5 / 133.9 / 131.0 -- at 5120 the chains of the larger groups no longer end before the main launches
// beside them, from 6144 eight blocks are the fastest at every order measured.
#define FWX_PERK_GROUP_CAP 8
#define FWX_PERK_GROUP_MIN_N_DEFAULT 6144
inline int perk_group_max_env() { return (int)env_digits("FWX_PERK_GROUP_MAX", 2, FWX_PERK_GROUP_CAP, 0) & ~1; }
inline int perk_group_max(int n)
{
    if (const int g = perk_group_max_env()) return g;
    return n >= FWX_PERK_GROUP_MIN_N_DEFAULT ? FWX_PERK_GROUP_CAP : 2;
}
// The size of the next group: `left` full blocks are still to be applied, the group before had `prev` blocks (0: this
// is the call's first group), at most `gmax` blocks per group.  The rule: the chain beside a main launch must end
// before that launch does.  The chain that prepares a group of G blocks runs beside the main launch of the group
// before, P blocks: per block of G one panel launch and one 64-pivot cross launch on the band, behind one cross launch
// through the P blocks.  At n = 16384 a main launch spends about 570 us per block of P and the chain beside it 180 to
// 380 us per block of G (profiles/r30_group_chain.txt: the panel launch alone takes 26 us by itself and 100 to 270 us
// beside a main launch), so G <= 2 * P: the chain of a 4-block group ends 300 us before the pair's launch does, the
// chain of a 2-block tail 2.7 ms before the 8-block launch, but the chain of an 8-block group ends about 180 us BEHIND
// the 4-block launch beside it (its last three blocks run alone, 80 us each): the one place where the rule is not met.
// It ships all the same: groups of at most 4 in its place are slower at every order from 6144
// (profiles/r30_group_crossover.txt).
// Nothing runs beside the work in front of the first main launch, so the first group is a pair, as in round 29.  A
// single block that is left is the odd last block.
inline int perk_group_size(int left, int prev, int gmax)
{
    if (left < 2) return left > 0 ? 1 : 0;
    return std::min(std::min(prev > 0 ? 2 * prev : 2, gmax), left & ~1);
}

// The fold of relax_kt's non-counting f32 sweeps: FWX_PERK_FOLD=compare forces the compare form in every tile, read on
// every call; anything else, or unset: automatic (each wave takes the max form where the operands it has loaded
// are all NaN or sign-clear).  For tests and A/B runs in one binary.  No result bit depends on it (DESIGN.md
// section 4.1, round 14).
inline bool perk_fold_compare()
{
    const char *e = getenv("FWX_PERK_FOLD");
    return e && !strcmp(e, "compare");
}

// Tier choice of the batched small solves (fwx_solve_batch_*, fwx_dev_solve_batch): matrices of order n <=
// FWX_BATCH_WAVE_MAX_N take the wave tier (one wave per matrix, registers only), larger ones the workgroup
// tier (small_solve's body, one workgroup per matrix).  An integer 0 ... FWX_BATCH_WAVE_N, read on every
// call; 0 turns the wave tier off; any other value: the default.  No result bit depends on it.
#define FWX_BATCH_WAVE_MAX_N_DEFAULT FWX_BATCH_WAVE_N
inline int batch_wave_max_n()
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
inline int batch_mid_min_n()
{
    return (int)env_digits("FWX_BATCH_MID_MIN_N", 1, FWX_BATCH_MID_MIN_N_DEFAULT, FWX_BATCH_MID_MIN_N_DEFAULT);
}

// Routing of the large batch entry points (fwx_solve_batch_large_*, fwx_dev_solve_batch_large): orders below
// FWX_BATCH_LARGE_MIN_N are forwarded to the mid entry path (which forwards further by FWX_BATCH_MID_MIN_N), orders
// from it up to FWX_BATCH_LARGE_MAX_N run the large tier (fwx_large.hip).  An integer 1 ... FWX_BATCH_MID_MAX_N + 1,
// read on every call; any other value: the default, FWX_BATCH_MID_MAX_N + 1.  No result bit depends on it.
#define FWX_BATCH_LARGE_MIN_N_DEFAULT (FWX_BATCH_MID_MAX_N + 1)
inline int batch_large_min_n()
{
    return (int)env_digits("FWX_BATCH_LARGE_MIN_N", 1, FWX_BATCH_LARGE_MIN_N_DEFAULT, FWX_BATCH_LARGE_MIN_N_DEFAULT);
}

// fwx_solve_batch_lists_*: items walked per launch.  The lists (cap int32 per item), the walk stacks
// (FWX_EXACT_SCRATCH_INTS(n)) and the item triples + lengths (4) of one launch stay within
// FWX_BATCH_LISTS_BUDGET_BYTES of device memory; FWX_BATCH_LISTS_CHUNK (environment, read per call: digits only,
// >= 1, anything else means the default) asks for fewer.  At least one item per launch.  No result depends on it.
#define FWX_BATCH_LISTS_BUDGET_BYTES ((long long)64 << 20)
inline long long batch_lists_chunk(int n, int cap)
{
    const long long per_item = 4ll * ((long long)cap + 3ll * ((long long)n + 2) + 4);
    long long fit = FWX_BATCH_LISTS_BUDGET_BYTES / per_item;
    if (fit < 1) fit = 1;
    return env_digits("FWX_BATCH_LISTS_CHUNK", 1, fit - 1, fit);
}

// Launches of the multi-pivot schedule by pivots per launch: [0] relax_k (ragged single pivots), [1] / [2] /
// [3] relax_kt with 2 / 4 / 8, [4] panel launches.  Test hook fwx_test_perk_pivots (fwx.h); relaxed host atomics.
// A 16-pivot sweep applies two 8-pivot groups and adds 2 to [3], so that the five counters read the same with the
// wide pass on and off; the number of 16-pivot launches themselves is g_perk_wide_launches (fwx_test_perk_wide).
inline std::atomic<uint64_t> g_perk_launches[5];
// A 32-pivot sweep (round 25) adds 4 to [3] and 2 to g_perk_wide_launches, for the same reason, and 1 to
// g_perk_deep_launches (fwx_test_perk_deep).
inline std::atomic<uint64_t> g_perk_wide_launches;
inline std::atomic<uint64_t> g_perk_deep_launches;
// A tile sweep (round 26) applies a whole 64-pivot block: 8 to [3], 4 to g_perk_wide_launches, 2 to g_perk_deep_launches,
// for the same reason, and 1 to g_perk_tile_launches (fwx_test_perk_tile).
inline std::atomic<uint64_t> g_perk_tile_launches;
// A 128-pivot main launch of the pair schedule (round 29) applies two blocks: 16 to [3], 8 / 4 / 2 to the three counters
// above, and 1 to g_perk_pair_launches (fwx_test_perk_pair).  The cross launches of its look-ahead chain add nothing:
// each entry still sees every pivot once in these counts.
inline std::atomic<uint64_t> g_perk_pair_launches;
// A main launch of the group schedule (round 30) that applies G blocks, G = 2, 4, 6 or 8, adds G / 2 to
// g_perk_pair_launches and in proportion to everything above, and 1 to g_perk_group_launches[G / 2 - 1]
// (fwx_test_perk_group).  The cross launches of its chain add nothing, as before.
inline std::atomic<uint64_t> g_perk_group_launches[FWX_PERK_GROUP_CAP / 2];

// Snapshot panels (W and Ct of one 64-pivot block) of the multi-pivot schedule: perk_kt_ws_bytes.  A blocking
// entry point that holds a per-call context passes that context's workspace.  fwx_dev_relax* has no workspace
// argument and returns with its launches queued, so there the panels live in a process-wide pool keyed by the
// stream (whose device is taken from the stream, not from the caller's current device): launches that read a
// buffer and the panel launch that next rewrites it are then always on ONE stream, in order, and two
// streams never share a buffer.  A buffer is allocated by the first call on its stream and kept; only a call
// that needs a larger one than its stream has waits for that stream, frees and allocates again.  The pool
// keeps at most kMax buffers: one more evicts the least recently used with hipFree, which waits for the
// device and so for any launch that may still read it, whether or not its stream still exists.  The pool
// mutex is held across those (rare) allocations.  Nothing is synchronised on the way out.
template <typename T> inline size_t perk_kt_ws_bytes(int n)
{
    const size_t ld = ((size_t)n + 3) & ~(size_t)3;
    return (size_t)FWX_FUSED_B * ((size_t)n + ld) * sizeof(T);
}
// The pair schedule (round 29) keeps more in the stream's entry: four panel sets instead of one (asked for only by the
// calls that take it), and a look-ahead stream with its two events.  Those are created by the first such call on the
// stream, on the stream's device -- the stream non-blocking, so that it orders itself against the caller's stream (the
// null stream included) through the events alone; the events without timing -- and destroyed with the entry.  Every call
// makes the caller's stream wait for the look-ahead stream before it returns, so "this stream's launches are the
// buffer's only readers" holds as before.
//
// An entry is IN USE from the `get` of a call to that call's return (PerkLease, held by relax_range_kt for its scope,
// error returns included): the call goes on queueing launches that read the buffer, on the look-ahead stream too, long
// after `get` has dropped the mutex, and hipFree waits only for what is queued already.  An entry in use is never
// evicted, whatever its stamp; the victim is the least recently used IDLE entry (perk_scratch_victim).  With every
// entry in use -- more callers inside the library at once than the pool keeps -- the pool exceeds kMax for the
// moment; a later `get` that adds an entry evicts idle ones until kMax are kept again.
struct PerkSide {
    hipStream_t s = nullptr;
    hipEvent_t main_done = nullptr, chain_done = nullptr;
};
// The victim rule over the entries' stamps and in-use marks: the index of the least recently used idle entry of a
// pool that holds `cap` entries or more, -1 if the pool is below `cap` or every entry is in use (fwx_test_perk_scratch_victim).
inline int perk_scratch_victim(const uint64_t *used, const int *busy, int count, int cap)
{
    if (count < cap) return -1;
    int v = -1;
    for (int i = 0; i < count; ++i)
        if (!busy[i] && (v < 0 || used[i] < used[v])) v = i;
    return v;
}
struct PerkLease {                                 // an entry of PerkScratch in use by one call
    hipStream_t s = nullptr;
    int dev = -1;
    bool held = false;
    PerkLease() = default;
    PerkLease(const PerkLease &) = delete;
    PerkLease &operator=(const PerkLease &) = delete;
    inline ~PerkLease();
};
class PerkScratch {
public:
    static constexpr size_t kMax = kPerkScratchMax;
    // lease: marks the entry in use until the lease is destroyed
    static int get(hipStream_t s, size_t bytes, void **out, PerkSide *side, PerkLease &lease)
    {
        int dev = 0, cur = 0;
        FWX_HIP(hipGetDevice(&cur));
        dev = cur;
        if (s) FWX_HIP(hipStreamGetDevice(s, &dev));
        Pool &p = pool();
        std::lock_guard<std::mutex> lk(p.mu);
        Entry *e = nullptr;
        for (Entry &x : p.all)
            if (x.s == s && x.dev == dev) { e = &x; break; }
        if (!e) {
            while (p.all.size() >= kMax) {         // evict the least recently used idle entries, down to kMax - 1
                std::vector<uint64_t> used;
                std::vector<int> busy;
                for (const Entry &x : p.all) { used.push_back(x.used); busy.push_back(x.busy); }
                const int v = perk_scratch_victim(used.data(), busy.data(), (int)p.all.size(), (int)kMax);
                if (v < 0) break;                  // every entry is in a call: the pool grows for the moment
                if (p.all[v].p) (void)hipFree(p.all[v].p);
                release(p.all[v].side);            // behind the hipFree, which has waited for the device
                p.all.erase(p.all.begin() + v);
                g_pool_stats[POOL_PERK].destroyed.fetch_add(1, std::memory_order_relaxed);
            }
            p.all.push_back(Entry{dev, s, nullptr, 0, 0, PerkSide(), 0});
            e = &p.all.back();
            g_pool_stats[POOL_PERK].created.fetch_add(1, std::memory_order_relaxed);
        }
        e->used = ++p.clock;
        ++e->busy;                                 // from here on every return path leaves the mark to the lease
        lease.s = s; lease.dev = dev; lease.held = true;
        g_pool_stats[POOL_PERK].lease();
        if (e->cap < bytes) {
            if (e->p) {
                if (s) (void)hipStreamSynchronize(s);   // its readers are queued on this stream and nowhere else
                (void)hipFree(e->p);
                e->p = nullptr; e->cap = 0;
            }
            if (dev != cur) FWX_HIP(hipSetDevice(dev));
            const hipError_t err = hipMalloc(&e->p, bytes);
            if (dev != cur) (void)hipSetDevice(cur);
            FWX_HIP(err);
            e->cap = bytes;
        }
        if (side && !e->side.chain_done) {         // all three or none: a failure half way releases what it made
            if (dev != cur) FWX_HIP(hipSetDevice(dev));
            hipError_t err = hipStreamCreateWithFlags(&e->side.s, hipStreamNonBlocking);
            if (err == hipSuccess) err = hipEventCreateWithFlags(&e->side.main_done, hipEventDisableTiming);
            if (err == hipSuccess) err = hipEventCreateWithFlags(&e->side.chain_done, hipEventDisableTiming);
            if (err != hipSuccess) release(e->side);
            if (dev != cur) (void)hipSetDevice(cur);
            FWX_HIP(err);
        }
        if (side) *side = e->side;
        *out = e->p;
        return FWX_OK;
    }
    static void put(hipStream_t s, int dev)
    {
        Pool &p = pool();
        std::lock_guard<std::mutex> lk(p.mu);
        for (Entry &x : p.all)
            if (x.s == s && x.dev == dev) {
                if (x.busy > 0) --x.busy;
                x.used = ++p.clock;                // idle from now: the stamp eviction goes by
                break;
            }
        g_pool_stats[POOL_PERK].unlease();
    }

private:
    struct Entry { int dev; hipStream_t s; void *p; size_t cap; uint64_t used; PerkSide side; int busy; };
    static void release(PerkSide &d)
    {
        if (d.main_done) (void)hipEventDestroy(d.main_done);
        if (d.chain_done) (void)hipEventDestroy(d.chain_done);
        if (d.s) (void)hipStreamDestroy(d.s);
        d = PerkSide();
    }
    struct Pool { std::mutex mu; std::vector<Entry> all; uint64_t clock = 0; };
    static Pool &pool() { static Pool *p = new Pool(); return *p; }   // leaked on purpose
};
inline PerkLease::~PerkLease() { if (held) PerkScratch::put(s, dev); }

// The multi-pivot schedule of relax_range (below) for a rates-only solve of the whole matrix in place.  Per
// block of <= 64 pivots: ONE panel launch (fused_panels, compare form: W and Ct of the block from the
// time-k0 matrix, which it does not modify), then the block's pivots `np` at a time, one relax_kt launch
// each, all on `s`.  A ragged end of a block goes down the powers of two; a last single pivot is a relax_k
// launch on the live row -- exact, because between launches the matrix is a consistent time-k state.
// An uncounted f32 call at np == 8 starts the ladder at 16 (perk_wide): the panels hold the snapshots of all 64
// pivots of the block, so the second 8-pivot sweep of a pair need not re-read the matrix; with the walk on as well it
// starts at 32 (perk_deep), one streaming pass per half block.
// A FULL block of such a call at n >= perk_tile_min_n() takes one relax_tile launch instead of the two 32-pivot sweeps
// (round 26): the block's 64 pivots in one pass on register tiles, the operands through LDS.
// From n >= perk_pair_min_n() such a call applies its full blocks two at a time behind a look-ahead chain on a second
// stream (round 29: the pair schedule, below); when it returns, `s` waits for everything it queued there.
template <typename T>
inline int relax_range_kt(T *rate, int n, int k_begin, int k_end, int serpentine, int np,
                          unsigned long long *d_updates, hipStream_t s, void *ws)
{
    constexpr int Bq = FWX_FUSED_B;
    const size_t ld = ((size_t)n + 3) & ~(size_t)3;
    const bool wide = np == 8 && !d_updates && std::is_same<T, float>::value && perk_wide();
    const int g_top = wide ? (perk_walk() && perk_deep() ? 32 : 16) : np;
    // a full block where the ladder would start at 32: one tile sweep (round 26) instead of the two 32-pivot sweeps
    const int tile_min_n = perk_tile_min_n();
    const bool tile = g_top == 32 && tile_min_n > 0 && n >= tile_min_n && n >= Bq;
    // The pair schedule (round 29; the comment above perk_pair_min_n): the stream's own scratch entry only, since a
    // caller's workspace holds one panel set and no look-ahead stream.
    const int k_a = (k_begin + 2 * Bq - 1) / (2 * Bq) * (2 * Bq);     // the first group starts on a tile boundary
    const int pair_min_n = perk_pair_min_n();
    bool pair = tile && !ws && pair_min_n > 0 && n >= pair_min_n && k_begin % Bq == 0 && k_end - k_a >= 4 * Bq;
    if (pair) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cap) != hipSuccess) {            // (a null stream beside a global capture)
            (void)hipGetLastError();
            pair = false;
        } else if (cap != hipStreamCaptureStatusNone) {
            pair = false;                                             // a captured graph gets no parallel branches
        }
    }
    // The group schedule (round 30): at most gmax blocks per main launch; 2 is the pair schedule itself.
    const int gmax = pair ? perk_group_max(n) : 1;
    const int sets = pair ? 2 * gmax : 1;
    PerkSide side;
    PerkLease lease;                               // the stream's entry stays in use until this call returns
    if (!ws) {
        const int rc0 = PerkScratch::get(s, (size_t)sets * perk_kt_ws_bytes<T>(n), &ws, pair ? &side : nullptr, lease);
        if (rc0) return rc0;
    }
    // `sets` panel sets: the W rows of all sets, then the Ct lines of all sets.  The group schedule keeps two halves of
    // gmax sets each, block i of group g in set (g & 1) * gmax + i, so that the panels of a group are contiguous rows of
    // W and lines of Ct whatever its size and no group wraps; with gmax 2 that is round 29's "block q in set q & 3".
    T *const w_all = (T *)ws, *const ct_all = w_all + (size_t)sets * Bq * n;
    T *w = w_all, *ct = ct_all;                    // the set in use
    auto use_set = [&](int g, int i) {
        const int at = (g & 1) * gmax + i;
        w = w_all + (size_t)at * Bq * n;
        ct = ct_all + (size_t)at * Bq * ld;
    };

    fwx::FusedArgs<T> pa;
    pa.rate = rate; pa.next = nullptr; pa.rows = n; pa.n = n; pa.row0 = 0; pa.w = nullptr; pa.ct = ct;
    pa.cnt = nullptr; pa.ct_ld = (int)ld; pa.updates = nullptr; pa.nonneg = false;
    fwx::RelaxKtArgs<T> a;
    a.rate = rate; a.ct_ld = (int)ld; a.n = n; a.updates = d_updates;
    a.temporal_bytes = perk_temporal_bytes((size_t)n * n * sizeof(T));
    a.store_bytes = perk_store_bytes();
    a.fold_compare = perk_fold_compare();
    a.walk = perk_walk();
    fwx::RelaxArgs<T> a1;
    a1.rate = rate; a1.next = nullptr; a1.hops = nullptr; a1.phops = nullptr; a1.rows = n; a1.n = n; a1.row0 = 0;
    a1.updates = d_updates; a1.temporal_bytes = a.temporal_bytes; a1.store_bytes = a.store_bytes;
    const int rev = FWX_XCD_SERPENTINE && a.temporal_bytes >= 0 ? 2 : 1;
    Throttle thr;
    int sweeps = 0;                                // launches alternate direction, whatever their width
    auto after = [&](hipError_t e, int slot, int groups = 1) -> int {
        if (e == hipErrorInvalidValue) return FWX_ERR_INVALID;
        FWX_HIP(e);
        if (slot >= 0) {                           // (a cross launch of the pair schedule counts nowhere)
            g_perk_launches[slot].fetch_add((uint64_t)groups, std::memory_order_relaxed);
            if (groups >= 2) g_perk_wide_launches.fetch_add((uint64_t)groups / 2, std::memory_order_relaxed);
            if (groups >= 4) g_perk_deep_launches.fetch_add((uint64_t)groups / 4, std::memory_order_relaxed);
            if (groups >= 8) g_perk_tile_launches.fetch_add((uint64_t)groups / 8, std::memory_order_relaxed);
            if (groups >= 16) g_perk_pair_launches.fetch_add((uint64_t)groups / 16, std::memory_order_relaxed);
        }
        return thr.tick(s);
    };
    // both panels of the block at k0 (bt pivots) into the set in use, from the matrix as `st` finds it
    auto panels = [&](int k0, int bt, hipStream_t st) -> int {
        pa.k0 = k0; pa.bt = bt; pa.ct = ct; pa.side = st != s;
        return after(fwx::launch_fused_panels<T>(pa, w, nullptr, st), 4);
    };
    // pivots [k0, k0 + bt) in one relax_tile launch, the panels from the set in use and the bt / 64 - 1 sets behind it
    auto tiles = [&](int k0, int bt, hipStream_t st, fwx::TileSel sel, int tx, int tw, int te) -> int {
        if constexpr (std::is_same<T, float>::value) {
            a.k = k0; a.np = bt; a.w = w; a.ct = ct;
            a.flip = 0;                            // not read: a tile is loaded and stored once, in any order
            const hipError_t e = fwx::launch_relax_tile(a, st, sel, tx, tw, te);
            if (e == hipSuccess && sel != fwx::TILES_CROSS && bt >= 2 * Bq)
                g_perk_group_launches[bt / (2 * Bq) - 1].fetch_add(1, std::memory_order_relaxed);
            return after(e, sel == fwx::TILES_CROSS ? -1 : 3, bt / 8);
        } else {
            return FWX_ERR_INVALID;                // (tile is false for f64)
        }
    };
    // one block as the serial schedule runs it, everything on `s`: its panels, then a tile sweep or the ladder
    auto block = [&](int k0, int bt, bool panels_ready) -> int {
        int t = 0;
        if (bt >= 2) {
            if (!panels_ready)
                if (const int rc = panels(k0, bt, s)) return rc;
            if (tile && bt == Bq) {
                if (const int rc = tiles(k0, bt, s, fwx::TILES_ALL, 0, 1, 0)) return rc;
                t = bt;
            }
            for (int g = g_top; g >= 2; g >>= 1)
                for (; bt - t >= g; t += g) {
                    a.k = k0 + t; a.np = g; a.w = w + (size_t)t * n; a.ct = ct + (size_t)t * ld;
                    a.flip = serpentine ? rev * (sweeps++ & 1) : 0;
                    if (const int rc = after(fwx::launch_relax_kt<T>(a, s), g >= 8 ? 3 : g == 4 ? 2 : 1, g >= 16 ? g / 8 : 1))
                        return rc;
                }
        }
        for (; t < bt; ++t) {
            a1.k = k0 + t; a1.prow = rate + (size_t)a1.k * n;
            a1.flip = serpentine ? rev * (sweeps++ & 1) : 0;
            if (const int rc = after(fwx::launch_relax<T>(a1, s), 0)) return rc;
        }
        return FWX_OK;
    };
    if (!pair) {
        for (int k0 = k_begin; k0 < k_end; k0 += Bq)
            if (const int rc = block(k0, std::min(Bq, k_end - k0), false)) return rc;
        return FWX_OK;
    }

    // ---- the group schedule (rounds 29 and 30; the model is the double pass of fused_range) ---
    // Blocks are numbered from k_a; a leading block at k_begin = k_a - 64 runs as above.  Group g = `sz` blocks from block
    // q (perk_group_size: 2, then 4, then 8 ... up to gmax, whatever even number is left at the end, a single odd block
    // last) = the pivots of the tile rows / columns [x, x + sz / 2): its band.  While the main launch applies group g,
    // the chain on the look-ahead stream prepares group g + 1: it takes the cross of band(g + 1) through group g in one
    // launch, then block after block of group g + 1 takes the block's panels from that cross and applies the block to
    // it.  With gmax > 2 it applies the group's last block as well: the band is then DONE -- through its own group --
    // and neither the next main launch nor the next chain's first launch touches it again with those pivots.  The main
    // launch of group g therefore steps over band(g) if that is done and over band(g + 1) if a chain runs beside it:
    // one contiguous range of tile indices.
    // Not done are the first group's band -- the work in front of the first main launch is round 29's chain(0), so the
    // first main launch folds block 0 into it a second time, with the same operands, which moves nothing -- the band
    // of an odd last block, which gets its panels the same way and one 64-pivot launch, and every band at gmax == 2,
    // which is round 29's schedule launch for launch.
    const int nfull = (k_end - k_a) / Bq;
    auto k_of = [&](int q) { return k_a + q * Bq; };
    bool chain_open = false;                       // launches are queued on side.s that `s` does not wait for yet
    auto join = [&]() -> hipError_t {
        chain_open = false;
        hipError_t e = hipEventRecord(side.chain_done, side.s);
        if (e == hipSuccess) e = hipStreamWaitEvent(s, side.chain_done, 0);
        return e;
    };
    auto run = [&]() -> int {
        if (k_begin < k_a) {
            use_set(1, gmax - 1);
            if (const int rc = block(k_begin, Bq, false)) return rc;
        }
        // chain(0), on the caller's stream: the first pair's panels need block 0 applied to its own tile row and column
        use_set(0, 0);
        if (const int rc = panels(k_of(0), Bq, s)) return rc;
        if (const int rc = tiles(k_of(0), Bq, s, fwx::TILES_CROSS, k_a / (2 * Bq), 1, 0)) return rc;
        use_set(0, 1);
        if (const int rc = panels(k_of(1), Bq, s)) return rc;
        int g = 0, q = 0, sz = perk_group_size(nfull, 0, gmax);
        bool done = false;                         // the chain has taken band(g) through group g
        for (; sz >= 2; ++g) {
            const int x = k_of(q) / (2 * Bq), xw = sz / 2;               // band(g)
            const int qn = q + sz, szn = perk_group_size(nfull - qn, sz, gmax);
            const int xn = x + xw, xnw = (szn + 1) / 2;                  // band(g + 1): adjacent
            const bool done_n = szn >= 2 && gmax > 2;
            if (szn > 0) {
                FWX_HIP(hipEventRecord(side.main_done, s));              // the last main launch and chain precede
                FWX_HIP(hipStreamWaitEvent(side.s, side.main_done, 0));
                chain_open = true;
                use_set(g, 0);                                           // what band(g) shares with it has seen group g
                if (const int rc = tiles(k_of(q), sz * Bq, side.s, fwx::TILES_CROSS, xn, xnw, done ? xw : 0)) return rc;
                for (int i = 0; i < szn; ++i) {
                    use_set(g + 1, i);
                    if (const int rc = panels(k_of(qn + i), Bq, side.s)) return rc;
                    if (i + 1 < szn || done_n)
                        if (const int rc = tiles(k_of(qn + i), Bq, side.s, fwx::TILES_CROSS, xn, xnw, 0)) return rc;
                }
            }
            use_set(g, 0);
            const int lo = done ? x : xn, hi = szn > 0 ? xn + xnw : xn;
            if (const int rc = tiles(k_of(q), sz * Bq, s, lo < hi ? fwx::TILES_EXCEPT : fwx::TILES_ALL, lo, hi - lo, 0))
                return rc;
            if (chain_open) FWX_HIP(join());
            q = qn; sz = szn; done = done_n;
        }
        if (sz == 1) {                             // the odd last block: its panels are ready
            use_set(g, 0);
            if (const int rc = block(k_of(q), Bq, true)) return rc;
            ++q; ++g;
        }
        if (k_of(q) < k_end) {                     // a ragged tail takes the ladder
            use_set(g, 0);
            if (const int rc = block(k_of(q), k_end - k_of(q), false)) return rc;
        }
        return FWX_OK;
    };
    const int rc = run();
    if (chain_open) (void)join();                  // an error return: the caller's stream still waits for the chain
    return rc;
}

// One launch per pivot over a slab; pivot rows from `prow0 + (k-k_begin)*stride`.  A rates-only call on
// the whole matrix in place with the pivots its own rows takes relax_range_kt instead: FWX_PERK_PIVOTS
// pivots per launch; kt_ws: perk_kt_ws_bytes of device scratch for it that the caller keeps until the launches
// have run, or null: the stream's buffer of PerkScratch.
template <typename T>
inline int relax_range(T *rate, int32_t *next, int32_t *hops, int rows, int n, int row0, const T *prow0,
                const int32_t *phops0, int64_t stride, int k_begin, int k_end, int serpentine,
                unsigned long long *d_updates, hipStream_t s, fwx::PathLog plog = fwx::PathLog(),
                int skip_lo = 0, int skip_hi = 0, const int32_t *pnext0 = nullptr, void *kt_ws = nullptr)
{
    const int np = perk_pivots();
    if (np > 1 && !next && !hops && !plog.last && row0 == 0 && rows == n && skip_hi <= skip_lo &&
        n % (16 / (int)sizeof(T)) == 0 && (uintptr_t)rate % 16 == 0 && stride == n &&
        prow0 == rate + (size_t)k_begin * n && k_end - k_begin >= 2)
        return relax_range_kt<T>(rate, n, k_begin, k_end, serpentine, np, d_updates, s, kt_ws);
    fwx::RelaxArgs<T> a;
    Throttle thr;
    a.rate = rate; a.next = next; a.hops = hops;
    a.rows = rows; a.n = n; a.row0 = row0; a.updates = d_updates; a.plog = plog;
    a.skip_lo = skip_lo; a.skip_hi = skip_hi;
    a.temporal_bytes = perk_temporal_bytes((size_t)rows * n * sizeof(T));
    a.store_bytes = perk_store_bytes();
    // serpentine: reversed in groups of 8 (tiles keep their XCD) where the split applies -- the regime
    // it was measured in (profiles/r05_tune_relax_policy.txt) -- tile by tile otherwise
    const int rev = FWX_XCD_SERPENTINE && a.temporal_bytes >= 0 ? 2 : 1;
    for (int k = k_begin; k < k_end; ++k) {
        a.prow = prow0 + (int64_t)(k - k_begin) * stride;
        a.phops = phops0 ? phops0 + (int64_t)(k - k_begin) * stride : nullptr;
        a.pnext = pnext0 ? pnext0 + (int64_t)(k - k_begin) * stride : nullptr;
        a.k = k;
        a.flip = serpentine ? rev * (k & 1) : 0;
        const hipError_t e = fwx::launch_relax<T>(a, s);
        if (e == hipErrorInvalidValue) return FWX_ERR_INVALID;   // misaligned skip range
        FWX_HIP(e);
        const int rc = thr.tick(s);
        if (rc) return rc;
    }
    return FWX_OK;
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
