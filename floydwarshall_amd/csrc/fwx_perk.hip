// fwx_perk.hip -- the host side of the per-k engine: its environment knobs (one reading per call: PerkKnobs), its
// launch tally, the per-stream pool of snapshot panels (PerkScratch), the multi-pivot schedule (relax_range_kt), the
// range entry relax_range (fwx_perk.h) that fwx_api.hip and fwx_multi.hip call, and the fwx_test_perk_* hooks.  Host
// code only: the kernels and their launchers are fwx_kernels.hip and fwx_fused.hip.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <type_traits>
#include <vector>

#include "fwx.h"
#include "fwx_internal.h"
#include "fwx_kernels.h"
#include "fwx_perk.h"

using namespace fwxi;

// Build switch for A/B runs (`python -m floydwarshall_amd.build --variant NAME -DFWX_XCD_SERPENTINE=0`): 0 =
// the serpentine sweep reverses tile by tile even where the split applies.
#ifndef FWX_XCD_SERPENTINE
#define FWX_XCD_SERPENTINE 1
#endif

namespace {

// ---- the knobs ---------------------------------------------------------------------------------------------------
// Every call of relax_range, and every hook, takes ONE reading of the environment (read_knobs) and works from that;
// nothing below it calls getenv.  No result bit depends on any of them (DESIGN.md section 4.1 has each one's story).
// The fields are initialised to the defaults: what a variable that is unset, or holds anything but what is named, gives.
#define FWX_PERK_GROUP_CAP 8
#define FWX_PERK_GROUP_MIN_N_DEFAULT 6144
struct PerkKnobs {
    // FWX_PERK_PIVOTS=<1|2|4|8>: pivots per streaming pass of a rates-only whole-matrix solve (relax_kt); 1 = one
    // relax_k launch per pivot.  As strtol reads it, the whole string consumed (profiles/r07_tune_relax_pivots.txt).
    int pivots = 8;
    // FWX_PERK_WIDE / FWX_PERK_WALK / FWX_PERK_DEEP: `0`, exactly, turns off the 16-pivot sweep of an uncounted f32
    // call at the width 8 / the relax_walk kernel under it (relax_kt then) / the ladder's start at 32 with both on
    // (profiles/r19_tune_relax_pivots.txt, r23_tune_relax_pivots.txt, r25_tune_relax_pivots.txt).
    bool wide = true, walk = true, deep = true;
    // FWX_PERK_TILE_MIN_N: the smallest order whose FULL 64-pivot blocks take one relax_tile launch where the deep pass
    // would issue two 32-pivot sweeps; 0 = never.  Digits only (profiles/r26_tune_relax_tile.txt).
    int tile_min_n = 1024;
    // FWX_PERK_PAIR_MIN_N: the smallest order at which a call that takes the tile sweep applies its full blocks two or
    // more at a time behind a look-ahead chain (the pair and group schedules); 0 = never, whatever FWX_PERK_GROUP_MAX
    // says.  Digits only (profiles/r29_pair_crossover.txt).
    int pair_min_n = 5120;
    // FWX_PERK_GROUP_MAX: the most blocks per main launch of such a call, 2 ... FWX_PERK_GROUP_CAP, an odd value
    // rounded down; 2 is the pair schedule.  Digits only.  0 = the default, which goes by the order of the matrix:
    // 8 from 6144, 2 below (group_max; profiles/r30_group_crossover.txt).
    int group_max_env = 0;
    // FWX_PERK_STORE_BYTES=<16|32|64|128>: store granularity of relax_k's rates-only path (RelaxArgs::store_bytes), as
    // atoi reads it (the default: fwx_kernels.h).
    int store_bytes = FWX_PERK_STORE_BYTES_DEFAULT;
    // FWX_PERK_TEMPORAL_MIB=<MiB>: the last rows of a slab that are loaded with the default cache policy in every
    // launch, the rest of a larger slab streamed non-temporally (RelaxArgs::temporal_bytes).  As strtod reads it, empty
    // as unset: 0 = the whole slab non-temporal, a huge value = all default policy (profiles/r05_tune_relax_policy.txt).
    double temporal_mib = 256;
    // FWX_PERK_FOLD=compare, exactly: the compare form of the fold in every tile of relax_kt's uncounted f32 sweeps;
    // anything else: each wave takes the max form where its operands allow it.
    bool fold_compare = false;

    int group_max(int n) const
    {
        if (group_max_env) return group_max_env;
        return n >= FWX_PERK_GROUP_MIN_N_DEFAULT ? FWX_PERK_GROUP_CAP : 2;
    }
    long long temporal_bytes(size_t slab_bytes) const
    {
        const double b = temporal_mib * (1 << 20);
        if (!(b < (double)slab_bytes)) return -1;      // the slab fits (or NaN): all default policy
        return (long long)b;
    }
};

bool env_not_zero(const char *name)
{
    const char *e = getenv(name);
    return !(e && !strcmp(e, "0"));
}

PerkKnobs read_knobs()
{
    PerkKnobs K;
    if (const char *e = getenv("FWX_PERK_PIVOTS")) {
        char *end = nullptr;
        const long v = strtol(e, &end, 10);
        if (end != e && *end == '\0' && (v == 1 || v == 2 || v == 4 || v == 8)) K.pivots = (int)v;
    }
    K.wide = env_not_zero("FWX_PERK_WIDE");
    K.walk = env_not_zero("FWX_PERK_WALK");
    K.deep = env_not_zero("FWX_PERK_DEEP");
    K.tile_min_n = (int)env_digits("FWX_PERK_TILE_MIN_N", 0, INT_MAX, K.tile_min_n);
    K.pair_min_n = (int)env_digits("FWX_PERK_PAIR_MIN_N", 0, INT_MAX, K.pair_min_n);
    K.group_max_env = (int)env_digits("FWX_PERK_GROUP_MAX", 2, FWX_PERK_GROUP_CAP, 0) & ~1;
    if (const char *e = getenv("FWX_PERK_STORE_BYTES")) {
        const int b = atoi(e);
        if (b == 16 || b == 32 || b == 64 || b == 128) K.store_bytes = b;
    }
    if (const char *e = getenv("FWX_PERK_TEMPORAL_MIB"))
        if (*e) K.temporal_mib = std::max(0.0, strtod(e, nullptr));
    const char *fold = getenv("FWX_PERK_FOLD");
    K.fold_compare = fold && !strcmp(fold, "compare");
    return K;
}

// The size of the next group: `left` full blocks are still to be applied, the group before had `prev` blocks (0: this
// is the call's first group), at most `gmax` blocks per group.  The rule: the chain that prepares a group of G blocks
// beside the main launch of the group before, P blocks, should end before that launch does.  At n = 16384 a main
// launch spends about 570 us per block of P and the chain 180 to 380 us per block of G (profiles/r30_group_chain.txt),
// so G <= 2 * P; only the chain of an 8-block group ends behind the 4-block launch beside it, and ships all the same
// (profiles/r30_group_crossover.txt).  Nothing runs beside the work in front of the first
// main launch, so the first group is a pair.  A single block that is left is the odd last block.
int perk_group_size(int left, int prev, int gmax)
{
    if (left < 2) return left > 0 ? 1 : 0;
    return std::min(std::min(prev > 0 ? 2 * prev : 2, gmax), left & ~1);
}

// ---- the tally ---------------------------------------------------------------------------------------------------
// Launches of the multi-pivot schedule in this process, relaxed host atomics, as the hooks report them (fwx.h):
// fwx_test_perk_pivots the five from PK_SINGLE -- relax_k (ragged single pivots), relax_kt with 2 / 4 / 8 pivots, panel
// launches --, _wide / _deep / _tile / _pair the launches of 16 / 32 / 64 / 128 pivots, _group the main launches of 2,
// 4, 6 and 8 blocks.  A wider launch counts in proportion in every narrower counter, so that each reads the same
// whichever switches are on; a cross launch of a look-ahead chain counts nowhere: each entry still sees every pivot
// once in these counts.
enum PerkSlot { PK_SINGLE, PK_2, PK_4, PK_8, PK_PANEL, PK_WIDE, PK_DEEP, PK_TILE, PK_PAIR, PK_GROUP,
                PK_COUNT = PK_GROUP + FWX_PERK_GROUP_CAP / 2 };
std::atomic<uint64_t> g_perk_tally[PK_COUNT];

// One launch that applies `groups` times what a launch of `slot` applies: a 16-pivot sweep is 2 in PK_8 and 1 in
// PK_WIDE, a main launch of G blocks 8 G / 4 G / 2 G / G / G / 2 from PK_8 to PK_PAIR and 1 in PK_GROUP + G / 2 - 1.
void perk_count(int slot, int groups)
{
    auto add = [](int i, int v) { g_perk_tally[i].fetch_add((uint64_t)v, std::memory_order_relaxed); };
    add(slot, groups);
    if (groups >= 2) add(PK_WIDE, groups / 2);
    if (groups >= 4) add(PK_DEEP, groups / 4);
    if (groups >= 8) add(PK_TILE, groups / 8);
    if (groups >= 16) { add(PK_PAIR, groups / 16); add(PK_GROUP + groups / 16 - 1, 1); }
}

void read_tally(int first, int count, uint64_t *out, int reset)
{
    for (int i = 0; i < count; ++i) {
        std::atomic<uint64_t> &c = g_perk_tally[first + i];
        const uint64_t v = reset ? c.exchange(0, std::memory_order_relaxed) : c.load(std::memory_order_relaxed);
        if (out) out[i] = v;
    }
}

// ---- the pool of snapshot panels -----------------------------------------------------------------------------------
// A blocking entry point that holds a per-call context passes that context's workspace (PerkRange::kt_ws).
// fwx_dev_relax* has no workspace argument and returns with its launches queued, so there the panels live in a
// process-wide pool keyed by the stream (whose device is the stream's, not the caller's current one): launches that
// read a buffer and the panel launch that next rewrites it are then always on ONE stream, in order, and two streams
// never share a buffer.  A buffer is allocated by the first call on its stream and kept; only a call that needs a
// larger one waits for that stream, frees and allocates again.  The pool keeps at most kMax buffers: one more evicts
// the least recently used with hipFree, which waits for the device and so for any launch that may still read it.  The
// pool mutex is held across those (rare) allocations.  Nothing is synchronised on the way out.
// The pair schedule keeps more in the stream's entry: 2 * gmax panel sets instead of one, and a look-ahead stream
// (non-blocking: it orders itself against the caller's stream, the null stream included, through the events alone)
// with its two events, made by the first such call on the stream and destroyed with the entry.  Every call makes the
// caller's stream wait for the look-ahead stream before it returns, so the buffer's only readers are still this
// stream's launches.
// An entry is IN USE from the `get` of a call to that call's return (PerkLease, error returns included): the call
// goes on queueing launches that read the buffer long after `get` has dropped the mutex, and hipFree waits only for
// what is queued already.  An entry in use is never evicted; the victim is the least recently used IDLE entry.  With
// every entry in use the pool exceeds kMax for the moment; a later `get` that adds an entry evicts idle ones until
// kMax are kept again.
struct PerkSide {
    hipStream_t s = nullptr;
    hipEvent_t main_done = nullptr, chain_done = nullptr;
};
// The victim rule over the entries' stamps and in-use marks: the index of the least recently used idle entry of a
// pool that holds `cap` entries or more, -1 if the pool is below `cap` or every entry is in use (fwx_test_perk_scratch_victim).
int perk_scratch_victim(const uint64_t *used, const int *busy, int count, int cap)
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

// ---- the multi-pivot schedule --------------------------------------------------------------------------------------
// For a rates-only solve of the whole matrix in place (relax_range, below, decides).  Per block of <= 64 pivots: ONE
// panel launch (fused_panels, compare form: W and Ct of the block from the time-k0 matrix, which it does not modify),
// then the block's pivots K.pivots at a time, one relax_kt launch each, all on `s`.  A ragged end of a block goes down
// the powers of two; a last single pivot is a relax_k launch on the live row -- exact, because between launches the
// matrix is a consistent time-k state.
// An uncounted f32 call at the width 8 starts the ladder at 16 (K.wide: the panels hold the snapshots of all 64
// pivots of the block), with the walk on as well at 32 (K.deep); a FULL block of such a call at n >= K.tile_min_n
// takes one relax_tile launch instead, and from n >= K.pair_min_n the call applies its full blocks two or more at a
// time behind a look-ahead chain on a second stream (the group schedule, below); when it returns, `s` waits for
// everything it queued there.
template <typename T>
int relax_range_kt(const PerkRange<T> &r, const PerkKnobs &K)
{
    constexpr int Bq = FWX_FUSED_B;
    T *const rate = r.rate;
    const int n = r.n, k_begin = r.k_begin, k_end = r.k_end, serpentine = r.serpentine, np = K.pivots;
    unsigned long long *const d_updates = r.d_updates;
    const hipStream_t s = r.stream;
    void *ws = r.kt_ws;                            // null: the stream's entry of PerkScratch
    const size_t ld = ((size_t)n + 3) & ~(size_t)3;
    const bool wide = np == 8 && !d_updates && std::is_same<T, float>::value && K.wide;
    const int g_top = wide ? (K.walk && K.deep ? 32 : 16) : np;
    // a full block where the ladder would start at 32: one tile sweep instead of the two 32-pivot sweeps
    const bool tile = g_top == 32 && K.tile_min_n > 0 && n >= K.tile_min_n && n >= Bq;
    // The pair schedule: the stream's own scratch entry only, since a caller's workspace holds one panel set and no
    // look-ahead stream.
    const int k_a = (k_begin + 2 * Bq - 1) / (2 * Bq) * (2 * Bq);     // the first group starts on a tile boundary
    bool pair = tile && !ws && K.pair_min_n > 0 && n >= K.pair_min_n && k_begin % Bq == 0 && k_end - k_a >= 4 * Bq;
    if (pair) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cap) != hipSuccess) {            // (a null stream beside a global capture)
            (void)hipGetLastError();
            pair = false;
        } else if (cap != hipStreamCaptureStatusNone) {
            pair = false;                                             // a captured graph gets no parallel branches
        }
    }
    // The group schedule: at most gmax blocks per main launch; 2 is the pair schedule itself.
    const int gmax = pair ? K.group_max(n) : 1;
    const int sets = pair ? 2 * gmax : 1;
    PerkSide side;
    PerkLease lease;                               // the stream's entry stays in use until this call returns
    if (!ws) {
        const int rc0 = PerkScratch::get(s, (size_t)sets * perk_kt_ws_bytes<T>(n), &ws, pair ? &side : nullptr, lease);
        if (rc0) return rc0;
    }
    // `sets` panel sets: the W rows of all sets, then the Ct lines of all sets.  The group schedule keeps two halves of
    // gmax sets each, block i of group g in set (g & 1) * gmax + i, so that the panels of a group are contiguous rows of
    // W and lines of Ct whatever its size and no group wraps; with gmax 2 that is "block q in set q & 3".
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
    a.temporal_bytes = K.temporal_bytes((size_t)n * n * sizeof(T));
    a.store_bytes = K.store_bytes;
    a.fold_compare = K.fold_compare;
    a.walk = K.walk;
    fwx::RelaxArgs<T> a1;
    a1.rate = rate; a1.next = nullptr; a1.hops = nullptr; a1.phops = nullptr; a1.rows = n; a1.n = n; a1.row0 = 0;
    a1.updates = d_updates; a1.temporal_bytes = a.temporal_bytes; a1.store_bytes = a.store_bytes;
    const int rev = FWX_XCD_SERPENTINE && a.temporal_bytes >= 0 ? 2 : 1;
    Throttle thr;
    int sweeps = 0;                                // launches alternate direction, whatever their width
    auto after = [&](hipError_t e, int slot, int groups = 1) -> int {
        if (e == hipErrorInvalidValue) return FWX_ERR_INVALID;
        FWX_HIP(e);
        if (slot >= 0) perk_count(slot, groups);   // (a cross launch of the group schedule counts nowhere)
        return thr.tick(s);
    };
    // both panels of the block at k0 (bt pivots) into the set in use, from the matrix as `st` finds it
    auto panels = [&](int k0, int bt, hipStream_t st) -> int {
        pa.k0 = k0; pa.bt = bt; pa.ct = ct; pa.side = st != s;
        return after(fwx::launch_fused_panels<T>(pa, w, nullptr, st), PK_PANEL);
    };
    // pivots [k0, k0 + bt) in one relax_tile launch, the panels from the set in use and the bt / 64 - 1 sets behind it
    auto tiles = [&](int k0, int bt, hipStream_t st, fwx::TileSel sel, int tx, int tw, int te) -> int {
        if constexpr (std::is_same<T, float>::value) {
            a.k = k0; a.np = bt; a.w = w; a.ct = ct;
            a.flip = 0;                            // not read: a tile is loaded and stored once, in any order
            return after(fwx::launch_relax_tile(a, st, sel, tx, tw, te), sel == fwx::TILES_CROSS ? -1 : PK_8, bt / 8);
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
                    if (const int rc = after(fwx::launch_relax_kt<T>(a, s), g >= 8 ? PK_8 : g == 4 ? PK_4 : PK_2,
                                             g >= 16 ? g / 8 : 1))
                        return rc;
                }
        }
        for (; t < bt; ++t) {
            a1.k = k0 + t; a1.prow = rate + (size_t)a1.k * n;
            a1.flip = serpentine ? rev * (sweeps++ & 1) : 0;
            if (const int rc = after(fwx::launch_relax<T>(a1, s), PK_SINGLE)) return rc;
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

}  // namespace

namespace fwxi {

template <typename T>
int relax_range(const PerkRange<T> &r)
{
    const PerkKnobs K = read_knobs();
    if (K.pivots > 1 && !r.next && !r.hops && !r.plog.last && r.row0 == 0 && r.rows == r.n && r.skip_hi <= r.skip_lo &&
        r.n % (16 / (int)sizeof(T)) == 0 && (uintptr_t)r.rate % 16 == 0 && r.stride == r.n &&
        r.prow0 == r.rate + (size_t)r.k_begin * r.n && r.k_end - r.k_begin >= 2)
        return relax_range_kt<T>(r, K);
    fwx::RelaxArgs<T> a;
    Throttle thr;
    a.rate = r.rate; a.next = r.next; a.hops = r.hops;
    a.rows = r.rows; a.n = r.n; a.row0 = r.row0; a.updates = r.d_updates; a.plog = r.plog;
    a.skip_lo = r.skip_lo; a.skip_hi = r.skip_hi;
    a.temporal_bytes = K.temporal_bytes((size_t)r.rows * r.n * sizeof(T));
    a.store_bytes = K.store_bytes;
    // serpentine: reversed in groups of 8 (tiles keep their XCD) where the split applies -- the regime
    // it was measured in (profiles/r05_tune_relax_policy.txt) -- tile by tile otherwise
    const int rev = FWX_XCD_SERPENTINE && a.temporal_bytes >= 0 ? 2 : 1;
    for (int k = r.k_begin; k < r.k_end; ++k) {
        const int64_t off = (int64_t)(k - r.k_begin) * r.stride;
        a.prow = r.prow0 + off;
        a.phops = r.phops0 ? r.phops0 + off : nullptr;
        a.pnext = r.pnext0 ? r.pnext0 + off : nullptr;
        a.k = k;
        a.flip = r.serpentine ? rev * (k & 1) : 0;
        const hipError_t e = fwx::launch_relax<T>(a, r.stream);
        if (e == hipErrorInvalidValue) return FWX_ERR_INVALID;   // misaligned skip range
        FWX_HIP(e);
        if (const int rc = thr.tick(r.stream)) return rc;
    }
    return FWX_OK;
}
template int relax_range<float>(const PerkRange<float> &);
template int relax_range<double>(const PerkRange<double> &);

}  // namespace fwxi

extern "C" {

int fwx_test_perk_pivots(uint64_t *launches, int reset)
{
    read_tally(PK_SINGLE, 5, launches, reset);
    return read_knobs().pivots;
}

int fwx_test_perk_wide(uint64_t *wide_launches, int reset)
{
    read_tally(PK_WIDE, 1, wide_launches, reset);
    return read_knobs().wide ? 1 : 0;
}

int fwx_test_perk_fold(void) { return read_knobs().fold_compare ? 1 : 0; }

int fwx_test_perk_walk(void) { return read_knobs().walk ? 1 : 0; }

int fwx_test_perk_deep(uint64_t *deep_launches, int reset)
{
    read_tally(PK_DEEP, 1, deep_launches, reset);
    return read_knobs().deep ? 1 : 0;
}

int fwx_test_perk_tile(uint64_t *launches, int reset)
{
    read_tally(PK_TILE, 1, launches, reset);
    return read_knobs().tile_min_n;
}

int fwx_test_perk_pair(uint64_t *launches, int reset)
{
    read_tally(PK_PAIR, 1, launches, reset);
    return read_knobs().pair_min_n;
}

int fwx_test_perk_group(uint64_t *launches, int reset)
{
    read_tally(PK_GROUP, FWX_PERK_GROUP_CAP / 2, launches, reset);
    return read_knobs().group_max_env;
}

int fwx_test_perk_group_plan(int n, int nfull, int gmax, int *size, int *set, int cap)
{
    if (gmax == 0) gmax = read_knobs().group_max(n);
    if (nfull < 0 || gmax < 2 || gmax > FWX_PERK_GROUP_CAP || (gmax & 1) || cap < 0) return -1;
    int g = 0;
    for (int q = 0, sz = perk_group_size(nfull, 0, gmax); sz > 0; q += sz, sz = perk_group_size(nfull - q, sz, gmax), ++g)
        if (g < cap) {
            if (size) size[g] = sz;
            if (set) set[g] = (g & 1) * gmax;
        }
    return g;
}

int fwx_test_perk_scratch_victim(const uint64_t *used, const int *busy, int count, int cap)
{
    if (count < 0 || cap < 0 || (count > 0 && (!used || !busy))) return -2;
    return perk_scratch_victim(used, busy, count, cap);
}

}  // extern "C"
