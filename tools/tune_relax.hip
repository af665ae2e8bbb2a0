// tune_relax.hip -- standalone sweep of relax_k launch configurations on one MI355X.
// Development tool (not part of libfwx): includes the kernel source directly so that every
// (NV, RPB, UNROLL) instantiation is available.  Build + run:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Iinclude \
//         -Ifloydwarshall_amd/csrc tools/tune_relax.hip -o gpurun_out/tune_relax && gpurun_out/tune_relax
#include "../floydwarshall_amd/csrc/fwx_kernels.hip"
#include "../floydwarshall_amd/csrc/fwx_fused.hip"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__, __LINE__); exit(1); } } while (0)

__global__ void fill_uniform(float *a, size_t n2, int n, unsigned seed)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n2; i += stride) {
        unsigned x = (unsigned)(i * 2654435761u) ^ seed;
        x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
        float u = (x >> 8) * (1.0f / 16777216.0f);
        a[i] = (i / n == i % n) ? 0.0f : 1.0f - u * 0.95f;
    }
}

struct Cfg { const char *name; hipError_t (*fn)(const fwx::RelaxArgs<float> &, hipStream_t); };

template <int NV, int RPB, int UNROLL, int MINW = 1>
static hipError_t run_cfg(const fwx::RelaxArgs<float> &a, hipStream_t s)
{
    return fwx::launch_relax_cfg<float, 4, NV, RPB, UNROLL, MINW>(a, s);
}

// `policy` mode: the production geometry (fwx::launch_relax) under every combination of temporal-tail
// budget (RelaxArgs::temporal_bytes: the slab's last rows that keep default-policy loads) and sweep order (flip 0 = plain stream, 1 = serpentine,
// 2 = serpentine reversed in groups of 8 so tiles keep their XCD), interleaved round by round in one
// process.  Run once per warm-up (early / late pivots):
//   tune_relax 16384 1024 32 8 policy      tune_relax 16384 9000 32 8 policy
static int policy_sweep(float *d, int n, int warm, int per, int rounds)
{
    const long long budgets[] = {-1, 0, 128, 160, 192, 224, 240, 256, 288};   // MiB; -1 = all default policy
    const int nb = sizeof(budgets) / sizeof(budgets[0]), modes = 3;
    fwx::RelaxArgs<float> a;
    a.rate = d; a.next = nullptr; a.hops = nullptr; a.phops = nullptr;
    a.rows = n; a.n = n; a.row0 = 0; a.updates = nullptr;
    int k = 0;
    auto step = [&](long long mib, int mode) {
        a.k = k % n; a.prow = d + (size_t)a.k * n; a.flip = (k & 1) * mode;
        a.temporal_bytes = mib < 0 ? -1 : mib << 20;
        CK(fwx::launch_relax<float>(a, 0));
        ++k;
    };
    for (int i = 0; i < warm; ++i) step(-1, 1);
    CK(hipDeviceSynchronize());
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<float> best(nb * modes, 1e30f), sum(nb * modes, 0.f);
    for (int r = 0; r < rounds; ++r)
        for (int b = 0; b < nb; ++b)
            for (int m = 0; m < modes; ++m) {
                step(budgets[b], m);   // first launch after a switch: not timed
                CK(hipEventRecord(e0, 0));
                for (int i = 0; i < per; ++i) step(budgets[b], m);
                CK(hipEventRecord(e1, 0));
                CK(hipEventSynchronize(e1));
                float ms; CK(hipEventElapsedTime(&ms, e0, e1));
                const float us = 1e3f * ms / per;
                best[b * modes + m] = std::min(best[b * modes + m], us);
                sum[b * modes + m] += us;
            }
    printf("policy n=%d warm=%d per=%d rounds=%d  (us/launch min | mean over rounds; pivots %d..%d)\n", n, warm,
           per, rounds, warm % n, k % n);
    printf("%-12s  %-21s  %-21s  %-21s\n", "tail MiB", "plain (flip 0)", "serpentine (flip 1)", "serp XCD (flip 2)");
    for (int b = 0; b < nb; ++b) {
        char name[32];
        if (budgets[b] < 0) snprintf(name, sizeof name, "all default"); else snprintf(name, sizeof name, "%lld", budgets[b]);
        printf("%-12s", name);
        for (int m = 0; m < modes; ++m)
            printf("  %7.1f | %7.1f    ", best[b * modes + m], sum[b * modes + m] / rounds);
        printf("\n");
    }
    return 0;
}

// `stores` mode: what relax_k's write path costs.  Every variant starts each pivot window from its own
// copy of the matrix state at the window's first pivot (the uniform D1 distribution, states made by the
// production path), runs the production geometry and sweep order with the temporal tail on (the
// default budget) and off, and is timed per window: the first `per` pivots, from k = 4096 and from
// k = 12000.  Variants (fwx::RELAX_SV_*): the legacy 16-byte store path (the parent's production), the
// same with every store suppressed (arithmetic and branch kept), the rare path compiled out, and the
// select path (wave ballot, one store per group) at G = 16 / 32 / 64 / 128 bytes, branch-free and behind
// a wave-uniform skip, and with non-temporal stores (everywhere / in the non-temporal rows only).  Results of the suppressed variants are wrong by design; the per-window update
// count U comes from a counting run of the production path.
//   tune_relax 16384 0 256 3 stores
template <int GL, int SV>
static hipError_t run_sv(const fwx::RelaxArgs<float> &a0, hipStream_t s)
{
    fwx::RelaxArgs<float> a = a0;
    a.store_bytes = GL * 16;
    return fwx::launch_relax_cfg<float, 4, 1, 4, 4, 1, SV>(a, s);
}

static int stores_sweep(float *d, int n, int per, int rounds)
{
    const std::vector<Cfg> vars = {
        {"legacy G16 (parent)", run_sv<1, fwx::RELAX_SV_LEGACY>},
        {"legacy, no stores", run_sv<1, fwx::RELAX_SV_NOSTORE>},
        {"rare path out", run_sv<1, fwx::RELAX_SV_NORARE>},
        {"select G16", run_sv<1, fwx::RELAX_SV_SELECT>},
        {"select G32", run_sv<2, fwx::RELAX_SV_SELECT>},
        {"select G64", run_sv<4, fwx::RELAX_SV_SELECT>},
        {"select G128", run_sv<8, fwx::RELAX_SV_SELECT>},
        {"skip+select G16", run_sv<1, fwx::RELAX_SV_SKIP>},
        {"skip+select G32", run_sv<2, fwx::RELAX_SV_SKIP>},
        {"skip+select G64", run_sv<4, fwx::RELAX_SV_SKIP>},
        {"skip+select G128", run_sv<8, fwx::RELAX_SV_SKIP>},
        {"select G64 nt-st", run_sv<4, fwx::RELAX_SV_NTST>},
        {"select G128 nt-st", run_sv<8, fwx::RELAX_SV_NTST>},
        {"G64 nt-st nt rows", run_sv<4, fwx::RELAX_SV_NTST_NTROWS>},
        {"G128 nt-st nt rows", run_sv<8, fwx::RELAX_SV_NTST_NTROWS>},
    };
    const int k0s[3] = {0, 4096, 12000}, nw = 3, nv = (int)vars.size();
    const size_t bytes = (size_t)n * n * sizeof(float);
    float *snap[3], *work;
    for (int w = 0; w < nw; ++w) CK(hipMalloc(&snap[w], bytes));
    CK(hipMalloc(&work, bytes));
    unsigned long long *upd;
    CK(hipMalloc(&upd, FWX_UPDATE_SHARDS_K * sizeof(unsigned long long)));
    fwx::RelaxArgs<float> a;
    a.rate = work; a.next = nullptr; a.hops = nullptr; a.phops = nullptr;
    a.rows = n; a.n = n; a.row0 = 0; a.updates = nullptr;
    const long long tb[2] = {256ll << 20, -1};   // tail on (the default 256 MiB) / off
    auto launch = [&](const Cfg &c, int k, int t) {
        a.k = k; a.prow = work + (size_t)k * n;
        a.temporal_bytes = tb[t];
        a.flip = (k & 1) * (t == 0 ? 2 : 1);   // relax_range's serpentine
        CK(c.fn(a, 0));
    };
    // window states: the production path from the pristine matrix
    const Cfg prod = {"production", fwx::launch_relax<float>};
    CK(hipMemcpy(work, d, bytes, hipMemcpyDeviceToDevice));
    for (int w = 0, k = 0; w < nw; ++w) {
        for (; k < k0s[w] && k < n; ++k) launch(prod, k, 0);
        CK(hipMemcpy(snap[w], work, bytes, hipMemcpyDeviceToDevice));
    }
    unsigned long long u[3];
    for (int w = 0; w < nw; ++w) {
        CK(hipMemcpy(work, snap[w], bytes, hipMemcpyDeviceToDevice));
        CK(hipMemset(upd, 0, FWX_UPDATE_SHARDS_K * sizeof(unsigned long long)));
        a.updates = upd;
        for (int k = k0s[w]; k < std::min(n, k0s[w] + per); ++k) launch(prod, k, 0);
        a.updates = nullptr;
        std::vector<unsigned long long> h(FWX_UPDATE_SHARDS_K);
        CK(hipMemcpy(h.data(), upd, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost));
        u[w] = 0;
        for (auto x : h) u[w] += x;
    }
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<float> best(nv * 2 * nw, 1e30f), sum(nv * 2 * nw, 0.f);
    for (int r = 0; r < rounds; ++r)
        for (int v = 0; v < nv; ++v)
            for (int t = 0; t < 2; ++t)
                for (int w = 0; w < nw; ++w) {
                    const int kb = k0s[w], ke = std::min(n, k0s[w] + per);
                    if (ke <= kb) continue;
                    CK(hipMemcpyAsync(work, snap[w], bytes, hipMemcpyDeviceToDevice, 0));
                    CK(hipEventRecord(e0, 0));
                    for (int k = kb; k < ke; ++k) launch(vars[v], k, t);
                    CK(hipEventRecord(e1, 0));
                    CK(hipEventSynchronize(e1));
                    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
                    const float us = 1e3f * ms / (ke - kb);
                    const int i = (v * 2 + t) * nw + w;
                    best[i] = std::min(best[i], us);
                    sum[i] += us;
                }
    printf("stores n=%d per=%d rounds=%d  (us/launch min | mean over rounds; windows from k = %d, %d, %d)\n", n,
           per, rounds, k0s[0], k0s[1], k0s[2]);
    printf("updates per launch (production, U / launches): %.0f  %.0f  %.0f\n", (double)u[0] / per,
           (double)u[1] / per, (double)u[2] / per);
    for (int t = 0; t < 2; ++t) {
        printf("\ntemporal tail %s\n%-20s", t == 0 ? "on (default budget)" : "off (all default policy)", "variant");
        for (int w = 0; w < nw; ++w) printf("  k=%-5d min | mean   ", k0s[w]);
        printf("\n");
        for (int v = 0; v < nv; ++v) {
            printf("%-20s", vars[v].name);
            for (int w = 0; w < nw; ++w) {
                const int i = (v * 2 + t) * nw + w;
                printf("  %7.1f | %7.1f    ", best[i], sum[i] / rounds);
            }
            printf("\n");
        }
    }
    return 0;
}

// `pivots` mode: the multi-pivot schedule of the per-k engine (relax_range_kt in fwx_perk.hip).  For NP = 1
// (relax_k, one launch per pivot) and NP = 2, 4, 8 (relax_kt, geometries RPB x UNROLL; `cmp`: the production
// geometry with the compare form of the fold forced in every tile, RelaxKtArgs::fold_compare) a window of `per`
// pivots -- from k = 0, 4096 and 12000, each started from a copy of the matrix state at its first pivot -- is
// issued as production issues it: per 64 pivots one fused_panels launch, then 64 / NP sweeps, serpentine in
// groups of 8, the default temporal tail.  Reported per window: us per pivot over the whole window (panel
// launches included) and us per sweep launch (the window minus its panel launches, which are timed on
// their own, back to back on an otherwise idle chip, and reported separately).  NP = 16 (round 19): the 16-pivot
// sweep of the non-counting f32 kernel in its candidate geometries, 64 / 16 sweeps per block.  An optional last
// argument keeps only the variants with at least that many pivots per launch (`8`: the 8- and 16-wide ones).
// NP = 32 (round 25): relax_walk with 8 bytes of a row per lane, 64 / 32 sweeps per block; a last table puts the 16-
// and 32-pivot rows on one scale, us of sweep launches per 16 pivots.
// NP = 64 (round 26): relax_tile, one sweep per block (`tile`; `tile cmp`: the compare form forced in every tile); a last
// table gives the 32- and 64-pivot rows per whole block, us per 64 pivots with the panel launch.
//   tune_relax 16384 0 256 3 pivots [min NP]
struct KtCfg { const char *name; int np; hipError_t (*fn)(const fwx::RelaxKtArgs<float> &, hipStream_t); bool cmp = false; };
template <int RPB, int UNROLL>
static hipError_t run_kt(const fwx::RelaxKtArgs<float> &a, hipStream_t s)
{
    return fwx::launch_relax_kt_cfg<float, RPB, UNROLL>(a, s);
}

template <int RPB, int UNROLL, int POL, bool ROLL>
static hipError_t run_walk(const fwx::RelaxKtArgs<float> &a, hipStream_t s)
{
    return fwx::launch_relax_walk_cfg<RPB, UNROLL, POL, ROLL>(a, s);
}

// round 25: relax_walk at 32 pivots per pass and 8 bytes of a row per lane, R rows per workgroup, U slots
template <int RPB, int UNROLL, bool ROLL = false>
static hipError_t run_deep(const fwx::RelaxKtArgs<float> &a, hipStream_t s)
{
    return fwx::launch_relax_walk_cfg<RPB, UNROLL, fwx::WALK_POL_PLAIN, ROLL, false, 32>(a, s);
}

// round 26: relax_tile, the block's 64 pivots in one pass on register tiles
static hipError_t run_tile(const fwx::RelaxKtArgs<float> &a, hipStream_t s) { return fwx::launch_relax_tile(a, s); }

static int pivots_sweep(float *d, int n, int per, int rounds, int min_np)
{
    std::vector<KtCfg> vars;
    if (min_np <= 1) vars.push_back({"NP1 relax_k", 1, nullptr});
    for (int np : {2, 4, 8}) {
        if (np < min_np) continue;
        vars.push_back({"RPB4 U4", np, run_kt<4, 4>});
        vars.push_back({"RPB8 U4", np, run_kt<8, 4>});
        vars.push_back({"RPB8 U8", np, run_kt<8, 8>});
        vars.push_back({"RPB8 U8 cmp", np, run_kt<8, 8>, true});   // the compare form forced in every tile
        vars.push_back({"RPB16 U8", np, run_kt<16, 8>});
    }
    const KtCfg state_path = {"RPB8 U8", 8, run_kt<8, 8>};        // what the window states are made with
    vars.push_back({"RPB8 U4", 16, run_kt<8, 4>});
    vars.push_back({"RPB8 U8", 16, run_kt<8, 8>});
    vars.push_back({"RPB16 U4", 16, run_kt<16, 4>});
    vars.push_back({"RPB16 U8", 16, run_kt<16, 8>});
    vars.push_back({"RPB16 U8 cmp", 16, run_kt<16, 8>, true});
    // round 23, relax_walk.  A: one body, three waves, relax_kt's batches (no walk).  wR Us pol: R rows walked, s slots
    // (8: three waves, 4: four), policy pl = plain loads, fn = chosen at the load (fenced), lp = two steady loops.
    vars.push_back({"A 16 U8 fn", 16, run_walk<16, 8, fwx::WALK_POL_FENCE, false>});
    vars.push_back({"A 16 U8 pl", 16, run_walk<16, 8, fwx::WALK_POL_PLAIN, false>});
#define FWX_TUNE_WALK(R, U)                                                                        \
    vars.push_back({"w" #R " U" #U " pl", 16, run_walk<R, U, fwx::WALK_POL_PLAIN, true>});         \
    vars.push_back({"w" #R " U" #U " fn", 16, run_walk<R, U, fwx::WALK_POL_FENCE, true>});         \
    vars.push_back({"w" #R " U" #U " lp", 16, run_walk<R, U, fwx::WALK_POL_LOOP, true>});
    FWX_TUNE_WALK(16, 8) FWX_TUNE_WALK(32, 8) FWX_TUNE_WALK(64, 8)
    FWX_TUNE_WALK(16, 4) FWX_TUNE_WALK(32, 4) FWX_TUNE_WALK(64, 4)
#undef FWX_TUNE_WALK
    vars.push_back({"w32 U8 cmp", 16, run_walk<32, 8, fwx::WALK_POL_FENCE, true>, true});
    // round 25, 32 pivots per pass: dR Us = R rows per workgroup, s slots, plain loads, batches (roll: the walk); 64 / 32
    // sweeps per block
    vars.push_back({"d32 U8", 32, run_deep<32, 8>});
    vars.push_back({"d16 U8", 32, run_deep<16, 8>});
    vars.push_back({"d32 U16", 32, run_deep<32, 16>});
    vars.push_back({"d64 U8", 32, run_deep<64, 8>});
    vars.push_back({"d128 U8", 32, run_deep<128, 8>});
    vars.push_back({"d32 U8 roll", 32, run_deep<32, 8, true>});      // slots reloaded one by one behind their folds
    vars.push_back({"d64 U8 roll", 32, run_deep<64, 8, true>});
    vars.push_back({"d32 U8 cmp", 32, run_deep<32, 8>, true});
    vars.push_back({"d64 U8 cmp", 32, run_deep<64, 8>, true});        // the production pair on an input that votes for the compare
    // round 26, 64 pivots per pass: relax_tile (fwx_fused.hip), one sweep per block; cmp: the compare form forced in
    // every tile, what an input with sign bits in every tile pays
    vars.push_back({"tile", 64, run_tile});
    vars.push_back({"tile cmp", 64, run_tile, true});
    if (min_np > 1) {
        std::vector<KtCfg> keep;
        for (const KtCfg &v : vars) if (v.np >= min_np) keep.push_back(v);
        vars.swap(keep);
    }
    const int k0s[3] = {0, 4096, 12000}, nw = 3, nv = (int)vars.size();
    if (n % 64 || per % 64) { printf("pivots mode: n and per must be multiples of 64\n"); return 1; }
    const size_t bytes = (size_t)n * n * sizeof(float);
    float *snap[3], *work, *w, *ct;
    for (int i = 0; i < nw; ++i) CK(hipMalloc(&snap[i], bytes));
    CK(hipMalloc(&work, bytes));
    CK(hipMalloc(&w, (size_t)64 * n * sizeof(float)));
    CK(hipMalloc(&ct, (size_t)64 * n * sizeof(float)));
    const long long tail = 256ll << 20;
    fwx::FusedArgs<float> pa;
    pa.rate = work; pa.next = nullptr; pa.rows = n; pa.n = n; pa.row0 = 0; pa.w = nullptr; pa.ct = ct;
    pa.cnt = nullptr; pa.ct_ld = n; pa.updates = nullptr; pa.nonneg = false;
    fwx::RelaxKtArgs<float> a;
    a.rate = work; a.ct_ld = n; a.n = n; a.temporal_bytes = tail;
    fwx::RelaxArgs<float> a1;
    a1.rate = work; a1.next = nullptr; a1.hops = nullptr; a1.phops = nullptr;
    a1.rows = n; a1.n = n; a1.row0 = 0; a1.updates = nullptr; a1.temporal_bytes = tail;
    int sweeps = 0;
    // pivots [kb, ke) with variant v; returns the number of sweep launches.  Timing only: a 64-block is
    // rounded DOWN to whole groups of np pivots (production sends a ragged end down the powers of two), so
    // the window starts and `per` must be multiples of 64 (the widest group) for the states to be the per-k states
    auto run = [&](const KtCfg &v, int kb, int ke) {
        int launches = 0;
        if (v.np == 1) {
            for (int k = kb; k < ke; ++k, ++launches) {
                a1.k = k; a1.prow = work + (size_t)k * n; a1.flip = 2 * (k & 1);
                CK(fwx::launch_relax<float>(a1, 0));
            }
            return launches;
        }
        for (int k0 = kb; k0 + v.np <= ke; k0 += 64) {
            const int bt = std::min(64, ke - k0) / v.np * v.np;
            pa.k0 = k0; pa.bt = bt;
            CK(fwx::launch_fused_panels<float>(pa, w, nullptr, 0));
            for (int t = 0; t < bt; t += v.np, ++launches) {
                a.k = k0 + t; a.np = v.np; a.w = w + (size_t)t * n; a.ct = ct + (size_t)t * n;
                a.flip = 2 * (sweeps++ & 1);
                a.fold_compare = v.cmp;
                CK(v.fn(a, 0));
            }
        }
        return launches;
    };
    // window states: the NP = 8 path from the pristine matrix (bit for bit the per-k states)
    CK(hipMemcpy(work, d, bytes, hipMemcpyDeviceToDevice));
    for (int i = 0, k = 0; i < nw; ++i) {
        if (k0s[i] > k) run(state_path, k, std::min(n, k0s[i]));
        k = std::min(n, k0s[i]);
        CK(hipMemcpy(snap[i], work, bytes, hipMemcpyDeviceToDevice));
    }
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    // the panel launch alone, per window state
    float panel_us[3] = {0, 0, 0};
    for (int i = 0; i < nw; ++i) {
        if (k0s[i] + 64 > n) continue;
        CK(hipMemcpy(work, snap[i], bytes, hipMemcpyDeviceToDevice));
        pa.k0 = k0s[i]; pa.bt = 64;
        CK(fwx::launch_fused_panels<float>(pa, w, nullptr, 0));
        CK(hipEventRecord(e0, 0));
        for (int r = 0; r < 16; ++r) CK(fwx::launch_fused_panels<float>(pa, w, nullptr, 0));
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        panel_us[i] = 1e3f * ms / 16;
    }
    std::vector<float> best(nv * nw, 1e30f), sum(nv * nw, 0.f);
    std::vector<int> nl(nv * nw, 0), npv(nv * nw, 0);
    for (int r = 0; r < rounds; ++r)
        for (int v = 0; v < nv; ++v)
            for (int i = 0; i < nw; ++i) {
                const int kb = k0s[i], ke = std::min(n, k0s[i] + per);
                if (ke - kb < 8) continue;
                CK(hipMemcpyAsync(work, snap[i], bytes, hipMemcpyDeviceToDevice, 0));
                CK(hipEventRecord(e0, 0));
                nl[v * nw + i] = run(vars[v], kb, ke);
                CK(hipEventRecord(e1, 0));
                CK(hipEventSynchronize(e1));
                float ms; CK(hipEventElapsedTime(&ms, e0, e1));
                npv[v * nw + i] = nl[v * nw + i] * vars[v].np;
                best[v * nw + i] = std::min(best[v * nw + i], 1e3f * ms);
                sum[v * nw + i] += 1e3f * ms;
            }
    printf("pivots n=%d per=%d rounds=%d  (windows from k = %d, %d, %d; min over rounds, mean in brackets)\n", n, per,
           rounds, k0s[0], k0s[1], k0s[2]);
    printf("panel launch alone (fused_panels, compare form, 64 pivots), us: %.1f  %.1f  %.1f\n", panel_us[0],
           panel_us[1], panel_us[2]);
    printf("%-4s %-12s", "NP", "geometry");
    for (int i = 0; i < nw; ++i) printf("  k=%-5d us/pivot  us/sweep launch ", k0s[i]);
    printf("\n");
    for (int v = 0; v < nv; ++v) {
        printf("%-4d %-12s", vars[v].np, vars[v].name);
        for (int i = 0; i < nw; ++i) {
            const int x = v * nw + i;
            if (!nl[x]) { printf("  %-34s", "-"); continue; }
            const float panels = vars[v].np == 1 ? 0.f : panel_us[i] * ((npv[x] + 63) / 64);
            printf("  %7.2f (%7.2f)  %7.1f         ", best[x] / npv[x], sum[x] / rounds / npv[x],
                   (best[x] - panels) / nl[x]);
        }
        printf("\n");
    }
    // round 25: the 16- and 32-pivot sweeps on one scale, us of sweep launches per 16 pivots (panels taken out)
    printf("\nsweeps per 16 pivots, us (min over rounds)\n%-4s %-12s", "NP", "geometry");
    for (int i = 0; i < nw; ++i) printf("  k=%-7d", k0s[i]);
    printf("\n");
    for (int v = 0; v < nv; ++v) {
        if (vars[v].np < 16) continue;
        printf("%-4d %-12s", vars[v].np, vars[v].name);
        for (int i = 0; i < nw; ++i) {
            const int x = v * nw + i;
            if (!nl[x]) { printf("  %-9s", "-"); continue; }
            printf("  %7.1f  ", (best[x] - panel_us[i] * ((npv[x] + 63) / 64)) / npv[x] * 16);
        }
        printf("\n");
    }
    // round 26: the 32- and 64-pivot sweeps per whole block, us per 64 pivots, the panel launch included
    printf("\nper 64 pivots with the panel launch, us (min over rounds)\n%-4s %-12s", "NP", "geometry");
    for (int i = 0; i < nw; ++i) printf("  k=%-7d", k0s[i]);
    printf("\n");
    for (int v = 0; v < nv; ++v) {
        if (vars[v].np < 32) continue;
        printf("%-4d %-12s", vars[v].np, vars[v].name);
        for (int i = 0; i < nw; ++i) {
            const int x = v * nw + i;
            if (!nl[x]) { printf("  %-9s", "-"); continue; }
            printf("  %7.1f  ", best[x] / npv[x] * 64);
        }
        printf("\n");
    }
    return 0;
}

// `crossover` mode (round 26): the default of FWX_PERK_TILE_MIN_N.  For every order m = 1024, 2048, ... up to n the
// first `per` pivots (at most m) of an m x m matrix, as production issues them: per 64 pivots one panel launch, then
// the two 32-pivot relax_walk sweeps of the deep pass, or one relax_tile sweep.  us per 64 pivots, min over rounds.
//   tune_relax 16384 0 256 5 crossover
static int tile_crossover(float *d, int n, int per, int rounds)
{
    float *work, *w, *ct;
    CK(hipMalloc(&work, (size_t)n * n * sizeof(float)));
    CK(hipMalloc(&w, (size_t)64 * n * sizeof(float)));
    CK(hipMalloc(&ct, (size_t)64 * n * sizeof(float)));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    printf("crossover per=%d rounds=%d  (us per 64 pivots with the panel launch, min over rounds)\n", per, rounds);
    printf("%-8s %-14s %-14s %s\n", "n", "2 x walk 32", "tile", "tile / pair");
    for (int m = 1024; m <= n; m *= 2) {
        const size_t bytes = (size_t)m * m * sizeof(float);
        const int ke = std::min(m, per) / 64 * 64;
        hipLaunchKernelGGL(fill_uniform, dim3(4096), dim3(256), 0, 0, d, (size_t)m * m, m, 12345u);
        fwx::FusedArgs<float> pa;
        pa.rate = work; pa.next = nullptr; pa.rows = m; pa.n = m; pa.row0 = 0; pa.w = nullptr; pa.ct = ct;
        pa.cnt = nullptr; pa.ct_ld = m; pa.updates = nullptr; pa.nonneg = false;
        fwx::RelaxKtArgs<float> a;
        a.rate = work; a.ct_ld = m; a.n = m; a.temporal_bytes = 256ll << 20; a.walk = true;
        float best[2] = {1e30f, 1e30f};
        for (int r = 0; r < rounds; ++r)
            for (int v = 0; v < 2; ++v) {
                CK(hipMemcpyAsync(work, d, bytes, hipMemcpyDeviceToDevice, 0));
                CK(hipEventRecord(e0, 0));
                for (int k0 = 0, sweeps = 0; k0 < ke; k0 += 64) {
                    pa.k0 = k0; pa.bt = 64;
                    CK(fwx::launch_fused_panels<float>(pa, w, nullptr, 0));
                    const int np = v ? 64 : 32;
                    for (int t = 0; t < 64; t += np) {
                        a.k = k0 + t; a.np = np; a.w = w + (size_t)t * m; a.ct = ct + (size_t)t * m;
                        a.flip = 2 * (sweeps++ & 1);
                        CK(v ? fwx::launch_relax_tile(a, 0) : fwx::launch_relax_kt<float>(a, 0));
                    }
                }
                CK(hipEventRecord(e1, 0));
                CK(hipEventSynchronize(e1));
                float ms; CK(hipEventElapsedTime(&ms, e0, e1));
                best[v] = std::min(best[v], 1e3f * ms / (ke / 64));
            }
        printf("%-8d %-14.1f %-14.1f %.3f\n", m, best[0], best[1], best[1] / best[0]);
    }
    return 0;
}

int main(int argc, char **argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 16384;
    const int warm = argc > 2 ? atoi(argv[2]) : 1024;
    const int per = argc > 3 ? atoi(argv[3]) : 48;
    const int rounds = argc > 4 ? atoi(argv[4]) : 3;
    const size_t n2 = (size_t)n * n;
    float *d;
    CK(hipMalloc(&d, n2 * sizeof(float)));
    hipLaunchKernelGGL(fill_uniform, dim3(4096), dim3(256), 0, 0, d, n2, n, 12345u);
    CK(hipDeviceSynchronize());

    if (argc > 5 && !strcmp(argv[5], "solve")) {
        // PMC probe mode: one full solve with the PRODUCTION launch path (fwx::launch_relax), so
        // that `rocprofv3 --pmc FETCH_SIZE|WRITE_SIZE -- build/tune_relax 16384 0 0 0 solve` sees
        // exactly the dispatches bench.py times (torch's bundled HIP runtime crashes under --pmc).
        fwx::RelaxArgs<float> a;
        a.rate = d; a.next = nullptr; a.hops = nullptr; a.phops = nullptr;
        a.rows = n; a.n = n; a.row0 = 0; a.updates = nullptr;
        hipEvent_t e0, e1;
        CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        CK(hipEventRecord(e0, 0));
        const int kmax = argc > 6 ? atoi(argv[6]) : n;      // optional: only the first kmax pivots
        const int sync_every = argc > 7 ? atoi(argv[7]) : 0; // optional: drain the queue regularly
        // optional: 2 | 4 | 8 = the multi-pivot schedule.  Timing / traffic only: kmax is rounded down to whole
        // groups of np pivots per 64-block (production sends a ragged end down the powers of two instead)
        const int np = argc > 8 ? atoi(argv[8]) : 1;
        if (np == 2 || np == 4 || np == 8) {
            float *w, *ct;
            CK(hipMalloc(&w, (size_t)64 * n * sizeof(float)));
            CK(hipMalloc(&ct, (size_t)64 * n * sizeof(float)));
            fwx::FusedArgs<float> pa;
            pa.rate = d; pa.next = nullptr; pa.rows = n; pa.n = n; pa.row0 = 0; pa.w = nullptr; pa.ct = ct;
            pa.cnt = nullptr; pa.ct_ld = n; pa.updates = nullptr; pa.nonneg = false;
            fwx::RelaxKtArgs<float> b;
            b.rate = d; b.ct_ld = n; b.n = n; b.np = np;
            for (int k0 = 0, sweeps = 0; k0 + np <= kmax; k0 += 64) {
                pa.k0 = k0; pa.bt = std::min(64, kmax - k0) / np * np;
                CK(fwx::launch_fused_panels<float>(pa, w, nullptr, 0));
                for (int t = 0; t < pa.bt; t += np) {
                    b.k = k0 + t; b.w = w + (size_t)t * n; b.ct = ct + (size_t)t * n; b.flip = sweeps++ & 1;
                    CK(fwx::launch_relax_kt<float>(b, 0));
                    if (sync_every && (k0 + t + np) % sync_every == 0) CK(hipDeviceSynchronize());
                }
            }
        } else {
            for (int k = 0; k < kmax; ++k) {
                a.k = k; a.prow = d + (size_t)k * n; a.flip = k & 1;
                CK(fwx::launch_relax<float>(a, 0));
                if (sync_every && (k + 1) % sync_every == 0) CK(hipDeviceSynchronize());
            }
        }
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        printf("solve n=%d: %.3f ms, %.1f us/launch, %.3e relax/s\n", n, ms, 1e3 * ms / n,
               (double)n * n * n / (ms * 1e-3));
        return 0;
    }

    if (argc > 5 && !strcmp(argv[5], "policy")) return policy_sweep(d, n, warm, per, rounds);
    if (argc > 5 && !strcmp(argv[5], "stores")) return stores_sweep(d, n, per, rounds);
    if (argc > 5 && !strcmp(argv[5], "crossover")) return tile_crossover(d, n, per, rounds);
    if (argc > 5 && !strcmp(argv[5], "pivots")) return pivots_sweep(d, n, per, rounds, argc > 6 ? atoi(argv[6]) : 1);

    if (argc > 5 && !strcmp(argv[5], "fused")) {
        // PMC probe mode for the fused engine: `passes` passes of 64 pivots (panel, colpanel, main
        // in max form), a device sync after every pass so that rocprofv3 --pmc survives.
        const int passes = argc > 6 ? atoi(argv[6]) : 16;
        float *w, *ct;
        CK(hipMalloc(&w, (size_t)64 * n * sizeof(float)));
        CK(hipMalloc(&ct, (size_t)64 * n * sizeof(float)));
        fwx::FusedArgs<float> a;
        a.rate = d; a.next = nullptr; a.rows = n; a.n = n; a.row0 = 0; a.w = w; a.ct = ct;
        a.cnt = nullptr; a.ct_ld = n; a.updates = nullptr; a.nonneg = true;
        hipEvent_t e0, e1;
        CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        CK(hipEventRecord(e0, 0));
        for (int p = 0; p < passes; ++p) {
            a.k0 = p * 64; a.bt = 64;
            CK(fwx::launch_fused_panel<float>(d + (size_t)a.k0 * n, n, a.k0, 64, w, 0));
            CK(fwx::launch_fused_relax<float>(a, 0));
            CK(hipDeviceSynchronize());
        }
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        printf("fused n=%d: %d passes, %.1f us/pass (synchronised after each pass)\n", n, passes,
               1e3 * ms / passes);
        return 0;
    }

    std::vector<Cfg> cfgs = {
        {"NV1 RPB8 U8", run_cfg<1, 8, 8>},        {"NV1 RPB8 U8 w2", run_cfg<1, 8, 8, 2>},
        {"NV1 RPB8 U4", run_cfg<1, 8, 4>},        {"NV1 RPB4 U4", run_cfg<1, 4, 4>},
        {"NV1 RPB8 U4 w2", run_cfg<1, 8, 4, 2>},  {"NV1 RPB16 U16", run_cfg<1, 16, 16>},
        {"NV1 RPB12 U12", run_cfg<1, 12, 12>},    {"NV1 RPB4 U4 w2", run_cfg<1, 4, 4, 2>},
        {"NV2 RPB4 U4", run_cfg<2, 4, 4>},        {"NV2 RPB8 U8", run_cfg<2, 8, 8>},
        {"NV1 RPB2 U2", run_cfg<1, 2, 2>},        {"NV1 RPB6 U6", run_cfg<1, 6, 6>},
    };

    fwx::RelaxArgs<float> a;
    a.rate = d; a.next = nullptr; a.hops = nullptr; a.phops = nullptr;
    a.rows = n; a.n = n; a.row0 = 0; a.updates = nullptr;
    int k = 0;
    auto step = [&](const Cfg &c, int serp) {
        a.k = k % n; a.prow = d + (size_t)a.k * n; a.flip = serp ? (k & 1) : 0;
        CK(c.fn(a, 0));
        ++k;
    };
    for (int i = 0; i < warm; ++i) step(cfgs[0], 1);
    CK(hipDeviceSynchronize());

    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<float> best(cfgs.size() * 2, 1e30f), sum(cfgs.size() * 2, 0.f);
    for (int r = 0; r < rounds; ++r)
        for (size_t c = 0; c < cfgs.size(); ++c)
            for (int serp = 1; serp >= 0; --serp) {
                CK(hipEventRecord(e0, 0));
                for (int i = 0; i < per; ++i) step(cfgs[c], serp);
                CK(hipEventRecord(e1, 0));
                CK(hipEventSynchronize(e1));
                float ms; CK(hipEventElapsedTime(&ms, e0, e1));
                float us = 1e3f * ms / per;
                if (us < best[c * 2 + serp]) best[c * 2 + serp] = us;
                sum[c * 2 + serp] += us;
            }
    printf("n=%d warm=%d per=%d rounds=%d  (us/launch min|mean, GB/s at min; serpentine on / off)\n", n, warm, per, rounds);
    const double bytes = (double)n2 * 4;
    for (size_t c = 0; c < cfgs.size(); ++c)
        printf("%-14s  serp: %7.1f | %7.1f us  %6.0f GB/s    noserp: %7.1f | %7.1f us  %6.0f GB/s\n", cfgs[c].name,
               best[c * 2 + 1], sum[c * 2 + 1] / rounds, bytes / best[c * 2 + 1] * 1e-3,
               best[c * 2], sum[c * 2] / rounds, bytes / best[c * 2] * 1e-3);
    return 0;
}
