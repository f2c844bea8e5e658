// evaluate(), contraction models: the int8 matrix-core screening pass, the exact recheck of its undecided pairs, the merge
// (kge_rank_screen.h: limbs, thresholds, rank_screen_kernel_v1, rank_recheck_kernel; kge_rank_screen_r.h: rank_screen_kernel_r).
#include "kge_rank_screen.h"
#include "kge_rank_screen_r.h"

namespace kge {

constexpr int SCREEN_KERNEL_DEFAULT = 4;   // (see run_screen: rank_screen_kernel_r where it applies -- rows of 4 .. 13 slabs --, rank_screen_kernel_v1 elsewhere)

// the screening sequence of one rank_counts call (see kge_rank_screen.h); counts of decided + rechecked pairs are merged into
// d_counts unless the recheck list overflowed (flag at counter[1]: the guarded exact kernel then produces them)
int run_screen(const amdkge_model* m, const float* d_ent, const int32_t* d_ent_ids, int64_t ent_lo, int64_t mcand, int64_t n,
               const RankGeom& g, const Workspace& w, const ModelConst& mc, int32_t* d_counts, void* d_screen, size_t screen_bytes,
               hipStream_t st) {
    ScreenBufs b = carve_screen(d_screen, screen_bytes, n, mcand, g.U);
    const float sgn_scale = mc.score_sign * mc.score_scale;
    if (hipError_t e = hipMemsetAsync(b.counter, 0, (size_t)screen_layout(n, mcand, g.U).qlimbs, st)) return set_error_hip(e, "hipMemsetAsync(screen counters)");
    const double u = ldexp(1.0, -24), gam = u * (1.0 + 2.0 * (double)g.U * u);   // x |W q|_2 |W e|_2: the chain's rounding bound
    hipLaunchKernelGGL(rank_limbs_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, w.Q, (int64_t)g.QW, (const int32_t*)nullptr, (int64_t)0, n, g.U, b.S,
                       (float)(gam * (1.0 + 1e-6)), b.qlimbs, b.qm, (const int*)nullptr);
    if (int rc = check_launch("rank_limbs(Q)")) return rc;
    // Which screening kernel: rank_screen_kernel_r (round 6, kge_rank_screen_r.h: one wave per SIMD, the query limbs resident in registers,
    // candidates on one scale per tile of 64) for rows of 4 .. 13 slabs -- 97 .. 416 int8 units: ComplEx k = 50 .. 208, DistMult k = 97 .. 416 (BASELINE's ComplEx k = 200 and
    // DistMult k = 400 are 13-slab rows; the reference's published DistMult k = 350 is 11) --,
    // rank_screen_kernel_v1 (rounds 3 - 5: query fragments L2 -> registers, entity slab register-staged through LDS) for every other width
    // and behind kernel r for wild tables.  The same counts either way; AMDKGE_SCREEN_KERNEL=1 pins v1 for A/B runs (read once).  The
    // variants that measured slower or no faster live in scripts/experiments/: round 5's register-staged LDS form, round 6's LDS-DMA
    // ring for both operands (g) and the paired-wave split of the limb products (p).
    static const int screen_kernel_env = [] { const char* ev = getenv("AMDKGE_SCREEN_KERNEL"); const int v = ev ? atoi(ev) : 0; return (v == 1 || v == 4) ? v : SCREEN_KERNEL_DEFAULT; }();
    int screen_kernel = screen_kernel_env;
    if (screen_kernel == 4 && (b.S < 4 || b.S > 13 || b.cap * 8 < mcand * 16)) screen_kernel = 1;   // (the instantiated widths; room for the row records)
    if (screen_kernel == 4) {
        // (the row records of the first pass live in the head of the pair list, unused until the screening kernel)
        float4* const stats = reinterpret_cast<float4*>(b.pairs);
        hipLaunchKernelGGL(rank_rowstats_kernel, dim3((unsigned)((mcand + 3) / 4)), dim3(256), 0, st, d_ent, (int64_t)g.K, d_ent_ids, ent_lo, mcand, g.U, stats);
        if (int rc = check_launch("rank_rowstats(E)")) return rc;
        hipLaunchKernelGGL(rank_limbs_tile_kernel, dim3((unsigned)(16 * ((mcand + 63) / 64))), dim3(256), 0, st, d_ent, (int64_t)g.K, d_ent_ids, ent_lo, mcand, g.U, b.S,
                           (const float4*)stats, b.elimbs, b.em, b.tm, b.counter);
        if (int rc = check_launch("rank_limbs_tile(E)")) return rc;
        // (a wild table -- see screen_wild -- is redone on per-row scales for rank_screen_kernel_v1; otherwise this launch returns at once)
        hipLaunchKernelGGL(rank_limbs_kernel, dim3((unsigned)std::min<int64_t>((mcand + 3) / 4, 512)), dim3(256), 0, st, d_ent, (int64_t)g.K, d_ent_ids, ent_lo, mcand, g.U, b.S, 1.f,
                           b.elimbs, b.em, (const int*)b.counter);
    } else
        hipLaunchKernelGGL(rank_limbs_kernel, dim3((unsigned)((mcand + 3) / 4)), dim3(256), 0, st, d_ent, (int64_t)g.K, d_ent_ids, ent_lo, mcand, g.U, b.S, 1.f,
                           b.elimbs, b.em, (const int*)nullptr);
    if (int rc = check_launch("rank_limbs(E)")) return rc;
    hipLaunchKernelGGL(rank_thresholds_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w.qpos, n, sgn_scale, b.qt);
    if (int rc = check_launch("rank_thresholds")) return rc;
    ScreenArgs sa{};
    sa.b = b; sa.n = n; sa.m = mcand; sa.U = g.U;
    // per unit: the three dropped limb products (2^23 + 2^14) and the cross term of the two fixed-point roundings (1/4), in units of
    // A B; + 2^25: the fp32 reconstruction of the 40-bit integer sum in the epilogue (inner sum rounds by <= 2^8 in units of 2^16 A B)
    // ... + the fp32 rebuild of f = L0 2^16 + L1 2^8 + L2 in the epilogue, in units of f: |L1| <= U 2^15 and |L2| <= 3 U 2^14 exceed
    // 2^24 for U > 512, so their conversions round too (half an ulp: <= 2 resp. 4 for U <= 2048, the first times 2^8), and the
    // inner fma rounds at up to 2^34 (half an ulp: 2^10): 2^9 + 4 + 2^10 < 2^11, i.e. 2^27 A B (the screening condition holds
    // U <= 2048; the outer fma's rounding is relative to |f| and sits in the thresholds)
    sa.drop = (float)(((double)g.U * (8388608.0 + 16384.0 + 0.25) + 134217728.0) * (1.0 + 1e-6));
    const int64_t qtiles = (n + SCR_Q - 1) / SCR_Q, etiles = (mcand + SCR_ET - 1) / SCR_ET;
    // Each block takes a run of entity tiles of one 128-query block.  The run length is the one with the shortest schedule: rounds of
    // `slots` co-resident blocks x (tiles + a block's start-up in tile-times) -- v1 / g: two workgroups per CU, ~0.35 (at C2, 160 x 227
    // tiles, runs of 4 give 18 rounds of 4: 78 tile-times instead of 84 with runs of 9); r: one per CU, and its 39 KB of query limbs come
    // first (~1 tile-time).
    static const int64_t run_cap = [] { const char* ev = getenv("AMDKGE_SCREEN_RUN"); const int v = ev ? atoi(ev) : 0; return (int64_t)(v > 0 ? v : 64); }();   // (A/B runs: longest run of tiles per block)
    auto schedule = [&](ScreenArgs& x, int64_t slots, double startup, int64_t max_run, int64_t& nblk) -> bool {
        int64_t tiles_per = 1;
        const int64_t qt8 = 8 * ((qtiles + 7) / 8), lim = std::min(etiles < run_cap ? etiles : run_cap, max_run);
        double best = 1e300;
        for (int64_t tp = 1; tp <= lim; ++tp) {
            const int64_t blocks = qt8 * ((etiles + tp - 1) / tp);
            const double cost = (double)((blocks + slots - 1) / slots) * ((double)tp + startup);
            if (cost <= best) { best = cost; tiles_per = tp; }   // (ties: the longer run)
        }
        // very large problems: keep the launch below 2^31 blocks and a lane's 16-bit counters (2 candidates per tile) in range
        while (tiles_per < etiles && tiles_per < max_run && qt8 * ((etiles + tiles_per - 1) / tiles_per) > (1ll << 24)) tiles_per *= 2;
        if (tiles_per > max_run) tiles_per = max_run;
        if (tiles_per > etiles) tiles_per = etiles;
        if (tiles_per < 1) tiles_per = 1;
        const int64_t splits = (etiles + tiles_per - 1) / tiles_per;
        x.ent_per_block = (int)(tiles_per * SCR_ET); x.qtiles = (int)qtiles; x.splits = (int)splits;
        nblk = qt8 * splits;
        return nblk <= 0x7FFFFFFFll;
    };
    static PerDeviceOnce v1_attr, v1_wild_attr, r_attr;
    if (int rc = ensure_dynamic_lds(v1_attr, {(const void*)rank_screen_kernel_v1}, SCR_LDS_BYTES, "rank_screen_v1")) return rc;
    if (int rc = ensure_dynamic_lds(v1_wild_attr, {(const void*)rank_screen_kernel_v1_wild}, SCR_LDS_BYTES, "rank_screen_v1_wild")) return rc;
    if (int rc = ensure_dynamic_lds(r_attr, {(const void*)rank_screen_kernel_r<13>, (const void*)rank_screen_kernel_r<12>, (const void*)rank_screen_kernel_r<11>, (const void*)rank_screen_kernel_r<10>,
                                             (const void*)rank_screen_kernel_r<9>, (const void*)rank_screen_kernel_r<8>, (const void*)rank_screen_kernel_r<7>, (const void*)rank_screen_kernel_r<6>,
                                             (const void*)rank_screen_kernel_r<5>, (const void*)rank_screen_kernel_r<4>}, SCRR_LDS_BYTES, "rank_screen_r")) return rc;
    int64_t nblk = 0;
    if (screen_kernel == 4) {
        ScreenArgs sr = sa;
        sr.wild_mode = 2;
        if (!schedule(sr, 256, 1.0, SCRR_TMCAP, nblk)) return set_error(AMDKGE_EUNSUPPORTED, "rank_counts: too many tiles for one launch");
        switch (b.S) {
#define KGE_SCR_R(N) case N: hipLaunchKernelGGL(rank_screen_kernel_r<N>, dim3((unsigned)nblk), dim3(SCR_THREADS), SCRR_LDS_BYTES, st, sr); break
            KGE_SCR_R(13); KGE_SCR_R(12); KGE_SCR_R(11); KGE_SCR_R(10); KGE_SCR_R(9); KGE_SCR_R(8); KGE_SCR_R(7); KGE_SCR_R(6); KGE_SCR_R(5);
            default: hipLaunchKernelGGL(rank_screen_kernel_r<4>, dim3((unsigned)nblk), dim3(SCR_THREADS), SCRR_LDS_BYTES, st, sr); break;
#undef KGE_SCR_R
        }
        if (int rc = check_launch("rank_screen_r")) return rc;
    }
    if (!schedule(sa, 512, 0.35, 16384, nblk)) return set_error(AMDKGE_EUNSUPPORTED, "rank_counts: too many tiles for one launch");
    sa.nblk = (int)nblk;
    if (screen_kernel == 4)   // (the per-row-scale kernel behind rank_screen_kernel_r: a wild table only)
        hipLaunchKernelGGL(rank_screen_kernel_v1_wild, dim3((unsigned)std::min<int64_t>(nblk, 512)), dim3(SCR_THREADS), SCR_LDS_BYTES, st, sa);
    else hipLaunchKernelGGL(rank_screen_kernel_v1, dim3((unsigned)nblk), dim3(SCR_THREADS), SCR_LDS_BYTES, st, sa);
    if (int rc = check_launch("rank_screen")) return rc;
    RecheckArgs ra{};
    ra.ent = d_ent; ra.Q = w.Q; ra.qpos = w.qpos; ra.ent_ids = d_ent_ids; ra.ent_lo = ent_lo; ra.U = g.U; ra.K = g.K; ra.QW = g.QW;
    ra.sgn_scale = sgn_scale; ra.b = b;
    static PerDeviceOnce rck_attr;
    if (int rc = ensure_dynamic_lds(rck_attr, {(const void*)rank_recheck_kernel<false>}, RCK_LDS_BYTES, "rank_recheck")) return rc;
    hipLaunchKernelGGL(rank_recheck_kernel<false>, dim3(1024), dim3(256), RCK_LDS_BYTES, st, ra);
    if (int rc = check_launch("rank_recheck")) return rc;
    hipLaunchKernelGGL(rank_screen_merge_kernel, dim3((unsigned)((2 * n + 255) / 256)), dim3(256), 0, st, b, n, d_counts);
    return check_launch("rank_screen_merge");
}

// the filter pass's pair list (kge_rank_filter.hip: filter_pairs_kernel) through the same exact chain
int launch_recheck_filter(const RecheckArgs& ra, unsigned nblk, hipStream_t st) {
    static PerDeviceOnce flt_attr;
    if (int rc = ensure_dynamic_lds(flt_attr, {(const void*)rank_recheck_kernel<true>}, RCK_LDS_BYTES, "rank_recheck<filter>")) return rc;
    hipLaunchKernelGGL(rank_recheck_kernel<true>, dim3(nblk), dim3(256), RCK_LDS_BYTES, st, ra);
    return check_launch("rank_filter_pairs");
}

}  // namespace kge
