// evaluate(): 1-vs-all ranking for gfx950.  Replaces AbstractScoringLayer.get_ranks
// (/root/reference/ampligraph/latent_features/layers/scoring/AbstractScoringLayer.py:156-422) and the
// five `_get_{subject,object}_corruption_scores` (TransE.py:56-114, DistMult.py:51-99,
// ComplEx.py:65-151, HolE.py:47-89, RotatE.py:107-217) without ever materialising the reference's
// (n, m, K) broadcast temporaries or the (n, m) score matrix:
//
//   rank_prep   : per test triple, the quantised positive score q(pos) and the side's "query vector"
//                 (everything of the corruption score that does not depend on the corrupting entity,
//                 rounded exactly where the reference rounds it, e.g. DistMult fl(p*o)).
//   rank_counts : validation, the choice of path and its run-length planning (here); the count kernels themselves live in one unit
//                 per family: kge_rank_tile.hip (VALU tiles, the distance models' early exit), kge_rank_mfma.hip (fp32 MFMA),
//                 kge_rank_screen.hip (int8 screening + exact recheck).  Only two int32 counters per triple leave the CU.
//   rank_filter : kge_rank_filter.hip.
//   rank_compose: tie strategy + filter subtraction + 1 (ScoringBasedEmbeddingModel.py:1684).
#include "kge_rank_common.h"

namespace kge {

RankConfig g_rank_cfg;

// ------------------------------------------------------------------------------------------------
// prep: one wave per test triple
// ------------------------------------------------------------------------------------------------
template <int MODEL>
__global__ __launch_bounds__(256) void rank_prep_kernel(const float* __restrict__ ent, const float* __restrict__ rel,
                                                        const int32_t* __restrict__ triples, int64_t n, int k, int K,
                                                        int side, int QW, ModelConst mc, float* __restrict__ Q,
                                                        int* __restrict__ qpos) {
    constexpr int NC = ModelTraits<MODEL>::NC;
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const float* rs = ent + (int64_t)triples[3 * i + 0] * K;
    const float* rp = rel + (int64_t)triples[3 * i + 1] * K;
    const float* ro = ent + (int64_t)triples[3 * i + 2] * K;
    float* q = Q + i * (int64_t)QW;
    float part = 0.f;
    for (int c = lane; c < k; c += KGE_WAVE) {
        float s[NC], p[NC], o[NC];
#pragma unroll
        for (int h = 0; h < NC; ++h) { s[h] = rs[c + h * k]; p[h] = rp[c + h * k]; o[h] = ro[c + h * k]; }
        prep_rel_exact<MODEL>(mc, p);   // RotatE: correctly rounded cos / sin (kge_device.h)
        part += score_unit<MODEL>(s, p, o);
        if constexpr (MODEL == AMDKGE_TRANSE) {
            q[c] = (side == AMDKGE_SIDE_S) ? (p[0] - o[0]) : (s[0] + p[0]);           // TransE.py:77-83,107-113
        } else if constexpr (MODEL == AMDKGE_DISTMULT) {
            q[c] = (side == AMDKGE_SIDE_S) ? (p[0] * o[0]) : (s[0] * p[0]);           // DistMult.py:71-73,96-98
        } else if constexpr (MODEL == AMDKGE_COMPLEX) {
            if (side == AMDKGE_SIDE_S) {   // ComplEx.py:93-107
                q[c] = p[0] * o[0] + p[1] * o[1];
                q[c + k] = p[0] * o[1] - p[1] * o[0];
            } else {                        // ComplEx.py:138-150
                q[c] = s[0] * p[0] - s[1] * p[1];
                q[c + k] = s[1] * p[0] + s[0] * p[1];
            }
        } else {
            if (side == AMDKGE_SIDE_S) {   // RotatE.py:151-160: needs cos, sin, o_re, o_im per unit
                q[c] = p[0]; q[c + k] = p[1]; q[c + 2 * k] = o[0]; q[c + 3 * k] = o[1];
            } else {                        // RotatE.py:209-212
                q[c] = s[0] * p[0] - s[1] * p[1];
                q[c + k] = s[0] * p[1] + s[1] * p[0];
            }
        }
    }
    const float tot = wave_sum(part);
    if (lane == 0) qpos[i] = quantise(mc.score_sign * mc.score_scale * tot);
}

__global__ void rank_compose_kernel(const int32_t* counts, const int32_t* sub, int64_t n, int strategy,
                                    int32_t* ranks, int64_t stride) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int gt = counts[2 * i], eq = counts[2 * i + 1];
    int r;
    if (strategy == AMDKGE_RANK_BEST) r = gt;                       // AbstractScoringLayer.py:221-227
    else if (strategy == AMDKGE_RANK_MIDDLE) r = gt + (eq + 1) / 2; // :232-244 ceil(#equal / 2)
    else r = gt + eq;                                               // :252-258
    if (sub) r -= sub[i];
    ranks[i * stride] = r + 1;                                      // ScoringBasedEmbeddingModel.py:1684
}

int run_prep(const amdkge_model* m, const float* d_ent, const float* d_rel, const int32_t* d_triples, int64_t n,
             int side, const RankGeom& g, const Workspace& w, hipStream_t st) {
    const ModelConst mc = model_const(m);
    const unsigned grid = (unsigned)((n + 3) / 4);
#define KGE_PREP(M) hipLaunchKernelGGL((rank_prep_kernel<M>), dim3(grid), dim3(256), 0, st, d_ent, d_rel, d_triples, n, stored_k(m), g.K, side, g.QW, mc, w.Q, w.qpos)
    KGE_MODEL_DISPATCH(m->scoring_type, KGE_PREP)
#undef KGE_PREP
    return check_launch("rank_prep");
}

static inline bool sgn_scale_positive(const ModelConst& mc) { return mc.score_sign * mc.score_scale > 0.f; }
// admission of a d_screen buffer: behind the fixed part of its walk, a pair list worth having
static inline bool holds_list(int64_t fixed, int64_t screen_bytes) { return fixed >= 0 && screen_bytes >= fixed + (1 << 16); }

}  // namespace kge

using namespace kge;

extern "C" int amdkge_set_rank_kernel(int which) {
    if (which < 0 || which > 3) return set_error(AMDKGE_EINVAL, "set_rank_kernel: 0 = automatic, 1 = VALU tile kernel, 2 = first MFMA kernel, 3 = pipelined fp32 MFMA kernel without the int8 screening pass");
    g_rank_cfg.kernel = which;
    return AMDKGE_OK;
}

extern "C" int amdkge_set_rank_early(int on, int check_l1, int check_rot, int cost, int probe) {
    g_rank_cfg.early.on = on ? 1 : 0;
    if (probe >= 0) g_rank_cfg.early.probe = probe ? 1 : 0;
    if (check_l1 > 0) g_rank_cfg.early.check_l1 = check_l1;
    if (check_rot > 0) g_rank_cfg.early.check_rot = check_rot;
    if (cost > 0) g_rank_cfg.early.cost = cost;
    return AMDKGE_OK;
}

extern "C" int amdkge_set_rank_rotate_fast(int fast) {
    g_rank_cfg.rotate_fast = fast ? 1 : 0;
    return AMDKGE_OK;
}

extern "C" int64_t amdkge_rank_workspace_bytes(const amdkge_model* m, int64_t n) {
    if (validate_model(m) != AMDKGE_OK || n < 0) return -1;
    return rank_layout(m, n).total;
}

static int rank_counts_impl(const amdkge_model* m, const float* d_ent, const float* d_rel, const int32_t* d_triples,
                            int64_t n, int32_t side, const int32_t* d_ent_ids, int64_t ent_lo, int64_t ent_hi,
                            int32_t* d_counts, void* d_work, void* d_screen, int64_t screen_bytes, void* stream);

extern "C" int amdkge_rank_counts(const amdkge_model* m, const float* d_ent, const float* d_rel, const int32_t* d_triples,
                                  int64_t n, int32_t side, const int32_t* d_ent_ids, int64_t ent_lo, int64_t ent_hi,
                                  int32_t* d_counts, void* d_work, void* stream) {
    return rank_counts_impl(m, d_ent, d_rel, d_triples, n, side, d_ent_ids, ent_lo, ent_hi, d_counts, d_work, nullptr, 0, stream);
}

extern "C" int64_t amdkge_rank_screen_workspace_bytes(const amdkge_model* m, int64_t n, int64_t n_cand) {
    if (validate_model(m) != AMDKGE_OK || n < 0 || n_cand < 0) return -1;
    // the fixed part + a pair list with room for ~3 % of the comparisons (typically ~0.2 % are undecided; a full list falls back to the
    // plain kernel), for a base of any alignment
    const bool early = mode_of(m->scoring_type, AMDKGE_SIDE_S) != MODE_DOT;   // TransE / RotatE: the exact early exit (kge_rank_early.h)
    if (early && !g_rank_cfg.early.on) return 0;
    int64_t pairs = n * n_cand / 32;
    const int64_t least = early ? 1 << 18 : 1 << 20;
    if (pairs < least) pairs = least;
    if (early && pairs > (1ll << 27)) pairs = 1ll << 27;
    Layout l;
    l.take(early ? early_layout(n, n_cand).pairs : screen_layout(n, n_cand, row_floats(m)).pairs);
    l.take(pairs, sizeof(int2));
    return l.any_base(l.end());
}

extern "C" int amdkge_rank_counts_screened(const amdkge_model* m, const float* d_ent, const float* d_rel, const int32_t* d_triples,
                                           int64_t n, int32_t side, const int32_t* d_ent_ids, int64_t ent_lo, int64_t ent_hi,
                                           int32_t* d_counts, void* d_work, void* d_screen, int64_t screen_bytes, void* stream) {
    return rank_counts_impl(m, d_ent, d_rel, d_triples, n, side, d_ent_ids, ent_lo, ent_hi, d_counts, d_work, d_screen, screen_bytes, stream);
}

static int rank_counts_impl(const amdkge_model* m, const float* d_ent, const float* d_rel, const int32_t* d_triples,
                            int64_t n, int32_t side, const int32_t* d_ent_ids, int64_t ent_lo, int64_t ent_hi,
                            int32_t* d_counts, void* d_work, void* d_screen, int64_t screen_bytes, void* stream) {
    if (int rc = validate_model(m)) return rc;
    if (side != AMDKGE_SIDE_S && side != AMDKGE_SIDE_O) return set_error(AMDKGE_EINVAL, "rank_counts: side must be AMDKGE_SIDE_S or AMDKGE_SIDE_O");
    if (n < 0 || ent_lo < 0 || ent_hi < ent_lo) return set_error(AMDKGE_EINVAL, "rank_counts: bad sizes");
    if (!d_ent_ids && ent_hi > m->n_ents) return set_error(AMDKGE_EINVAL, "rank_counts: entity range outside the table");
    if (n == 0 || ent_hi == ent_lo) return AMDKGE_OK;
    if (!d_ent || !d_rel || !d_triples || !d_counts || !d_work) return set_error(AMDKGE_EINVAL, "rank_counts: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    const RankGeom g = geom_of(m, side);
    const Workspace w = carve(d_work, m, n);
    if (int rc = run_prep(m, d_ent, d_rel, d_triples, n, side, g, w, st)) return rc;

    const ModelConst mc = model_const(m);
    CountArgs a{};
    a.ent = d_ent; a.Q = w.Q; a.qpos = w.qpos; a.ent_ids = d_ent_ids; a.counts = d_counts; a.n = n;
    a.ent_lo = ent_lo; a.ent_hi = ent_hi; a.g = g; a.sgn_scale = mc.score_sign * mc.score_scale;
    const int mode = mode_of(m->scoring_type, side);
    const bool rot_exact = (mode == MODE_ROT_O || mode == MODE_ROT_S) && !g_rank_cfg.rotate_fast;
    const bool v4 = (rot_exact || g.U % 4 == 0) && (g.eplane % 4 == 0) && (g.K % 4 == 0);
    const int force = g_rank_cfg.kernel;   // amdkge_set_rank_kernel (tests): 1 forces the VALU tile kernel, 2 the first MFMA kernel, 3 the pipelined one unscreened
    const bool mfma = (mode == MODE_DOT) && force != 1;
    const int qt = mfma ? MQ : QT, et_ = mfma ? ME : ET;
    const int64_t qtiles = (n + qt - 1) / qt;
    const int64_t etiles = (ent_hi - ent_lo + et_ - 1) / et_;
    // Entity tiles per block: the grid is (query tiles) x (entity splits).  VALU kernel: pick the split that minimises
    // (rounds of resident blocks) x (tiles per block), i.e. the tail of the last round, with a mild bias towards longer
    // blocks (one counter flush per block).  MFMA kernel: the two workgroups resident on a CU share its matrix pipes, so
    // what counts is the work of the busiest CU, ceil(blocks / 256) x (tiles per block + ~3/16 tile of prologue and
    // flush) -- and a CU needs a SUCCESSION of blocks to keep two of them out of phase: measured on C3 (23 x 320 tiles)
    // 5-10 tiles per block 1.96 ms, 15 (two blocks per CU, started together) 2.16 ms, 30 (one block per CU) 2.85 ms.
    // So: at least 4 blocks per CU when the problem is large enough, else the cheapest split with a lone block priced
    // at its measured ~0.6 efficiency.
    const int64_t slots = mfma ? 256 : 2048;   // CUs resp. resident workgroups (8 per CU)
    int64_t tiles_per = 1, best_cost = -1;
    for (int pass = 0; pass < 2 && best_cost < 0; ++pass) {
        for (int64_t tp = 1; tp <= (mfma ? 256 : 4096) && tp <= etiles; ++tp) {
            const int64_t sp = (etiles + tp - 1) / tp;
            if (sp > 65535) continue;
            const int64_t blocks = qtiles * sp;
            if (mfma && pass == 0 && blocks < 4 * slots) continue;
            const int64_t rounds = (blocks + slots - 1) / slots;
            int64_t cost = rounds * (tp * 16 + (mfma ? 3 : 1));
            if (mfma && rounds == 1) cost = cost * 5 / 3;
            if (best_cost < 0 || cost < best_cost) { best_cost = cost; tiles_per = tp; }
        }
        if (!mfma) break;
    }
    if (best_cost < 0) return set_error(AMDKGE_EUNSUPPORTED, "rank_counts: entity range too large for one launch; split [ent_lo, ent_hi)");
    // distance models whose probe picked the early-exit kernel: runs of >= 4 tiles amortise its per-block thresholds, and keep the
    // blocks of the fall-back launch behind it (the plain kernel, run only if the hand-over list overflowed) few
    const int64_t mcand_e = ent_hi - ent_lo;
    const bool rot_m = mode == MODE_ROT_O || mode == MODE_ROT_S;
    bool use_early = !mfma && d_screen && g_rank_cfg.early.on && force == 0 && v4 && (!rot_m || rot_exact) && a.sgn_scale < 0.f && n >= 64 && mcand_e >= 256 &&
                     g.U >= 64 && mcand_e < 0x7FFFFFFFll && n < 0x7FFFFFFFll && holds_list(early_layout(n, mcand_e).pairs, screen_bytes);
    bool probe_measured = false;
    if (use_early)   // the probe: is the exit going to fire on these tables?  (host decision, see early_probe)
        if (int rc = early_probe(mode, d_ent, d_ent_ids, ent_lo, mcand_e, n, g, w, a.sgn_scale, d_screen, (size_t)screen_bytes, &use_early, &probe_measured, st)) return rc;
    if (use_early && tiles_per < 4) {
        // (the same rounds x length cost as above over runs of 4 .. 16 tiles: a run length whose last round is nearly full -- the
        // plain kernel, when the probe picks it, pays for an underfull last round in full: runs of 8 cost it 10 % at C2)
        int64_t best = -1, pick = etiles < 4 ? etiles : 4;
        for (int64_t tp = pick; tp <= 16 && tp <= etiles; ++tp) {
            const int64_t blocks = qtiles * ((etiles + tp - 1) / tp);
            if (blocks > 16 * slots) continue;
            const int64_t cost = ((blocks + slots - 1) / slots) * (tp * 16 + 1);
            if (best < 0 || cost < best) { best = cost; pick = tp; }
        }
        tiles_per = pick;
        while (tiles_per < etiles && (etiles + tiles_per - 1) / tiles_per > 65535) ++tiles_per;   // (the grid's y extent)
    }
    int64_t splits;
    a.ent_per_block = (int)(tiles_per * et_);
    splits = (etiles + tiles_per - 1) / tiles_per;
    const dim3 grid((unsigned)qtiles, (unsigned)splits);
    if (mfma) {
        a.qtiles = (int)qtiles; a.splits = (int)splits;
        const int64_t nblk = 8 * ((qtiles + 7) / 8) * splits;
        if (nblk > 0x7FFFFFFFll) return set_error(AMDKGE_EUNSUPPORTED, "rank_counts: too many tiles for one launch; split the triples or the entity range");
        const bool pipe = force != 2;
        // ---- int8 screening pass + exact recheck (kge_rank_screen.hip) when the caller supplied its workspace: same counts, bit
        //      for bit; the exact kernel below then runs only as the fall-back of an overflowing recheck list ----
        const int64_t mcand = ent_hi - ent_lo;
        if (d_screen && force == 0 && v4 && pipe && g.eplane == 0 && g.U <= 2048 && n >= 128 && mcand >= 512 && sgn_scale_positive(mc) &&
            holds_list(screen_layout(n, mcand, g.U).pairs, screen_bytes)) {
            if (int rc = run_screen(m, d_ent, d_ent_ids, ent_lo, mcand, n, g, w, mc, d_counts, d_screen, (size_t)screen_bytes, st)) return rc;
            a.guard = carve_screen(d_screen, (size_t)screen_bytes, n, mcand, g.U).counter + 1;
        }
        return launch_count_mfma(v4, pipe, a, (unsigned)nblk, st);
    }
    // ---- distance models: the exact early exit (kge_rank_tile.hip, kge_rank_early.h) when the caller supplied its workspace: same counts, bit for
    //      bit; the plain kernel below then runs only as the fall-back of an overflowing list ----
    {
        if (use_early) {
            if (int rc = run_early(mode, m, d_ent, d_ent_ids, ent_lo, mcand_e, n, g, w, a, grid, d_screen, (size_t)screen_bytes, &a.guard, probe_measured, st)) return rc;
            a.guard_mode = GUARD_FLAG;   // the plain kernel below: only if the list overflowed
        }
    }
    return launch_count_tile(mode, v4, rot_exact, a, grid, st);
}

extern "C" int amdkge_rank_compose(const int32_t* d_counts, const int32_t* d_sub, int64_t n, int32_t strategy,
                                   int32_t* d_ranks, int64_t rank_stride, void* stream) {
    if (n < 0 || rank_stride < 1) return set_error(AMDKGE_EINVAL, "rank_compose: bad sizes");
    if (strategy < AMDKGE_RANK_WORST || strategy > AMDKGE_RANK_MIDDLE) return set_error(AMDKGE_EINVAL, "rank_compose: unknown ranking strategy");
    if (n == 0) return AMDKGE_OK;
    if (!d_counts || !d_ranks) return set_error(AMDKGE_EINVAL, "rank_compose: NULL pointer");
    hipLaunchKernelGGL(rank_compose_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_counts, d_sub, n, strategy, d_ranks, rank_stride);
    return check_launch("rank_compose");
}

extern "C" int amdkge_row_dots(const float* d_q, int64_t n, const float* d_table, int32_t row_floats, const int32_t* d_ent_ids,
                               int64_t ent_lo, int64_t ent_hi, float* d_out, int64_t ld, void* stream) {
    if (n < 0 || row_floats < 1 || ent_lo < 0 || ent_hi < ent_lo || ld < ent_hi - ent_lo) return set_error(AMDKGE_EINVAL, "row_dots: bad sizes");
    if (n == 0 || ent_hi == ent_lo) return AMDKGE_OK;
    if (!d_q || !d_table || !d_out) return set_error(AMDKGE_EINVAL, "row_dots: NULL pointer");
    CountArgs a{};
    a.ent = d_table; a.Q = d_q; a.qpos = nullptr; a.ent_ids = d_ent_ids; a.n = n; a.ent_lo = ent_lo; a.ent_hi = ent_hi;
    a.g = RankGeom{row_floats, 0, 0, row_floats, row_floats, 1.f};
    a.sgn_scale = 1.f; a.scores = d_out; a.ld = ld;
    const bool v4 = row_floats % 4 == 0 && (((uintptr_t)d_q | (uintptr_t)d_table) & 15) == 0;
    return launch_store(MODE_DOT, v4, a, n, ent_hi - ent_lo, (hipStream_t)stream);
}
