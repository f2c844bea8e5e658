// Owner-computes training step for gfx950 (no global atomics on the entity table).
//
// Why: on MI355X `global_atomic_add_f32` retires ~10.4 G cache-line operations/s chip-wide whatever the
// line's occupancy (scripts/atomic_bench.hip), which floors the atomic gradient scatter of
// kge_train.hip at 230 000 rows x 12.5 lines = 0.28 ms per C2 step, 3x the HBM time of the same bytes.
//
// How: two kernels per step.
//   F  train_fwdbwd_kernel<.., STAGE=true> (kge_train_kernel.h, instantiated in kge_train_stage.hip): the fused
//      forward + loss + per-positive backward.  Instead of scattering replacement-row gradients it APPENDS one 16-byte entry
//      {positive, role|local row, dL/dscore, row id} per corruption (and one per s / o row of the positive) to
//      the bucket of the table TILE that owns the destination row (one returning atomic per entry on a
//      128-byte-strided counter; full buckets spill to one shared overflow list), and stores per positive
//      four K-float rows with plain 16-byte coalesced stores: the complete gradient rows of its own s and o,
//      and two "side" rows A, B (trilinear models: A = d score/d o (s,p), B = d score/d s (p,o), which do not
//      depend on the replaced row; TransE: copies of the s and o rows as read by the forward pass, plus one packed
//      byte per unit and corruption with the sign of s + p - o; RotatE: A = s o r, B = o o conj(r)).
//      The relation-row gradient (237 hot rows at C2) keeps the atomic row-add into the dense relation
//      gradient buffer, which the ordinary sweep (kge_opt.hip) consumes.
//   T  tile_backward_kernel (kge_train_tile.hip; rows beyond 2 KB with few entries: tile_direct_kernel,
//      kge_train_direct.hip): one workgroup OWNS a tile of entity rows and keeps their gradient accumulators in LDS
//      (<= 150 KB).  It walks its bucket (+ the overflow list), adds g * A|B (trilinear),
//      -/+ g with the stored sign bits (TransE; grad_unit on three rows where a unit is (near) zero) or
//      g (e - S) / |e - S| on the side row S and its own live row e (RotatE) -- every wave into the rows it
//      owns, plain LDS read-modify-writes --, and finally applies the optimizer + regulariser to its rows straight from LDS: the
//      entity gradient never exists in HBM and the entity table needs no separate optimizer sweep.
//      The side rows are staged copies because other tiles update their rows in place while this one
//      is still reading.
//
// Replaces the same reference code as kge_train.hip + kge_opt.hip: ScoringBasedEmbeddingModel.train_step
// (/root/reference/ampligraph/latent_features/models/ScoringBasedEmbeddingModel.py:370-429) including
// optimizer.minimize (optimizers.py:136-168) and the LP regulariser (regularizers.py:35-37).
//
// This unit is the host side of the step: the plan (tile size, bucket capacity, workspace layout), the guard that keeps one plan's
// counters safe from another's lists, the C entry points, and the three small kernels around F and T.  The kernels of F, T and of the
// column-sharded step are instantiated in units of their own and reached through the launch functions of kge_train_tiled.h.
#include <stdlib.h>
#include <mutex>
#include <unordered_map>

#include "kge_train_tiled.h"

namespace kge {

// Deterministic mode: the relation-row gradient.  One workgroup per relation collects the positives of its relation IN BATCH ORDER
// and adds their staged fifth rows in that order, every thread owning fixed columns of the row: the same additions in the same
// order on every run (and in oracle/train_ordered.py).
// Round 5: the first version walked the batch 256 positions at a time -- a dependent chain of (triple load, two barriers, row loads)
// per step, 40 steps at B = 10 000: 61.6 us of latency for 42 rows per relation (profiles/r05a_splits.log).  Now the batch is taken in
// segments of 8 192 positions: every wave scans its contiguous quarter of the segment with all 32 triple loads issued up front
// and compacts its hits into its own LDS list (wave-local ballots, no barrier); the four lists, read one after the other, are the
// segment's hits in batch order; the rows are then added with 16 loads in flight per thread and the adds in list order
// (24.7 us with 4 096-position segments and 8 loads in flight, profiles/r05b_c4_direct_short_rows_and_splits.txt).
constexpr int RELDET_SEG = 8192, RELDET_Q = RELDET_SEG / 4, RELDET_UN = 16;   // (32 KB of lists; B = 10 000: two segments)
__global__ __launch_bounds__(256) void rel_backward_det_kernel(const int32_t* __restrict__ triples, int64_t B, const float* __restrict__ stage_rows,
                                                               int ns, int K, float* __restrict__ g_rel) {
    __shared__ int s_list[4][RELDET_Q];
    __shared__ int s_cnt[4];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float acc[16];   // K <= 4096 floats (k <= 2048 complex units): 16 columns per thread
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = 0.f;
    for (int64_t seg = 0; seg < B; seg += RELDET_SEG) {
        const int64_t q0 = seg + (int64_t)wv * RELDET_Q;
        int pv[RELDET_Q / 64];
#pragma unroll
        for (int j = 0; j < RELDET_Q / 64; ++j) {
            const int64_t i = q0 + j * 64 + lane;
            pv[j] = i < B ? triples[3 * i + 1] : -1;
        }
        int n = 0;
#pragma unroll
        for (int j = 0; j < RELDET_Q / 64; ++j) {
            const bool hit = pv[j] == r;
            const unsigned long long m = __ballot(hit);
            if (hit) s_list[wv][n + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0))] = wv * RELDET_Q + j * 64 + lane;
            n += __popcll(m);
        }
        if (lane == 0) s_cnt[wv] = n;
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const int col = tid + 256 * c;
            if (col >= K) break;
            float a = acc[c];
            for (int w = 0; w < 4; ++w) {
                const int nw = s_cnt[w];
                for (int h0 = 0; h0 < nw; h0 += RELDET_UN) {
                    float v[RELDET_UN];
#pragma unroll
                    for (int u = 0; u < RELDET_UN; ++u)
                        v[u] = (h0 + u < nw) ? stage_rows[((seg + s_list[w][h0 + u]) * (int64_t)ns + 4) * K + col] : 0.f;
#pragma unroll
                    for (int u = 0; u < RELDET_UN; ++u)
                        if (h0 + u < nw) a += v[u];
                }
            }
            acc[c] = a;
        }
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < 16; ++c)
        if (tid + 256 * c < K) g_rel[(int64_t)r * K + tid + 256 * c] += acc[c];
}

// RotatE: cos / sin of every relation phase, once per step, in the declared correctly rounded form (prep_rel_exact, kge_device.h); the tile pass sees the
// very values the forward kernel used)
__global__ __launch_bounds__(256) void rel_phase_kernel(const float* __restrict__ rel, int64_t n_rels, int k, int K, ModelConst mc,
                                                        float* __restrict__ cs) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_rels * k) return;
    const int64_t r = idx / k;
    const int c = (int)(idx - r * k);
    float p[2] = {rel[r * K + c], 0.f};
    prep_rel_exact<AMDKGE_ROTATE>(mc, p);
    cs[r * K + c] = p[0];
    cs[r * K + k + c] = p[1];
}

// ---- plan: tile size, bucket capacity and workspace layout (shared by the two entry points) ------------------
struct TiledPlan {
    int tile_rows, n_tiles, cap, ovf_cap, rb;
    int ns, sort_cap;   // deterministic mode: 5 staged rows per positive, LDS sort buffer entries (0 otherwise)
    int64_t off_cnt, off_lists, off_ovf, off_rows, off_cs, off_touch, off_loss, off_flag, off_hot_map, off_hot_buf, off_codes, total;   // the walk (the library aligns d_work up itself)
    bool own_cache;     // RotatE, queued form, >= 4 corruption entries per table row and step: own rows cached in LDS
    bool codes;         // TransE with one wave per positive: the forward kernel hands the signs of d_j to the tile pass (ENTRY_EXACT)
    bool direct;        // long rows (> 128 quads per half): the row-direct tile pass (kge_train_direct.hip)
};

static int g_tile_direct = 1;   // amdkge_set_tile_direct (A/B measurements, tests): 0 keeps long rows on tile_backward_kernel
// (Round 5 also offered the row-direct pass to SHORTER rows -- 32 .. 128 quads per half, BASELINE configs[3]'s 1.6 KB rows, one or two
// waves per row.  MEASURED SLOWER than the LDS-accumulator tiles where it was meant to help: C4 tile pass 339 us vs 476 us, whole step
// 0.393 vs 0.551 ms, profiles/r05b_c4_direct_short_rows_and_splits.txt -- one wave per row is a serial chain of row round trips, the
// LDS tiles keep 16 waves of a CU on 16 different rows.  Removed from the product in round 6: `git show db3a690` has it.)

static bool make_plan(const amdkge_model* m, int64_t B, int32_t eta, TiledPlan& p, bool det = false, bool det_wide = false) {
    const int ks = stored_k(m), K = row_floats(m);
    if (ks % 4 != 0 || ks > 2048) return false;   // 16-byte layout; one wave (k <= 512) or one workgroup (k <= 2048) per positive
    if ((ks <= 512 ? (size_t)4 * slot_lds_bytes(eta, 1) + 32 + 16 * (size_t)K : slot_lds_bytes(eta, 4) + 8 + 4 * (size_t)K) +
            sign_stash_bytes(m->scoring_type, eta, 2) > 150 * 1024) return false;
    const int64_t entries = B * (eta + 2);
    if (entries >= (1ll << 31)) return false;
    p.ns = det ? 5 : 4;
    p.sort_cap = 0;
    // deterministic mode shares the LDS between the accumulators and the sort buffer: shrink the tiles until a bucket
    // (+ slack for overflow entries) fits the buffer next to them
    const int model_t = m->scoring_type == AMDKGE_HOLE ? AMDKGE_COMPLEX : m->scoring_type;
    const size_t queue_bytes = tile_queued(model_t, tile_ch_of(ks / 4), K) ? TILE_QUEUE_BYTES : 0;
    // (few entries per row -- one GPU's C5 shard sees 0.7 -- would only halve the tiles)
    p.own_cache = !det && m->scoring_type == AMDKGE_ROTATE && queue_bytes != 0 && B * (int64_t)eta >= 4 * m->n_ents;
    const size_t row_bytes = (size_t)K * 4 * (p.own_cache ? 2 : 1);
#ifndef KGE_DIRECT_BUDGET_KB
#define KGE_DIRECT_BUDGET_KB 1200
#endif
    // (long rows on the row-direct pass keep nothing but their entry list in LDS: the tile size is not an LDS question there)
    // The row-direct pass pays off while a row sees few entries per step (one GPU's C5 shard: 0.7; a 1 M-row table at the same
    // batch: 4.3 -- 21.8 vs 26.2 ms); where rows collect many (ComplEx k = 1000 on 14 505 entities: 15 -- 0.88 vs 0.72 ms) the
    // LDS accumulators win, so the form is chosen by the batch's mean entries per row.
    const bool direct_long = g_tile_direct && !det && ks / 4 > 128 && B * (int64_t)(eta + 2) <= 8 * m->n_ents;
    const bool direct_shape = direct_long;
    const size_t nodet_budget = direct_shape ? (size_t)KGE_DIRECT_BUDGET_KB * 1024 : 150 * 1024 - queue_bytes;
    for (size_t budget = det ? 96 * 1024 : nodet_budget;; budget = budget * 3 / 4) {
        // Whole ownership blocks per tile (block-interleaved ownership, see tile_backward_kernel).  The block size is the largest
        // power of two <= TILE_RB that still lets the tiles fill the 256 CUs evenly: a tile's rows come in multiples of the
        // block, and at C2 (14 505 rows, ~57 per tile) blocks of 8 would leave 11 % of the CUs without a tile.
        int fit = (int)(budget / row_bytes);
        if (direct_shape && fit > 160) fit = 160;   // (<= 8 entries per row: a bucket of at most 2 * 1 280 + 256 entries -- the row-direct pass's LDS list)
        if (fit < 1) return false;
        double best_eff = -1.0;
        for (int rb = (int)TILE_RB; rb >= 1; rb >>= 1) {
            if (rb > fit) continue;
            const int64_t blocks = (m->n_ents + rb - 1) / rb;
            int64_t per = 0;
            for (int64_t mm = 1;; ++mm) {   // smallest number of CU rounds whose tile fits the LDS
                per = (blocks + 256 * mm - 1) / (256 * mm);
                if (per * rb <= fit && per * rb <= 4096) break;
            }
            const int64_t nt = (blocks + per - 1) / per, rounds = (nt + 255) / 256;
            const double eff = (double)m->n_ents / (double)(per * rb) / (double)(rounds * 256);
            if (eff > best_eff + 0.03 || best_eff < 0) {   // a smaller block must buy at least 3 % of the chip
                best_eff = eff; p.rb = rb; p.tile_rows = (int)(per * rb); p.n_tiles = (int)nt;
            }
            if (eff >= 0.97) break;
        }
        if (best_eff < 0) return false;
        // bucket capacity: twice the mean + slack (Poisson tail; anything beyond goes to the overflow list)
        const int64_t mean = (entries + p.n_tiles - 1) / p.n_tiles;
        p.cap = (int)(2 * mean + (mean >= 224 ? 256 : 32 + mean));
        // development aid (scripts/nan_hunt.py): a tiny bucket capacity sends most entries through the shared overflow list
        static const int dbg_cap = [] { const char* e = getenv("AMDKGE_DEBUG_BUCKET_CAP"); return e ? atoi(e) : 0; }();
        if (dbg_cap > 0 && p.cap > dbg_cap) p.cap = dbg_cap;
        if (!det) break;
        // the sort buffer holds a whole bucket + slack for overflow entries.  (Rounds 2 - 4 sorted the bucket with a bitonic network
        // and needed a POWER OF TWO here: 4 096 entries = 64 KB for C2's buckets of 2 330, which did not fit beside 57-row tiles --
        // the deterministic mode ran 45-row tiles in two rounds on the 256 CUs.  The index sorts of round 5 need no such rounding:
        // the deterministic mode now has the default mode's tile geometry.)
        int sc = (p.cap + 64 + 63) & ~63;
        if (det_wide) {   // AMDKGE_TILED_DET_WIDE_SORT (skewed graphs): room for a hub's tile -- at least twice a bucket, a power of two as in rounds 2 - 4
            sc = 64;
            while (sc < 2 * (p.cap + 64)) sc <<= 1;
        }
        const size_t fixed = (size_t)p.tile_rows * K * 4 + 4096 + 16 + 1024;
        if (sc <= 8192 && fixed + (size_t)sc * 20 <= 158 * 1024) {   // per entry: its 16 bytes + two 16-bit index arrays (+ 1 KB of chunk counters)
            // take what the LDS still offers (up to 8192 entries): a hub's tile receives many times the mean
            while (sc * 2 <= 8192 && fixed + (size_t)sc * 2 * 20 <= 158 * 1024) sc *= 2;
            p.sort_cap = sc;
            break;
        }
        if (p.tile_rows == 1) return false;   // one row per tile and its bucket still does not fit: not a shape for this mode
    }
    p.ovf_cap = (int)(entries > 0 ? entries : 1);
    // row-direct pass: one wave group per tile, the bucket sorted in LDS, rows through registers -- long rows only, and only
    // while a bucket (+ slack for overflow entries) is a small LDS list
    p.direct = direct_shape && p.cap <= 3000 && p.tile_rows <= 2048;
    Layout l;
    p.off_loss = l.take((int64_t)LOSS_PARTS * LOSS_PART_STRIDE, 8);   // first: the same place in every plan (kept zero between steps)
    p.off_flag = l.take(256);                                        // sticky status flag (amdkge_train_tiled_status): also plan-independent
    p.off_hot_map = l.take(m->n_ents);                               // hot-row map and replicas: also independent of B / eta / mode,
    p.off_hot_buf = l.take((int64_t)HOT_MAX * HOT_REPL * K, 4);      // written by amdkge_train_tiled_set_hot_rows
    p.off_touch = l.take(m->n_ents);                                 // byte per entity row (lazy optimizer + POS_ATOMIC), kept zero between steps
    // Everything from here on moves with the plan (n_tiles and cap depend on B through own_cache, the bucket capacity and the
    // deterministic mode's LDS split): see plan_guard() for what keeps the counters of one plan safe from the lists of another.
    p.off_cnt = l.take((int64_t)(p.n_tiles + 2) * 32, 4);   // bucket fills, overflow count, finished-tiles ticket
    p.off_lists = l.take((int64_t)p.n_tiles * p.cap, sizeof(StageEntry));
    p.off_ovf = l.take(p.ovf_cap, sizeof(StageEntry));
    p.off_rows = l.take(B * p.ns * K, 4);
    p.off_cs = l.take(m->scoring_type == AMDKGE_ROTATE ? m->n_rels * K : 0, 4);
    const int64_t code_bytes = B * eta * (ks / 4) * 4;
    p.codes = !det && m->scoring_type == AMDKGE_TRANSE && ks <= 512 && eta <= 65535 && code_bytes <= ((int64_t)8 << 30);   // (det: sorted path, three-row form)
    p.off_codes = l.take(p.codes ? code_bytes : 0);
    p.total = l.any_base(l.next());
    return true;
}

// One workspace serves steps of different batch sizes (fit() ends every epoch with a short batch), and the position of the
// bucket lists depends on the plan: the lists and staged rows of one plan may lie where another plan keeps its counters.  A
// plan's counters are zero when its step ends, so they only have to be re-zeroed when a step with a DIFFERENT geometry has
// used the buffer in between.  The library remembers, per workspace address, the geometry of the last step enqueued on it and
// clears the counter region on the step's stream when it changes (first sight of an address counts as a change; the
// caller's zero-fill contract covers a buffer that is freed and re-allocated at the same address).
// The memory is per (device, address) -- the same address on another GPU is another workspace -- and bounded: past
// PLAN_GUARD_MAX remembered workspaces (or on amdkge_release_scratch()) everything is forgotten, which only costs the next step on
// each workspace one memset.  The guard is HOST state: a step captured into a hipGraph and replayed does not pass through it, so
// a graph must not be replayed on a workspace that a step of another geometry has used since the capture (include/amdkge.h).
namespace {
constexpr size_t PLAN_GUARD_MAX = 4096;
std::mutex g_plan_mu;
std::unordered_map<uint64_t, uint64_t> g_plan_last[16];   // per device ordinal (mod 16): workspace address -> geometry signature
}
void release_plan_guard() {   // (kge::, called by amdkge_release_scratch)
    std::lock_guard<std::mutex> lk(g_plan_mu);
    for (auto& mp : g_plan_last) mp.clear();
}
static int plan_guard(const void* d_work, const TiledPlan& p, char* w, hipStream_t st) {
    const uint64_t sig = ((uint64_t)(uint32_t)p.n_tiles << 32) ^ ((uint64_t)p.off_cnt * 0x9E3779B97F4A7C15ull) ^ (uint64_t)(uint32_t)p.cap;
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev)) return set_error_hip(e, "hipGetDevice");
    bool changed;
    {
        std::lock_guard<std::mutex> lk(g_plan_mu);
        auto& last = g_plan_last[dev & 15];
        if (last.size() >= PLAN_GUARD_MAX) last.clear();
        const uint64_t key = (uint64_t)(uintptr_t)d_work ^ ((uint64_t)(dev >> 4) << 56);
        auto it = last.find(key);
        changed = it == last.end() || it->second != sig;
        if (changed) {
            try {
                last[key] = sig;
            } catch (...) {   // (out of host memory for the registry node: forget everything -- every workspace then pays one memset)
                last.clear();
            }
        }
    }
    if (changed)
        if (hipError_t e = hipMemsetAsync(w + p.off_cnt, 0, (size_t)(p.n_tiles + 2) * 32 * 4, st)) return set_error_hip(e, "hipMemsetAsync(tile counters)");
    return AMDKGE_OK;
}

// One step's launches behind the plan: F (or C of the column-sharded step in its place), the deterministic mode's relation-row pass, T.
static int run_tiled(int model, TrainArgs& f, TileArgs& te, hipStream_t st, float* given = nullptr) {
    int rc = given ? run_cols_stage(model, f, given, st) : run_forward_stage(model, f, st);
    if (rc) return rc;
    if (te.det && f.B > 0) {   // deterministic mode: relation-row gradient from the staged fifth rows, in batch order
        hipLaunchKernelGGL(rel_backward_det_kernel, dim3((unsigned)te.n_rels), dim3(256), 0, st, f.triples, f.B, f.stage_rows, f.ns, f.K, f.g_rel);
        if ((rc = check_launch("rel_backward_det"))) return rc;
    }
    // T: entity tiles (the owner applies the optimizer)
    te.gw = f.nq <= 128 ? 1 : (f.nq <= 256 ? 4 : 8);
    return te.direct ? run_tile_direct(model, te, st) : run_tile_backward(model, te, st);
}

}  // namespace kge

using namespace kge;

extern "C" int amdkge_set_tile_direct(int on) {
    g_tile_direct = on ? 1 : 0;   // (2 selected round 5's short-row form, since removed: it now means 1)
    return AMDKGE_OK;
}

extern "C" int64_t amdkge_train_tiled_workspace_bytes(const amdkge_model* m, int64_t B, int32_t eta) {
    if (validate_model(m) != AMDKGE_OK || B < 0 || B >= (1ll << 30) || eta < 1) return -1;
    TiledPlan p, pd;
    if (!make_plan(m, B, eta, p)) return 0;   // 0 = shape not supported by the owner-computes path
    // one buffer serves both modes: the deterministic plan (five staged rows, smaller tiles) is the larger one where it exists
    int64_t det_total = make_plan(m, B, eta, pd, true) ? pd.total : 0;
    if (make_plan(m, B, eta, pd, true, true) && pd.total > det_total) det_total = pd.total;   // (AMDKGE_TILED_DET_WIDE_SORT: smaller tiles, more of them)
    return p.total > det_total ? p.total : det_total;
}

extern "C" int amdkge_train_step_tiled(const amdkge_model* m, const amdkge_loss* loss, const amdkge_opt* opt,
                                       float* d_ent, float* d_rel, float* d_ent_slot0, float* d_ent_slot1,
                                       float* d_rel_slot0, float* d_rel_slot1, float rel_reg_lambda,
                                       const int32_t* d_triples, int64_t B, int32_t eta, int64_t sample_base,
                                       int64_t sample_range, uint64_t seed, uint64_t step, int64_t row_offset,
                                       int64_t b_global, const int32_t* d_neg_override, float* d_grad_ent,
                                       float* d_grad_rel, int32_t apply_update, int32_t flags, double* d_loss_sum, double* d_reg_loss,
                                       float* d_pos_scores, float* d_neg_scores, void* d_work, void* stream) {
    if (int rc = validate_model(m)) return rc;
    if (int rc = validate_opt(opt)) return rc;
    if (!loss || loss->kind < 0 || loss->kind > AMDKGE_LOSS_MULTICLASS_NLL) return set_error(AMDKGE_EINVAL, "train_step_tiled: unknown loss kind");
    if (loss->focus_nonlinearity < AMDKGE_FOCUS_OFF || loss->focus_nonlinearity > AMDKGE_FOCUS_SOFTPLUS || (loss->focus_nonlinearity && !loss->d_focus_w))
        return set_error(AMDKGE_EINVAL, "train_step_tiled: bad FocusE settings (unknown non-linearity or NULL weights)");
    if (!d_ent || !d_rel || !d_grad_rel || !d_loss_sum || !d_work) return set_error(AMDKGE_EINVAL, "train_step_tiled: NULL pointer");
    if (!d_grad_ent && (!apply_update || (flags & AMDKGE_TILED_POS_ATOMIC))) return set_error(AMDKGE_EINVAL, "train_step_tiled: d_grad_ent is required unless the step updates in place with staged positives");
    if (B < 0 || B >= (1ll << 30) || eta < 1) return set_error(AMDKGE_EINVAL, "train_step_tiled: B must be in [0, 2^30) and eta >= 1");
    const bool det = (flags & AMDKGE_TILED_DETERMINISTIC) != 0;
    if (det && (flags & AMDKGE_TILED_POS_ATOMIC)) return set_error(AMDKGE_EINVAL, "train_step_tiled: DETERMINISTIC excludes POS_ATOMIC (atomics add in arrival order)");
    const bool given = (flags & AMDKGE_TILED_GIVEN_COEFFS) != 0;
    if (given) {   // column-sharded step, phase C: d_pos_scores / d_neg_scores carry dL/dscore IN (amdkge_cols_loss)
        if (flags & (AMDKGE_TILED_DETERMINISTIC | AMDKGE_TILED_POS_ATOMIC | AMDKGE_TILED_HOT_ROWS)) return set_error(AMDKGE_EUNSUPPORTED, "train_step_tiled: GIVEN_COEFFS excludes DETERMINISTIC / POS_ATOMIC / HOT_ROWS");
        if (loss->focus_nonlinearity) return set_error(AMDKGE_EUNSUPPORTED, "train_step_tiled: GIVEN_COEFFS with FocusE is not offered (fold the weights into the coefficients)");
        if (!d_pos_scores || d_neg_scores != d_pos_scores + B) return set_error(AMDKGE_EINVAL, "train_step_tiled: GIVEN_COEFFS needs one coefficient buffer: d_pos_scores [B], d_neg_scores = d_pos_scores + B [eta][B]");
        if (stored_k(m) > 256) return set_error(AMDKGE_EUNSUPPORTED, "train_step_tiled: GIVEN_COEFFS serves column slices of up to 256 stored units per half");
    }
    TiledPlan p;
    if (!make_plan(m, B, eta, p, det, det && (flags & AMDKGE_TILED_DET_WIDE_SORT) != 0))
        return set_error(AMDKGE_EUNSUPPORTED, "train_step_tiled: shape not supported (stored half width not a multiple of 4 -- set k_pad = amdkge_padded_k(k) --, > 2048, or eta too large); use amdkge_train_fwdbwd + amdkge_opt_step");
    if (apply_update) {
        if (opt_nslots(opt->kind) >= 1 && !d_ent_slot0) return set_error(AMDKGE_EINVAL, "train_step_tiled: optimizer slot 0 is NULL");
        if (opt_nslots(opt->kind) == 2 && !d_ent_slot1) return set_error(AMDKGE_EINVAL, "train_step_tiled: optimizer slot 1 is NULL");
    }
    const bool d_rel_slot_ok = (opt_nslots(opt->kind) < 1 || d_rel_slot0) && (opt_nslots(opt->kind) < 2 || d_rel_slot1);
    if (apply_update && !d_rel_slot_ok && (d_rel_slot0 || d_rel_slot1))
        return set_error(AMDKGE_EINVAL, "train_step_tiled: relation optimizer slots incomplete for this optimizer");
    if (B > 0 && !d_triples) return set_error(AMDKGE_EINVAL, "train_step_tiled: null triples");
    if (!d_neg_override && (sample_range <= 0 || sample_range > 0xFFFFFFFFll || sample_base < 0 || sample_base + sample_range > m->n_ents))
        return set_error(AMDKGE_EINVAL, "train_step_tiled: sampling range outside the entity table");
    const int ks = stored_k(m), K = row_floats(m);
    hipStream_t st = (hipStream_t)stream;
    char* w = aligned_base(d_work);
    if (int rc = plan_guard(d_work, p, w, st)) return rc;
    int* counters = (int*)(w + p.off_cnt);
    StageEntry* lists = (StageEntry*)(w + p.off_lists);
    StageEntry* ovf = (StageEntry*)(w + p.off_ovf);
    float* stage_rows = (float*)(w + p.off_rows);
    float* rel_cs = (float*)(w + p.off_cs);
    const bool lazy = opt->lazy != 0;
    uint8_t* touched = (lazy && apply_update && (flags & AMDKGE_TILED_POS_ATOMIC)) ? (uint8_t*)(w + p.off_touch) : nullptr;

    TrainArgs f{};
    f.ent = d_ent; f.rel = d_rel; f.triples = d_triples; f.neg_override = d_neg_override;
    f.g_ent = d_grad_ent; f.g_rel = d_grad_rel; f.pos_atomic = (flags & AMDKGE_TILED_POS_ATOMIC) ? 1 : 0; f.loss_sum = d_loss_sum; f.pos_scores = d_pos_scores; f.neg_scores = d_neg_scores;
    f.B = B; f.eta = eta; f.k = ks; f.K = K; f.k_live = m->k; f.nq = ks / 4;
    f.sc = SampleCfg{sample_base, (uint32_t)sample_range, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step,
                     (uint32_t)(step >> 32), row_offset, b_global > 0 ? b_global : B};
    f.mc = model_const(m); f.loss = *loss;
    const bool hot = (flags & AMDKGE_TILED_HOT_ROWS) && !det && !(flags & AMDKGE_TILED_POS_ATOMIC);
    f.hot_map = hot ? (const uint8_t*)(w + p.off_hot_map) : nullptr; f.hot_buf = (float*)(w + p.off_hot_buf);
    f.rel_cs = (m->scoring_type == AMDKGE_ROTATE && B > 0) ? rel_cs : nullptr;   // filled by rel_phase_kernel below, before F
    f.touched = touched; f.ns = p.ns; f.det = det ? 1 : 0;
    f.sign_codes = (p.codes && !given) ? (uint32_t*)(w + p.off_codes) : nullptr;   // (the column-sharded stage kernel hands TransE tiles the three-row form)
    if (given) { f.pos_scores = nullptr; f.neg_scores = nullptr; }
    f.loss_parts = (double*)(w + p.off_loss);
    f.stage_rows = stage_rows; f.st_lists = lists; f.st_ovf = ovf; f.st_counters = counters;
    f.st_tile_rows = p.tile_rows; f.st_n_tiles = p.n_tiles; f.st_cap = p.cap; f.st_ovf_cap = p.ovf_cap; f.st_rb = p.rb;
#ifdef KGE_ABLATE
    { const char* e = getenv("AMDKGE_DEBUG"); f.dbg = e ? atoi(e) : 0; }
#endif

    TileArgs te{};
    te.x = d_ent; te.s0 = d_ent_slot0; te.s1 = d_ent_slot1; te.g_ent = d_grad_ent; te.apply_update = apply_update ? 1 : 0; te.pos_atomic = (flags & AMDKGE_TILED_POS_ATOMIC) ? 1 : 0; te.rel = d_rel;
    te.rel_cs = rel_cs; te.lazy = lazy ? 1 : 0; te.touched = touched; te.ns = p.ns; te.det = det ? 1 : 0; te.sort_cap = p.sort_cap;
    te.pos_bits = 0;
    while (te.pos_bits < 31 && ((int64_t)1 << te.pos_bits) < B) ++te.pos_bits;
    te.sign_codes = f.sign_codes; te.eta = eta; te.own_cache = p.own_cache ? 1 : 0; te.direct = p.direct ? 1 : 0;
    te.n_rels = m->n_rels; te.loss_parts = f.loss_parts; te.loss_sum = d_loss_sum; te.hot_map = f.hot_map; te.hot_buf = f.hot_buf;
#ifdef KGE_ABLATE
    te.dbg = f.dbg;
#endif
    te.triples = d_triples; te.stage_rows = stage_rows; te.lists = lists; te.ovf = ovf; te.counters = counters; te.status_flag = (int*)(w + p.off_flag);
    te.reg_loss = d_reg_loss; te.n_rows = m->n_ents; te.k = ks; te.K = K; te.k_live = m->k; te.nq = ks / 4;
    te.tile_rows = p.tile_rows; te.n_tiles = p.n_tiles; te.cap = p.cap; te.ovf_cap = p.ovf_cap; te.rb = p.rb; te.mc = f.mc;
    fill_opt_args(te.opt, opt);
    // Whole step in two launches when nothing in the tile pass reads the live relation table and the tables are updated in
    // place: the relation sweep rides in extra workgroups of the tile kernel.  That holds for the trilinear models (their
    // entries need the staged side row only) and for RotatE (staged side row, already rotated, + the owner's row; the forward
    // kernel read the relation through the per-step phase table).  TransE tiles read live relation rows (the three-row form of
    // an entry: all of them in deterministic mode, the near-zero units otherwise), so its sweep stays a separate launch behind.
    const bool rel_here = apply_update && d_rel_slot_ok;
    // (the touched-rows relation sweep is row-wise: it runs as its own launch behind the tiles)
    const bool fuse_rel = rel_here && !lazy && m->scoring_type != AMDKGE_TRANSE;
    te.rel_blocks = 0;
    if (rel_here) {
        te.rel_opt = te.opt;
        te.rel_opt.x = d_rel; te.rel_opt.g = d_grad_rel; te.rel_opt.s0 = d_rel_slot0; te.rel_opt.s1 = d_rel_slot1;
        te.rel_opt.n = (int64_t)m->n_rels * K; te.rel_opt.reg_loss = d_reg_loss;
        set_reg_terms(te.rel_opt, opt->rel_reg_p > 0 ? opt->rel_reg_p : opt->reg_p, rel_reg_lambda, opt->rel_reg2_p, opt->rel_reg2_lambda);
        if (fuse_rel) {
            const int64_t n4 = (te.rel_opt.n + 3) / 4;
            te.rel_blocks = (int)((n4 + TILE_THREADS - 1) / TILE_THREADS < 64 ? (n4 + TILE_THREADS - 1) / TILE_THREADS : 64);
        }
    }
    // B == 0 still runs the tiles: with no gradient the optimizer sweep must decay the slots / apply the
    // regulariser exactly like the dense path does
    int rc;
    if (m->scoring_type == AMDKGE_ROTATE && B > 0) {
        const int64_t nel = (int64_t)m->n_rels * ks;
        hipLaunchKernelGGL(rel_phase_kernel, dim3((unsigned)((nel + 255) / 256)), dim3(256), 0, st, d_rel, (int64_t)m->n_rels, ks, K, f.mc, rel_cs);
        if ((rc = check_launch("rel_phase"))) return rc;
    }
    rc = run_tiled(m->scoring_type, f, te, st, given ? d_pos_scores : nullptr);
    if (rc != AMDKGE_OK || !rel_here || fuse_rel) return rc;
    amdkge_opt ro = *opt;
    ro.reg_lambda = rel_reg_lambda;
    if (opt->rel_reg_p > 0) ro.reg_p = opt->rel_reg_p;
    ro.reg2_p = opt->rel_reg2_p; ro.reg2_lambda = opt->rel_reg2_lambda;
    ro.row_floats = K;
    return amdkge_opt_step(&ro, d_rel, d_grad_rel, d_rel_slot0, d_rel_slot1, (int64_t)m->n_rels * K, d_reg_loss, stream);
}

extern "C" int amdkge_train_tiled_status(const amdkge_model* m, int64_t B, int32_t eta, int32_t flags, void* d_work, int32_t* status, void* stream) {
    if (int rc = validate_model(m)) return rc;
    if (!d_work || !status) return set_error(AMDKGE_EINVAL, "train_tiled_status: NULL pointer");
    *status = 0;
    TiledPlan p;
    if (!make_plan(m, B, eta, p, (flags & AMDKGE_TILED_DETERMINISTIC) != 0)) return set_error(AMDKGE_EUNSUPPORTED, "train_tiled_status: shape not supported");
    char* w = aligned_base(d_work);
    int* flag = (int*)(w + p.off_flag);   // the same place whatever B / flags the flagged step ran with
    hipStream_t st = (hipStream_t)stream;
    if (hipError_t e = hipMemcpyAsync(status, flag, sizeof(int), hipMemcpyDeviceToHost, st)) return set_error_hip(e, "hipMemcpyAsync(status)");
    if (hipError_t e = hipStreamSynchronize(st)) return set_error_hip(e, "hipStreamSynchronize");
    if (*status) { if (hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), st)) return set_error_hip(e, "hipMemsetAsync(status)"); }
    return AMDKGE_OK;
}

namespace kge {
__global__ void hot_map_kernel(const int32_t* ids, int n, int64_t n_ents, uint8_t* map) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && ids[i] >= 0 && ids[i] < n_ents) map[ids[i]] = (uint8_t)(i + 1);
}
}  // namespace kge

extern "C" int amdkge_train_tiled_set_hot_rows(const amdkge_model* m, void* d_work, const int32_t* d_hot_ids, int32_t n_hot, void* stream) {
    if (int rc = validate_model(m)) return rc;
    if (!d_work || n_hot < 0 || n_hot > HOT_MAX || (n_hot > 0 && !d_hot_ids)) return set_error(AMDKGE_EINVAL, "set_hot_rows: bad arguments (at most 64 hot rows)");
    TiledPlan p;
    if (!make_plan(m, 1, 1, p)) return set_error(AMDKGE_EUNSUPPORTED, "set_hot_rows: shape not supported by the owner-computes path");
    char* w = aligned_base(d_work);
    hipStream_t st = (hipStream_t)stream;
    const int K = row_floats(m);
    if (hipError_t e = hipMemsetAsync(w + p.off_hot_map, 0, (size_t)m->n_ents, st)) return set_error_hip(e, "hipMemsetAsync(hot map)");
    if (hipError_t e = hipMemsetAsync(w + p.off_hot_buf, 0, (size_t)HOT_MAX * HOT_REPL * K * 4, st)) return set_error_hip(e, "hipMemsetAsync(hot replicas)");
    if (n_hot > 0) {
        hipLaunchKernelGGL(hot_map_kernel, dim3(1), dim3(64), 0, st, d_hot_ids, (int)n_hot, (int64_t)m->n_ents, (uint8_t*)(w + p.off_hot_map));
        return check_launch("set_hot_rows");
    }
    return AMDKGE_OK;
}
