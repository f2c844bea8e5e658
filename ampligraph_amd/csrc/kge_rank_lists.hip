// evaluate_candidates(): ranks against PER-TRIPLE candidate lists (include/amdkge_lists.h).
//   rank_lists : triple i is ranked against the table rows d_cand_ids[d_cand_lo[i] .. d_cand_hi[i]) -- sampled negatives (ogbl-wikikg2's
//                500 heads and 500 tails per test triple), the output of a first retrieval stage, a relation's domain / range --
//                instead of one candidate set shared by the whole call.  Same prep (run_prep: query vector, quantised positive
//                score), same accumulation chain (rank_op / rot_exact_op, kge_rank_common.h) and same quantisation as the tile, filter
//                and recheck kernels: a list that is the id range 0 .. N-1 gives amdkge_rank_counts' counts, bit for bit.
// The pass is a gather: n x C entity rows, each used once, so what matters is how the rows are fetched.  One lane walking its own
// row 16 bytes at a time is bound by the address path, not by the bytes (kge_rank_screen.h, section 3), so the list kernel fetches
// like the recheck kernels do: a wave takes 64 candidates, loads a chunk of their 64 rows COALESCED (whole 128- / 64-byte pieces
// of a row per 8 / 16 lanes), parks it in its private LDS region, and every lane then walks its own candidate's chunk in unit
// order from LDS (row stride CH + 4 floats: conflict-free).  The chunk after the one being multiplied is already in flight.
// Unlike the recheck kernels' pairs the 64 candidates of a wave share ONE query: its chunk is loaded once per wave (NQF x CH / 4
// lanes, one 16-byte piece each) and read back as an LDS broadcast.
// Work split: a workgroup serves one query; its 4 waves, and those of the `splits` workgroups of that query (grid.y, planned on the
// host from max_len), take the query's groups of 64 candidates round robin -- a handful of queries with long lists still fills the
// device, thousands of queries with 500 candidates need no second dimension.  A list longer than max_len is walked all the same.
// LDS: one-plane modes (contraction models, TransE) 32-unit chunks, 4 waves x 64 rows x 36 floats = 36 KB (37.5 KB with the query
// chunks and the staged filter ids) -> 4 workgroups per CU; RotatE (two entity planes) 16-unit chunks, 4 x 2 x 64 x 20 floats = 40 KB
// (42 KB) -> 3 workgroups per CU.  32-unit chunks would cost RotatE 74 KB (2 workgroups per CU, and the dynamic-LDS attribute) for
// nothing: its time is the square roots, not the fetches.  Measured: DESIGN section 3, "Candidate lists".
#include "kge_rank_common.h"

namespace kge {

struct ListArgs {
    const float* ent;
    const float* Q;
    const int* qpos;
    const int64_t* cand_lo;
    const int64_t* cand_hi;
    const int32_t* cand_ids;
    const int64_t* flt_lo;     // all three NULL: unfiltered
    const int64_t* flt_hi;
    const int32_t* flt_ids;
    int32_t* counts;
    int32_t* sub;
    float* scores;             // NULL, or parallel to cand_ids
    int64_t n_ents;
    RankGeom g;
    float sgn_scale;
};

// A triple's known positives, as the wave that ranks it sees them.  Every candidate that outranks the positive is looked up among
// them -- on untrained tables that is half of all candidates --, and a lookup in global memory is a chain of dependent loads at
// the end of each group of 64.  Ranges of up to FLT_STAGE ids (all but a few: a (p, o) key has a handful of subjects) are
// copied once per wave into LDS and searched there; a longer range is searched where it lies.
constexpr int FLT_STAGE = 64;
struct KnownIds {
    const int32_t* lds = nullptr;
    const int32_t* glob = nullptr;
    int64_t lo = 0, hi = 0;
    // stage: this wave's FLT_STAGE ints of LDS
    __device__ __forceinline__ void init(const int64_t* flt_lo, const int64_t* flt_hi, const int32_t* flt_ids, int64_t i, int lane, int32_t* stage) {
        if (!flt_ids) return;
        lo = flt_lo[i]; hi = flt_hi[i];
        glob = flt_ids;
        if (hi - lo <= FLT_STAGE) {
            if (lane < hi - lo) stage[lane] = flt_ids[lo + lane];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            lds = stage;
        }
    }
    __device__ __forceinline__ bool active() const { return glob != nullptr; }
    __device__ __forceinline__ bool has(int32_t id) const {
        if (hi <= lo) return false;
        return lds ? sorted_contains<int>(lds, 0, (int)(hi - lo), id) : sorted_contains<int64_t>(glob, lo, hi, id);
    }
};

// what a lane does with its candidate's finished chain: the three comparisons, the score
struct ListTally {
    int gt = 0, eq = 0, sub = 0;
    __device__ __forceinline__ void add(const ListArgs& a, bool have, bool ok, int32_t id, int64_t p, float acc, int qp, const KnownIds& known) {
        const float s = a.sgn_scale * acc;
        if (a.scores && have) a.scores[p] = ok ? s : -INFINITY;
        if (!ok) return;
        const int qs = quantise(s);
        gt += qp < qs ? 1 : 0;
        eq += qp == qs ? 1 : 0;
        // always "<=", whatever the tie strategy (AbstractScoringLayer.py:292-303)
        if (known.active() && qp <= qs && known.has(id)) ++sub;
    }
    __device__ __forceinline__ void flush(const ListArgs& a, int64_t i, int lane) {
        // integer adds: the order the waves arrive in does not change the result
        const int g = wave_sum_i(gt), e = wave_sum_i(eq), s = wave_sum_i(sub);
        if (lane == 0) {
            if (g) atomicAdd(&a.counts[2 * i + 0], g);
            if (e) atomicAdd(&a.counts[2 * i + 1], e);
            if (s) atomicAdd(&a.sub[i], s);
        }
    }
};

// whole-float4 layouts (U % 4 == 0 -- RotatE's exact mode: the stored planes --, eplane % 4 == 0, K % 4 == 0)
template <int MODE, bool EXACT_ROT>
__global__ __launch_bounds__(256) void rank_lists_kernel(ListArgs a) {
    constexpr int NQF = ModeTraits<MODE>::NQF, NEF = ModeTraits<MODE>::NEF;
    constexpr int CH = NEF == 1 ? 32 : 16;   // units per chunk
    constexpr int LD = CH + 4;               // LDS row stride in floats (144 / 80 bytes)
    constexpr int PCS = CH / 4;              // 16-byte pieces per row chunk = load instructions per plane and chunk
    constexpr int RPI = 64 / PCS;            // rows per load instruction
    static_assert(NQF * PCS <= 64, "the query chunk is one piece per lane");
    __shared__ __attribute__((aligned(16))) float Es[4][NEF][64][LD];
    __shared__ __attribute__((aligned(16))) float Qs[4][NQF][CH];
    __shared__ int32_t Fs[4][FLT_STAGE];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t i = blockIdx.x;
    const int64_t lo = a.cand_lo[i], hi = a.cand_hi[i];
    const int64_t ngroups = hi > lo ? (hi - lo + 63) / 64 : 0;
    int64_t grp = (int64_t)blockIdx.y * 4 + wv;
    if (grp >= ngroups) return;   // (no workgroup barrier below: the waves are independent)
    const int64_t gstep = (int64_t)gridDim.y * 4;
    const int U = a.g.U;
    const int qp = a.qpos[i];
    KnownIds known;
    known.init(a.flt_lo, a.flt_hi, a.flt_ids, i, lane, Fs[wv]);
    const int lrow = lane / PCS, lpc = lane % PCS;   // entity loader: RPI rows per instruction, PCS pieces per row chunk
    const bool qldr = lane < NQF * PCS;              // query loader: plane lrow, piece lpc
    const float* qsrc = a.Q + i * (int64_t)a.g.QW + (qldr ? (int64_t)lrow * a.g.qplane : 0) + 4 * lpc;
    float (*E)[64][LD] = Es[wv];
    float (*Qw)[CH] = Qs[wv];
    ListTally t;
    for (; grp < ngroups; grp += gstep) {
        const int64_t p = lo + grp * 64 + lane;
        const bool have = p < hi;
        const int32_t id = have ? a.cand_ids[p] : -1;
        const bool ok = id >= 0 && (int64_t)id < a.n_ents;   // an id outside the table is no candidate: its row is never read
        const int64_t eoff = ok ? (int64_t)id * a.g.K : 0;
        int64_t eo[PCS];
#pragma unroll
        for (int r = 0; r < PCS; ++r) eo[r] = __shfl(eoff, RPI * r + lrow, 64) + 4 * lpc;
        float4 re[NEF][PCS], rq;
        auto fetch = [&](int u0) __attribute__((always_inline)) {
            const bool in = u0 + 4 * lpc < U;   // (pieces are loaded whole: the stored planes are whole float4s)
#pragma unroll
            for (int r = 0; r < PCS; ++r)
#pragma unroll
                for (int f = 0; f < NEF; ++f)
                    re[f][r] = in ? *reinterpret_cast<const float4*>(a.ent + eo[r] + (int64_t)f * a.g.eplane + u0) : make_float4(0.f, 0.f, 0.f, 0.f);
            rq = (in && qldr) ? *reinterpret_cast<const float4*>(qsrc + u0) : make_float4(0.f, 0.f, 0.f, 0.f);
        };
        float acc = 0.f;
        fetch(0);
        for (int u0 = 0; u0 < U; u0 += CH) {
#pragma unroll
            for (int r = 0; r < PCS; ++r)
#pragma unroll
                for (int f = 0; f < NEF; ++f) *reinterpret_cast<float4*>(&E[f][RPI * r + lrow][4 * lpc]) = re[f][r];
            if (qldr) *reinterpret_cast<float4*>(&Qw[lrow][4 * lpc]) = rq;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (u0 + CH < U) fetch(u0 + CH);
#pragma unroll
            for (int c = 0; c < PCS; ++c) {
                if (u0 + 4 * c < U) {
                    float qv[NQF][4], ev[NEF][4];
#pragma unroll
                    for (int f = 0; f < NQF; ++f) {
                        const float4 v = *reinterpret_cast<const float4*>(&Qw[f][4 * c]);   // one address for the wave: a broadcast
                        qv[f][0] = v.x; qv[f][1] = v.y; qv[f][2] = v.z; qv[f][3] = v.w;
                    }
#pragma unroll
                    for (int f = 0; f < NEF; ++f) {
                        const float4 v = *reinterpret_cast<const float4*>(&E[f][lane][4 * c]);
                        ev[f][0] = v.x; ev[f][1] = v.y; ev[f][2] = v.z; ev[f][3] = v.w;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        float qq[NQF], ee[NEF];
#pragma unroll
                        for (int f = 0; f < NQF; ++f) qq[f] = qv[f][u];
#pragma unroll
                        for (int f = 0; f < NEF; ++f) ee[f] = ev[f][u];
                        if constexpr (EXACT_ROT) {   // live units only (U = k)
                            if (u0 + 4 * c + u < U) acc = rot_exact_op<MODE>(acc, qq, ee);
                        } else {
                            acc = rank_op<MODE>(acc, qq, ee, a.g.sgn);
                        }
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        t.add(a, have, ok, id, p, acc, qp, known);
    }
    t.flush(a, i, lane);
}

// any layout: the same split, every lane reads its own candidate's row unit by unit (as rank_filter_kernel<MODE, false>).  Correct,
// not tuned: the product stores padded rows.
template <int MODE>
__global__ __launch_bounds__(256) void rank_lists_scalar_kernel(ListArgs a) {
    constexpr int NQF = ModeTraits<MODE>::NQF, NEF = ModeTraits<MODE>::NEF;
    __shared__ int32_t Fs[4][FLT_STAGE];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t i = blockIdx.x;
    const int64_t lo = a.cand_lo[i], hi = a.cand_hi[i];
    const int64_t ngroups = hi > lo ? (hi - lo + 63) / 64 : 0;
    int64_t grp = (int64_t)blockIdx.y * 4 + wv;
    if (grp >= ngroups) return;
    const int64_t gstep = (int64_t)gridDim.y * 4;
    const int qp = a.qpos[i];
    KnownIds known;
    known.init(a.flt_lo, a.flt_hi, a.flt_ids, i, lane, Fs[wv]);
    const float* qrow = a.Q + i * (int64_t)a.g.QW;
    ListTally t;
    for (; grp < ngroups; grp += gstep) {
        const int64_t p = lo + grp * 64 + lane;
        const bool have = p < hi;
        const int32_t id = have ? a.cand_ids[p] : -1;
        const bool ok = id >= 0 && (int64_t)id < a.n_ents;
        const float* erow = a.ent + (ok ? (int64_t)id : 0) * a.g.K;
        float acc = 0.f;
        for (int u = 0; u < a.g.U; ++u) {
            float qq[NQF], ee[NEF];
#pragma unroll
            for (int f = 0; f < NQF; ++f) qq[f] = qrow[f * a.g.qplane + u];
#pragma unroll
            for (int f = 0; f < NEF; ++f) ee[f] = erow[f * a.g.eplane + u];
            acc = rank_op<MODE>(acc, qq, ee, a.g.sgn);
        }
        t.add(a, have, ok, id, p, acc, qp, known);
    }
    t.flush(a, i, lane);
}

}  // namespace kge

using namespace kge;

extern "C" int64_t amdkge_rank_lists_workspace_bytes(const amdkge_model* m, int64_t n) { return amdkge_rank_workspace_bytes(m, n); }

extern "C" int amdkge_rank_lists(const amdkge_model* m, const float* d_ent, const float* d_rel, int64_t n_ents,
                                 const int32_t* d_triples, int64_t n, int32_t side,
                                 const int64_t* d_cand_lo, const int64_t* d_cand_hi, const int32_t* d_cand_ids, int64_t max_len,
                                 const int64_t* d_flt_lo, const int64_t* d_flt_hi, const int32_t* d_flt_ids,
                                 int32_t* d_counts, int32_t* d_sub, float* d_scores, void* d_work, void* stream) {
    if (int rc = validate_model(m)) return rc;
    if (side != AMDKGE_SIDE_S && side != AMDKGE_SIDE_O) return set_error(AMDKGE_EINVAL, "rank_lists: side must be AMDKGE_SIDE_S or AMDKGE_SIDE_O");
    if (n < 0 || max_len < 0 || n_ents < 1 || n_ents > 0x7FFFFFFFll) return set_error(AMDKGE_EINVAL, "rank_lists: bad sizes");
    const int nflt = (d_flt_lo ? 1 : 0) + (d_flt_hi ? 1 : 0) + (d_flt_ids ? 1 : 0);
    if (nflt != 0 && nflt != 3) return set_error(AMDKGE_EINVAL, "rank_lists: d_flt_lo, d_flt_hi and d_flt_ids are given together or not at all");
    if (n == 0 || max_len == 0) return AMDKGE_OK;
    if (!d_ent || !d_rel || !d_triples || !d_cand_lo || !d_cand_hi || !d_cand_ids || !d_counts || !d_work || (nflt && !d_sub))
        return set_error(AMDKGE_EINVAL, "rank_lists: NULL pointer");
    if (n >= (1ll << 24)) return set_error(AMDKGE_EUNSUPPORTED, "rank_lists: too many triples for one launch; split them");
    const RankGeom g = geom_of(m, side);
    const int mode = mode_of(m->scoring_type, side);
    const bool rot_exact = (mode == MODE_ROT_O || mode == MODE_ROT_S) && !g_rank_cfg.rotate_fast;
    const bool v4 = (rot_exact || g.U % 4 == 0) && (g.eplane % 4 == 0) && (g.K % 4 == 0);
    if (rot_exact && !v4) return set_error(AMDKGE_EUNSUPPORTED, "rank_lists: RotatE's exact mode needs the padded stored layout (k_pad = amdkge_padded_k(k))");
    hipStream_t st = (hipStream_t)stream;
    const Workspace w = carve(d_work, m, n);
    if (int rc = run_prep(m, d_ent, d_rel, d_triples, n, side, g, w, st)) return rc;
    const ModelConst mc = model_const(m);
    ListArgs a{};
    a.ent = d_ent; a.Q = w.Q; a.qpos = w.qpos; a.cand_lo = d_cand_lo; a.cand_hi = d_cand_hi; a.cand_ids = d_cand_ids;
    a.flt_lo = d_flt_lo; a.flt_hi = d_flt_hi; a.flt_ids = d_flt_ids; a.counts = d_counts; a.sub = d_sub; a.scores = d_scores;
    a.n_ents = n_ents; a.g = g; a.sgn_scale = mc.score_sign * mc.score_scale;
    // workgroups per query: enough of them for 8 per CU when the queries alone are too few, never more than the longest list has
    // groups of 4 x 64 candidates for (max_len only plans: the kernels stride over whatever a list holds)
    const int64_t wg_groups = ((max_len + 63) / 64 + 3) / 4;
    int64_t splits = (2048 + n - 1) / n;
    if (splits > wg_groups) splits = wg_groups;
    if (splits > 65535) splits = 65535;
    if (splits < 1) splits = 1;
    const dim3 grid((unsigned)n, (unsigned)splits);
#define KGE_LISTS(MODE) do { if (v4) hipLaunchKernelGGL((rank_lists_kernel<MODE, false>), grid, dim3(256), 0, st, a); \
                             else hipLaunchKernelGGL((rank_lists_scalar_kernel<MODE>), grid, dim3(256), 0, st, a); } while (0)
    if (rot_exact) {
        if (mode == MODE_ROT_S) hipLaunchKernelGGL((rank_lists_kernel<MODE_ROT_S, true>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((rank_lists_kernel<MODE_ROT_O, true>), grid, dim3(256), 0, st, a);
        return check_launch("rank_lists_rot");
    }
    switch (mode) {
        case MODE_DOT: KGE_LISTS(MODE_DOT); break;
        case MODE_L1: KGE_LISTS(MODE_L1); break;
        case MODE_L1_SUB: KGE_LISTS(MODE_L1_SUB); break;
        case MODE_ROT_O: KGE_LISTS(MODE_ROT_O); break;
        default: KGE_LISTS(MODE_ROT_S); break;
    }
#undef KGE_LISTS
    return check_launch("rank_lists");
}
