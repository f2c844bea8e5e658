// Relation prediction: the scores of (s_i, r_j, o_i) for EVERY candidate relation r_j of every query pair -- a 1-vs-all pass over
// the RELATION table -- and the rank counts of a true relation against them.  (The reference completes a relation by materialising
// one string triple per candidate and calling predict, discovery/discovery.py:1096-1120; it has no relation ranks.)
//
// Contract: every score has the bits amdkge_score returns for the materialised triple.  The chain of score_kernel (kge_score.hip)
// is kept literally: unit group q of a row belongs to lane q % 64 (q = lane, lane + 64, ...), a lane adds its units' score_unit
// values in (q, u) order into one fp32 partial starting at +0, the 64 partials meet in wave_sum's tree -- wave_sum_multi
// (kge_device.h) forms it for eight relations at once -- and the total is scaled by score_sign * score_scale.
//
// What changes is where the operands come from.  A wave keeps the s and o fragments of QPW queries in registers and walks the
// candidate relations in groups of eight: a relation fragment is loaded once and used for all QPW queries, the 8 x QPW partials
// stay in registers until the group's transposing reduction, and lanes 0 .. 7 store eight adjacent scores of a row.  Nothing is
// materialised: the parent's way reads three rows per (query, relation) pair, this one reads a relation row per QPW pairs.
//   register form : padded stored layout (VEC = 4), up to four lane iterations (stored half width <= 1024 units); QPW = 4 / 2 / 1
//                   by the size of a query's fragments (<= 16 / <= 32 / <= 64 registers)
//   reload form   : every other width (more lane iterations, or the unpadded ABI layouts with VEC = 2 / 1): one query per wave,
//                   the unit-group loop outside the eight relations, the s / o fragment of a group reloaded once per eight relations
// RotatE: prep_rel_exact's fp64 sincos runs once per candidate relation unit per call (relation_prep_kernel) into [cos || sin]
// rows of the caller's workspace; the main kernel reads those rows -- the same floats score_kernel computes per pair.
#include "kge_rank_common.h"

namespace kge {

struct RelArgs {
    const float* ent;
    const float* rel;          // the relation table, or (RotatE) the prepared [cos || sin] rows of the candidates
    const int32_t* triples;
    const int32_t* rel_ids;    // candidate j is row rel_ids[rel_lo + j], or rel_lo + j
    int64_t rel_lo;
    int64_t n;
    int m;                     // candidates
    int rch;                   // candidates per blockIdx.y slice (a multiple of 8)
    int k, K, nq;              // stored units per half, floats per row, VEC-groups per half
    ModelConst mc;
    float* out;
    int64_t ld;
};

template <int MODEL, int VEC>
__device__ __forceinline__ void load_frag(const float* row, int q, int k, bool ok, float (&f)[VEC][ModelTraits<MODEL>::NC]) {
    constexpr int NC = ModelTraits<MODEL>::NC;
#pragma unroll
    for (int h = 0; h < NC; ++h) {
        fvec<VEC> v;
        if (ok) {
            v = ldg<VEC>(row + q * VEC + h * k);
        } else {
#pragma unroll
            for (int u = 0; u < VEC; ++u) v.v[u] = 0.f;
        }
#pragma unroll
        for (int u = 0; u < VEC; ++u) f[u][h] = v.v[u];
    }
}

__device__ __forceinline__ const float* rel_row(const RelArgs& a, int j) {
    const int64_t r = a.rel_ids ? (int64_t)a.rel_ids[a.rel_lo + j] : a.rel_lo + j;
    return a.rel + r * a.K;
}

// lanes 0 .. 7 hold the eight totals of a group (lane l that of relation j0 + wave_multi_slot(l)): eight adjacent floats of a row
__device__ __forceinline__ void store_group(const RelArgs& a, int64_t i, int j0, int j_end, int lane, float tot) {
    const int j = j0 + wave_multi_slot(lane);
    if (lane < 8 && j < j_end) a.out[i * a.ld + j] = a.mc.score_sign * a.mc.score_scale * tot;
}

template <int MODEL, int NIT, int QPW>
__global__ __launch_bounds__(256) void relation_scores_kernel(RelArgs a) {
    constexpr int NC = ModelTraits<MODEL>::NC, VEC = 4;
    const int lane = threadIdx.x & 63;
    const int64_t i0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * QPW;
    if (i0 >= a.n) return;
    const WaveMultiSel sel = wave_multi_sel(lane);
    float s[QPW][NIT][VEC][NC], o[QPW][NIT][VEC][NC];
#pragma unroll
    for (int qi = 0; qi < QPW; ++qi) {
        const int64_t i = i0 + qi < a.n ? i0 + qi : a.n - 1;   // (a short last group recomputes the last query; it stores nothing)
        const float* rs = a.ent + (int64_t)a.triples[3 * i + 0] * a.K;
        const float* ro = a.ent + (int64_t)a.triples[3 * i + 2] * a.K;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int q = lane + it * KGE_WAVE;
            load_frag<MODEL, VEC>(rs, q, a.k, q < a.nq, s[qi][it]);
            load_frag<MODEL, VEC>(ro, q, a.k, q < a.nq, o[qi][it]);
        }
    }
    const int j_begin = blockIdx.y * a.rch;
    const int j_end = j_begin + a.rch < a.m ? j_begin + a.rch : a.m;
    for (int j0 = j_begin; j0 < j_end; j0 += 8) {
        float part[QPW][8];
#pragma unroll
        for (int qi = 0; qi < QPW; ++qi)
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) part[qi][jj] = 0.f;
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            const float* rp = rel_row(a, j0 + jj < j_end ? j0 + jj : j_end - 1);   // (past the end: the last row again, not stored)
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int q = lane + it * KGE_WAVE;
                const bool ok = q < a.nq;
                float p[VEC][NC];
                load_frag<MODEL, VEC>(rp, q, a.k, ok, p);
#pragma unroll
                for (int u = 0; u < VEC; ++u)
#pragma unroll
                    for (int qi = 0; qi < QPW; ++qi) {
                        const float x = score_unit<MODEL>(s[qi][it][u], p[u], o[qi][it][u]);
                        part[qi][jj] = ok ? part[qi][jj] + x : part[qi][jj];   // score_kernel's lanes beyond nq add nothing
                    }
            }
        }
#pragma unroll
        for (int qi = 0; qi < QPW; ++qi) {
            const float tot = wave_sum_multi<8>(part[qi], sel);
            if (i0 + qi < a.n) store_group(a, i0 + qi, j0, j_end, lane, tot);
        }
    }
}

template <int MODEL, int VEC>
__global__ __launch_bounds__(256) void relation_scores_reload_kernel(RelArgs a) {
    constexpr int NC = ModelTraits<MODEL>::NC;
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= a.n) return;
    const WaveMultiSel sel = wave_multi_sel(lane);
    const float* rs = a.ent + (int64_t)a.triples[3 * i + 0] * a.K;
    const float* ro = a.ent + (int64_t)a.triples[3 * i + 2] * a.K;
    const int j_begin = blockIdx.y * a.rch;
    const int j_end = j_begin + a.rch < a.m ? j_begin + a.rch : a.m;
    for (int j0 = j_begin; j0 < j_end; j0 += 8) {
        const float* rp[8];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) rp[jj] = rel_row(a, j0 + jj < j_end ? j0 + jj : j_end - 1);
        float part[8];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) part[jj] = 0.f;
        for (int q = lane; q < a.nq; q += KGE_WAVE) {
            float s[VEC][NC], o[VEC][NC];
            load_frag<MODEL, VEC>(rs, q, a.k, true, s);
            load_frag<MODEL, VEC>(ro, q, a.k, true, o);
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                float p[VEC][NC];
                load_frag<MODEL, VEC>(rp[jj], q, a.k, true, p);
#pragma unroll
                for (int u = 0; u < VEC; ++u) part[jj] += score_unit<MODEL>(s[u], p[u], o[u]);
            }
        }
        const float tot = wave_sum_multi<8>(part, sel);
        store_group(a, i, j0, j_end, lane, tot);
    }
}

// RotatE: candidate j's phases -> the declared (cos, sin) of prep_rel_exact, as a row [cos(k) || sin(k)] of the workspace
__global__ __launch_bounds__(256) void relation_prep_kernel(const float* __restrict__ rel, const int32_t* __restrict__ rel_ids, int64_t rel_lo,
                                                            int m, int k, int K, ModelConst mc, float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)m * k) return;
    const int j = (int)(t / k), u = (int)(t % k);
    const int64_t r = rel_ids ? (int64_t)rel_ids[rel_lo + j] : rel_lo + j;
    float p[2] = {rel[r * K + u], 0.f};
    prep_rel_exact<AMDKGE_ROTATE>(mc, p);
    out[(int64_t)j * K + u] = p[0];
    out[(int64_t)j * K + k + u] = p[1];
}

// One wave per row of the score block: quantised comparisons of the positive against every column, and -- for the columns whose
// relation the row's filter holds -- the "<=" count amdkge_rank_compose subtracts.  With a subset, a relation's column is
// subset_pos[id] (a repeated id: the last one, as on the entity sides).
__global__ __launch_bounds__(256) void relation_counts_kernel(const float* __restrict__ scores, int64_t n, int m, int64_t ld, const float* __restrict__ pos,
                                                              const int32_t* __restrict__ col_ids, int64_t id_base, const int64_t* __restrict__ flt_lo,
                                                              const int64_t* __restrict__ flt_hi, const int32_t* __restrict__ flt_ids,
                                                              const int32_t* __restrict__ subset_pos, int32_t* __restrict__ counts, int32_t* __restrict__ sub) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int qp = quantise(pos[i]);
    const int64_t lo = flt_lo ? flt_lo[i] : 0, hi = flt_lo ? flt_hi[i] : 0;
    const float* row = scores + i * ld;
    int gt = 0, eq = 0, known = 0;
    for (int j = lane; j < m; j += KGE_WAVE) {
        const int q = quantise(row[j]);
        gt += qp < q ? 1 : 0;
        eq += qp == q ? 1 : 0;
        if (lo < hi && qp <= q) {
            const int64_t id = col_ids ? (int64_t)col_ids[j] : id_base + j;
            if ((!subset_pos || subset_pos[id] == j) && sorted_contains(flt_ids, lo, hi, id)) ++known;
        }
    }
    gt = wave_sum_i(gt); eq = wave_sum_i(eq);
    if (lane == 0) { counts[2 * i] += gt; counts[2 * i + 1] += eq; }
    if (flt_lo) {
        known = wave_sum_i(known);
        if (lane == 0 && known) sub[i] += known;
    }
}

// queries per wave of the register form: by the registers a query's s + o fragments take (NIT * 4 * NC * 2)
constexpr int rel_qpw(int nc, int nit) { return nit * 8 * nc <= 16 ? 4 : (nit * 8 * nc <= 32 ? 2 : 1); }

template <int MODEL>
static int launch_relation(const RelArgs& a0, hipStream_t st) {
    RelArgs a = a0;
    constexpr int NC = ModelTraits<MODEL>::NC;
    const int vec = a.k % 4 == 0 ? 4 : (a.k % 2 == 0 ? 2 : 1);
    a.nq = a.k / vec;
    const int nit = (a.nq + KGE_WAVE - 1) / KGE_WAVE;
    const bool regs = vec == 4 && nit <= 4;
    const int qpw = regs ? rel_qpw(NC, nit) : 1;
    const int64_t wgs = (a.n + 4 * qpw - 1) / (4 * qpw);
    // few queries: the candidates are split over blockIdx.y so that the device still fills (each slice reloads the query fragments)
    int64_t slices = wgs >= 1024 ? 1 : (1024 + wgs - 1) / wgs;
    int rch = (int)((a.m + slices - 1) / slices);
    rch = (rch + 7) / 8 * 8;
    a.rch = rch;
    const dim3 grid((unsigned)wgs, (unsigned)((a.m + rch - 1) / rch));
#define KGE_REL_REG(NIT) hipLaunchKernelGGL((relation_scores_kernel<MODEL, NIT, rel_qpw(NC, NIT)>), grid, dim3(256), 0, st, a)
    if (regs) {
        switch (nit) {
            case 1: KGE_REL_REG(1); break;
            case 2: KGE_REL_REG(2); break;
            case 3: KGE_REL_REG(3); break;
            default: KGE_REL_REG(4); break;
        }
    } else if (vec == 4) hipLaunchKernelGGL((relation_scores_reload_kernel<MODEL, 4>), grid, dim3(256), 0, st, a);
    else if (vec == 2) hipLaunchKernelGGL((relation_scores_reload_kernel<MODEL, 2>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((relation_scores_reload_kernel<MODEL, 1>), grid, dim3(256), 0, st, a);
#undef KGE_REL_REG
    return check_launch("relation_scores");
}

}  // namespace kge

using namespace kge;

// the walk (RotatE only): the candidates' prepared rows, at the base that the library aligns up itself
static int64_t relation_work_bytes(const amdkge_model* m, int64_t n_cand) { Layout l; l.take(n_cand, (int64_t)row_floats(m) * 4); return l.any_base(l.end()); }

extern "C" int64_t amdkge_relation_workspace_bytes(const amdkge_model* m, int64_t n_cand) {
    if (validate_model(m) || n_cand < 0) return -1;
    if (m->scoring_type != AMDKGE_ROTATE) return 0;
    return relation_work_bytes(m, n_cand);
}

extern "C" int amdkge_relation_scores(const amdkge_model* m, const float* d_ent, const float* d_rel, const int32_t* d_triples, int64_t n,
                                      const int32_t* d_rel_ids, int64_t rel_lo, int64_t rel_hi, float* d_scores, int64_t ld, void* d_work,
                                      void* stream) {
    if (int rc = validate_model(m)) return rc;
    if (n < 0 || rel_lo < 0 || rel_hi < rel_lo || ld < rel_hi - rel_lo || rel_hi - rel_lo > 0x7FFFFFF0ll)
        return set_error(AMDKGE_EINVAL, "relation_scores: bad sizes (0 <= rel_lo <= rel_hi, ld >= rel_hi - rel_lo)");
    if (!d_rel_ids && rel_hi > m->n_rels) return set_error(AMDKGE_EINVAL, "relation_scores: rel_hi beyond the relation table");
    if (n > 0x7FFFFFFFll) return set_error(AMDKGE_EUNSUPPORTED, "relation_scores: too many queries for one call");
    const int64_t mc_ = rel_hi - rel_lo;
    if (n == 0 || mc_ == 0) return AMDKGE_OK;
    if (!d_ent || !d_rel || !d_triples || !d_scores) return set_error(AMDKGE_EINVAL, "relation_scores: NULL pointer");
    if (m->scoring_type == AMDKGE_ROTATE && !d_work) return set_error(AMDKGE_EINVAL, "relation_scores: RotatE needs the workspace of amdkge_relation_workspace_bytes");
    hipStream_t st = (hipStream_t)stream;
    RelArgs a{};
    a.ent = d_ent; a.rel = d_rel; a.triples = d_triples; a.rel_ids = d_rel_ids; a.rel_lo = rel_lo; a.n = n; a.m = (int)mc_;
    a.k = stored_k(m); a.K = row_floats(m); a.mc = model_const(m); a.out = d_scores; a.ld = ld;
    if (m->scoring_type == AMDKGE_ROTATE) {
        float* w = (float*)aligned_base(d_work);
        const int64_t units = mc_ * a.k;
        hipLaunchKernelGGL(relation_prep_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, st, d_rel, d_rel_ids, rel_lo, a.m, a.k, a.K, a.mc, w);
        if (int rc = check_launch("relation_prep")) return rc;
        a.rel = w; a.rel_ids = nullptr; a.rel_lo = 0;
    }
#define KGE_RUN(M) return launch_relation<M>(a, st)
    KGE_MODEL_DISPATCH(m->scoring_type, KGE_RUN)
#undef KGE_RUN
}

extern "C" int amdkge_relation_rank_counts(const float* d_scores, int64_t n, int64_t m, int64_t ld, const float* d_pos, const int32_t* d_col_ids,
                                           int64_t id_base, const int64_t* d_flt_lo, const int64_t* d_flt_hi, const int32_t* d_flt_ids,
                                           const int32_t* d_subset_pos, int32_t* d_counts, int32_t* d_sub, void* stream) {
    if (n < 0 || m < 0 || ld < m || m > 0x7FFFFFF0ll) return set_error(AMDKGE_EINVAL, "relation_rank_counts: bad sizes (ld >= m)");
    if ((d_flt_lo == nullptr) != (d_flt_hi == nullptr) || (d_flt_lo == nullptr) != (d_flt_ids == nullptr))
        return set_error(AMDKGE_EINVAL, "relation_rank_counts: the filter is (lo, hi, ids) or three NULLs");
    if (n == 0) return AMDKGE_OK;
    if (!d_pos || !d_counts || (m > 0 && !d_scores) || (d_flt_lo && !d_sub)) return set_error(AMDKGE_EINVAL, "relation_rank_counts: NULL pointer");
    hipLaunchKernelGGL(relation_counts_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, d_scores, n, (int)m, ld, d_pos, d_col_ids,
                       id_base, d_flt_lo, d_flt_hi, d_flt_ids, d_subset_pos, d_counts, d_sub);
    return check_launch("relation_rank_counts");
}
