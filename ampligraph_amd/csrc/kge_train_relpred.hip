// The relation-prediction training objective (include/amdkge_relation_objective.h): every positive (s_i, p_i, o_i) is scored against
// every relation, score(s_i, j, o_i) = <q_i, rel[j]> with q_i the pair query, so the B x R scores are ONE fp32 matrix product over the
// relation table read in place, and both gradients are matrix products too.  The step is DEFINED in the header as amdkge_train_fwdbwd's
// with eta = R on the override rows (s_i, j, o_i); tests/relation_objective_ref.py restates it on the oracle.
//   relpred_query_kernel : a wave per positive.  q_i = s * o (DistMult), [s0 o0 + s1 o1 || s0 o1 - s1 o0] (ComplEx / HolE) over the
//                          live units, exact zeros in the padding units; the positive's raw score comes out of the same pass
//                          (ComplEx / HolE: in the reference's operation order, which differs from <q_i, rel[p_i]> only where an inf
//                          makes both halves of q infinite).
//   relpred_gemm_kernel  : the product tile of kge_product_tile.h (exact fp32 MFMA, 64 x 64 per workgroup; which element a
//                          thread stages, which a lane feeds and which result a register holds is stated there), without
//                          groups and without an id gather: the list is the table itself.  Three MODES:
//                            FWD  : S    = Q Rel^T     (rows x K by K x R)                      -> the score buffer [rows, R]
//                            DQ   : dQ   = C' Rel      (rows x R by R x K)                      -> dQ [B, K]
//                            DREL : dRel += C'^T Q     (R x rows by rows x K), C read transposed -> atomic adds into d_grad_rel
//                          C' = weight * C, multiplied where a coefficient is staged.  Elements past a matrix edge and the padding
//                          units of a relation row are staged as zeros, so R = 1, K = 7 and a last tile of 5 rows are one code path.
//                          DREL contracts over the batch: a workgroup takes a slice of RP_SLICE rows of the chunk, so a float of a
//                          relation gradient row takes one atomic per slice, not one per positive.
//   relpred_chain_kernel : a wave per positive.  t_i = dQ_i + c_pos' rel[p_i] = dL/dq_i; the transpose of the pair-query map sends it to
//                          the s_i and o_i gradient rows, c_pos' q_i goes to row p_i of the relation gradient: three atomic row-adds.
//   relpred_loss_kernel  : one thread: *d_loss_sum += weight * (the step's loss sum, gathered in the workspace).
// The mask and the loss are shared_mask_kernel (IDENTITY list; a zeroed side array makes the pair ranges the "object" ranges) and
// shared_loss_kernel of kge_train_shared.hip, through shared_loss_stage (kge_train_shared.h), the loss stage of the shared-list steps.
// Rows, not groups, are processed in chunks of at most CHUNK_SCORES scores, so the step keeps its own chunk loop.
#include "kge_train_shared.h"
#include "kge_product_tile.h"
#include "../../include/amdkge_relation_objective.h"

namespace kge {

enum { RP_FWD = 0, RP_DQ = 1, RP_DREL = 2 };
constexpr int RP_SLICE = 512;   // DREL: batch rows per workgroup (a multiple of PKC)

// ---- pair queries -------------------------------------------------------------------------------------------------------------------
template <bool CPLX>
__global__ __launch_bounds__(256) void relpred_query_kernel(const float* __restrict__ ent, const float* __restrict__ rel, const int32_t* __restrict__ triples, int64_t B,
                                                            int ks, int k, float* __restrict__ Q, float* __restrict__ pos_raw) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= B) return;   // (wave-uniform; the kernel has no barrier)
    const int K = CPLX ? 2 * ks : ks;
    const float* S = ent + (int64_t)triples[3 * i] * K;
    const float* P = rel + (int64_t)triples[3 * i + 1] * K;
    const float* O = ent + (int64_t)triples[3 * i + 2] * K;
    float* q = Q + i * K;
    float acc = 0.f;
    for (int u = lane; u < ks; u += 64) {
        if (u >= k) {   // a padding unit: an exact zero whatever the tables hold there
            q[u] = 0.f;
            if constexpr (CPLX) q[ks + u] = 0.f;
            continue;
        }
        if constexpr (CPLX) {
            const float s0 = S[u], s1 = S[ks + u], o0 = O[u], o1 = O[ks + u];
            const float q0 = s0 * o0 + s1 * o1, q1 = s0 * o1 - s1 * o0;
            const float p0 = P[u], p1 = P[ks + u];
            q[u] = q0; q[ks + u] = q1;
            // the positive's own score in the reference's operation order (score_unit of kge_device.h): with an inf in s or o both
            // halves of q are infinite and <q, p> would be inf - inf = NaN where the reference has +-inf
            acc += s0 * (p0 * o0 + p1 * o1) + s1 * (p0 * o1 - p1 * o0);
        } else {
            const float qq = S[u] * O[u];
            q[u] = qq;
            acc += qq * P[u];
        }
    }
    acc = wave_sum_shfl(acc);
    if (lane == 0) pos_raw[i] = acc;
}

// ---- the three matrix products ------------------------------------------------------------------------------------------------------
struct RelGemmArgs {
    const float* ent;
    const float* rel;
    const int32_t* triples;
    const float* Q;   // [B, K]
    float* S;         // [rows, R]: scores, then dL/dscore
    float* dQ;        // [B, K]
    float* g_rel;
    int64_t row0;     // first batch row of the chunk
    int rows;         // rows of the chunk (rows * R <= max(CHUNK_SCORES, R))
    int R, K;
    int ks, k;        // units per half as stored, live units
    int cplx;         // ComplEx / HolE: a non-finite score is recomputed in the reference's operation order
    float w;          // the weight: C' = w * C where a coefficient is staged
    int tiles_n;
    int per_slice;    // tiles_m * tiles_n
};

// The score of (s_i, j, o_i) of a ComplEx / HolE positive in the reference's own operation order (cplx_reference_score): only for a
// score that the matrix product made +-inf or NaN.
__device__ float relpred_reference_score(const RelGemmArgs& a, int64_t i, int j) {
    const int32_t* t = a.triples + 3 * i;
    return cplx_reference_score(a.ent + (int64_t)t[0] * a.K, a.rel + (int64_t)j * a.K, a.ent + (int64_t)t[2] * a.K, a.ks, a.k);
}

template <int MODE>
__global__ __launch_bounds__(256) void relpred_gemm_kernel(RelGemmArgs a) {
    __shared__ float As[PKC][PLD];
    __shared__ float Bs[PKC][PLD];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tile = blockIdx.x % a.per_slice;
    const int sl0 = MODE == RP_DREL ? (int)(blockIdx.x / a.per_slice) * RP_SLICE : 0;   // first chunk row of the slice
    const int m0 = (tile / a.tiles_n) * PT, n0 = (tile % a.tiles_n) * PT;
    const int mdim = MODE == RP_DREL ? a.R : a.rows;
    const int ndim = MODE == RP_FWD ? a.R : a.K;
    const int kdim = MODE == RP_FWD ? a.K : (MODE == RP_DQ ? a.R : ((a.rows - sl0) < RP_SLICE ? (a.rows - sl0) : RP_SLICE));
    const float* Qc = a.Q + a.row0 * a.K;   // the chunk's queries

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    for (int k0 = 0; k0 < kdim; k0 += PKC) {
        // ---- stage A[m][kk] ----
        if (MODE == RP_DREL) {   // contiguous along m: C[kk][m]
            const int mm = product_x_x(tid);
#pragma unroll
            for (int r = 0; r < PSTAGE; ++r) {
                const int kk = product_x_kk(tid, r);
                float v = 0.f;
                if (m0 + mm < mdim && k0 + kk < kdim) v = a.w * a.S[(int64_t)(sl0 + k0 + kk) * a.R + (m0 + mm)];
                As[kk][mm] = v;
            }
        } else {                 // contiguous along the contraction: Q[m][kk] / C[m][kk]
            const int kk = product_k_kk(tid);
#pragma unroll
            for (int r = 0; r < PSTAGE; ++r) {
                const int mm = product_k_x(tid, r);
                float v = 0.f;
                if (m0 + mm < mdim && k0 + kk < kdim)
                    v = MODE == RP_FWD ? Qc[(int64_t)(m0 + mm) * a.K + (k0 + kk)] : a.w * a.S[(int64_t)(m0 + mm) * a.R + (k0 + kk)];
                As[kk][mm] = v;
            }
        }
        // ---- stage B[kk][n] ----
        if (MODE == RP_FWD) {    // contiguous along the contraction: Rel[n][kk]; a padding unit is staged as zero
            const int kk = product_k_kk(tid);
            const bool live = k0 + kk < kdim && (k0 + kk) % a.ks < a.k;
#pragma unroll
            for (int r = 0; r < PSTAGE; ++r) {
                const int nn = product_k_x(tid, r);
                float v = 0.f;
                if (n0 + nn < ndim && live) v = a.rel[(int64_t)(n0 + nn) * a.K + (k0 + kk)];
                Bs[kk][nn] = v;
            }
        } else {                 // contiguous along n: Rel[kk][n] / Q[kk][n]
            const int nn = product_x_x(tid);
            const bool live = n0 + nn < ndim && (n0 + nn) % a.ks < a.k;
#pragma unroll
            for (int r = 0; r < PSTAGE; ++r) {
                const int kk = product_x_kk(tid, r);
                float v = 0.f;
                if (live && k0 + kk < kdim)
                    v = MODE == RP_DQ ? a.rel[(int64_t)(k0 + kk) * a.K + (n0 + nn)] : Qc[(int64_t)(sl0 + k0 + kk) * a.K + (n0 + nn)];
                Bs[kk][nn] = v;
            }
        }
        __syncthreads();
        const int wm = product_quad_row(wv) * PQ + product_in_quad(lane), wn = product_quad_col(wv) * PQ + product_in_quad(lane), kh = product_kh(lane);
#pragma unroll
        for (int kk = 0; kk < PKC; kk += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + kh][wm], Bs[kk + kh][wn], acc, 0, 0, 0);
        __syncthreads();
    }
    const int col = product_col(n0, product_quad_col(wv), lane);
    if (col >= ndim) return;
    // the padding floats of a gradient row are never written (DQ's padding columns are exact zeros or NaN: the chain kernel skips them)
    if (MODE == RP_DREL && col % a.ks >= a.k) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = product_row(m0, product_quad_row(wv), lane, r);
        if (row >= mdim) continue;
        float v = acc[r];
        if (MODE == RP_FWD) {
            // (an inf in a table: rare, divergent.  NaN too: an inf in s or o makes BOTH halves of q infinite, and inf - inf is NaN
            // where the reference's order has +-inf)
            if (a.cplx && !__builtin_isfinite(v)) v = relpred_reference_score(a, a.row0 + row, col);
            a.S[(int64_t)row * a.R + col] = v;
        }
        else if (MODE == RP_DQ) a.dQ[(a.row0 + row) * a.K + col] = v;
        else if (v != 0.f) atomic_add_f32(a.g_rel + (int64_t)row * a.K + col, v);   // (true for NaN; exact zeros add nothing)
    }
}

// ---- the transpose of the pair-query map --------------------------------------------------------------------------------------------
template <bool CPLX>
__global__ __launch_bounds__(256) void relpred_chain_kernel(const float* __restrict__ ent, const float* __restrict__ rel, const int32_t* __restrict__ triples, int64_t B,
                                                            int ks, int k, float w, const float* __restrict__ Q, const float* __restrict__ dQ,
                                                            const float* __restrict__ cpos, float* g_ent, float* g_rel) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= B) return;
    const int K = CPLX ? 2 * ks : ks;
    const int64_t so = (int64_t)triples[3 * i] * K, po = (int64_t)triples[3 * i + 1] * K, oo = (int64_t)triples[3 * i + 2] * K;
    const float* S = ent + so;
    const float* P = rel + po;
    const float* O = ent + oo;
    const float* q = Q + i * K;
    const float* d = dQ + i * K;
    const float c = w * cpos[i];
    float* g_s = g_ent + so;
    float* g_o = g_ent + oo;
    float* g_p = g_rel + po;
    for (int u = lane; u < k; u += 64) {   // the live units only
        if constexpr (CPLX) {
            const float s0 = S[u], s1 = S[ks + u], o0 = O[u], o1 = O[ks + u];
            const float t0 = d[u] + c * P[u], t1 = d[ks + u] + c * P[ks + u];   // dL/dq
            add_nz(g_s + u, t0 * o0 + t1 * o1); add_nz(g_s + ks + u, t0 * o1 - t1 * o0);
            add_nz(g_o + u, t0 * s0 - t1 * s1); add_nz(g_o + ks + u, t0 * s1 + t1 * s0);
            add_nz(g_p + u, c * q[u]); add_nz(g_p + ks + u, c * q[ks + u]);
        } else {
            const float t = d[u] + c * P[u];
            add_nz(g_s + u, t * O[u]);
            add_nz(g_o + u, t * S[u]);
            add_nz(g_p + u, c * q[u]);
        }
    }
}

__global__ void relpred_loss_kernel(const double* __restrict__ step_sum, float w, double* loss_sum) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const double t = (double)w * *step_sum;
        if (t != 0.0) atomicAdd(loss_sum, t);   // (true for NaN)
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// the workspace of a step: the step's loss sum (a double), Q, dQ [B, K], the positives' raw scores and coefficients [B], the zeroed
// side array of the mask [B], the score buffer of one chunk [rows, R]
struct RelPlan {
    int64_t rpc, off_sum, off_q, off_dq, off_pos, off_cpos, off_side, off_s, total;
};
static bool relpred_plan(const amdkge_model* m, int64_t B, RelPlan& p) {
    const int64_t R = m->n_rels, K = row_floats(m);
    if (B < 1 || R < 1 || R > AMDKGE_SHARED_MAX_NEGS) return false;
    p.rpc = CHUNK_SCORES / R;
    if (p.rpc < 1) p.rpc = 1;
    if (p.rpc > B) p.rpc = B;
    Layout l;   // (the caller's base is used as it is)
    p.off_sum = l.take(256);
    p.off_q = l.take(B * K, 4); p.off_dq = l.take(B * K, 4);
    p.off_pos = l.take(B, 4); p.off_cpos = l.take(B, 4); p.off_side = l.take(B, 4);
    p.off_s = l.take(p.rpc * R, 4); p.total = l.next();
    return true;
}

template <bool CPLX>
static int run_relpred(const amdkge_model* m, const amdkge_loss* loss, float w, const float* d_ent, const float* d_rel, const int32_t* d_triples, int64_t B,
                       float* g_ent, float* g_rel, double* d_loss_sum, float* d_pos_scores, float* d_rel_scores, char* work, const RelPlan& p,
                       const SharedMaskArgs* mask, hipStream_t st) {
    const int ks = stored_k(m), K = row_floats(m), k = m->k, R = (int)m->n_rels;
    const ModelConst mc = model_const(m);
    const float scale = mc.score_sign * mc.score_scale;
    double* step_sum = reinterpret_cast<double*>(work + p.off_sum);
    float* Q = reinterpret_cast<float*>(work + p.off_q);
    float* dQ = reinterpret_cast<float*>(work + p.off_dq);
    float* pos_raw = reinterpret_cast<float*>(work + p.off_pos);
    float* cpos = reinterpret_cast<float*>(work + p.off_cpos);
    int32_t* side = reinterpret_cast<int32_t*>(work + p.off_side);
    float* S = reinterpret_cast<float*>(work + p.off_s);
    const int64_t wave_blocks = (B + 3) / 4;
    if (wave_blocks > 0x7FFFFFFFll) return set_error(AMDKGE_EUNSUPPORTED, "train_relation: too many positives for one launch; split them");
    if (hipError_t e = hipMemsetAsync(step_sum, 0, 8, st)) return set_error_hip(e, "train_relation: hipMemsetAsync");
    if (mask)
        if (hipError_t e = hipMemsetAsync(side, 0, (size_t)B * 4, st)) return set_error_hip(e, "train_relation: hipMemsetAsync");
    hipLaunchKernelGGL(relpred_query_kernel<CPLX>, dim3((unsigned)wave_blocks), dim3(256), 0, st, d_ent, d_rel, d_triples, B, ks, k, Q, pos_raw);
    if (int rc = check_launch("relpred_query")) return rc;
    RelGemmArgs a{};
    a.ent = d_ent; a.rel = d_rel; a.triples = d_triples; a.Q = Q; a.S = S; a.dQ = dQ; a.g_rel = g_rel; a.R = R; a.K = K; a.ks = ks; a.k = k; a.cplx = CPLX ? 1 : 0; a.w = w;
    // the loss stage of a chunk: the list is the relation table (G = 1, M = R, no ids), the zeroed side array, the step's own loss sum
    SharedStep ls{};
    ls.S = S; ls.pos_raw = pos_raw; ls.cpos = cpos; ls.B = B; ls.G = 1; ls.M = R; ls.side = side; ls.st = st; ls.scale = scale; ls.loss = loss; ls.mask = mask;
    ls.loss_sum = step_sum; ls.pos_scores = d_pos_scores; ls.neg_scores = d_rel_scores;
    const int64_t tr = (R + PT - 1) / PT, tk = (K + PT - 1) / PT;
    for (int64_t row0 = 0; row0 < B; row0 += p.rpc) {
        const int64_t rows = (B - row0) < p.rpc ? (B - row0) : p.rpc;
        const int64_t tb = (rows + PT - 1) / PT, slices = (rows + RP_SLICE - 1) / RP_SLICE;
        const int64_t nb_fwd = tb * tr, nb_dq = tb * tk, nb_drel = tr * tk * slices;
        if (nb_fwd > 0x7FFFFFFFll || nb_dq > 0x7FFFFFFFll || nb_drel > 0x7FFFFFFFll) return set_error(AMDKGE_EUNSUPPORTED, "train_relation: too many tiles for one launch");
        a.row0 = row0; a.rows = (int)rows;
        a.tiles_n = (int)tr; a.per_slice = (int)nb_fwd;
        hipLaunchKernelGGL(relpred_gemm_kernel<RP_FWD>, dim3((unsigned)nb_fwd), dim3(256), 0, st, a);
        if (int rc = check_launch("relpred_gemm_fwd")) return rc;
        if (int rc = shared_loss_stage(ls, row0, rows)) return rc;   // (the mask: known relations -> -inf)
        a.tiles_n = (int)tk; a.per_slice = (int)nb_dq;
        hipLaunchKernelGGL(relpred_gemm_kernel<RP_DQ>, dim3((unsigned)nb_dq), dim3(256), 0, st, a);
        if (int rc = check_launch("relpred_gemm_dq")) return rc;
        a.tiles_n = (int)tk; a.per_slice = (int)(tr * tk);
        hipLaunchKernelGGL(relpred_gemm_kernel<RP_DREL>, dim3((unsigned)nb_drel), dim3(256), 0, st, a);
        if (int rc = check_launch("relpred_gemm_drel")) return rc;
    }
    hipLaunchKernelGGL(relpred_chain_kernel<CPLX>, dim3((unsigned)wave_blocks), dim3(256), 0, st, d_ent, d_rel, d_triples, B, ks, k, w, Q, dQ, cpos, g_ent, g_rel);
    if (int rc = check_launch("relpred_chain")) return rc;
    hipLaunchKernelGGL(relpred_loss_kernel, dim3(1), dim3(64), 0, st, step_sum, w, d_loss_sum);
    return check_launch("relpred_loss");
}

}  // namespace kge

using namespace kge;

extern "C" int64_t amdkge_train_relation_workspace_bytes(const amdkge_model* m, int64_t B) {
    if (validate_model(m) || !shared_model_ok(m)) return 0;
    RelPlan p;
    return relpred_plan(m, B, p) ? p.total : 0;
}

extern "C" int amdkge_train_relation_fwdbwd(const amdkge_model* m, const amdkge_loss* loss, float weight, const float* d_ent, const float* d_rel,
                                            const int32_t* d_triples, int64_t B, const int64_t* d_lo, const int64_t* d_hi, const int32_t* d_known,
                                            float* d_grad_ent, float* d_grad_rel, double* d_loss_sum, float* d_pos_scores, float* d_rel_scores, void* d_work,
                                            int64_t* d_stats, void* stream) {
    if (int rc = validate_model(m)) return rc;
    if (!shared_model_ok(m)) return set_error(AMDKGE_EUNSUPPORTED, "train_relation: the score of TransE and RotatE is a distance in the relation row, not a contraction with it: only DistMult, ComplEx and HolE take the relation objective");
    if (!loss || loss->kind < 0 || loss->kind > AMDKGE_LOSS_MULTICLASS_NLL) return set_error(AMDKGE_EINVAL, "train_relation: unknown loss kind");
    if (loss->focus_nonlinearity) return set_error(AMDKGE_EUNSUPPORTED, "train_relation: FocusE is not offered with the relation objective");
    if (!(weight >= 0.f) || __builtin_isinf(weight)) return set_error(AMDKGE_EINVAL, "train_relation: weight must be finite and >= 0");
    if (B < 0) return set_error(AMDKGE_EINVAL, "train_relation: B must be >= 0");
    if (!d_ent || !d_rel || !d_grad_ent || !d_grad_rel || !d_loss_sum) return set_error(AMDKGE_EINVAL, "train_relation: NULL table / gradient / loss pointer");
    const int given = (d_lo != nullptr) + (d_hi != nullptr) + (d_known != nullptr);
    if (given != 0 && given != 3) return set_error(AMDKGE_EINVAL, "train_relation: the three range arrays are given together or not at all");
    if (B == 0 || weight == 0.f) return AMDKGE_OK;
    if (!d_triples || !d_work) return set_error(AMDKGE_EINVAL, "train_relation: NULL triples / workspace");
    RelPlan p;
    if (!relpred_plan(m, B, p)) return set_error(AMDKGE_EUNSUPPORTED, "train_relation: more than 2^24 - 1 relations");
    SharedMaskArgs ma{};
    if (given == 3) {   // the pair ranges stand where the mask reads the object-side ranges (the workspace's side array is all zero)
        ma.o_lo = d_lo; ma.o_hi = d_hi; ma.o_ids = d_known;
        ma.s_lo = d_lo; ma.s_hi = d_hi; ma.s_ids = d_known;
        ma.identity = 1;
        ma.fill = -INFINITY;
        ma.stats = reinterpret_cast<unsigned long long*>(d_stats);
    }
    hipStream_t st = (hipStream_t)stream;
    char* work = static_cast<char*>(d_work);
    if (m->scoring_type != AMDKGE_DISTMULT)   // ComplEx, and HolE on its instantiation (the 2/k scale travels in ModelConst)
        return run_relpred<true>(m, loss, weight, d_ent, d_rel, d_triples, B, d_grad_ent, d_grad_rel, d_loss_sum, d_pos_scores, d_rel_scores, work, p, given == 3 ? &ma : nullptr, st);
    return run_relpred<false>(m, loss, weight, d_ent, d_rel, d_triples, B, d_grad_ent, d_grad_rel, d_loss_sum, d_pos_scores, d_rel_scores, work, p, given == 3 ? &ma : nullptr, st);
}
