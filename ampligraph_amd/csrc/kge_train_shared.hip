// Shared-negative training (include/amdkge_shared.h): the G positives of a group share one list of M replacement entities, so the
// group's G x M corruption scores are ONE fp32 matrix product of its query vectors with the M gathered rows, and both gradients are
// matrix products too.  The step is DEFINED in the header as amdkge_train_fwdbwd's on the equivalent override rows; tests/shared_ref.py
// restates the draw and that equivalence in numpy.
//   shared_draw_kernel  : ids [n_groups, M] and sides [B], one Philox block per value (the draw of the header).
//   shared_query_kernel : a wave per positive.  q_i = s*p or p*o (DistMult), the a|b halves of survey row a9 (ComplEx / HolE), built
//                         for the positive's OWN side; the positive's raw score <q_i, own_i> falls out of the same pass.
//   shared_gemm_kernel  : the product tile of kge_product_tile.h (exact fp32 MFMA, 64 x 64 per workgroup; which element a
//                         thread stages, which a lane feeds and which result a register holds is stated there).  Three
//                         MODES differ in where an operand element comes from and where a result goes:
//                           FWD : S_g  = Q_g E^T     (G x K by K x M)   E gathered by id          -> the score buffer [rows, M]
//                           DQ  : dQ_g = C_g E       (G x M by M x K)   E gathered by id          -> dQ [B, K]
//                           DE  : dE   = C_g^T Q_g   (M x G by G x K)   C read transposed         -> atomic row-adds into d_grad_ent
//                         Elements past a matrix edge are staged as zeros, so every tile shape is one code path.  Non-finite tables:
//                         a +-inf FWD result of ComplEx / HolE is computed again in the reference's order (shared_reference_score);
//                         DE and the chain kernel never write a padding unit (NaN coefficient * zero padding = NaN).
//   shared_loss_kernel  : a wave per positive walks loss_call (kge_loss.h) over its row of the score buffer: scores -> dL/dscore in
//                         place.  The buffer holds the plain sums; HolE's 2/k is applied where a score is loaded (the reference's
//                         rounding: reduce_sum, then scale) and again where a coefficient is stored (the chain rule through it).
//   shared_chain_kernel : a wave per positive.  With t_i = dQ_i + c_pos own_i = dL/dq_i, the gradients of the two kept rows are the
//                         transpose of the query map applied to t_i, that of the replaced row's original is c_pos q_i; three
//                         atomic row-adds per positive.
//   shared_mask_kernel  : (include/amdkge_shared_mask.h, optional, between FWD and the loss) a wave per positive sets the scores of the
//                         corruptions that are KNOWN statements to -inf, which every loss of loss_call already defines: no loss term, an
//                         exact-zero coefficient, nothing for DQ / DE to add where the rows are finite (0 * NaN = NaN where not).
//   shared_label_loss_kernel : (include/amdkge_shared_labels.h, kge_train_shared_labels.hip; in place of the mask and the loss) KvsAll:
//                         labels from the known ranges and binary cross-entropy in one pass over the buffer.
// Groups are processed in chunks of at most CHUNK_SCORES scores, so the score buffer is bounded whatever B * M is.
// The host side of a step is shared_step (kge_train_shared.h), defined here for this unit's family and for the distance tiles of
// kge_train_shared_dist.hip alike: the checks, the plan and the chunk loop once, each family's launches in its own unit
// (product_launch here).  The loss stage of a chunk is shared_loss_stage, also the relation objective's (kge_train_relpred.hip).
#include "kge_train_shared.h"
#include "kge_product_tile.h"
#include "kge_loss.h"
#include <string>

namespace kge {

constexpr uint32_t SHARED_TAG_IDS = 0xF0u << 24, SHARED_TAG_SIDE = 0xF1u << 24;

struct SharedDrawArgs {
    const int32_t* triples;
    int64_t B, G, n_groups;
    int M;
    int64_t base;
    uint32_t range, seed_lo, seed_hi, step_lo, step_hi;
    int side_mode;
    const uint32_t* side_thr;
    const int32_t* pool;
    uint32_t pool_n;
    int32_t* ids;
    int32_t* side;
};

__global__ __launch_bounds__(256) void shared_draw_kernel(SharedDrawArgs a) {
    const int64_t n_ids = a.n_groups * a.M;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_ids) {
        const uint32_t g = (uint32_t)(t / a.M), j = (uint32_t)(t % a.M);
        const u32x4 r = philox4x32_10(g, j | SHARED_TAG_IDS, a.step_lo, a.step_hi, a.seed_lo, a.seed_hi);
        a.ids[t] = a.pool ? a.pool[__umulhi(r.x, a.pool_n)] : (int)(a.base + (int64_t)__umulhi(r.x, a.range));
    } else if (t < n_ids + a.B) {
        const uint64_t i = (uint64_t)(t - n_ids);
        bool subj;
        if (a.side_mode == AMDKGE_NEG_SIDE_S_ONLY) subj = true;
        else if (a.side_mode == AMDKGE_NEG_SIDE_O_ONLY) subj = false;
        else {
            const u32x4 r = philox4x32_10((uint32_t)i, (uint32_t)(i >> 32) | SHARED_TAG_SIDE, a.step_lo, a.step_hi, a.seed_lo, a.seed_hi);
            subj = a.side_mode == AMDKGE_NEG_SIDE_BERNOULLI ? r.x < a.side_thr[a.triples[3 * i + 1]] : (r.x & 1u) == 0u;
        }
        a.side[i] = subj ? 1 : 0;
    }
}

// ---- query vectors ------------------------------------------------------------------------------------------------------------------
template <bool CPLX>
__global__ __launch_bounds__(256) void shared_query_kernel(const float* __restrict__ ent, const float* __restrict__ rel, const int32_t* __restrict__ triples,
                                                           const int32_t* __restrict__ side, int64_t B, int ks, float* __restrict__ Q, float* __restrict__ pos_raw) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= B) return;   // (wave-uniform; the kernel has no barrier)
    const int K = CPLX ? 2 * ks : ks;
    const bool subj = side[i] != 0;
    const float* S = ent + (int64_t)triples[3 * i] * K;
    const float* P = rel + (int64_t)triples[3 * i + 1] * K;
    const float* O = ent + (int64_t)triples[3 * i + 2] * K;
    const float* own = subj ? S : O;
    float* q = Q + i * K;
    float acc = 0.f;
    for (int u = lane; u < ks; u += 64) {
        if constexpr (CPLX) {
            const float p0 = P[u], p1 = P[ks + u];
            float q0, q1;
            if (subj) {   // score = <(p0 o0 + p1 o1, p0 o1 - p1 o0), s>
                const float o0 = O[u], o1 = O[ks + u];
                q0 = p0 * o0 + p1 * o1; q1 = p0 * o1 - p1 * o0;
            } else {      // score = <(s0 p0 - s1 p1, s0 p1 + s1 p0), o>
                const float s0 = S[u], s1 = S[ks + u];
                q0 = s0 * p0 - s1 * p1; q1 = s0 * p1 + s1 * p0;
            }
            q[u] = q0; q[ks + u] = q1;
            acc += q0 * own[u] + q1 * own[ks + u];
        } else {
            const float qq = P[u] * (subj ? O[u] : S[u]);
            q[u] = qq;
            acc += qq * own[u];
        }
    }
    acc = wave_sum_shfl(acc);
    if (lane == 0) pos_raw[i] = acc;
}

// ---- the three matrix products ------------------------------------------------------------------------------------------------------
enum { GEMM_FWD = 0, GEMM_DQ = 1, GEMM_DE = 2 };

struct SharedGemmArgs {
    const float* ent;
    const float* rel;
    const int32_t* triples;
    const int32_t* side;
    const int32_t* ids;   // [n_groups, M]
    float* Q;             // [B, K]
    float* S;             // [rows of the chunk, M]: scores, then dL/dscore
    float* dQ;            // [B, K]
    float* g_ent;
    int64_t B, G;
    int M, K;
    int ks, k;            // units per half as stored, live units (DE: the padding units of a gradient row are never written)
    int cplx;             // ComplEx / HolE: an infinite score is recomputed in the reference's operation order (shared_reference_score)
    int64_t g0;           // first group of the chunk (row0 = g0 * G)
    int tiles_m, tiles_n;
};

// The score of ONE corruption of a ComplEx / HolE positive in the reference's own operation order (cplx_reference_score).  Only for a
// score that the matrix product made +-inf: <q, e> with an inf in e is (a - b) * inf = +-inf where the reference forms
// a * inf - b * inf, which is NaN when a and b have one sign -- a NaN loss and NaN coefficients for the whole positive, where +-inf
// is clipped to a finite loss.  Which of the three non-finite values it is depends only on the units' terms, not on the order of
// their sum.
__device__ float shared_reference_score(const SharedGemmArgs& a, int64_t i, int id) {
    const int32_t* t = a.triples + 3 * i;
    const bool subj = a.side[i] != 0;
    const float* S = a.ent + (int64_t)(subj ? id : t[0]) * a.K;
    const float* P = a.rel + (int64_t)t[1] * a.K;
    const float* O = a.ent + (int64_t)(subj ? t[2] : id) * a.K;
    return cplx_reference_score(S, P, O, a.ks, a.k);
}

template <int MODE>
__global__ __launch_bounds__(256) void shared_gemm_kernel(SharedGemmArgs a) {
    __shared__ float As[PKC][PLD];
    __shared__ float Bs[PKC][PLD];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int per_group = a.tiles_m * a.tiles_n;
    const int64_t g = a.g0 + blockIdx.x / per_group;
    const int tile = blockIdx.x % per_group;
    const int m0 = (tile / a.tiles_n) * PT, n0 = (tile % a.tiles_n) * PT;
    const int64_t row_first = g * a.G;                                         // the group's first positive
    const int Gg = (int)((a.B - row_first) < a.G ? (a.B - row_first) : a.G);   // its positives
    const int64_t srow = row_first - a.g0 * a.G;                               // its first row in the score buffer
    const int mdim = MODE == GEMM_DE ? a.M : Gg;
    const int ndim = MODE == GEMM_FWD ? a.M : a.K;
    const int kdim = MODE == GEMM_FWD ? a.K : (MODE == GEMM_DQ ? a.M : Gg);
    if (m0 >= mdim) return;   // (the last, short group: uniform over the workgroup)
    const int32_t* gid = a.ids + g * a.M;

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    for (int k0 = 0; k0 < kdim; k0 += PKC) {
        // ---- stage A[m][kk] ----
        if (MODE == GEMM_DE) {   // contiguous along m: C[kk][m]
            const int mm = product_x_x(tid);
#pragma unroll
            for (int r = 0; r < PSTAGE; ++r) {
                const int kk = product_x_kk(tid, r);
                float v = 0.f;
                if (m0 + mm < mdim && k0 + kk < kdim) v = a.S[(srow + k0 + kk) * a.M + (m0 + mm)];
                As[kk][mm] = v;
            }
        } else {                 // contiguous along the contraction: Q[m][kk] / C[m][kk]
            const int kk = product_k_kk(tid);
#pragma unroll
            for (int r = 0; r < PSTAGE; ++r) {
                const int mm = product_k_x(tid, r);
                float v = 0.f;
                if (m0 + mm < mdim && k0 + kk < kdim)
                    v = MODE == GEMM_FWD ? a.Q[(row_first + m0 + mm) * a.K + (k0 + kk)] : a.S[(srow + m0 + mm) * a.M + (k0 + kk)];
                As[kk][mm] = v;
            }
        }
        // ---- stage B[kk][n] ----
        if (MODE == GEMM_FWD) {  // contiguous along the contraction: E[id_n][kk]
            const int kk = product_k_kk(tid);
#pragma unroll
            for (int r = 0; r < PSTAGE; ++r) {
                const int nn = product_k_x(tid, r);
                float v = 0.f;
                if (n0 + nn < ndim && k0 + kk < kdim) v = a.ent[(int64_t)gid[n0 + nn] * a.K + (k0 + kk)];
                Bs[kk][nn] = v;
            }
        } else {                 // contiguous along n: E[id_kk][n] / Q[kk][n]
            const int nn = product_x_x(tid);
#pragma unroll
            for (int r = 0; r < PSTAGE; ++r) {
                const int kk = product_x_kk(tid, r);
                float v = 0.f;
                if (n0 + nn < ndim && k0 + kk < kdim)
                    v = MODE == GEMM_DQ ? a.ent[(int64_t)gid[k0 + kk] * a.K + (n0 + nn)] : a.Q[(row_first + k0 + kk) * a.K + (n0 + nn)];
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
    // A padding unit of Q is an exact zero, but a NaN coefficient times it is NaN: the padding floats of d_grad_ent stay untouched.
    if (MODE == GEMM_DE && col % a.ks >= a.k) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = product_row(m0, product_quad_row(wv), lane, r);
        if (row >= mdim) continue;
        float v = acc[r];
        if (MODE == GEMM_FWD) {
            if (a.cplx && __builtin_isinf(v)) v = shared_reference_score(a, row_first + row, gid[col]);   // (an inf in a table: rare, divergent)
            a.S[(srow + row) * a.M + col] = v;
        }
        else if (MODE == GEMM_DQ) a.dQ[(row_first + row) * a.K + col] = v;
        else if (v != 0.f) atomic_add_f32(a.g_ent + (int64_t)gid[row] * a.K + col, v);   // (true for NaN; exact zeros add nothing)
    }
}

// ---- Loss.__call__ on a positive's row of the score buffer --------------------------------------------------------------------------
// store(): masked_zero()'s -0.0f marker (kge_loss.h) does not survive scale < 0 -- the distance tiles run with scale = -1 and it comes
// out +0.0f.  The shared paths do not need it: the marker tells the tile pass of kge_train_tile.hip to KEEP an entry whose coefficient
// is zero, and here no entry is ever dropped -- every coefficient of the buffer, a zero of either sign included, is an operand of DQ /
// DE, where 0 * NaN = NaN does what the marker asks for (tests/test_gpu_nonfinite_shared.py).
struct SharedWalk {
    float* s;
    int lane;
    float scale;
    __device__ __forceinline__ int first() const { return lane; }
    __device__ __forceinline__ int stride() const { return KGE_WAVE; }
    __device__ __forceinline__ float load(int j) const { return scale * s[j]; }
    __device__ __forceinline__ void store(int j, float v) const { s[j] = v * scale; }
    __device__ __forceinline__ float sum(float v) const { return wave_sum(v); }
    __device__ __forceinline__ float max(float v) const { return wave_max(v); }
};

__global__ __launch_bounds__(256) void shared_loss_kernel(float* __restrict__ S, const float* __restrict__ pos_raw, float* __restrict__ cpos, int64_t row0, int64_t rows,
                                                          int64_t B, int M, amdkge_loss L, float scale, double* loss_sum, float* pos_scores, float* neg_scores) {
    __shared__ double s_loss[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double tot = 0.0;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wv; r < rows; r += (int64_t)gridDim.x * 4) {   // (wave-uniform)
        const int64_t i = row0 + r;
        float* s = S + r * M;
        const float P = scale * pos_raw[i];
        if (neg_scores)
            for (int j = lane; j < M; j += 64) neg_scores[(int64_t)j * B + i] = scale * s[j];
        float per, dP;
        loss_call(L, P, M, SharedWalk{s, lane, scale}, per, dP);
        if (lane == 0) {
            cpos[i] = dP * scale;
            if (pos_scores) pos_scores[i] = P;
            tot += (double)per;
        }
    }
    if (lane == 0) s_loss[wv] = tot;
    __syncthreads();
    if (tid == 0) {
        const double t = s_loss[0] + s_loss[1] + s_loss[2] + s_loss[3];
        if (t != 0.0) atomicAdd(loss_sum, t);
    }
}

// ---- the mask of known statements (include/amdkge_shared_mask.h) ---------------------------------------------------------------------

// A wave per row.  GIVEN: lanes stride over j and look ids[g][j] up in the row's range.  A store cannot be undone and a FULLY KNOWN
// row stays unmasked, so while every entry seen so far was a hit nothing is stored; the first miss (a wave-uniform event) stores the
// whole prefix [0, j0) at once -- all of it was hits -- and from then on hits are stored where they are found: one search per entry.
// IDENTITY: ids[g][j] == j, the hits are the range's ids below M; a strictly ascending range is fully known iff it has M of them.
__global__ __launch_bounds__(256) void shared_mask_kernel(SharedMaskArgs a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int64_t n_masked = 0, n_full = 0;   // (lane 0's are the wave's totals)
    for (int64_t r = (int64_t)blockIdx.x * 4 + wv; r < a.rows; r += (int64_t)gridDim.x * 4) {   // (wave-uniform)
        const int64_t i = a.row0 + r;
        const bool subj = a.side[i] != 0;
        const int64_t lo = subj ? a.s_lo[i] : a.o_lo[i], hi = subj ? a.s_hi[i] : a.o_hi[i];
        if (hi <= lo) continue;
        const int32_t* __restrict__ kid = subj ? a.s_ids : a.o_ids;
        float* s = a.S + r * a.M;
        if (a.identity) {
            int64_t b = lo, e = hi;   // the first id >= M
            while (b < e) {
                const int64_t mid = b + ((e - b) >> 1);
                if (kid[mid] < a.M) b = mid + 1; else e = mid;
            }
            const int64_t c = b - lo;
            if (c >= a.M) { ++n_full; continue; }
            for (int64_t t = lo + lane; t < b; t += 64) {
                const int id = kid[t];
                if (id >= 0) s[id] = a.fill;
            }
            n_masked += c;
            continue;
        }
        const int32_t* __restrict__ gid = a.ids + (i / a.G) * a.M;
        bool all = true;
        int cnt = 0;
        for (int j0 = 0; j0 < a.M; j0 += 64) {   // (wave-uniform)
            const int j = j0 + lane;
            const bool in = j < a.M;
            const bool hit = in && sorted_contains<int64_t>(kid, lo, hi, gid[j]);
            if (all && __ballot(in && !hit) != 0ull) {
                all = false;
                for (int jj = lane; jj < j0; jj += 64) { s[jj] = a.fill; ++cnt; }
            }
            if (!all && hit) { s[j] = a.fill; ++cnt; }
        }
        if (all) ++n_full;
        else n_masked += wave_sum_i(cnt);
    }
    if (a.stats && lane == 0) {
        if (n_masked) atomicAdd(&a.stats[0], (unsigned long long)n_masked);
        if (n_full) atomicAdd(&a.stats[1], (unsigned long long)n_full);
    }
}

// ---- the transpose of the query map -------------------------------------------------------------------------------------------------
template <bool CPLX>
__global__ __launch_bounds__(256) void shared_chain_kernel(const float* __restrict__ ent, const float* __restrict__ rel, const int32_t* __restrict__ triples,
                                                           const int32_t* __restrict__ side, int64_t B, int ks, int k, const float* __restrict__ Q, const float* __restrict__ dQ,
                                                           const float* __restrict__ cpos, float* g_ent, float* g_rel) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= B) return;
    const int K = CPLX ? 2 * ks : ks;
    const bool subj = side[i] != 0;
    const int64_t so = (int64_t)triples[3 * i] * K, po = (int64_t)triples[3 * i + 1] * K, oo = (int64_t)triples[3 * i + 2] * K;
    const float* S = ent + so;
    const float* P = rel + po;
    const float* O = ent + oo;
    const float* q = Q + i * K;
    const float* d = dQ + i * K;
    const float c = cpos[i];
    float* g_own = g_ent + (subj ? so : oo);    // the replaced row's original: c_pos q_i
    float* g_kept = g_ent + (subj ? oo : so);   // the kept entity row
    float* g_p = g_rel + po;
    for (int u = lane; u < k; u += 64) {   // the live units: dQ of a padding unit is NaN where a coefficient is (NaN * 0)
        if constexpr (CPLX) {
            const float p0 = P[u], p1 = P[ks + u];
            const float w0 = subj ? S[u] : O[u], w1 = subj ? S[ks + u] : O[ks + u];   // own
            const float t0 = d[u] + c * w0, t1 = d[ks + u] + c * w1;                  // dL/dq
            float dp0, dp1, dk0, dk1;
            if (subj) {   // q = q(p, o); t stands where s does in the score
                const float o0 = O[u], o1 = O[ks + u];
                dp0 = t0 * o0 + t1 * o1; dp1 = t0 * o1 - t1 * o0;
                dk0 = t0 * p0 - t1 * p1; dk1 = t0 * p1 + t1 * p0;
            } else {      // q = q(s, p); t stands where o does
                const float s0 = S[u], s1 = S[ks + u];
                dk0 = p0 * t0 + p1 * t1; dk1 = p0 * t1 - p1 * t0;
                dp0 = s0 * t0 + s1 * t1; dp1 = s0 * t1 - s1 * t0;
            }
            add_nz(g_own + u, c * q[u]); add_nz(g_own + ks + u, c * q[ks + u]);
            add_nz(g_kept + u, dk0); add_nz(g_kept + ks + u, dk1);
            add_nz(g_p + u, dp0); add_nz(g_p + ks + u, dp1);
        } else {
            const float p = P[u], w = subj ? S[u] : O[u], kept = subj ? O[u] : S[u];
            const float t = d[u] + c * w;
            add_nz(g_own + u, c * q[u]);
            add_nz(g_kept + u, t * p);
            add_nz(g_p + u, t * kept);
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// groups per chunk of the score buffer
static int64_t shared_chunk_groups(int64_t n_groups, int64_t G, int64_t M) {
    int64_t gpc = CHUNK_SCORES / (G * M);
    if (gpc < 1) gpc = 1;
    return gpc < n_groups ? gpc : n_groups;
}
bool shared_plan(const amdkge_model* m, int64_t B, int64_t G, int64_t M, SharedPlan& p) {
    if (B < 1 || G < 1 || M < 1 || M > AMDKGE_SHARED_MAX_NEGS) return false;
    if (G > B) G = B;
    if (G > (1ll << 40) / M) return false;   // (G * M stays far inside 64 bits)
    const int64_t K = row_floats(m);
    p.n_groups = (B + G - 1) / G;
    p.gpc = shared_chunk_groups(p.n_groups, G, M);
    int64_t rows = p.gpc * G;
    if (rows > B) rows = B;
    Layout l;   // (the caller's base is used as it is)
    p.off_q = l.take(B * K, 4); p.off_dq = l.take(B * K, 4);
    p.off_pos = l.take(B, 4); p.off_cpos = l.take(B, 4);
    p.off_s = l.take(rows * M, 4); p.total = l.next();
    return true;
}

int launch_shared_mask(const SharedMaskArgs& a, hipStream_t st) {
    int64_t lb = (a.rows + 3) / 4;
    if (lb > 2048) lb = 2048;
    hipLaunchKernelGGL(shared_mask_kernel, dim3((unsigned)lb), dim3(256), 0, st, a);
    return check_launch("shared_mask");
}

int launch_shared_loss(float* S, const float* pos_raw, float* cpos, int64_t row0, int64_t rows, int64_t B, int M, const amdkge_loss& L, float scale, double* loss_sum,
                       float* pos_scores, float* neg_scores, hipStream_t st) {
    int64_t lb = (rows + 3) / 4;
    if (lb > 2048) lb = 2048;
    hipLaunchKernelGGL(shared_loss_kernel, dim3((unsigned)lb), dim3(256), 0, st, S, pos_raw, cpos, row0, rows, B, M, L, scale, loss_sum, pos_scores, neg_scores);
    return check_launch("shared_loss");
}

int shared_loss_stage(const SharedStep& s, int64_t row0, int64_t rows) {
    if (s.labels) {   // KvsAll (include/amdkge_shared_labels.h): labels + BCE in one pass, in place of mask + loss
        SharedLabelArgs la = *s.labels;
        la.S = s.S; la.row0 = row0; la.rows = rows; la.G = s.G; la.B = s.B; la.M = s.M; la.ids = s.ids; la.side = s.side; la.scale = s.scale;
        la.pos_raw = s.pos_raw; la.cpos = s.cpos; la.pos_scores = s.pos_scores; la.neg_scores = s.neg_scores; la.loss_sum = s.loss_sum;
        return launch_shared_label_loss(la, s.st);
    }
    if (s.mask) {   // known statements -> a score of -inf, on the chunk's own rows
        SharedMaskArgs ma = *s.mask;
        ma.S = s.S; ma.row0 = row0; ma.rows = rows; ma.G = s.G; ma.M = s.M; ma.ids = s.ids; ma.side = s.side;
        ma.fill = s.scale < 0.f ? INFINITY : -INFINITY;
        if (int rc = launch_shared_mask(ma, s.st)) return rc;
    }
    return launch_shared_loss(s.S, s.pos_raw, s.cpos, row0, rows, s.B, s.M, *s.loss, s.scale, s.loss_sum, s.pos_scores, s.neg_scores, s.st);
}

// ---- the driver ---------------------------------------------------------------------------------------------------------------------
int64_t shared_step_workspace_bytes(const SharedFamily& f, const amdkge_model* m, int64_t B, int64_t G, int32_t M) {
    if (validate_model(m) || !f.model_ok(m)) return 0;
    SharedPlan p;
    return shared_plan(m, B, G, M, p) ? p.total : 0;
}

int shared_step(const SharedFamily& f, const amdkge_model* m, const amdkge_loss* loss, const float* d_ent, const float* d_rel, const int32_t* d_triples, int64_t B, int64_t G,
                int32_t M, const int32_t* d_neg_ids, const int32_t* d_side, float* d_grad_ent, float* d_grad_rel, double* d_loss_sum, float* d_pos_scores,
                float* d_neg_scores, void* d_work, const SharedMaskArgs* mask, const SharedLabelArgs* labels, void* stream) {
    const auto refuse = [&f](int code, const char* what) { return set_error(code, (std::string(f.who) + ": " + what).c_str()); };
    if (int rc = validate_model(m)) return rc;
    if (!f.model_ok(m)) return refuse(AMDKGE_EUNSUPPORTED, f.wrong_model);
    if (!labels) {
        if (!loss || loss->kind < 0 || loss->kind > AMDKGE_LOSS_MULTICLASS_NLL) return refuse(AMDKGE_EINVAL, "unknown loss kind");
        if (loss->focus_nonlinearity) return refuse(AMDKGE_EUNSUPPORTED, "FocusE is not offered with shared negatives");
    }
    if (B < 0 || G < 1 || M < 1 || M > AMDKGE_SHARED_MAX_NEGS) return refuse(AMDKGE_EINVAL, "bad sizes (B >= 0, G >= 1, 1 <= M < 2^24)");
    if (!d_ent || !d_rel || !d_grad_ent || !d_grad_rel || !d_loss_sum) return refuse(AMDKGE_EINVAL, "NULL table / gradient / loss pointer");
    if (B == 0) return AMDKGE_OK;
    if (!d_triples || !d_neg_ids || !d_side || !d_work) return refuse(AMDKGE_EINVAL, "NULL triples / ids / sides / workspace");
    if (G > B) G = B;
    SharedPlan p;
    if (!shared_plan(m, B, G, M, p)) return refuse(AMDKGE_EINVAL, "bad sizes");
    char* work = static_cast<char*>(d_work);
    const auto at = [work](int64_t off) { return reinterpret_cast<float*>(work + off); };
    const ModelConst mc = model_const(m);
    const SharedStep s{m, d_ent, d_rel, d_triples, d_neg_ids, d_side, B, G, M, d_grad_ent, d_grad_rel, at(p.off_q), at(p.off_dq), at(p.off_pos), at(p.off_cpos), at(p.off_s),
                       (hipStream_t)stream, mc.score_sign * mc.score_scale, loss, mask, labels, d_loss_sum, d_pos_scores, d_neg_scores};
    const int64_t wave_blocks = (B + 3) / 4;
    if (wave_blocks > 0x7FFFFFFFll) return refuse(AMDKGE_EUNSUPPORTED, "too many positives for one launch; split them");
    if (int rc = f.launch(s, SHARED_QUERY, (unsigned)wave_blocks, 0, 0, 0)) return rc;
    const int tg = (int)((G + SHARED_TILE - 1) / SHARED_TILE), tm = (M + SHARED_TILE - 1) / SHARED_TILE, tk = f.unit_tiles(m);
    for (int64_t g0 = 0; g0 < p.n_groups; g0 += p.gpc) {
        const int64_t ng = (p.n_groups - g0) < p.gpc ? (p.n_groups - g0) : p.gpc;
        const int64_t row0 = g0 * G;
        const int64_t rows = ((g0 + ng) * G < B ? (g0 + ng) * G : B) - row0;
        const int64_t nb_fwd = ng * tg * tm, nb_dq = ng * tg * tk, nb_de = ng * tm * tk;
        if (nb_fwd > 0x7FFFFFFFll || nb_dq > 0x7FFFFFFFll || nb_de > 0x7FFFFFFFll) return refuse(AMDKGE_EUNSUPPORTED, "too many tiles for one launch");
        if (int rc = f.launch(s, SHARED_FWD, (unsigned)nb_fwd, g0, tg, tm)) return rc;
        if (int rc = shared_loss_stage(s, row0, rows)) return rc;
        if (int rc = f.launch(s, SHARED_DQ, (unsigned)nb_dq, g0, tg, tk)) return rc;
        if (int rc = f.launch(s, SHARED_DE, (unsigned)nb_de, g0, tm, tk)) return rc;
    }
    return f.launch(s, SHARED_CHAIN, (unsigned)wave_blocks, 0, 0, 0);
}

// ---- the product family: its kernels' launches ----------------------------------------------------------------------------------------
template <bool CPLX>
static int product_launch(const SharedStep& s, SharedStage stage, unsigned blocks, int64_t g0, int tiles_m, int tiles_n) {
    const int ks = stored_k(s.m), k = s.m->k;
    SharedGemmArgs a{};
    a.ent = s.ent; a.rel = s.rel; a.triples = s.triples; a.side = s.side; a.cplx = CPLX ? 1 : 0; a.ids = s.ids; a.Q = s.Q; a.S = s.S; a.dQ = s.dQ; a.g_ent = s.g_ent; a.B = s.B; a.G = s.G; a.M = s.M; a.K = row_floats(s.m); a.ks = ks; a.k = k;
    a.g0 = g0; a.tiles_m = tiles_m; a.tiles_n = tiles_n;
    static const char* const NAMES[] = {"shared_query", "shared_gemm_fwd", "shared_gemm_dq", "shared_gemm_de", "shared_chain"};   // (by SharedStage)
    switch (stage) {
    case SHARED_QUERY: hipLaunchKernelGGL(shared_query_kernel<CPLX>, dim3(blocks), dim3(256), 0, s.st, s.ent, s.rel, s.triples, s.side, s.B, ks, s.Q, s.pos_raw); break;
    case SHARED_FWD: hipLaunchKernelGGL(shared_gemm_kernel<GEMM_FWD>, dim3(blocks), dim3(256), 0, s.st, a); break;
    case SHARED_DQ: hipLaunchKernelGGL(shared_gemm_kernel<GEMM_DQ>, dim3(blocks), dim3(256), 0, s.st, a); break;
    case SHARED_DE: hipLaunchKernelGGL(shared_gemm_kernel<GEMM_DE>, dim3(blocks), dim3(256), 0, s.st, a); break;
    case SHARED_CHAIN: hipLaunchKernelGGL(shared_chain_kernel<CPLX>, dim3(blocks), dim3(256), 0, s.st, s.ent, s.rel, s.triples, s.side, s.B, ks, k, s.Q, s.dQ, s.cpos, s.g_ent, s.g_rel); break;
    }
    return check_launch(NAMES[stage]);
}
static const SharedFamily PRODUCTS = {
    "train_shared", shared_model_ok, "TransE and RotatE score a distance, not a contraction: only DistMult, ComplEx and HolE share negatives",
    [](const amdkge_model* m) { return (row_floats(m) + PT - 1) / PT; },
    [](const SharedStep& s, SharedStage stage, unsigned blocks, int64_t g0, int tiles_m, int tiles_n) {
        return s.m->scoring_type != AMDKGE_DISTMULT ? product_launch<true>(s, stage, blocks, g0, tiles_m, tiles_n)   // ComplEx, and HolE on its instantiation (the 2/k scale travels in ModelConst)
                                                    : product_launch<false>(s, stage, blocks, g0, tiles_m, tiles_n);
    }};

}  // namespace kge

using namespace kge;

extern "C" int amdkge_sample_shared(const int32_t* d_triples, int64_t B, int64_t G, int32_t M, int64_t sample_base, int64_t sample_range, uint64_t seed, uint64_t step,
                                    int32_t side_mode, const uint32_t* d_side_thr, const int32_t* d_pool, int64_t pool_n, int32_t* d_ids, int32_t* d_side, void* stream) {
    if (B < 0 || G < 1 || M < 1 || M > AMDKGE_SHARED_MAX_NEGS) return set_error(AMDKGE_EINVAL, "sample_shared: bad sizes (B >= 0, G >= 1, 1 <= M < 2^24)");
    if (!d_ids || !d_side) return set_error(AMDKGE_EINVAL, "sample_shared: NULL pointer");
    if (side_mode < AMDKGE_NEG_SIDE_UNIFORM || side_mode > AMDKGE_NEG_SIDE_O_ONLY) return set_error(AMDKGE_EINVAL, "sample_shared: unknown side_mode");
    if (side_mode == AMDKGE_NEG_SIDE_BERNOULLI && (!d_side_thr || (B > 0 && !d_triples))) return set_error(AMDKGE_EINVAL, "sample_shared: AMDKGE_NEG_SIDE_BERNOULLI needs d_side_thr and d_triples");
    if (d_pool && (pool_n < 1 || pool_n > 0xFFFFFFFFll)) return set_error(AMDKGE_EINVAL, "sample_shared: a pool needs pool_n in [1, 2^32)");
    if (!d_pool && (sample_range <= 0 || sample_range > 0xFFFFFFFFll || sample_base < 0)) return set_error(AMDKGE_EINVAL, "sample_shared: sample_range must be in [1, 2^32), sample_base >= 0");
    if (B == 0) return AMDKGE_OK;
    if (G > B) G = B;
    SharedDrawArgs a{};
    a.triples = d_triples; a.B = B; a.G = G; a.n_groups = (B + G - 1) / G; a.M = M;
    a.base = sample_base; a.range = d_pool ? 1u : (uint32_t)sample_range;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.step_lo = (uint32_t)step; a.step_hi = (uint32_t)(step >> 32);
    a.side_mode = side_mode; a.side_thr = d_side_thr; a.pool = d_pool; a.pool_n = d_pool ? (uint32_t)pool_n : 0u;
    a.ids = d_ids; a.side = d_side;
    if (a.n_groups > 0x7FFFFFFFll) return set_error(AMDKGE_EUNSUPPORTED, "sample_shared: too many groups");
    const int64_t blocks = (a.n_groups * M + B + 255) / 256;
    if (blocks > 0x7FFFFFFFll) return set_error(AMDKGE_EUNSUPPORTED, "sample_shared: too many values for one launch; split them");
    hipLaunchKernelGGL(shared_draw_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("sample_shared");
}

extern "C" int64_t amdkge_train_shared_workspace_bytes(const amdkge_model* m, int64_t B, int64_t G, int32_t M) {
    return shared_step_workspace_bytes(PRODUCTS, m, B, G, M);
}

// the three step entry points are shared_step on the product family: no mask (the plain step), the mask, or the labels
extern "C" int amdkge_train_shared_fwdbwd(const amdkge_model* m, const amdkge_loss* loss, const float* d_ent, const float* d_rel, const int32_t* d_triples, int64_t B,
                                          int64_t G, int32_t M, const int32_t* d_neg_ids, const int32_t* d_side, float* d_grad_ent, float* d_grad_rel, double* d_loss_sum,
                                          float* d_pos_scores, float* d_neg_scores, void* d_work, void* stream) {
    return shared_step(PRODUCTS, m, loss, d_ent, d_rel, d_triples, B, G, M, d_neg_ids, d_side, d_grad_ent, d_grad_rel, d_loss_sum, d_pos_scores, d_neg_scores, d_work, nullptr,
                       nullptr, stream);
}

// (declared in kge_train_shared.h)
int kge::shared_mask_args(const char* who, const int32_t* d_neg_ids, const int64_t* d_s_lo, const int64_t* d_s_hi, const int32_t* d_s_ids, const int64_t* d_o_lo,
                            const int64_t* d_o_hi, const int32_t* d_o_ids, int32_t list_mode, int64_t* d_stats, bool ranges_required, SharedMaskArgs& a, bool& masked) {
    const int given = (d_s_lo != nullptr) + (d_s_hi != nullptr) + (d_s_ids != nullptr) + (d_o_lo != nullptr) + (d_o_hi != nullptr) + (d_o_ids != nullptr);
    if (given != 6 && (given != 0 || ranges_required)) return set_error(AMDKGE_EINVAL, (std::string(who) + (ranges_required ? ": the six range arrays are all required" : ": the six range arrays are given together or not at all")).c_str());
    if (list_mode != AMDKGE_SHARED_LIST_GIVEN && list_mode != AMDKGE_SHARED_LIST_IDENTITY) return set_error(AMDKGE_EINVAL, (std::string(who) + ": unknown list_mode").c_str());
    if (list_mode == AMDKGE_SHARED_LIST_GIVEN && !d_neg_ids) return set_error(AMDKGE_EINVAL, (std::string(who) + ": AMDKGE_SHARED_LIST_GIVEN needs d_neg_ids").c_str());
    masked = given == 6;
    a = SharedMaskArgs{};
    a.s_lo = d_s_lo; a.s_hi = d_s_hi; a.s_ids = d_s_ids; a.o_lo = d_o_lo; a.o_hi = d_o_hi; a.o_ids = d_o_ids;
    a.identity = list_mode == AMDKGE_SHARED_LIST_IDENTITY;
    a.fill = -INFINITY;
    a.stats = reinterpret_cast<unsigned long long*>(d_stats);
    return AMDKGE_OK;
}

extern "C" int amdkge_shared_mask_scores(float* d_scores, int64_t row0, int64_t rows, int64_t G, int32_t M, const int32_t* d_neg_ids, const int32_t* d_side,
                                         const int64_t* d_s_lo, const int64_t* d_s_hi, const int32_t* d_s_ids, const int64_t* d_o_lo, const int64_t* d_o_hi,
                                         const int32_t* d_o_ids, int32_t list_mode, int64_t* d_stats, void* stream) {
    if (row0 < 0 || rows < 0 || G < 1 || M < 1 || M > AMDKGE_SHARED_MAX_NEGS) return set_error(AMDKGE_EINVAL, "shared_mask_scores: bad sizes (row0 >= 0, rows >= 0, G >= 1, 1 <= M < 2^24)");
    if (!d_scores || !d_side) return set_error(AMDKGE_EINVAL, "shared_mask_scores: NULL scores / sides");
    SharedMaskArgs a;
    bool masked;
    if (int rc = shared_mask_args("shared_mask_scores", d_neg_ids, d_s_lo, d_s_hi, d_s_ids, d_o_lo, d_o_hi, d_o_ids, list_mode, d_stats, true, a, masked)) return rc;
    if (rows == 0) return AMDKGE_OK;
    a.S = d_scores; a.row0 = row0; a.rows = rows; a.G = G; a.M = M; a.ids = d_neg_ids; a.side = d_side;
    return launch_shared_mask(a, (hipStream_t)stream);
}

extern "C" int amdkge_train_shared_masked_fwdbwd(const amdkge_model* m, const amdkge_loss* loss, const float* d_ent, const float* d_rel, const int32_t* d_triples, int64_t B,
                                                 int64_t G, int32_t M, const int32_t* d_neg_ids, const int32_t* d_side, float* d_grad_ent, float* d_grad_rel,
                                                 double* d_loss_sum, float* d_pos_scores, float* d_neg_scores, void* d_work, const int64_t* d_s_lo, const int64_t* d_s_hi,
                                                 const int32_t* d_s_ids, const int64_t* d_o_lo, const int64_t* d_o_hi, const int32_t* d_o_ids, int32_t list_mode,
                                                 int64_t* d_stats, void* stream) {
    SharedMaskArgs a;
    bool masked;
    if (int rc = shared_mask_args("train_shared_masked", d_neg_ids, d_s_lo, d_s_hi, d_s_ids, d_o_lo, d_o_hi, d_o_ids, list_mode, d_stats, false, a, masked)) return rc;
    return shared_step(PRODUCTS, m, loss, d_ent, d_rel, d_triples, B, G, M, d_neg_ids, d_side, d_grad_ent, d_grad_rel, d_loss_sum, d_pos_scores, d_neg_scores, d_work,
                       masked ? &a : nullptr, nullptr, stream);
}

// (include/amdkge_shared_labels.h)
extern "C" int amdkge_train_shared_labels_fwdbwd(const amdkge_model* m, float label_smoothing, int32_t reduction_mean, const float* d_ent, const float* d_rel,
                                                 const int32_t* d_triples, int64_t B, int64_t G, int32_t M, const int32_t* d_neg_ids, const int32_t* d_side,
                                                 float* d_grad_ent, float* d_grad_rel, double* d_loss_sum, float* d_pos_scores, float* d_neg_scores, void* d_work,
                                                 const int64_t* d_s_lo, const int64_t* d_s_hi, const int32_t* d_s_ids, const int64_t* d_o_lo, const int64_t* d_o_hi,
                                                 const int32_t* d_o_ids, int32_t list_mode, const float* d_w_s, const float* d_w_o, int64_t* d_stats, void* stream) {
    SharedLabelArgs la;
    if (int rc = shared_label_args("train_shared_labels", d_neg_ids, d_s_lo, d_s_hi, d_s_ids, d_o_lo, d_o_hi, d_o_ids, list_mode, label_smoothing, reduction_mean, d_w_s,
                                   d_w_o, d_stats, la)) return rc;
    return shared_step(PRODUCTS, m, nullptr, d_ent, d_rel, d_triples, B, G, M, d_neg_ids, d_side, d_grad_ent, d_grad_rel, d_loss_sum, d_pos_scores, d_neg_scores, d_work, nullptr,
                       &la, stream);
}
