// Batch regularisers (include/amdkge_batch_reg.h): N3 and per-occurrence Lp on the rows the positives of a step use.  The header's text
// DEFINES the arithmetic, the lane order of the penalty's sum and the NaN / inf rule; tests/batch_reg_ref.py restates it in numpy.
//   batch_reg_kernel<CPLX, VEC> : a wave per positive, lanes stride over the live units in groups of VEC.  The three rows are read once
//                                 -- 16 bytes per lane where the stored half width is a multiple of 4 (VEC = 4), a float per lane
//                                 otherwise (VEC = 1: k = 1, k = 7 dense rows) -- and the per-float gradient goes into the dense gradient
//                                 tables with fp32 atomics: three atomic row-adds per positive, what shared_chain_kernel costs.  The adds
//                                 are issued in the shape the memory side wants, one wave-instruction = 64 consecutive floats: the VEC = 4
//                                 path first transposes its four registers over the lanes (lane_transpose4).  The penalty is one wave
//                                 reduction per positive, summed in double per wave, and leaves as ONE double atomic per workgroup, the
//                                 scheme of shared_loss_kernel.
// CPLX is the row LAYOUT ([re || im] halves: ComplEx, HolE, RotatE), not the norm: a FLOAT-mode term on such rows treats both halves as
// units of their own.  p, the norm mode and c = fp32(p * lambda) of a term are wave-uniform run-time values.
#include "kge_host.h"
#include "../../include/amdkge_batch_reg.h"

namespace kge {

struct BatchRegTerm {
    int on;        // lambda != 0
    int cube;      // p == 3
    int modulus;   // AMDKGE_BATCH_REG_MODULUS
    float c;       // fp32(p * lambda)
    float lambda;
};

struct BatchRegArgs {
    const float* ent;
    const float* rel;
    const int32_t* triples;
    int64_t B;
    int ks, k;   // units per half as stored, live units
    BatchRegTerm e, r;
    float* g_ent;
    float* g_rel;
    double* reg_sum;
};

// Penalty and gradient of ONE unit of one row, in the header's operation order.  Real layout: im, g1 are not used.
template <bool CPLX>
__device__ __forceinline__ float reg_unit(const BatchRegTerm& t, float re, float im, float& g0, float& g1) {
    if (CPLX && t.modulus) {
        const float m2 = re * re + im * im;
        const float m = sqrtf(m2);
        const float f = t.cube ? t.c * m : t.c;
        g0 = f * re;
        g1 = f * im;
        return t.cube ? m2 * m : m2;
    }
    const float a0 = re * re, n0 = fabsf(re);
    g0 = t.cube ? (t.c * n0) * re : t.c * re;
    float pen = t.cube ? a0 * n0 : a0;
    if (CPLX) {
        const float a1 = im * im, n1 = fabsf(im);
        g1 = t.cube ? (t.c * n1) * im : t.c * im;
        pen += t.cube ? a1 * n1 : a1;
    }
    return pen;
}

__device__ __forceinline__ float sel4(const float (&v)[4], int i) {
    const float v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3];   // (values first: a conditional on the array elements selects ADDRESSES)
    const float lo = (i & 1) ? v1 : v0, hi = (i & 1) ? v3 : v2;
    return (i & 2) ? hi : lo;
}

// Lane l holds v[c] = x[4 l + c] of 256 consecutive floats x (what a 16-byte load per lane gives); afterwards w[j] = x[64 j + l], so
// that the atomic instruction of slot j adds 64 consecutive floats.  x[64 j + l] lives in lane 16 j + (l >> 2) as component l & 3: in
// round t lane l = 4 q + c reads slot j = (t + c) & 3 from lane 16 j + q, so that the four lanes that share q read four different
// lanes, and a source lane 16 a + q hands out component (a - t) & 3, the one its single reader of that round wants.
__device__ __forceinline__ void lane_transpose4(const float (&v)[4], int lane, float (&w)[4]) {
    const int q = lane >> 2, c = lane & 3, a = lane >> 4;
    float recv[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float send = sel4(v, (a - t) & 3);
        recv[t] = __shfl(send, 16 * ((t + c) & 3) + q, 64);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = sel4(recv, (j - c) & 3);
}

// the gradient floats of the units [u0, u0 + VEC) of this lane -> row `g`, half offset `h`; floats of units >= k are never written
template <int VEC>
__device__ __forceinline__ void add_units(float* g, int h, int c0, int lane, int k, const float (&v)[4]) {
    if constexpr (VEC == 4) {
        float w[4];
        lane_transpose4(v, lane, w);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int u = c0 + 64 * j + lane;
            if (u < k && w[j] != 0.f) atomic_add_f32(g + h + u, w[j]);   // (true for NaN; exact zeros add nothing)
        }
    } else {
        const int u = c0 + lane;
        if (u < k && v[0] != 0.f) atomic_add_f32(g + h + u, v[0]);
    }
}

// one row of one positive: reads the units of this lane, adds their gradient, returns this lane's share of the row's penalty
template <bool CPLX, int VEC>
__device__ __forceinline__ float reg_row(const BatchRegTerm& t, const float* __restrict__ row, float* g, int ks, int k, int c0, int lane) {
    const int u0 = c0 + VEC * lane;
    float g0[4] = {0.f, 0.f, 0.f, 0.f}, g1[4] = {0.f, 0.f, 0.f, 0.f};
    float pen = 0.f;
    if (u0 < k) {   // (u0 + VEC <= ks: the stored half is whole groups)
        const fvec<VEC> re = ldg<VEC>(row + u0);
        fvec<VEC> im = re;
        if constexpr (CPLX) im = ldg<VEC>(row + ks + u0);
#pragma unroll
        for (int j = 0; j < VEC; ++j)
            if (u0 + j < k) pen += reg_unit<CPLX>(t, re.v[j], im.v[j], g0[j], g1[j]);   // (a padding unit enters nothing)
    }
    // (every lane of the wave: the transposition reads its neighbours)
    add_units<VEC>(g, 0, c0, lane, k, g0);
    if constexpr (CPLX) add_units<VEC>(g, ks, c0, lane, k, g1);
    return pen;
}

template <bool CPLX, int VEC>
__global__ __launch_bounds__(256) void batch_reg_kernel(BatchRegArgs a) {
    __shared__ double s_pen[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t K = CPLX ? 2 * (int64_t)a.ks : (int64_t)a.ks;
    double tot = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 4 + wv; i < a.B; i += (int64_t)gridDim.x * 4) {   // (wave-uniform)
        const int64_t so = (int64_t)a.triples[3 * i] * K, po = (int64_t)a.triples[3 * i + 1] * K, oo = (int64_t)a.triples[3 * i + 2] * K;
        float acc_e = 0.f, acc_r = 0.f;
        for (int c0 = 0; c0 < a.k; c0 += 64 * VEC) {   // (wave-uniform)
            if (a.e.on) {
                acc_e += reg_row<CPLX, VEC>(a.e, a.ent + so, a.g_ent + so, a.ks, a.k, c0, lane);
                acc_e += reg_row<CPLX, VEC>(a.e, a.ent + oo, a.g_ent + oo, a.ks, a.k, c0, lane);
            }
            if (a.r.on) acc_r += reg_row<CPLX, VEC>(a.r, a.rel + po, a.g_rel + po, a.ks, a.k, c0, lane);
        }
        const float E = wave_sum(acc_e), R = wave_sum(acc_r);
        tot += (double)a.e.lambda * (double)E + (double)a.r.lambda * (double)R;
    }
    if (lane == 0) s_pen[wv] = tot;
    __syncthreads();
    if (tid == 0) {
        const double t = s_pen[0] + s_pen[1] + s_pen[2] + s_pen[3];
        if (t != 0.0) atomicAdd(a.reg_sum, t);   // (true for NaN)
    }
}

static bool complex_layout(const amdkge_model* m) {
    return m->scoring_type == AMDKGE_COMPLEX || m->scoring_type == AMDKGE_HOLE || m->scoring_type == AMDKGE_ROTATE;
}

static int batch_reg_term(const char* which, int32_t p, float lambda, int32_t norm, bool modulus_ok, const char* why_not, BatchRegTerm& t) {
    char msg[200];
    if (p != 2 && p != 3) {
        snprintf(msg, sizeof(msg), "batch_reg: p of the %s term must be 2 or 3", which);
        return set_error(AMDKGE_EINVAL, msg);
    }
    if (norm != AMDKGE_BATCH_REG_FLOAT && norm != AMDKGE_BATCH_REG_MODULUS) {
        snprintf(msg, sizeof(msg), "batch_reg: unknown norm mode of the %s term", which);
        return set_error(AMDKGE_EINVAL, msg);
    }
    if (!(lambda >= 0.f) || __builtin_isinf(lambda)) {
        snprintf(msg, sizeof(msg), "batch_reg: lambda of the %s term must be finite and >= 0", which);
        return set_error(AMDKGE_EINVAL, msg);
    }
    if (norm == AMDKGE_BATCH_REG_MODULUS && !modulus_ok) {
        snprintf(msg, sizeof(msg), "batch_reg: AMDKGE_BATCH_REG_MODULUS is not offered for the %s term of this model: %s", which, why_not);
        return set_error(AMDKGE_EUNSUPPORTED, msg);
    }
    t.on = lambda != 0.f;
    t.cube = p == 3;
    t.modulus = norm == AMDKGE_BATCH_REG_MODULUS;
    t.c = (float)p * lambda;
    t.lambda = lambda;
    return AMDKGE_OK;
}

template <bool CPLX, int VEC>
static int launch_batch_reg(const BatchRegArgs& a, hipStream_t st) {
    int64_t blocks = (a.B + 3) / 4;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL((batch_reg_kernel<CPLX, VEC>), dim3((unsigned)blocks), dim3(256), 0, st, a);
    return check_launch("batch_reg");
}

}  // namespace kge

using namespace kge;

extern "C" int amdkge_batch_reg_fwdbwd(const amdkge_model* m, const float* d_ent, const float* d_rel, const int32_t* d_triples, int64_t B, int32_t p_ent,
                                       float lambda_ent, int32_t norm_ent, int32_t p_rel, float lambda_rel, int32_t norm_rel, float* d_grad_ent,
                                       float* d_grad_rel, double* d_reg_sum, void* stream) {
    if (int rc = validate_model(m)) return rc;
    const bool cplx = complex_layout(m);
    BatchRegArgs a{};
    if (int rc = batch_reg_term("entity", p_ent, lambda_ent, norm_ent, cplx, "TransE and DistMult rows hold real units", a.e)) return rc;
    if (int rc = batch_reg_term("relation", p_rel, lambda_rel, norm_rel, cplx && m->scoring_type != AMDKGE_ROTATE,
                                cplx ? "a RotatE relation row holds phases, its modulus is 1" : "TransE and DistMult rows hold real units", a.r))
        return rc;
    if (B < 0) return set_error(AMDKGE_EINVAL, "batch_reg: B must be >= 0");
    if (!d_ent || !d_rel || !d_reg_sum) return set_error(AMDKGE_EINVAL, "batch_reg: NULL table / penalty pointer");
    if ((a.e.on && !d_grad_ent) || (a.r.on && !d_grad_rel)) return set_error(AMDKGE_EINVAL, "batch_reg: NULL gradient table of a term whose lambda is not 0");
    if (B == 0) return AMDKGE_OK;
    if (!d_triples) return set_error(AMDKGE_EINVAL, "batch_reg: NULL triples");
    if (!a.e.on && !a.r.on) return AMDKGE_OK;
    a.ent = d_ent; a.rel = d_rel; a.triples = d_triples; a.B = B; a.ks = stored_k(m); a.k = m->k;
    a.g_ent = d_grad_ent; a.g_rel = d_grad_rel; a.reg_sum = d_reg_sum;
    // 16-byte loads: whole groups of four units per stored half, and rows that start on 16 bytes
    const uintptr_t bits = (uintptr_t)d_ent | (uintptr_t)d_rel;
    const bool vec = a.ks % 4 == 0 && bits % 16 == 0;
    hipStream_t st = (hipStream_t)stream;
    if (cplx) return vec ? launch_batch_reg<true, 4>(a, st) : launch_batch_reg<true, 1>(a, st);
    return vec ? launch_batch_reg<false, 4>(a, st) : launch_batch_reg<false, 1>(a, st);
}
