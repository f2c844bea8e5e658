// Shared-negative training for the distance models (include/amdkge_shared_dist.h): the step of kge_train_shared.hip for TransE and
// RotatE.  A distance against a shared list is no matrix product, but it is still a tile: a group's G query vectors and its M gathered
// rows are each read once, and the G x M x k pair-units are arithmetic on operands in LDS and registers.  The header declares the
// arithmetic; tests/shared_dist_ref.py restates it in numpy.
//   dist_query_kernel<MODEL> : a wave per positive.  q_i = s + p / o - p (TransE), s o r / o o conj(r) (RotatE) for the positive's OWN
//                              side, and the positive's raw distance sum_u |q_i - own_i|.
//   dist_tile_kernel<MODEL, MODE> : 256 threads, operands staged through LDS (row stride 65: a chunk staged along the units lands on
//                              distinct banks), every thread a small block of sums in registers.
//                                FWD : a 64 x 64 tile of D(i, j) = sum_u |q_iu - e_ju|, Q and the gathered E staged in chunks of 32 units,
//                                      a 4 x 4 block per thread, plain stores into the score buffer [rows, M]: the same bits every run.
//                                DQ  : a workgroup owns 64 rows x 32 units (q in registers, a 4 x 2 block per thread) and loops over the
//                                      group's WHOLE list in chunks of 32 entries: dQ [B, K] by plain stores, no atomics.
//                                DE  : a workgroup owns 64 list entries x 32 units (e in registers) and loops over the group's rows:
//                                      atomic row-adds into d_grad_ent[ids[j]] (an id may repeat anywhere).
//                              DQ and DE are ONE loop: the owner operand in registers, the other staged, the coefficients staged as
//                              C[loop][owner]; they differ in where an operand comes from and where the result goes.  The chunk after
//                              the one being computed is already on its way into registers (dist_load_chunk).  Everything past a
//                              matrix edge is staged as zero: a zero coefficient adds nothing, units past k are never written out.
//   dist_chain_kernel<MODEL> : a wave per positive.  t_i = dQ_i + c_pos n_i = dL/dq_i (n = sign / unit vector of q_i - own_i); the two
//                              kept rows get the transpose of the query map (RotatE: the phase gradient / phase_div), the replaced
//                              row's original gets -c_pos n_i.
// The score buffer holds the plain distance sums and the loss runs with scale = -1, so shared_mask_kernel (fill = +inf) and
// shared_loss_kernel of kge_train_shared.hip run unchanged on it, through shared_loss_stage of kge_train_shared.h; the
// coefficients they leave are dL/dD = -dL/dscore.  Only the model's k live units are visited: a padding unit of RotatE has modulus 0.
// The host side of a step is shared_step (kge_train_shared.h, defined in kge_train_shared.hip); this unit gives it the DISTANCES family:
// the prefix and model test of its messages, ceil(k / 32) tiles along the units, and dist_launch for the kernels above.
#include "kge_train_shared.h"
#include "../../include/amdkge_shared_dist.h"

namespace kge {

template <int MODEL>
struct DistTraits {
    static constexpr int NC = MODEL == AMDKGE_ROTATE ? 2 : 1;   // floats per unit: component c of unit u is at c * ks + u of a stored row
};

// c * sign(d): sign(0) = 0, NaN kept (kge_device.h, grad_unit).  Written on the bits -- c with d's sign bit folded in, and d itself where
// d is a zero (a signed zero adds nothing) or a NaN: one class test and one select.  As nested ?: on comparisons the compiler turned
// every pair-unit of the tile loop into two exec-mask branches.
__device__ __forceinline__ float sign_times(float d, float c) {
    constexpr int ZERO_OR_NAN = 0x001 | 0x002 | 0x020 | 0x040;   // v_cmp_class_f32: signalling NaN, quiet NaN, -0, +0
    const float sc = __uint_as_float(__float_as_uint(c) ^ (__float_as_uint(d) & 0x80000000u));
    return __builtin_amdgcn_class(d, ZERO_OR_NAN) ? d : sc;
}

// |z|^2 of a complex residual.  The unit is built with -ffp-contract=off like the rest of the library; the fused form is written out
// where the header leaves the rounding open (one instruction less per pair-unit in the tiles), and used by all four kernels alike.
__device__ __forceinline__ float dist_mod2(float z0, float z1) { return fmaf(z1, z1, z0 * z0); }

// ---- query vectors ------------------------------------------------------------------------------------------------------------------
template <int MODEL>
__device__ __forceinline__ void dist_query_unit(const ModelConst& mc, bool subj, const float* S, const float* P, const float* O, int ks, int u, float (&q)[DistTraits<MODEL>::NC]) {
    if constexpr (MODEL == AMDKGE_TRANSE) {
        q[0] = subj ? O[u] - P[u] : S[u] + P[u];
    } else {
        float r[2] = {P[u], 0.f};
        prep_rel<AMDKGE_ROTATE>(mc, r);   // (cos, sin) of theta / phase_div
        if (subj) {   // o o conj(r)
            const float o0 = O[u], o1 = O[ks + u];
            q[0] = o0 * r[0] + o1 * r[1]; q[1] = o1 * r[0] - o0 * r[1];
        } else {      // s o r
            const float s0 = S[u], s1 = S[ks + u];
            q[0] = s0 * r[0] - s1 * r[1]; q[1] = s0 * r[1] + s1 * r[0];
        }
    }
}

template <int MODEL>
__global__ __launch_bounds__(256) void dist_query_kernel(const float* __restrict__ ent, const float* __restrict__ rel, const int32_t* __restrict__ triples,
                                                         const int32_t* __restrict__ side, int64_t B, int ks, int k, ModelConst mc, float* __restrict__ Q,
                                                         float* __restrict__ pos_raw) {
    constexpr int NC = DistTraits<MODEL>::NC;
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= B) return;   // (wave-uniform; the kernel has no barrier)
    const int K = NC * ks;
    const bool subj = side[i] != 0;
    const float* S = ent + (int64_t)triples[3 * i] * K;
    const float* P = rel + (int64_t)triples[3 * i + 1] * K;
    const float* O = ent + (int64_t)triples[3 * i + 2] * K;
    const float* own = subj ? S : O;
    float* q = Q + i * K;
    float acc = 0.f;
    for (int u = lane; u < k; u += 64) {
        float qq[NC];
        dist_query_unit<MODEL>(mc, subj, S, P, O, ks, u, qq);
        if constexpr (MODEL == AMDKGE_TRANSE) {
            q[u] = qq[0];
            acc += fabsf(qq[0] - own[u]);
        } else {
            q[u] = qq[0]; q[ks + u] = qq[1];
            const float z0 = qq[0] - own[u], z1 = qq[1] - own[ks + u];
            acc += __builtin_amdgcn_sqrtf(dist_mod2(z0, z1));
        }
    }
    acc = wave_sum_shfl(acc);
    if (lane == 0) pos_raw[i] = acc;
}

// ---- the three tiles ----------------------------------------------------------------------------------------------------------------
enum { DIST_FWD = 0, DIST_DQ = 1, DIST_DE = 2 };
constexpr int DT = 64;        // tile edge: rows of a group / entries of its list
constexpr int DKC = 32;       // units per chunk
constexpr int DLC = 32;       // entries of the loop dimension staged at once (DQ: list entries, DE: rows)
constexpr int DLD = DT + 1;   // LDS row stride

struct DistTileArgs {
    const float* ent;
    const int32_t* ids;   // [n_groups, M]
    const float* Q;       // [B, K]
    float* S;             // [rows of the chunk, M]: distance sums, then dL/dD
    float* dQ;            // [B, K]
    float* g_ent;
    int64_t B, G;
    int M, K, ks, k;      // floats per stored row, units per half as stored, live units
    int64_t g0;           // first group of the chunk (row0 = g0 * G)
    int tiles_m, tiles_n;
};

// One chunk of the backward tiles' loop dimension (DLC entries from l0) into registers: this thread's 4 elements per component of the
// loop operand (DQ: gathered rows of E, DE: rows of Q; contiguous along the units) and its 8 coefficients (DQ: C[i][j] contiguous along
// the list, DE: contiguous along the owners).  Zeros past every edge.
template <int MODEL, int MODE>
__device__ __forceinline__ void dist_load_chunk(const DistTileArgs& a, const int32_t* __restrict__ gid, int64_t row_first, int64_t srow, int m0, int u0, int mdim, int ldim,
                                                int l0, int tid, float (&ny)[DistTraits<MODEL>::NC][4], float (&nc)[8]) {
    constexpr int NC = DistTraits<MODEL>::NC;
    const int kk = tid & 31;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int ll = (tid >> 5) + 8 * r;
        const bool ok = l0 + ll < ldim && u0 + kk < a.k;
        const float* p = MODE == DIST_DQ ? a.ent + (ok ? (int64_t)gid[l0 + ll] * a.K + (u0 + kk) : 0) : a.Q + (row_first + l0 + ll) * a.K + (u0 + kk);
#pragma unroll
        for (int h = 0; h < NC; ++h) ny[h][r] = ok ? p[h * a.ks] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        if constexpr (MODE == DIST_DQ) {
            const int ll = tid & 31, oo = (tid >> 5) + 8 * r;
            nc[r] = (m0 + oo < mdim && l0 + ll < ldim) ? a.S[(srow + m0 + oo) * a.M + (l0 + ll)] : 0.f;
        } else {
            const int oo = tid & 63, ll = (tid >> 6) + 4 * r;
            nc[r] = (m0 + oo < mdim && l0 + ll < ldim) ? a.S[(srow + l0 + ll) * a.M + (m0 + oo)] : 0.f;
        }
    }
}

template <int MODEL, int MODE>
__global__ __launch_bounds__(256) void dist_tile_kernel(DistTileArgs a) {
    constexpr int NC = DistTraits<MODEL>::NC;
    const int tid = threadIdx.x;
    const int per_group = a.tiles_m * a.tiles_n;
    const int64_t g = a.g0 + blockIdx.x / per_group;
    const int tile = blockIdx.x % per_group;
    const int64_t row_first = g * a.G;                                         // the group's first positive
    const int Gg = (int)((a.B - row_first) < a.G ? (a.B - row_first) : a.G);   // its positives
    const int64_t srow = row_first - a.g0 * a.G;                               // its first row in the score buffer
    const int32_t* gid = a.ids + g * a.M;

    if constexpr (MODE == DIST_FWD) {
        __shared__ float Qs[NC][DKC][DLD];
        __shared__ float Es[NC][DKC][DLD];
        const int m0 = (tile / a.tiles_n) * DT, n0 = (tile % a.tiles_n) * DT;
        if (m0 >= Gg) return;   // (the last, short group: uniform over the workgroup)
        const int tj = tid & 15, ti = tid >> 4;   // the thread's sums: rows ti + 16 r, columns tj + 16 c
        float acc[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
        for (int k0 = 0; k0 < a.k; k0 += DKC) {
            {   // stage both operands: contiguous along the units
                const int kk = tid & 31;
                const bool uok = k0 + kk < a.k;
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const int mm = (tid >> 5) + 8 * r;
                    const bool qok = uok && m0 + mm < Gg, eok = uok && n0 + mm < a.M;
                    const float* qp = a.Q + (row_first + m0 + mm) * a.K + (k0 + kk);
                    const float* ep = a.ent + (eok ? (int64_t)gid[n0 + mm] * a.K + (k0 + kk) : 0);
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        Qs[c][kk][mm] = qok ? qp[c * a.ks] : 0.f;
                        Es[c][kk][mm] = eok ? ep[c * a.ks] : 0.f;
                    }
                }
            }
            __syncthreads();
#pragma unroll 8
            for (int kk = 0; kk < DKC; ++kk) {
                float q[NC][4], e[NC][4];
#pragma unroll
                for (int c = 0; c < NC; ++c)
#pragma unroll
                    for (int r = 0; r < 4; ++r) { q[c][r] = Qs[c][kk][ti + 16 * r]; e[c][r] = Es[c][kk][tj + 16 * r]; }
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        if constexpr (MODEL == AMDKGE_TRANSE) {
                            acc[r][c] += fabsf(q[0][r] - e[0][c]);
                        } else {
                            const float z0 = q[0][r] - e[0][c], z1 = q[1][r] - e[1][c];
                            acc[r][c] += __builtin_amdgcn_sqrtf(dist_mod2(z0, z1));   // (a staged-zero unit: sqrt(0) = 0)
                        }
                    }
            }
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = m0 + ti + 16 * r;
            if (row >= Gg) continue;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int col = n0 + tj + 16 * c;
                if (col < a.M) a.S[(srow + row) * a.M + col] = acc[r][c];
            }
        }
    } else {
        // the OWNER operand (DQ: the group's rows, DE: its list) sits in registers, the LOOP operand (DQ: the list, DE: the rows) goes
        // through LDS with the coefficients C[loop][owner]
        __shared__ float Ys[NC][DLC][DKC];
        __shared__ float Cs[DLC][DLD];
        const int m0 = (tile / a.tiles_n) * DT, u0 = (tile % a.tiles_n) * DKC;
        const int mdim = MODE == DIST_DQ ? Gg : a.M;
        const int ldim = MODE == DIST_DQ ? a.M : Gg;
        if (m0 >= mdim) return;   // (uniform over the workgroup)
        const int tu = tid & 15, to = tid >> 4;   // the thread's sums: owners to + 16 r, units tu + 16 c
        float own[NC][4][2], acc[NC][4][2];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = m0 + to + 16 * r;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int u = u0 + tu + 16 * c;
                const bool ok = o < mdim && u < a.k;
                const float* p = MODE == DIST_DQ ? a.Q + (row_first + o) * a.K + u : a.ent + (ok ? (int64_t)gid[o] * a.K + u : 0);
#pragma unroll
                for (int h = 0; h < NC; ++h) {
                    own[h][r][c] = ok ? p[h * a.ks] : 0.f;
                    acc[h][r][c] = 0.f;
                }
            }
        }
        // The chunk after the one being computed is loaded into registers first and stored to LDS behind the barrier that ends the
        // computation: the gathers' latency (comparable to a chunk's arithmetic) runs beside the arithmetic instead of in front of it.
        float ny[NC][4], nc[8];
        dist_load_chunk<MODEL, MODE>(a, gid, row_first, srow, m0, u0, mdim, ldim, 0, tid, ny, nc);
        for (int l0 = 0; l0 < ldim; l0 += DLC) {
            {   // Ys[l][u] (staged contiguous along the units) and C[loop][owner]
                const int kk = tid & 31;
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int h = 0; h < NC; ++h) Ys[h][(tid >> 5) + 8 * r][kk] = ny[h][r];
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    if constexpr (MODE == DIST_DQ) Cs[tid & 31][(tid >> 5) + 8 * r] = nc[r];
                    else Cs[(tid >> 6) + 4 * r][tid & 63] = nc[r];
                }
            }
            __syncthreads();
            if (l0 + DLC < ldim) dist_load_chunk<MODEL, MODE>(a, gid, row_first, srow, m0, u0, mdim, ldim, l0 + DLC, tid, ny, nc);   // (uniform)
#pragma unroll 4
            for (int ll = 0; ll < DLC; ++ll) {
                float cf[4], y[NC][2];
#pragma unroll
                for (int r = 0; r < 4; ++r) cf[r] = Cs[ll][to + 16 * r];
#pragma unroll
                for (int h = 0; h < NC; ++h)
#pragma unroll
                    for (int c = 0; c < 2; ++c) y[h][c] = Ys[h][ll][tu + 16 * c];
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        if constexpr (MODEL == AMDKGE_TRANSE) {   // d = q - e
                            const float d = MODE == DIST_DQ ? own[0][r][c] - y[0][c] : y[0][c] - own[0][r][c];
                            acc[0][r][c] += sign_times(d, cf[r]);
                        } else {                                  // z = q - e, c z / |z|; a zero coefficient (a masked entry, an edge) adds nothing
                            const float z0 = MODE == DIST_DQ ? own[0][r][c] - y[0][c] : y[0][c] - own[0][r][c];
                            const float z1 = MODE == DIST_DQ ? own[1][r][c] - y[1][c] : y[1][c] - own[1][r][c];
                            const float w = cf[r] != 0.f ? cf[r] * __builtin_amdgcn_rsqf(dist_mod2(z0, z1)) : 0.f;
                            acc[0][r][c] = fmaf(w, z0, acc[0][r][c]);
                            acc[1][r][c] = fmaf(w, z1, acc[1][r][c]);
                        }
                    }
            }
            __syncthreads();
        }
        // acc = sum c' sigma with c' = dL/dD: dL/dq = +acc, dL/de = -acc
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = m0 + to + 16 * r;
            if (o >= mdim) continue;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int u = u0 + tu + 16 * c;
                if (u >= a.k) continue;
#pragma unroll
                for (int h = 0; h < NC; ++h) {
                    if constexpr (MODE == DIST_DQ) {
                        a.dQ[(row_first + o) * a.K + h * a.ks + u] = acc[h][r][c];
                    } else {
                        const float v = -acc[h][r][c];
                        if (v != 0.f) atomic_add_f32(a.g_ent + (int64_t)gid[o] * a.K + h * a.ks + u, v);   // (true for NaN)
                    }
                }
            }
        }
    }
}

// ---- the transpose of the query map -------------------------------------------------------------------------------------------------
template <int MODEL>
__global__ __launch_bounds__(256) void dist_chain_kernel(const float* __restrict__ ent, const float* __restrict__ rel, const int32_t* __restrict__ triples,
                                                         const int32_t* __restrict__ side, int64_t B, int ks, int k, ModelConst mc, const float* __restrict__ Q,
                                                         const float* __restrict__ dQ, const float* __restrict__ cpos, float* g_ent, float* g_rel) {
    constexpr int NC = DistTraits<MODEL>::NC;
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= B) return;
    const int K = NC * ks;
    const bool subj = side[i] != 0;
    const int64_t so = (int64_t)triples[3 * i] * K, po = (int64_t)triples[3 * i + 1] * K, oo = (int64_t)triples[3 * i + 2] * K;
    const float* own = ent + (subj ? so : oo);
    const float* P = rel + po;
    const float* q = Q + i * K;
    const float* d = dQ + i * K;
    const float c = cpos[i];                    // dL/dD of the positive's own distance
    float* g_own = g_ent + (subj ? so : oo);    // the replaced row's original
    float* g_kept = g_ent + (subj ? oo : so);   // the kept entity row
    float* g_p = g_rel + po;
    for (int u = lane; u < k; u += 64) {
        if constexpr (MODEL == AMDKGE_TRANSE) {
            const float n = sign_times(q[u] - own[u], c);   // c sigma
            const float t = d[u] + n;                       // dL/dq
            add_nz(g_own + u, -n);
            add_nz(g_kept + u, t);
            add_nz(g_p + u, subj ? -t : t);            // q = o - p : s + p
        } else {
            const float q0 = q[u], q1 = q[ks + u];
            const float z0 = q0 - own[u], z1 = q1 - own[ks + u];
            const float w = c * __builtin_amdgcn_rsqf(dist_mod2(z0, z1));   // (no guard: a modulus of zero is NaN, as in the reference)
            const float n0 = w * z0, n1 = w * z1;
            const float t0 = d[u] + n0, t1 = d[ks + u] + n1;
            float r[2] = {P[u], 0.f};
            prep_rel<AMDKGE_ROTATE>(mc, r);
            float k0, k1, dphi;
            if (subj) {   // q = o o conj(r): dq/do is r, dq/dphi = (q1, -q0)
                k0 = t0 * r[0] - t1 * r[1]; k1 = t0 * r[1] + t1 * r[0];
                dphi = t0 * q1 - t1 * q0;
            } else {      // q = s o r: dq/ds is conj(r), dq/dphi = (-q1, q0)
                k0 = t0 * r[0] + t1 * r[1]; k1 = t1 * r[0] - t0 * r[1];
                dphi = t1 * q0 - t0 * q1;
            }
            add_nz(g_own + u, -n0); add_nz(g_own + ks + u, -n1);
            add_nz(g_kept + u, k0); add_nz(g_kept + ks + u, k1);
            add_nz(g_p + u, dphi / mc.phase_div);
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
static bool dist_model_ok(const amdkge_model* m) { return m->scoring_type == AMDKGE_TRANSE || m->scoring_type == AMDKGE_ROTATE; }

// the family's launches for shared_step (kge_train_shared.h)
static_assert(DT == SHARED_TILE, "the driver counts the tiles");
template <int MODEL>
static int dist_launch(const SharedStep& s, SharedStage stage, unsigned blocks, int64_t g0, int tiles_m, int tiles_n) {
    const int ks = stored_k(s.m), k = s.m->k;
    const ModelConst mc = model_const(s.m);
    DistTileArgs a{};
    a.ent = s.ent; a.ids = s.ids; a.Q = s.Q; a.S = s.S; a.dQ = s.dQ; a.g_ent = s.g_ent; a.B = s.B; a.G = s.G; a.M = s.M; a.K = row_floats(s.m); a.ks = ks; a.k = k;
    a.g0 = g0; a.tiles_m = tiles_m; a.tiles_n = tiles_n;
    static const char* const NAMES[] = {"dist_query", "dist_tile_fwd", "dist_tile_dq", "dist_tile_de", "dist_chain"};   // (by SharedStage)
    switch (stage) {
    case SHARED_QUERY: hipLaunchKernelGGL(dist_query_kernel<MODEL>, dim3(blocks), dim3(256), 0, s.st, s.ent, s.rel, s.triples, s.side, s.B, ks, k, mc, s.Q, s.pos_raw); break;
    case SHARED_FWD: hipLaunchKernelGGL((dist_tile_kernel<MODEL, DIST_FWD>), dim3(blocks), dim3(256), 0, s.st, a); break;
    case SHARED_DQ: hipLaunchKernelGGL((dist_tile_kernel<MODEL, DIST_DQ>), dim3(blocks), dim3(256), 0, s.st, a); break;
    case SHARED_DE: hipLaunchKernelGGL((dist_tile_kernel<MODEL, DIST_DE>), dim3(blocks), dim3(256), 0, s.st, a); break;
    case SHARED_CHAIN: hipLaunchKernelGGL(dist_chain_kernel<MODEL>, dim3(blocks), dim3(256), 0, s.st, s.ent, s.rel, s.triples, s.side, s.B, ks, k, mc, s.Q, s.dQ, s.cpos, s.g_ent, s.g_rel); break;
    }
    return check_launch(NAMES[stage]);
}
static const SharedFamily DISTANCES = {
    "train_shared_dist", dist_model_ok, "DistMult, ComplEx and HolE score a contraction, not a distance: use amdkge_train_shared_fwdbwd",
    [](const amdkge_model* m) { return (m->k + DKC - 1) / DKC; },
    [](const SharedStep& s, SharedStage stage, unsigned blocks, int64_t g0, int tiles_m, int tiles_n) {
        return s.m->scoring_type == AMDKGE_ROTATE ? dist_launch<AMDKGE_ROTATE>(s, stage, blocks, g0, tiles_m, tiles_n)
                                                  : dist_launch<AMDKGE_TRANSE>(s, stage, blocks, g0, tiles_m, tiles_n);
    }};

}  // namespace kge

using namespace kge;

extern "C" int64_t amdkge_train_shared_dist_workspace_bytes(const amdkge_model* m, int64_t B, int64_t G, int32_t M) {
    return shared_step_workspace_bytes(DISTANCES, m, B, G, M);
}

// both step entry points are shared_step on this family: the (optional) mask, or the labels

extern "C" int amdkge_train_shared_dist_fwdbwd(const amdkge_model* m, const amdkge_loss* loss, const float* d_ent, const float* d_rel, const int32_t* d_triples, int64_t B,
                                               int64_t G, int32_t M, const int32_t* d_neg_ids, const int32_t* d_side, float* d_grad_ent, float* d_grad_rel,
                                               double* d_loss_sum, float* d_pos_scores, float* d_neg_scores, void* d_work, const int64_t* d_s_lo, const int64_t* d_s_hi,
                                               const int32_t* d_s_ids, const int64_t* d_o_lo, const int64_t* d_o_hi, const int32_t* d_o_ids, int32_t list_mode,
                                               int64_t* d_stats, void* stream) {
    SharedMaskArgs ma;
    bool masked;
    if (int rc = shared_mask_args("train_shared_dist", d_neg_ids, d_s_lo, d_s_hi, d_s_ids, d_o_lo, d_o_hi, d_o_ids, list_mode, d_stats, false, ma, masked)) return rc;
    return shared_step(DISTANCES, m, loss, d_ent, d_rel, d_triples, B, G, M, d_neg_ids, d_side, d_grad_ent, d_grad_rel, d_loss_sum, d_pos_scores, d_neg_scores, d_work,
                       masked ? &ma : nullptr, nullptr, stream);
}

// (include/amdkge_shared_labels.h)
extern "C" int amdkge_train_shared_dist_labels_fwdbwd(const amdkge_model* m, float label_smoothing, int32_t reduction_mean, const float* d_ent, const float* d_rel,
                                                      const int32_t* d_triples, int64_t B, int64_t G, int32_t M, const int32_t* d_neg_ids, const int32_t* d_side,
                                                      float* d_grad_ent, float* d_grad_rel, double* d_loss_sum, float* d_pos_scores, float* d_neg_scores, void* d_work,
                                                      const int64_t* d_s_lo, const int64_t* d_s_hi, const int32_t* d_s_ids, const int64_t* d_o_lo,
                                                      const int64_t* d_o_hi, const int32_t* d_o_ids, int32_t list_mode, const float* d_w_s, const float* d_w_o,
                                                      int64_t* d_stats, void* stream) {
    SharedLabelArgs la;
    if (int rc = shared_label_args("train_shared_dist_labels", d_neg_ids, d_s_lo, d_s_hi, d_s_ids, d_o_lo, d_o_hi, d_o_ids, list_mode, label_smoothing, reduction_mean,
                                   d_w_s, d_w_o, d_stats, la)) return rc;
    return shared_step(DISTANCES, m, nullptr, d_ent, d_rel, d_triples, B, G, M, d_neg_ids, d_side, d_grad_ent, d_grad_rel, d_loss_sum, d_pos_scores, d_neg_scores, d_work,
                       nullptr, &la, stream);
}
