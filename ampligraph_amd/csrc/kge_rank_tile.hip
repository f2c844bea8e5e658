// evaluate(): the VALU tile kernels of the 1-vs-all count pass and everything built on them.
//   rank_count_kernel : LDS-tiled (64 queries x 64 entities x 16 units) score tile with a quantise -> compare -> count epilogue;
//                       only two int32 counters per triple leave the CU.  STORE variants write the scores instead (discovery),
//                       EARLY variants are the distance models' exact early exit (kge_rank_early.h).
//   rank_rot_kernel   : the same tiling for RotatE's exact mode (correctly rounded modulus).
// The chain is rank_op / rot_exact_op of kge_rank_common.h: bitwise the scores of the MFMA, filter and recheck kernels.
#include "kge_rank_common.h"
#include "kge_rank_early.h"   // the distance models' exact early exit: thresholds, the check-point protocol, probe, recheck, merge

namespace kge {

// ------------------------------------------------------------------------------------------------
// tile kernel
// ------------------------------------------------------------------------------------------------
template <int MODE, bool V4, bool STORE = false, bool EARLY = false>
__global__ __launch_bounds__(256) void rank_count_kernel(CountArgs a) {
    constexpr int NQF = ModeTraits<MODE>::NQF, NEF = ModeTraits<MODE>::NEF;
    static_assert(!EARLY || ((MODE == MODE_L1 || MODE == MODE_L1_SUB) && V4 && !STORE), "early exit: the TransE count kernels");
    __shared__ __attribute__((aligned(16))) float Qs[NQF][KT][LDP];
    __shared__ __attribute__((aligned(16))) float Es[NEF][KT][LDP];
    __shared__ EarlyShared es_;   // (referenced by the EARLY variants only: elsewhere it is never allocated)
    if (a.guard_mode ? !guard_says_run(a.guard_mode, a.guard, a.e_probe) : (a.guard && *a.guard == 0)) return;   // a launch that turned out not to be needed

    const int tid = threadIdx.x;
    const int tq = tid >> 4, te = tid & 15;
    const int64_t q0 = (int64_t)blockIdx.x * QT;
    const int64_t e_begin = a.ent_lo + (int64_t)blockIdx.y * a.ent_per_block;
    const int64_t e_end = min(a.ent_hi, e_begin + a.ent_per_block);

    int qp[4] = {0, 0, 0, 0};
    if constexpr (!STORE) {
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int64_t qi = q0 + tq * 4 + x;
            qp[x] = a.qpos[qi < a.n ? qi : a.n - 1];
        }
    }
    int cgt[4] = {0, 0, 0, 0}, ceq[4] = {0, 0, 0, 0};
    // EARLY: per query the partial sum beyond which the pair is decided (it can no longer reach the positive's quantised score);
    // +inf for a query row that must not be decided early; rows beyond n take no part
    float thr[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t qvalid = 0u;
    if constexpr (EARLY) {
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int64_t qi = q0 + tq * 4 + x;
            thr[x] = early_threshold(qp[x], a.sgn_scale);
            if (qi < a.n) { qvalid |= 0xFu << (4 * x); if (a.e_qbad[qi]) thr[x] = INFINITY; }
        }
        if (tid == 0) es_.n = 0;
    }

    // loader mapping: row = tid / 4 (0..63), 4-unit group = tid % 4
    const int lrow = tid >> 2, lgrp = tid & 3;
    const int64_t lq = q0 + lrow;
    const float* qrow = a.Q + (lq < a.n ? lq : a.n - 1) * (int64_t)a.g.QW;

    for (int64_t et = e_begin; et < e_end; et += ET) {
        const int64_t le = et + lrow;
        const int64_t le_c = le < e_end ? le : e_end - 1;
        const int64_t erow_id = a.ent_ids ? (int64_t)a.ent_ids[le_c] : le_c;
        const float* erow = a.ent + erow_id * a.g.K;
        float acc[4][4];
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int y = 0; y < 4; ++y) acc[x][y] = 0.f;
        // EARLY: which of the thread's 16 pairs exist at all (query < n, candidate inside the range) and which must stay undecided
        uint32_t pvalid = 0u, pkeep = 0u;
        bool ended = false;
        if constexpr (EARLY) {
#pragma unroll
            for (int y = 0; y < 4; ++y) {
                const int64_t ej = et + te * 4 + y;
                if (ej < e_end) { pvalid |= 0x1111u << y; if (a.e_ebad[ej - a.ent_lo]) pkeep |= 0x1111u << y; }
            }
            pvalid &= qvalid;
            pkeep &= pvalid;
        }

        for (int k0 = 0; k0 < a.g.U; k0 += KT) {
            const int ku = k0 + lgrp * 4;
            // ---- global -> LDS (transposed: [plane][unit][row]) ----
#pragma unroll
            for (int f = 0; f < NQF; ++f) {
                float v[4];
                if (V4 && ku + 3 < a.g.U) {
                    const float4 t = *reinterpret_cast<const float4*>(qrow + f * a.g.qplane + ku);
                    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u) v[u] = (ku + u < a.g.U) ? qrow[f * a.g.qplane + ku + u] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) Qs[f][lgrp * 4 + u][lrow] = v[u];
            }
#pragma unroll
            for (int f = 0; f < NEF; ++f) {
                float v[4];
                if (V4 && ku + 3 < a.g.U) {
                    const float4 t = *reinterpret_cast<const float4*>(erow + f * a.g.eplane + ku);
                    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u) v[u] = (ku + u < a.g.U) ? erow[f * a.g.eplane + ku + u] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) Es[f][lgrp * 4 + u][lrow] = v[u];
            }
            __syncthreads();
            // ---- 4x4 micro tile over the KT units, strictly in unit order ----
#pragma unroll
            for (int kk = 0; kk < KT; ++kk) {
                float qv[NQF][4], ev[NEF][4];
#pragma unroll
                for (int f = 0; f < NQF; ++f) {
                    const float4 t = *reinterpret_cast<const float4*>(&Qs[f][kk][tq * 4]);
                    qv[f][0] = t.x; qv[f][1] = t.y; qv[f][2] = t.z; qv[f][3] = t.w;
                }
#pragma unroll
                for (int f = 0; f < NEF; ++f) {
                    const float4 t = *reinterpret_cast<const float4*>(&Es[f][kk][te * 4]);
                    ev[f][0] = t.x; ev[f][1] = t.y; ev[f][2] = t.z; ev[f][3] = t.w;
                }
                if constexpr (MODE == MODE_L1 || MODE == MODE_L1_SUB) {
                    // rank_op's two operations with the first one packed: v_pk_add_f32 forms q +- e for two entities at
                    // once (q broadcast through op_sel), add_abs accumulates each -- 3 issue slots per 2 units
#pragma unroll
                    for (int x = 0; x < 4; ++x)
#pragma unroll
                        for (int y = 0; y < 4; y += 2) {
                            const f32x2 qq = {qv[0][x], qv[0][x]}, ee = {ev[0][y], ev[0][y + 1]};
                            const f32x2 d = (MODE == MODE_L1) ? qq + ee : qq - ee;
                            acc[x][y] = add_abs(acc[x][y], d.x);
                            acc[x][y + 1] = add_abs(acc[x][y + 1], d.y);
                        }
                } else {
#pragma unroll
                    for (int x = 0; x < 4; ++x)
#pragma unroll
                        for (int y = 0; y < 4; ++y) {
                            float qq[NQF], ee[NEF];
#pragma unroll
                            for (int f = 0; f < NQF; ++f) qq[f] = qv[f][x];
#pragma unroll
                            for (int f = 0; f < NEF; ++f) ee[f] = ev[f][y];
                            acc[x][y] = rank_op<MODE>(acc[x][y], qq, ee, a.g.sgn);
                        }
                }
            }
            // EARLY, every e_check stages (not behind the last one): count the pairs that are still undecided; the stage's own
            // barrier publishes the four wave sums
            bool chk = false;
            uint32_t und = 0u;
            if constexpr (EARLY) {
                chk = ((k0 / KT + 1) % a.e_check == 0) && (k0 + KT < a.g.U);
                if (chk) {
#pragma unroll
                    for (int x = 0; x < 4; ++x)
#pragma unroll
                        for (int y = 0; y < 4; ++y) und |= (acc[x][y] > thr[x]) ? 0u : (1u << (4 * x + y));   // (NaN: undecided)
                    und = (und | pkeep) & pvalid;
                    const int c = wave_sum_i(__popc(und));
                    if ((tid & 63) == 0) es_.red[tid >> 6] = c;
                }
            }
            __syncthreads();
            if constexpr (EARLY) {
                int total;
                if (chk && early_decide(es_, k0 + KT, a.g.U, a.e_cost, total)) {
                    early_spill(es_, a.e_list, und, total, q0 + tq * 4, et + te * 4 - a.ent_lo);
                    ended = true;
                    break;
                }
            }
        }
        if constexpr (EARLY) { if (ended) continue; }   // decided or handed over: nothing of this tile is counted here
        if constexpr (STORE) {
            // ---- epilogue of the STORE variant: the scores themselves (discovery: top-k / nearest neighbours) ----
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const int64_t qi = q0 + tq * 4 + x;
#pragma unroll
                for (int y = 0; y < 4; ++y) {
                    const int64_t ej = et + te * 4 + y;
                    if (qi < a.n && ej < e_end) a.scores[qi * a.ld + (ej - a.ent_lo)] = a.sgn_scale * acc[x][y];
                }
            }
            continue;
        }
        // ---- epilogue: quantise, compare, count ----
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            const bool valid = (et + te * 4 + y) < e_end;
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const int q = quantise(a.sgn_scale * acc[x][y]);
                cgt[x] += (valid && qp[x] < q) ? 1 : 0;
                ceq[x] += (valid && qp[x] == q) ? 1 : 0;
            }
        }
    }
    if constexpr (STORE) return;
    // reduce over the 16 lanes (te) that share the same queries, one atomic pair per query per block
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        int g = cgt[x], e = ceq[x];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) { g += __shfl_xor(g, o, 64); e += __shfl_xor(e, o, 64); }
        const int64_t qi = q0 + tq * 4 + x;
        if (te == 0 && qi < a.n) {
            if (g) atomicAdd(&a.counts[2 * qi + 0], g);
            if (e) atomicAdd(&a.counts[2 * qi + 1], e);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// RotatE, exact mode (the default): the tile kernel with the per-unit modulus CORRECTLY ROUNDED, so that the whole chain
//     acc = fl(acc + sqrt_rn(fl(fl(re * re) + fl(im * im))))          (RotatE.py:151-160,209-214, unit order)
// is a function of the inputs alone and a CPU restatement (oracle/csrc/rank_ordered.c) reproduces the ranks bit for bit.
// Same tiling as rank_count_kernel (64 queries x 64 entities, 16 units per LDS stage, 4 x 4 micro tile per thread); the
// arithmetic is written on PAIRS of entities so that it issues as packed fp32 (v_pk_add / v_pk_mul / v_pk_fma_f32: two lanes
// of work per slot) and the modulus is sqrt_rn's fast sequence without its branch: v_rsq_f32 + 4 packed operations per pair.
// Its domain (x >= 2^-100: exhaustively verified, see sqrt_rn in kge_device.h) is checked per entity tile and costs half a
// slot per unit: every thread keeps the maximum of its v_rsq results (x < 2^-100, zero or denormal <=> g > 2^50) and looks at
// its 16 accumulators (x = inf or NaN poisons them); if anything in the WORKGROUP is outside, the tile is redone with libm's
// sqrtf.  Padding units of the stored layout are not walked at all (U = the model's k: their x is an exact 0, which is
// outside the fast domain); live units with re = im = 0 exactly (a corruption that coincides with the rotated subject in
// both components) take the slow path and are the only realistic trigger.
// ------------------------------------------------------------------------------------------------
template <bool SLOW, bool SUBJ>
__device__ __forceinline__ void rot_micro(const float (&qv)[SUBJ ? 4 : 2][4], const float (&ev)[2][4], f32x2 (&acc)[4][2], float& gmax) {
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const f32x2 e0 = {ev[0][2 * y], ev[0][2 * y + 1]}, e1 = {ev[1][2 * y], ev[1][2 * y + 1]};
            f32x2 re, im;
            if constexpr (!SUBJ) {   // q = s o r                                    RotatE.py:209-214
                const f32x2 q0 = {qv[0][x], qv[0][x]}, q1 = {qv[1][x], qv[1][x]};
                re = q0 - e0;
                im = q1 - e1;
            } else {                 // q = (cos, sin, o_re, o_im)                   RotatE.py:151-160
                const f32x2 c = {qv[0][x], qv[0][x]}, sn = {qv[1][x], qv[1][x]}, orr = {qv[2][x], qv[2][x]}, oi = {qv[3][x], qv[3][x]};
                re = e0 * c - e1 * sn - orr;
                im = e0 * sn + e1 * c - oi;
            }
            const f32x2 xx = re * re + im * im;
            f32x2 m;
            if constexpr (SLOW) {
                m.x = sqrtf(xx.x);
                m.y = sqrtf(xx.y);
            } else {
                f32x2 g;
                g.x = __builtin_amdgcn_rsqf(xx.x);
                g.y = __builtin_amdgcn_rsqf(xx.y);
                gmax = fmaxf(fmaxf(gmax, g.x), g.y);
                const f32x2 yv = xx * g, h = g * 0.5f;
                const f32x2 r = __builtin_elementwise_fma(-yv, yv, xx);
                m = __builtin_elementwise_fma(r, h, yv);
            }
            acc[x][y] = acc[x][y] + m;
        }
}

template <bool SUBJ, bool STORE, bool EARLY = false>
__global__ __launch_bounds__(256) void rank_rot_kernel(CountArgs a) {
    constexpr int NQF = SUBJ ? 4 : 2, NEF = 2;
    static_assert(!EARLY || !STORE, "early exit: the count form only");
    __shared__ __attribute__((aligned(16))) float Qs[NQF][KT][LDP];
    __shared__ __attribute__((aligned(16))) float Es[NEF][KT][LDP];
    __shared__ EarlyShared es_;   // (referenced by the EARLY variants only: elsewhere it is never allocated)
    if (a.guard_mode ? !guard_says_run(a.guard_mode, a.guard, a.e_probe) : (a.guard && *a.guard == 0)) return;   // a launch that turned out not to be needed

    const int tid = threadIdx.x;
    const int tq = tid >> 4, te = tid & 15;
    const int64_t q0 = (int64_t)blockIdx.x * QT;
    const int64_t e_begin = a.ent_lo + (int64_t)blockIdx.y * a.ent_per_block;
    const int64_t e_end = min(a.ent_hi, e_begin + a.ent_per_block);
    const int U = a.g.U;   // live units; the planes of Q and of a table row are a.g.qplane / a.g.eplane (stored width) apart

    int qp[4] = {0, 0, 0, 0};
    if constexpr (!STORE) {
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int64_t qi = q0 + tq * 4 + x;
            qp[x] = a.qpos[qi < a.n ? qi : a.n - 1];
        }
    }
    int cgt[4] = {0, 0, 0, 0}, ceq[4] = {0, 0, 0, 0};
    float thr[4] = {0.f, 0.f, 0.f, 0.f};   // EARLY: see rank_count_kernel
    uint32_t qvalid = 0u;
    if constexpr (EARLY) {
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int64_t qi = q0 + tq * 4 + x;
            thr[x] = early_threshold(qp[x], a.sgn_scale);
            if (qi < a.n) { qvalid |= 0xFu << (4 * x); if (a.e_qbad[qi]) thr[x] = INFINITY; }
        }
        if (tid == 0) es_.n = 0;
    }

    const int lrow = tid >> 2, lgrp = tid & 3;   // loader: row 0..63, 4-unit group 0..3
    const int64_t lq = q0 + lrow;
    const float* qrow = a.Q + (lq < a.n ? lq : a.n - 1) * (int64_t)a.g.QW;

    for (int64_t et = e_begin; et < e_end; et += ET) {
        const int64_t le = et + lrow;
        const int64_t le_c = le < e_end ? le : e_end - 1;
        const int64_t erow_id = a.ent_ids ? (int64_t)a.ent_ids[le_c] : le_c;
        const float* erow = a.ent + erow_id * a.g.K;
        f32x2 acc[4][2];
        float gmax = 0.f;
        uint32_t pvalid = 0u, pkeep = 0u;   // EARLY: the thread's existing pairs / those that must stay undecided (bit 4 x + y)
        if constexpr (EARLY) {
#pragma unroll
            for (int y = 0; y < 4; ++y) {
                const int64_t ej = et + te * 4 + y;
                if (ej < e_end) { pvalid |= 0x1111u << y; if (a.e_ebad[ej - a.ent_lo]) pkeep |= 0x1111u << y; }
            }
            pvalid &= qvalid;
            pkeep &= pvalid;
        }

        // returns true when the tile ended early (EARLY, fast form only): its undecided pairs are on the list
        auto run_tile = [&](auto slow_c) __attribute__((always_inline)) -> bool {
            constexpr bool SLOW = decltype(slow_c)::value;
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y) acc[x][y] = f32x2{0.f, 0.f};
            for (int k0 = 0; k0 < U; k0 += KT) {
                // ---- global -> LDS, transposed to [plane][unit][row]; a 4-unit group that starts inside the row is loaded
                //      whole (the stored row is a whole number of float4s; what lies beyond U is never multiplied) ----
                const int ku = k0 + lgrp * 4;
                const bool in = ku < U;
#pragma unroll
                for (int f = 0; f < NQF; ++f) {
                    const float4 t = in ? *reinterpret_cast<const float4*>(qrow + f * a.g.qplane + ku) : make_float4(0.f, 0.f, 0.f, 0.f);
                    Qs[f][lgrp * 4 + 0][lrow] = t.x; Qs[f][lgrp * 4 + 1][lrow] = t.y; Qs[f][lgrp * 4 + 2][lrow] = t.z; Qs[f][lgrp * 4 + 3][lrow] = t.w;
                }
#pragma unroll
                for (int f = 0; f < NEF; ++f) {
                    const float4 t = in ? *reinterpret_cast<const float4*>(erow + f * a.g.eplane + ku) : make_float4(0.f, 0.f, 0.f, 0.f);
                    Es[f][lgrp * 4 + 0][lrow] = t.x; Es[f][lgrp * 4 + 1][lrow] = t.y; Es[f][lgrp * 4 + 2][lrow] = t.z; Es[f][lgrp * 4 + 3][lrow] = t.w;
                }
                __syncthreads();
                auto unit = [&](int kk) __attribute__((always_inline)) {
                    float qv[NQF][4], ev[NEF][4];
#pragma unroll
                    for (int f = 0; f < NQF; ++f) {
                        const float4 t = *reinterpret_cast<const float4*>(&Qs[f][kk][tq * 4]);
                        qv[f][0] = t.x; qv[f][1] = t.y; qv[f][2] = t.z; qv[f][3] = t.w;
                    }
#pragma unroll
                    for (int f = 0; f < NEF; ++f) {
                        const float4 t = *reinterpret_cast<const float4*>(&Es[f][kk][te * 4]);
                        ev[f][0] = t.x; ev[f][1] = t.y; ev[f][2] = t.z; ev[f][3] = t.w;
                    }
                    rot_micro<SLOW, SUBJ>(qv, ev, acc, gmax);
                };
                if (U - k0 >= KT) {
#pragma unroll
                    for (int kk = 0; kk < KT; ++kk) unit(kk);
                } else {
                    for (int kk = 0; kk < U - k0; ++kk) unit(kk);   // the row's last, partial stage: live units only
                }
                bool chk = false;
                uint32_t und = 0u;
                if constexpr (EARLY && !SLOW) {
                    chk = ((k0 / KT + 1) % a.e_check == 0) && (k0 + KT < U);
                    if (chk) {
#pragma unroll
                        for (int x = 0; x < 4; ++x)
#pragma unroll
                            for (int y = 0; y < 4; ++y) {
                                const float sc = (y & 1) ? acc[x][y >> 1].y : acc[x][y >> 1].x;
                                und |= (sc > thr[x]) ? 0u : (1u << (4 * x + y));   // (NaN: undecided)
                            }
                        und = (und | pkeep) & pvalid;
                        const int c = wave_sum_i(__popc(und));
                        // a modulus outside the fast form's domain so far (the partial sums cannot be trusted): no exit for this tile
                        const bool dom = __ballot(!(gmax <= 0x1p50f)) != 0ull;
                        if ((tid & 63) == 0) es_.red[tid >> 6] = c | (dom ? (1 << 30) : 0);
                    }
                }
                __syncthreads();
                if constexpr (EARLY && !SLOW) {
                    int total;
                    if (chk && early_decide(es_, k0 + KT, U, a.e_cost, total)) {
                        early_spill(es_, a.e_list, und, total, q0 + tq * 4, et + te * 4 - a.ent_lo);
                        return true;
                    }
                }
            }
            return false;
        };
        if (run_tile(std::false_type{})) continue;
        bool bad = !(gmax <= 0x1p50f);
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y) bad |= !(fabsf(acc[x][y].x) < INFINITY) || !(fabsf(acc[x][y].y) < INFINITY);
        if (__syncthreads_or(bad ? 1 : 0)) run_tile(std::true_type{});

        if constexpr (STORE) {
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const int64_t qi = q0 + tq * 4 + x;
#pragma unroll
                for (int y = 0; y < 4; ++y) {
                    const int64_t ej = et + te * 4 + y;
                    const float sc = (y & 1) ? acc[x][y >> 1].y : acc[x][y >> 1].x;
                    if (qi < a.n && ej < e_end) a.scores[qi * a.ld + (ej - a.ent_lo)] = a.sgn_scale * sc;
                }
            }
            continue;
        }
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            const bool valid = (et + te * 4 + y) < e_end;
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const float sc = (y & 1) ? acc[x][y >> 1].y : acc[x][y >> 1].x;
                const int q = quantise(a.sgn_scale * sc);
                cgt[x] += (valid && qp[x] < q) ? 1 : 0;
                ceq[x] += (valid && qp[x] == q) ? 1 : 0;
            }
        }
    }
    if constexpr (STORE) return;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        int g = cgt[x], e = ceq[x];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) { g += __shfl_xor(g, o, 64); e += __shfl_xor(e, o, 64); }
        const int64_t qi = q0 + tq * 4 + x;
        if (te == 0 && qi < a.n) {
            if (g) atomicAdd(&a.counts[2 * qi + 0], g);
            if (e) atomicAdd(&a.counts[2 * qi + 1], e);
        }
    }
}

// The early-exit PROBE of one rank_counts call of a distance model (kge_rank_early.h): 4 096 sampled pairs, how many are decided at
// half their units.  Round 5: the answer is read back on the HOST (8 bytes, one stream synchronisation of ~15 us against a
// count pass of a millisecond and more) and only the kernel it picks is launched, with the geometry that suits IT.  (Remembering the
// answer per table address was tried and dropped: a model that trains between two evaluations keeps its address, and a stale "no"
// cost the planted TransE tables 10.7 -> 6.3 M ranks/s, profiles/r05f_*; the round trip itself is not what an untrained table's
// evaluation loses against the plain kernel alone -- see bench.py eval_bench on the order of the two measurements.)  Round 4 let
// the device decide: both tile kernels were launched with the early kernel's geometry (runs of >= 4 tiles) and one returned at
// once -- on tables where the exit does not fire the plain kernel then ran in a geometry that costs it 8 - 10 % (C2 shape, TransE
// k = 200: 7.37 vs 8.00 M ranks/s, profiles/r04u_models.jsonl) behind ~70 000 empty workgroups.
int early_probe(int mode, const float* d_ent, const int32_t* d_ent_ids, int64_t ent_lo, int64_t mcand, int64_t n, const RankGeom& g,
                const Workspace& w, float sgn_scale, void* d_screen, size_t screen_bytes, bool* yes, bool* measured, hipStream_t st) {
    *yes = true;
    *measured = false;   // (true: this call ran the probe kernel -- the workspace's probe words hold its counts)
    if (!g_rank_cfg.early.probe) return AMDKGE_OK;   // (tests: the early-exit kernel always)
    EarlyBufs eb = carve_early(d_screen, screen_bytes, n, mcand);
    if (hipError_t e = hipMemsetAsync(eb.b.counter, 0, 256, st)) return set_error_hip(e, "hipMemsetAsync(early probe)");
    ProbeArgs pa{};
    pa.ent = d_ent; pa.Q = w.Q; pa.qpos = w.qpos; pa.ent_ids = d_ent_ids; pa.ent_lo = ent_lo; pa.m = mcand; pa.n = n; pa.g = g; pa.sgn_scale = sgn_scale;
    pa.probe = eb.b.counter + 4;
    switch (mode) {
        case MODE_L1: hipLaunchKernelGGL(rank_early_probe_kernel<MODE_L1>, dim3(16), dim3(256), 0, st, pa); break;
        case MODE_L1_SUB: hipLaunchKernelGGL(rank_early_probe_kernel<MODE_L1_SUB>, dim3(16), dim3(256), 0, st, pa); break;
        case MODE_ROT_S: hipLaunchKernelGGL(rank_early_probe_kernel<MODE_ROT_S>, dim3(16), dim3(256), 0, st, pa); break;
        default: hipLaunchKernelGGL(rank_early_probe_kernel<MODE_ROT_O>, dim3(16), dim3(256), 0, st, pa); break;
    }
    if (int rc = check_launch("rank_early_probe")) return rc;
    int h[2] = {0, 0};
    if (hipError_t e = hipMemcpyAsync(h, eb.b.counter + 4, sizeof(h), hipMemcpyDeviceToHost, st)) return set_error_hip(e, "hipMemcpyAsync(early probe)");
    if (hipError_t e = hipStreamSynchronize(st)) return set_error_hip(e, "hipStreamSynchronize(early probe)");
    *yes = h[0] * 2 >= h[1] && h[1] > 0;   // (early_probe_says_yes)
    *measured = true;
    return AMDKGE_OK;
}

// the early-exit sequence of one rank_counts call of a distance model (kge_rank_early.h): row flags, the EARLY tile kernel (counts
// of the tiles it finishes + the list of the pairs it hands over), the exact recheck of the list, the merge into the caller's
// counts (skipped when the list overflowed: the caller then runs the plain kernel behind the same flag).  `a`: the plain
// kernel's arguments (grid geometry included).  Called when the probe said yes.
int run_early(int mode, const amdkge_model* m, const float* d_ent, const int32_t* d_ent_ids, int64_t ent_lo, int64_t mcand, int64_t n,
              const RankGeom& g, const Workspace& w, CountArgs a, dim3 grid, void* d_screen, size_t screen_bytes, const int** guard_out,
              bool probe_measured, hipStream_t st) {
    int32_t* const caller_counts = a.counts;
    EarlyBufs eb = carve_early(d_screen, screen_bytes, n, mcand);
    // counters [0 .. 3] and everything behind the probe words; words [4], [5] keep what the probe counted in THIS call (decided,
    // sampled: "yes" -- the host read them before this sequence was enqueued; the recheck and merge kernels still look at them), or
    // are set to 1, 1 when no probe ran (a remembered answer, or the probe switched off)
    if (hipError_t e = hipMemsetAsync(eb.b.counter, 0, 16, st)) return set_error_hip(e, "hipMemsetAsync(early counters)");
    if (hipError_t e = hipMemsetAsync(eb.b.counter + 8, 0, (size_t)early_layout(n, mcand).qbad - 32, st)) return set_error_hip(e, "hipMemsetAsync(early counts)");
    if (!probe_measured)
        if (hipError_t e = hipMemsetD32Async((hipDeviceptr_t)(eb.b.counter + 4), 1, 2, st)) return set_error_hip(e, "hipMemsetD32Async(probe)");
    // rows that must not be decided early: the query vectors (every plane) and the candidate rows (stored width)
    hipLaunchKernelGGL(rank_rowflags_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, w.Q, (int64_t)g.QW, (const int32_t*)nullptr, (int64_t)0, n, g.QW, eb.qbad);
    if (int rc = check_launch("rank_rowflags(Q)")) return rc;
    hipLaunchKernelGGL(rank_rowflags_kernel, dim3((unsigned)((mcand + 3) / 4)), dim3(256), 0, st, d_ent, (int64_t)g.K, d_ent_ids, ent_lo, mcand, g.K, eb.ebad);
    if (int rc = check_launch("rank_rowflags(E)")) return rc;
    a.counts = eb.b.counts;
    a.guard = nullptr; a.guard_mode = GUARD_NONE; a.e_probe = eb.b.counter + 4;
    a.e_list = EarlyList{eb.b.counter, eb.b.pairs, eb.b.cap};
    a.e_qbad = eb.qbad; a.e_ebad = eb.ebad;
    a.e_cost = g_rank_cfg.early.cost < 1 ? 1 : g_rank_cfg.early.cost;
    const bool rot = mode == MODE_ROT_O || mode == MODE_ROT_S;
    a.e_check = rot ? g_rank_cfg.early.check_rot : g_rank_cfg.early.check_l1;
    const int nstages = (g.U + KT - 1) / KT;   // short rows: at least three checks per row
    if (a.e_check > nstages / 4) a.e_check = nstages / 4;
    if (a.e_check < 1) a.e_check = 1;
    RecheckDistArgs ra{};
    ra.ent = d_ent; ra.Q = w.Q; ra.qpos = w.qpos; ra.ent_ids = d_ent_ids; ra.ent_lo = ent_lo; ra.g = g; ra.sgn_scale = a.sgn_scale; ra.b = eb.b;
#define KGE_RD(MODE) do { \
        static PerDeviceOnce attr; \
        if (int rc = ensure_dynamic_lds(attr, {(const void*)rank_recheck_dist_kernel<MODE>}, rd_lds_bytes<MODE>(), "rank_recheck_dist")) return rc; \
        hipLaunchKernelGGL(rank_recheck_dist_kernel<MODE>, dim3(1024), dim3(256), rd_lds_bytes<MODE>(), st, ra); } while (0)
    switch (mode) {
        case MODE_L1:
            hipLaunchKernelGGL((rank_count_kernel<MODE_L1, true, false, true>), grid, dim3(256), 0, st, a);
            if (int rc = check_launch("rank_counts_early")) return rc;
            KGE_RD(MODE_L1); break;
        case MODE_L1_SUB:
            hipLaunchKernelGGL((rank_count_kernel<MODE_L1_SUB, true, false, true>), grid, dim3(256), 0, st, a);
            if (int rc = check_launch("rank_counts_early")) return rc;
            KGE_RD(MODE_L1_SUB); break;
        case MODE_ROT_S:
            hipLaunchKernelGGL((rank_rot_kernel<true, false, true>), grid, dim3(256), 0, st, a);
            if (int rc = check_launch("rank_counts_early")) return rc;
            KGE_RD(MODE_ROT_S); break;
        default:
            hipLaunchKernelGGL((rank_rot_kernel<false, false, true>), grid, dim3(256), 0, st, a);
            if (int rc = check_launch("rank_counts_early")) return rc;
            KGE_RD(MODE_ROT_O); break;
    }
#undef KGE_RD
    if (int rc = check_launch("rank_recheck_dist")) return rc;
    hipLaunchKernelGGL(rank_early_merge_kernel, dim3((unsigned)((2 * n + 255) / 256)), dim3(256), 0, st, eb.b, n, caller_counts);
    if (int rc = check_launch("rank_early_merge")) return rc;
    *guard_out = eb.b.counter + 1;
    return AMDKGE_OK;
}

// the plain count kernel of a call: the whole call, or (a.guard set) the fall-back behind the early-exit sequence
int launch_count_tile(int mode, bool v4, bool rot_exact, const CountArgs& a, dim3 grid, hipStream_t st) {
    if (rot_exact) {
        if (!v4) return set_error(AMDKGE_EUNSUPPORTED, "rank_counts: RotatE's exact mode needs the padded stored layout (k_pad = amdkge_padded_k(k)); dense rows with k % 4 != 0 only have the fast mode (amdkge_set_rank_rotate_fast)");
        if (mode == MODE_ROT_S) hipLaunchKernelGGL((rank_rot_kernel<true, false>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((rank_rot_kernel<false, false>), grid, dim3(256), 0, st, a);
        return check_launch("rank_counts_rot");
    }
#define KGE_CNT(MODE) do { if (v4) hipLaunchKernelGGL((rank_count_kernel<MODE, true>), grid, dim3(256), 0, st, a); \
                           else hipLaunchKernelGGL((rank_count_kernel<MODE, false>), grid, dim3(256), 0, st, a); } while (0)
    switch (mode) {
        case MODE_DOT: KGE_CNT(MODE_DOT); break;
        case MODE_L1: KGE_CNT(MODE_L1); break;
        case MODE_L1_SUB: KGE_CNT(MODE_L1_SUB); break;
        case MODE_ROT_O: KGE_CNT(MODE_ROT_O); break;
        default: KGE_CNT(MODE_ROT_S); break;
    }
#undef KGE_CNT
    return check_launch("rank_counts");
}

// ------------------------------------------------------------------------------------------------
// Discovery: the un-quantised corruption scores themselves, for a bounded chunk of queries, through the
// SAME prep + tile kernels (same rounding points and accumulation chain as the ranks).  Callers stream chunks through
// amdkge_topk_rows (kge_discovery.hip), so the reference's (n, m) score matrix never exists for more than a chunk.
// ------------------------------------------------------------------------------------------------
int launch_store(int mode, bool v4, CountArgs& a, int64_t n, int64_t m, hipStream_t st) {
    const int64_t qtiles = (n + QT - 1) / QT, etiles = (m + ET - 1) / ET;
    int64_t tiles_per = (etiles * qtiles + 4095) / 4096;   // ~4096 blocks: enough to fill the chip, few enough to amortise the Q reloads
    if (tiles_per < 1) tiles_per = 1;
    const int64_t splits = (etiles + tiles_per - 1) / tiles_per;
    if (splits > 65535 || qtiles > 0x7FFFFFFFll) return set_error(AMDKGE_EUNSUPPORTED, "scores: too many tiles for one launch; split the queries");
    a.ent_per_block = (int)(tiles_per * ET);
    const dim3 grid((unsigned)qtiles, (unsigned)splits);
    if ((mode == MODE_ROT_O || mode == MODE_ROT_S) && !g_rank_cfg.rotate_fast) {
        if (!v4) return set_error(AMDKGE_EUNSUPPORTED, "scores: RotatE's exact mode needs the padded stored layout (k_pad = amdkge_padded_k(k))");
        if (mode == MODE_ROT_S) hipLaunchKernelGGL((rank_rot_kernel<true, true>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((rank_rot_kernel<false, true>), grid, dim3(256), 0, st, a);
        return check_launch("corruption_scores_rot");
    }
#define KGE_STORE(MODE) do { if (v4) hipLaunchKernelGGL((rank_count_kernel<MODE, true, true>), grid, dim3(256), 0, st, a); \
                             else hipLaunchKernelGGL((rank_count_kernel<MODE, false, true>), grid, dim3(256), 0, st, a); } while (0)
    switch (mode) {
        case MODE_DOT: KGE_STORE(MODE_DOT); break;
        case MODE_L1: KGE_STORE(MODE_L1); break;
        case MODE_L1_SUB: KGE_STORE(MODE_L1_SUB); break;
        case MODE_ROT_O: KGE_STORE(MODE_ROT_O); break;
        default: KGE_STORE(MODE_ROT_S); break;
    }
#undef KGE_STORE
    return check_launch("corruption_scores");
}

}  // namespace kge

using namespace kge;

extern "C" int amdkge_corruption_scores(const amdkge_model* m, const float* d_ent, const float* d_rel, const int32_t* d_triples,
                                        int64_t n, int32_t side, const int32_t* d_ent_ids, int64_t ent_lo, int64_t ent_hi,
                                        float* d_scores, int64_t ld, void* d_work, void* stream) {
    if (int rc = validate_model(m)) return rc;
    if (side != AMDKGE_SIDE_S && side != AMDKGE_SIDE_O) return set_error(AMDKGE_EINVAL, "corruption_scores: side must be AMDKGE_SIDE_S or AMDKGE_SIDE_O");
    if (n < 0 || ent_lo < 0 || ent_hi < ent_lo || ld < ent_hi - ent_lo) return set_error(AMDKGE_EINVAL, "corruption_scores: bad sizes");
    if (!d_ent_ids && ent_hi > m->n_ents) return set_error(AMDKGE_EINVAL, "corruption_scores: entity range outside the table");
    if (n == 0 || ent_hi == ent_lo) return AMDKGE_OK;
    if (!d_ent || !d_rel || !d_triples || !d_scores || !d_work) return set_error(AMDKGE_EINVAL, "corruption_scores: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    const RankGeom g = geom_of(m, side);
    const Workspace w = carve(d_work, m, n);
    if (int rc = run_prep(m, d_ent, d_rel, d_triples, n, side, g, w, st)) return rc;
    const ModelConst mc = model_const(m);
    CountArgs a{};
    a.ent = d_ent; a.Q = w.Q; a.qpos = w.qpos; a.ent_ids = d_ent_ids; a.n = n; a.ent_lo = ent_lo; a.ent_hi = ent_hi; a.g = g;
    a.sgn_scale = mc.score_sign * mc.score_scale; a.scores = d_scores; a.ld = ld;
    const int mode = mode_of(m->scoring_type, side);
    const bool rot_exact = (mode == MODE_ROT_O || mode == MODE_ROT_S) && !g_rank_cfg.rotate_fast;
    const bool v4 = (rot_exact || g.U % 4 == 0) && (g.eplane % 4 == 0) && (g.K % 4 == 0);
    return launch_store(mode, v4, a, n, ent_hi - ent_lo, st);
}
