// evaluate(), contraction models: the exact fp32 MFMA count kernels (the int8 screening pass in front of them: kge_rank_screen.hip).
#include "kge_rank_common.h"

namespace kge {

// ------------------------------------------------------------------------------------------------
// MFMA tile kernel for the contraction models (DistMult / ComplEx / HolE: score = query . entity row).
// v_mfma_f32_32x32x2_f32 is exact fp32 and bit-for-bit a k-ordered fmaf chain (cdna_hip_programming.md,
// "FP32-input MFMA"), i.e. it produces the very bits of rank_op<MODE_DOT> accumulated in unit order: the
// VALU tile kernel (kge_rank_tile.hip), this kernel and the filter kernel stay bitwise interchangeable.
//   workgroup = 4 waves = 128 queries x 128 entities; each wave owns 64 x 64 = 2 x 2 MFMA tiles (64 accumulator
//   registers); K is streamed through LDS 32 units at a time in [unit][row] layout (the lane->operand map of
//   the instruction, A[i = l & 31][k = l >> 5], then reads consecutive LDS words), next stage prefetched into
//   registers while the current one is multiplied; epilogue = quantise -> compare with q(pos) -> packed count.
// ------------------------------------------------------------------------------------------------
#ifndef KGE_MLD
#define KGE_MLD 132
#endif
constexpr int MK = 32, MLD = KGE_MLD;   // (MQ = ME = 128: kge_rank_common.h)
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr size_t MFMA_LDS_BYTES = (size_t)2 * 2 * MK * MLD * sizeof(float) + MQ * sizeof(int);

template <bool V4>
__global__ __launch_bounds__(256, 2) void rank_count_mfma_kernel(CountArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_rank[];
    typedef float (*tile_t)[MK][MLD];
    tile_t Qs = reinterpret_cast<tile_t>(smem_rank);                                     // [2][MK][MLD]
    tile_t Es = reinterpret_cast<tile_t>(smem_rank + (size_t)2 * MK * MLD * sizeof(float));
    int* qps = reinterpret_cast<int*>(smem_rank + (size_t)4 * MK * MLD * sizeof(float));

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wq = (wv >> 1) * 64, we = (wv & 1) * 64;   // this wave's 64 x 64 corner of the 128 x 128 tile
    const int l31 = lane & 31, lh = lane >> 5;
    // XCD-aware work order (speed only, no correctness dependence): workgroup b lands on XCD b % 8 (round-robin
    // dispatch), every XCD has its own 4 MB L2.  XCD c takes a contiguous eighth of the query tiles and walks it
    // in groups of 8 query tiles x all entity splits, so the ~64 workgroups resident on one XCD at a time are
    // 8 query tiles x 8 entity ranges: their Q and E slabs (~3 MB) are shared through that L2 instead of each
    // workgroup streaming its own from the Infinity Cache.
    int bx, by;
    {
        const int xcd = blockIdx.x & 7;
        const int64_t i = blockIdx.x >> 3;
        const int qlo = (int)(((int64_t)a.qtiles * xcd) / 8), qhi = (int)(((int64_t)a.qtiles * (xcd + 1)) / 8);
        const int nq = qhi - qlo;
        if (i >= (int64_t)nq * a.splits) return;
        const int full = nq / 8;
        const int64_t per_group = (int64_t)8 * a.splits;
        if (i < full * per_group) {
            const int64_t r = i % per_group;
            bx = qlo + (int)(i / per_group) * 8 + (int)(r & 7);
            by = (int)(r >> 3);
        } else {
            const int rem = nq - full * 8;
            const int64_t r = i - full * per_group;
            bx = qlo + full * 8 + (int)(r % rem);
            by = (int)(r / rem);
        }
    }
    const int64_t q0 = (int64_t)bx * MQ;
    const int64_t e_begin = a.ent_lo + (int64_t)by * a.ent_per_block;
    const int64_t e_end = min(a.ent_hi, e_begin + a.ent_per_block);
    const int U = a.g.U;
    const int S = (U + MK - 1) / MK;                       // LDS stages per tile
    const int64_t ntile = (e_end - e_begin + ME - 1) / ME;

    if (tid < MQ) { const int64_t qi = q0 + tid; qps[tid] = a.qpos[qi < a.n ? qi : a.n - 1]; }

    // loader: float4 f = tid + 256 * i, i < 4 : row = f >> 3 (128 rows), 4-unit group = f & 7 (8 groups = 32 units)
    const float* qrow[4];
    const float* erow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t lq = q0 + ((tid + 256 * i) >> 3);
        qrow[i] = a.Q + (lq < a.n ? lq : a.n - 1) * (int64_t)a.g.QW + ((tid + 256 * i) & 7) * 4;
    }
    auto set_erow = [&](int64_t et) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t le = et + ((tid + 256 * i) >> 3);
            const int64_t le_c = le < e_end ? le : e_end - 1;
            const int64_t id = a.ent_ids ? (int64_t)a.ent_ids[le_c] : le_c;
            erow[i] = a.ent + id * a.g.K + ((tid + 256 * i) & 7) * 4;
        }
    };
    auto fetch = [&](const float* src, int ku) -> float4 {   // 4 consecutive units starting at ku, zero beyond U
        if (V4) {
            if (ku < U) return *reinterpret_cast<const float4*>(src);
            return make_float4(0.f, 0.f, 0.f, 0.f);
        }
        float4 t;
        t.x = (ku + 0 < U) ? src[0] : 0.f; t.y = (ku + 1 < U) ? src[1] : 0.f;
        t.z = (ku + 2 < U) ? src[2] : 0.f; t.w = (ku + 3 < U) ? src[3] : 0.f;
        return t;
    };
    float4 pq[4], pe[4];
    auto load_stage = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ku = k0 + ((tid + 256 * i) & 7) * 4;
            pq[i] = fetch(qrow[i] + k0, ku);
            pe[i] = fetch(erow[i] + k0, ku);
        }
    };
    auto store_stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = tid + 256 * i, row = f >> 3, kg = (f & 7) * 4;
            Qs[buf][kg + 0][row] = pq[i].x; Qs[buf][kg + 1][row] = pq[i].y; Qs[buf][kg + 2][row] = pq[i].z; Qs[buf][kg + 3][row] = pq[i].w;
            Es[buf][kg + 0][row] = pe[i].x; Es[buf][kg + 1][row] = pe[i].y; Es[buf][kg + 2][row] = pe[i].z; Es[buf][kg + 3][row] = pe[i].w;
        }
    };

    int cnt[2][16];   // per (query tile mi, accumulator register): gt | eq << 16 over this lane's entity columns
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) cnt[mi][r] = 0;

    // The (tile, stage) sequence is one software pipeline: while stage s is multiplied out of LDS buffer `buf`,
    // the global loads of the next stage (possibly the first stage of the NEXT entity tile) are in flight and are
    // written to the other buffer afterwards: one workgroup barrier per stage.
    set_erow(e_begin);
    load_stage(0);
    store_stage(0);
    __syncthreads();
    int buf = 0;
    for (int64_t t = 0; t < ntile; ++t) {
        const int64_t et = e_begin + t * ME;
        f32x16 acc[2][2];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
        for (int st = 0; st < S; ++st) {
            const bool last_stage = (st == S - 1);
            const bool has_next = !(last_stage && t == ntile - 1);
            if (has_next) {
                if (last_stage) set_erow(et + ME);
                load_stage(last_stage ? 0 : (st + 1) * MK);
            }
            // operands of unit pair kk + 2 are read from LDS before the four MFMAs of pair kk are issued, so the
            // LDS latency hides behind 256 cycles of matrix-pipe work even for a lone wave on the SIMD
            float opa[2][2], opb[2][2];
            opa[0][0] = Qs[buf][lh][wq + l31]; opa[0][1] = Qs[buf][lh][wq + 32 + l31];
            opb[0][0] = Es[buf][lh][we + l31]; opb[0][1] = Es[buf][lh][we + 32 + l31];
#pragma unroll
            for (int kk = 0; kk < MK; kk += 2) {
                const int cur = (kk >> 1) & 1, nxt = cur ^ 1;
                if (kk + 2 < MK) {
                    opa[nxt][0] = Qs[buf][kk + 2 + lh][wq + l31]; opa[nxt][1] = Qs[buf][kk + 2 + lh][wq + 32 + l31];
                    opb[nxt][0] = Es[buf][kk + 2 + lh][we + l31]; opb[nxt][1] = Es[buf][kk + 2 + lh][we + 32 + l31];
                }
                __builtin_amdgcn_sched_barrier(0);   // keep the reads above the MFMAs (the scheduler sinks them otherwise)
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(opa[cur][0], opb[cur][0], acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(opa[cur][0], opb[cur][1], acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(opa[cur][1], opb[cur][0], acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(opa[cur][1], opb[cur][1], acc[1][1], 0, 0, 0);
            }
            if (has_next) store_stage(buf ^ 1);
            __syncthreads();
            buf ^= 1;
        }
        // ---- epilogue: C/D map col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) ----
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const bool valid = (et + we + ni * 32 + l31) < e_end;
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int qp = qps[wq + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh];
                    const int q = quantise(a.sgn_scale * acc[mi][ni][r]);
                    cnt[mi][r] += (valid && qp < q) ? 1 : 0;
                    cnt[mi][r] += (valid && qp == q) ? 0x10000 : 0;
                }
        }
    }
    // ---- per query row: sum over the 32 lanes that share it, one atomic pair per row per wave ----
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            int g = cnt[mi][r] & 0xFFFF, e = cnt[mi][r] >> 16;
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) { g += __shfl_xor(g, o, 64); e += __shfl_xor(e, o, 64); }
            const int64_t qi = q0 + wq + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (l31 == 0 && qi < a.n) {
                if (g) atomicAdd(&a.counts[2 * qi + 0], g);
                if (e) atomicAdd(&a.counts[2 * qi + 1], e);
            }
        }
}

// ------------------------------------------------------------------------------------------------
// The same tile computation as rank_count_mfma_kernel<true>, organised as ONE instruction stream per stage in which every
// non-matrix instruction sits between two MFMAs.  A wave issues in order, so whatever is placed after the four MFMAs of a
// unit pair only starts when the last of them has been issued; in the kernel above the global prefetch (with its bounds
// branches), the 32 transposing ds_write_b32 and the barrier therefore run with the matrix pipe idle (MfmaUtil 0.70).  Here:
//   * loads are two stages ahead (two register sets): stage g issues the global loads of stage g + 2 during its first four
//     unit pairs and writes the set loaded during stage g - 1 to the other LDS buffer during its last eight pairs, one or
//     two instructions behind each MFMA; a stage of matrix work (>= 4 096 cycles) covers the load latency;
//   * no branches inside a stage: out-of-range units read the row start and are zeroed by a select, the load cursor runs
//     past the last stage onto clamped addresses instead of being guarded;
//   * operands of pair kk + 2 are read behind the first two MFMAs of pair kk.
// Same MFMA order per accumulator => the same bits as the kernel above and as rank_op<MODE_DOT>.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void rank_count_mfma_pipe_kernel(CountArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_rank[];
    typedef float (*tile_t)[MK][MLD];
    tile_t Qs = reinterpret_cast<tile_t>(smem_rank);                                     // [2][MK][MLD]
    tile_t Es = reinterpret_cast<tile_t>(smem_rank + (size_t)2 * MK * MLD * sizeof(float));
    int* qps = reinterpret_cast<int*>(smem_rank + (size_t)4 * MK * MLD * sizeof(float));

    if (a.guard && *a.guard == 0) return;   // (screened call that did not overflow its recheck list: nothing to do)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wq = (wv >> 1) * 64, we = (wv & 1) * 64;
    const int l31 = lane & 31, lh = lane >> 5;
    int bx, by;   // XCD-aware work order, see rank_count_mfma_kernel
    {
        const int xcd = blockIdx.x & 7;
        const int64_t i = blockIdx.x >> 3;
        const int qlo = (int)(((int64_t)a.qtiles * xcd) / 8), qhi = (int)(((int64_t)a.qtiles * (xcd + 1)) / 8);
        const int nq = qhi - qlo;
        if (i >= (int64_t)nq * a.splits) return;
        const int full = nq / 8;
        const int64_t per_group = (int64_t)8 * a.splits;
        if (i < full * per_group) {
            const int64_t r = i % per_group;
            bx = qlo + (int)(i / per_group) * 8 + (int)(r & 7);
            by = (int)(r >> 3);
        } else {
            const int rem = nq - full * 8;
            const int64_t r = i - full * per_group;
            bx = qlo + full * 8 + (int)(r % rem);
            by = (int)(r / rem);
        }
    }
    const int64_t q0 = (int64_t)bx * MQ;
    const int64_t e_begin = a.ent_lo + (int64_t)by * a.ent_per_block;
    const int64_t e_end = min(a.ent_hi, e_begin + a.ent_per_block);
    const int U = a.g.U;
    const int S = (U + MK - 1) / MK;
    const int64_t ntile = (e_end - e_begin + ME - 1) / ME;
    const int64_t G = ntile * S;

    if (tid < MQ) { const int64_t qi = q0 + tid; qps[tid] = a.qpos[qi < a.n ? qi : a.n - 1]; }

    // loader: float4 f = tid + 256 * i, i < 4 : row = f >> 3 (128 rows), 4-unit group kg = (f & 7) * 4 (32 units)
    const int kg = (tid & 7) * 4, lrow = tid >> 3;   // (tid + 256 i) & 7 == tid & 7 ; row = lrow + 32 i
    const float* qbase[4];
    const float* ebase[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t lq = q0 + lrow + 32 * i;
        qbase[i] = a.Q + (lq < a.n ? lq : a.n - 1) * (int64_t)a.g.QW;
    }
    auto set_erow = [&](int64_t et) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t le = et + lrow + 32 * i;
            const int64_t le_c = le < e_end ? le : e_end - 1;
            const int64_t id = a.ent_ids ? (int64_t)a.ent_ids[le_c] : le_c;
            ebase[i] = a.ent + id * a.g.K;
        }
    };
    int ld_k0 = 0;          // load cursor: unit offset of the stage the next loads belong to ...
    int64_t ld_tile = 0;    // ... and its entity tile (clamped to the last one once the cursor runs past the end)
    // raw load of 4 units; units beyond U read the row start instead and are zeroed when the registers go to LDS (a select
    // right here would make the wave wait for the load it has just issued)
    auto fetch = [&](const float* base, int k0) -> float4 {
        const int ku = k0 + kg;
        return *reinterpret_cast<const float4*>(base + (ku < U ? ku : 0));
    };
    auto advance = [&]() {
        ld_k0 += MK;
        if (ld_k0 >= S * MK) {
            ld_k0 = 0;
            ld_tile = (ld_tile + 1 < ntile) ? ld_tile + 1 : ntile - 1;
            set_erow(e_begin + ld_tile * ME);
        }
    };
    float4 pq[2][4], pe[2][4];

    int cnt[2][16];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) cnt[mi][r] = 0;
    f32x16 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    // prologue: stage 0 -> LDS buffer 0, stage 1 -> register set 1
    set_erow(e_begin);
#pragma unroll
    for (int i = 0; i < 4; ++i) { pq[0][i] = fetch(qbase[i], 0); pe[0][i] = fetch(ebase[i], 0); }
    advance();
#pragma unroll
    for (int i = 0; i < 4; ++i) { pq[1][i] = fetch(qbase[i], ld_k0); pe[1][i] = fetch(ebase[i], ld_k0); }
    advance();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = lrow + 32 * i;
        const float z = (kg < U) ? 1.f : 0.f;   // U % 4 == 0: a 4-unit group is inside or outside as a whole
        Qs[0][kg + 0][row] = z * pq[0][i].x; Qs[0][kg + 1][row] = z * pq[0][i].y; Qs[0][kg + 2][row] = z * pq[0][i].z; Qs[0][kg + 3][row] = z * pq[0][i].w;
        Es[0][kg + 0][row] = z * pe[0][i].x; Es[0][kg + 1][row] = z * pe[0][i].y; Es[0][kg + 2][row] = z * pe[0][i].z; Es[0][kg + 3][row] = z * pe[0][i].w;
    }
    __syncthreads();

    int st = 0;
    int64_t t = 0;
    auto stage = [&](auto set_c) {
        constexpr int SET = decltype(set_c)::value;   // LDS buffer of this stage == register set that is free for new loads
        constexpr int OTH = SET ^ 1;                  // register set holding the next stage's data == LDS buffer it goes to
        const bool okn = ((st + 1 == S) ? 0 : (st + 1) * MK) + kg < U;   // is this lane's unit group of the NEXT stage inside the row?
        float opa[2][2], opb[2][2];
        opa[0][0] = Qs[SET][lh][wq + l31]; opa[0][1] = Qs[SET][lh][wq + 32 + l31];
        opb[0][0] = Es[SET][lh][we + l31]; opb[0][1] = Es[SET][lh][we + 32 + l31];
        __builtin_amdgcn_sched_barrier(0);
        // unit pairs 0..7: the four MFMAs of a pair, each followed by its share of the stage's other work
#pragma unroll
        for (int it = 0; it < MK / 4; ++it) {
            const int kk = 2 * it, cur = it & 1, nxt = cur ^ 1;
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(opa[cur][0], opb[cur][0], acc[0][0], 0, 0, 0);
            opa[nxt][0] = Qs[SET][kk + 2 + lh][wq + l31]; opb[nxt][0] = Es[SET][kk + 2 + lh][we + l31];
            __builtin_amdgcn_sched_barrier(0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(opa[cur][0], opb[cur][1], acc[0][1], 0, 0, 0);
            opa[nxt][1] = Qs[SET][kk + 2 + lh][wq + 32 + l31]; opb[nxt][1] = Es[SET][kk + 2 + lh][we + 32 + l31];
            __builtin_amdgcn_sched_barrier(0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(opa[cur][1], opb[cur][0], acc[1][0], 0, 0, 0);
            if (it < 4) {
                pq[SET][it] = fetch(qbase[it], ld_k0);
            } else {
                const int i = it - 4, row = lrow + 32 * i;
                Qs[OTH][kg + 0][row] = okn ? pq[OTH][i].x : 0.f; Qs[OTH][kg + 1][row] = okn ? pq[OTH][i].y : 0.f;
                Qs[OTH][kg + 2][row] = okn ? pq[OTH][i].z : 0.f; Qs[OTH][kg + 3][row] = okn ? pq[OTH][i].w : 0.f;
            }
            __builtin_amdgcn_sched_barrier(0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(opa[cur][1], opb[cur][1], acc[1][1], 0, 0, 0);
            if (it < 4) {
                pe[SET][it] = fetch(ebase[it], ld_k0);
            } else {
                const int i = it - 4, row = lrow + 32 * i;
                Es[OTH][kg + 0][row] = okn ? pe[OTH][i].x : 0.f; Es[OTH][kg + 1][row] = okn ? pe[OTH][i].y : 0.f;
                Es[OTH][kg + 2][row] = okn ? pe[OTH][i].z : 0.f; Es[OTH][kg + 3][row] = okn ? pe[OTH][i].w : 0.f;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // unit pairs 8..15: nothing but matrix work and operand reads -- skipped as a whole when the stage holds <= 16 real
        // units (the zero-padded half of a row's last stage: U = 400 -> 16 of 32 units; acc + 0 * 0 == acc)
        if (U - st * MK > MK / 2) {
#pragma unroll
            for (int it = MK / 4; it < MK / 2; ++it) {
                const int kk = 2 * it, cur = it & 1, nxt = cur ^ 1;
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(opa[cur][0], opb[cur][0], acc[0][0], 0, 0, 0);
                if (kk + 2 < MK) { opa[nxt][0] = Qs[SET][kk + 2 + lh][wq + l31]; opb[nxt][0] = Es[SET][kk + 2 + lh][we + l31]; }
                __builtin_amdgcn_sched_barrier(0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(opa[cur][0], opb[cur][1], acc[0][1], 0, 0, 0);
                if (kk + 2 < MK) { opa[nxt][1] = Qs[SET][kk + 2 + lh][wq + 32 + l31]; opb[nxt][1] = Es[SET][kk + 2 + lh][we + 32 + l31]; }
                __builtin_amdgcn_sched_barrier(0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(opa[cur][1], opb[cur][0], acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(opa[cur][1], opb[cur][1], acc[1][1], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        advance();
        __syncthreads();
        if (++st == S) {   // ---- tile epilogue: C/D map col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) ----
            const int64_t et = e_begin + t * ME;
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const bool valid = (et + we + ni * 32 + l31) < e_end;
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int qp = qps[wq + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh];
                        const int q = quantise(a.sgn_scale * acc[mi][ni][r]);
                        cnt[mi][r] += (valid && qp < q) ? 1 : 0;
                        cnt[mi][r] += (valid && qp == q) ? 0x10000 : 0;
                        acc[mi][ni][r] = 0.f;
                    }
            }
            st = 0;
            ++t;
        }
    };
    for (int64_t g = 0; g < G; g += 2) {
        stage(std::integral_constant<int, 0>{});
        if (g + 1 < G) stage(std::integral_constant<int, 1>{});
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            int g = cnt[mi][r] & 0xFFFF, e = cnt[mi][r] >> 16;
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) { g += __shfl_xor(g, o, 64); e += __shfl_xor(e, o, 64); }
            const int64_t qi = q0 + wq + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (l31 == 0 && qi < a.n) {
                if (g) atomicAdd(&a.counts[2 * qi + 0], g);
                if (e) atomicAdd(&a.counts[2 * qi + 1], e);
            }
        }
}

int launch_count_mfma(bool v4, bool pipe, const CountArgs& a, unsigned nblk, hipStream_t st) {
    static PerDeviceOnce attr_done;
    if (int rc = ensure_dynamic_lds(attr_done, {(const void*)rank_count_mfma_kernel<true>, (const void*)rank_count_mfma_kernel<false>, (const void*)rank_count_mfma_pipe_kernel},
                                    MFMA_LDS_BYTES, "rank_count_mfma")) return rc;
    const dim3 grid1(nblk);
    if (v4 && pipe) hipLaunchKernelGGL(rank_count_mfma_pipe_kernel, grid1, dim3(256), MFMA_LDS_BYTES, st, a);
    else if (v4) hipLaunchKernelGGL((rank_count_mfma_kernel<true>), grid1, dim3(256), MFMA_LDS_BYTES, st, a);
    else hipLaunchKernelGGL((rank_count_mfma_kernel<false>), grid1, dim3(256), MFMA_LDS_BYTES, st, a);
    return check_launch("rank_counts_mfma");
}

}  // namespace kge
