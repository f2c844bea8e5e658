// evaluate(): the filter pass.
//   (the range lookup in front of it -- per test triple, the run of its known positives in the sorted filter index -- is
//   amdkge_filter_ranges, kge_filter.hip, beside the index build it reads)
//   rank_filter   : per triple, recomputes the few true-positive corruptions with the SAME k-ordered accumulation chain (rank_op /
//                   rot_exact_op, kge_rank_common.h: bitwise the scores the tile kernels produced) and counts those that outrank the
//                   positive (always "<=", AbstractScoringLayer.py:292-303).  Contraction models: the pairs go as a flat list through
//                   rank_recheck_kernel<true> (launch_recheck_filter, kge_rank_screen.hip); the one-wave-per-query kernel is its fall-back.
#include "kge_rank_common.h"

namespace kge {

// Filter pass, contraction models: the (query, known positive) pairs as a flat list for rank_recheck_kernel<true> -- 64 pairs
// per wave with coalesced row fetches, instead of one wave per query whose lanes each walk a whole row 16 bytes at a time
// (at C2 a query has 1.1 known positives on average: 63 idle lanes, 100 dependent load steps: 150 us).  A block takes 256
// queries, scans their list lengths, reserves its run of the list with ONE atomic and writes it cooperatively (pair j of the
// block: its query by binary search in the scanned offsets), so a query with thousands of known positives is no slower than
// thousands of queries with one.  An id outside the candidate set is listed as (query, -1).
__global__ __launch_bounds__(256) void filter_pairs_kernel(FilterArgs a, int2* __restrict__ pairs, int* __restrict__ counter, int64_t cap) {
    __shared__ long long off_s[257];
    __shared__ long long lo_s[256];
    __shared__ long long base_s;
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * 256 + tid;
    long long lo = 0, c = 0;
    if (i < a.n) { lo = a.flt_lo[i]; c = a.flt_hi[i] - lo; if (c < 0) c = 0; }
    lo_s[tid] = lo;
    off_s[tid + 1] = c;
    if (tid == 0) off_s[0] = 0;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {   // inclusive scan of the 256 lengths (off_s[1..256])
        const long long v = (tid >= o) ? off_s[tid + 1 - o] : 0;
        __syncthreads();
        off_s[tid + 1] += v;
        __syncthreads();
    }
    const long long total = off_s[256];
    if (tid == 0) {
        long long b = -1;
        if (total > 0 && total <= cap) b = (long long)atomicAdd(counter, (int)total);
        if (total > cap || (b >= 0 && b + total > cap)) { counter[1] = 1; b = -1; }
        base_s = b;
    }
    __syncthreads();
    const long long base = base_s;
    if (base < 0) return;
    for (long long j = tid; j < total; j += 256) {
        int x = 0, y = 256;   // the query q with off_s[q] <= j < off_s[q + 1]
        while (y - x > 1) { const int mid = (x + y) >> 1; if (off_s[mid] <= j) x = mid; else y = mid; }
        const int64_t q = (int64_t)blockIdx.x * 256 + x;
        int64_t id = (int64_t)a.flt_ids[lo_s[x] + (j - off_s[x])];
        bool ok;
        if (a.subset_pos) {   // mapping_dict.lookup + drop -1 (AbstractScoringLayer.py:266-275)
            const int pos = a.subset_pos[id];
            ok = pos >= 0 && pos >= a.ent_lo && pos < a.ent_hi;
        } else {
            ok = id >= a.ent_lo && id < a.ent_hi;   // partition rule :280-288
        }
        pairs[base + j] = make_int2((int)q, ok ? (int)id : -1);
    }
}

template <int MODE, bool V4, bool EXACT_ROT = false>
__global__ __launch_bounds__(256) void rank_filter_kernel(FilterArgs a) {
    constexpr int NQF = ModeTraits<MODE>::NQF, NEF = ModeTraits<MODE>::NEF;
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= a.n) return;
    if (a.guard && *a.guard == 0) return;
    const int64_t lo = a.flt_lo[i], hi = a.flt_hi[i];
    const float* qrow = a.Q + i * (int64_t)a.g.QW;
    const int qp = a.qpos[i];
    int cnt = 0;
    for (int64_t f0 = lo; f0 < hi; f0 += KGE_WAVE) {
        const int64_t f = f0 + lane;
        bool ok = f < hi;
        int64_t id = ok ? (int64_t)a.flt_ids[f] : 0;
        if (ok && a.subset_pos) {   // mapping_dict.lookup + drop -1 (AbstractScoringLayer.py:266-275)
            const int pos = a.subset_pos[id];
            ok = pos >= 0;
            // the corruption row of position `pos` is the table row `id` itself
            if (ok) ok = (pos >= a.ent_lo) && (pos < a.ent_hi);
        } else if (ok) {
            ok = (id >= a.ent_lo) && (id < a.ent_hi);   // partition rule :280-288
        }
        const float* erow = a.ent + (ok ? id : 0) * a.g.K;
        float acc = 0.f;
        if constexpr (EXACT_ROT) {   // live units only (a.g.U = k), float4 loads inside the stored (padded) row
            for (int u0 = 0; u0 < a.g.U; u0 += 4) {
                float qv[NQF][4], ev[NEF][4];
#pragma unroll
                for (int p = 0; p < NQF; ++p) {
                    const float4 t = *reinterpret_cast<const float4*>(qrow + p * a.g.qplane + u0);
                    qv[p][0] = t.x; qv[p][1] = t.y; qv[p][2] = t.z; qv[p][3] = t.w;
                }
#pragma unroll
                for (int p = 0; p < NEF; ++p) {
                    const float4 t = *reinterpret_cast<const float4*>(erow + p * a.g.eplane + u0);
                    ev[p][0] = t.x; ev[p][1] = t.y; ev[p][2] = t.z; ev[p][3] = t.w;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (u0 + u >= a.g.U) break;
                    float qq[NQF], ee[NEF];
#pragma unroll
                    for (int p = 0; p < NQF; ++p) qq[p] = qv[p][u];
#pragma unroll
                    for (int p = 0; p < NEF; ++p) ee[p] = ev[p][u];
                    acc = rot_exact_op<MODE>(acc, qq, ee);
                }
            }
        } else if (V4) {
            for (int u0 = 0; u0 < a.g.U; u0 += 4) {
                float qv[NQF][4], ev[NEF][4];
#pragma unroll
                for (int p = 0; p < NQF; ++p) {
                    const float4 t = *reinterpret_cast<const float4*>(qrow + p * a.g.qplane + u0);
                    qv[p][0] = t.x; qv[p][1] = t.y; qv[p][2] = t.z; qv[p][3] = t.w;
                }
#pragma unroll
                for (int p = 0; p < NEF; ++p) {
                    const float4 t = *reinterpret_cast<const float4*>(erow + p * a.g.eplane + u0);
                    ev[p][0] = t.x; ev[p][1] = t.y; ev[p][2] = t.z; ev[p][3] = t.w;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    float qq[NQF], ee[NEF];
#pragma unroll
                    for (int p = 0; p < NQF; ++p) qq[p] = qv[p][u];
#pragma unroll
                    for (int p = 0; p < NEF; ++p) ee[p] = ev[p][u];
                    acc = rank_op<MODE>(acc, qq, ee, a.g.sgn);
                }
            }
        } else {
            for (int u = 0; u < a.g.U; ++u) {
                float qq[NQF], ee[NEF];
#pragma unroll
                for (int p = 0; p < NQF; ++p) qq[p] = qrow[p * a.g.qplane + u];
#pragma unroll
                for (int p = 0; p < NEF; ++p) ee[p] = erow[p * a.g.eplane + u];
                acc = rank_op<MODE>(acc, qq, ee, a.g.sgn);
            }
        }
        const int q = quantise(a.sgn_scale * acc);
        cnt += (ok && qp <= q) ? 1 : 0;
    }
    cnt = wave_sum_i(cnt);
    if (lane == 0 && cnt) atomicAdd(&a.sub[i], cnt);
}

}  // namespace kge

using namespace kge;

extern "C" int amdkge_rank_filter(const amdkge_model* m, const float* d_ent, const float* d_rel, const int32_t* d_triples,
                                  int64_t n, int32_t side, const int64_t* d_flt_lo, const int64_t* d_flt_hi,
                                  const int32_t* d_flt_ids, const int32_t* d_subset_pos, int64_t ent_lo, int64_t ent_hi,
                                  int32_t* d_sub, void* d_work, void* stream) {
    if (int rc = validate_model(m)) return rc;
    if (side != AMDKGE_SIDE_S && side != AMDKGE_SIDE_O) return set_error(AMDKGE_EINVAL, "rank_filter: side must be AMDKGE_SIDE_S or AMDKGE_SIDE_O");
    if (n < 0 || ent_lo < 0 || ent_hi < ent_lo) return set_error(AMDKGE_EINVAL, "rank_filter: bad sizes");
    if (n == 0) return AMDKGE_OK;
    if (!d_ent || !d_rel || !d_triples || !d_flt_lo || !d_flt_hi || !d_sub || !d_work) return set_error(AMDKGE_EINVAL, "rank_filter: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    const RankGeom g = geom_of(m, side);
    const Workspace w = carve(d_work, m, n);
    if (int rc = run_prep(m, d_ent, d_rel, d_triples, n, side, g, w, st)) return rc;
    const ModelConst mc = model_const(m);
    FilterArgs a{};
    a.ent = d_ent; a.Q = w.Q; a.qpos = w.qpos; a.flt_lo = d_flt_lo; a.flt_hi = d_flt_hi; a.flt_ids = d_flt_ids;
    a.subset_pos = d_subset_pos; a.sub = d_sub; a.n = n; a.ent_lo = ent_lo; a.ent_hi = ent_hi; a.g = g;
    a.sgn_scale = mc.score_sign * mc.score_scale;
    const unsigned grid = (unsigned)((n + 3) / 4);
    const int mode = mode_of(m->scoring_type, side);
    const bool rot_exact = (mode == MODE_ROT_O || mode == MODE_ROT_S) && !g_rank_cfg.rotate_fast;
    const bool v4 = (rot_exact || g.U % 4 == 0) && (g.eplane % 4 == 0) && (g.K % 4 == 0);
    if (rot_exact) {
        if (!v4) return set_error(AMDKGE_EUNSUPPORTED, "rank_filter: RotatE's exact mode needs the padded stored layout (k_pad = amdkge_padded_k(k))");
        if (mode == MODE_ROT_S) hipLaunchKernelGGL((rank_filter_kernel<MODE_ROT_S, true, true>), dim3(grid), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((rank_filter_kernel<MODE_ROT_O, true, true>), dim3(grid), dim3(256), 0, st, a);
        return check_launch("rank_filter_rot");
    }
    if (mode == MODE_DOT && v4 && g_rank_cfg.kernel == 0) {   // (a forced count kernel, amdkge_set_rank_kernel, also keeps round 2's filter pass)
        // contraction models: flat pair list + the coalesced exact-chain kernel; the one-wave-per-query kernel behind it runs
        // only if the list overflowed (device-side flag, no host round trip)
        if (hipError_t e = hipMemsetAsync(w.flt_counter, 0, 8, st)) return set_error_hip(e, "hipMemsetAsync(filter pair counter)");
        hipLaunchKernelGGL(filter_pairs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, w.flt_pairs, w.flt_counter, w.flt_cap);
        if (int rc = check_launch("filter_pairs")) return rc;
        RecheckArgs ra{};
        ra.ent = d_ent; ra.Q = w.Q; ra.qpos = w.qpos; ra.ent_ids = nullptr; ra.ent_lo = 0; ra.U = g.U; ra.K = g.K; ra.QW = g.QW;
        ra.sgn_scale = a.sgn_scale;
        ra.b.counter = w.flt_counter; ra.b.pairs = w.flt_pairs; ra.b.cap = w.flt_cap; ra.b.counts = d_sub;
        const int64_t groups = (w.flt_cap + 63) / 64;
        if (int rc = launch_recheck_filter(ra, (unsigned)(groups / 4 < 1024 ? (groups + 3) / 4 : 1024), st)) return rc;
        a.guard = w.flt_counter + 1;
    }
#define KGE_FLT(MODE) do { if (v4) hipLaunchKernelGGL((rank_filter_kernel<MODE, true>), dim3(grid), dim3(256), 0, st, a); \
                           else hipLaunchKernelGGL((rank_filter_kernel<MODE, false>), dim3(grid), dim3(256), 0, st, a); } while (0)
    switch (mode) {
        case MODE_DOT: KGE_FLT(MODE_DOT); break;
        case MODE_L1: KGE_FLT(MODE_L1); break;
        case MODE_L1_SUB: KGE_FLT(MODE_L1_SUB); break;
        case MODE_ROT_O: KGE_FLT(MODE_ROT_O); break;
        default: KGE_FLT(MODE_ROT_S); break;
    }
#undef KGE_FLT
    return check_launch("rank_filter");
}
