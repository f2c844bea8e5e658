// discover_facts(strategy="exhaustive") on the device: the selection behind the 1-vs-all score blocks of amdkge_corruption_scores.
// A candidate (s, r, o) ranks <= R on a side exactly when its quantised positive score exceeds T, the R-th largest quantised score
// among the corruptions evaluate() counts for its query row (every entity but the row's filter ids; the reflexive column and the
// candidate's own column are counted).  amdkge_discover_select computes T per row and emits every column that could hold such a
// candidate: not a filter id, not the row's own entity, quantised score >= T - margin_q (margin_q bounds the distance between the
// prep kernel's and the tile chain's value of one pair: DESIGN.md section 3).  The caller intersects the two sides' lists and ranks the
// survivors exactly, so the emitted set only has to be a superset.
#include "kge_rank_common.h"
#include "kge_topk.h"

namespace kge {

constexpr int64_t SELECT_BITMAP_MAX_BYTES = 128 * 1024;   // beside the 16 KB selection buffer inside the 160 KB LDS of a CU

__device__ __forceinline__ bool select_non_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) == 0x7F800000u; }

// is column c one of the row's filter ids?  LDS bitmap of the columns, or a binary search in the ascending id list
__device__ __forceinline__ bool select_masked(const uint32_t* bitmap, bool use_bitmap, const int32_t* __restrict__ ids, int64_t lo, int64_t hi, int64_t c) {
    if (use_bitmap) return (bitmap[c >> 5] >> (c & 31)) & 1u;
    return sorted_contains(ids, lo, hi, c);
}

// One workgroup per query row.  Sweep one: streaming top-R of the quantised keys of the counted columns (TopkStream, kge_topk.h;
// key = quantised score << 32 | ~column, so the R-th key holds the R-th largest value WITH multiplicity).
// Sweep two: emission, one vector atomic per wave (ballot + popcount); the row was just read, so this pass is served by the caches.
__global__ __launch_bounds__(256) void discover_select_kernel(const float* __restrict__ scores, int64_t m, int64_t ld, const int32_t* __restrict__ queries,
                                                              int own_col, const int64_t* __restrict__ flt_lo, const int64_t* __restrict__ flt_hi,
                                                              const int32_t* __restrict__ flt_ids, int R, int margin_q, int32_t* __restrict__ thr,
                                                              int thr_given, int use_bitmap, int64_t row_base, int32_t* __restrict__ pairs, int64_t cap,
                                                              unsigned long long* __restrict__ count) {
    __shared__ unsigned long long buf[TOPK_BUF];
    __shared__ int n_stage;
    __shared__ int any_bad;
    extern __shared__ uint32_t bitmap[];
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const float* row = scores + r * ld;
    const int64_t lo = flt_lo ? flt_lo[r] : 0, hi = flt_lo ? flt_hi[r] : 0;
    const int64_t own = queries[3 * r + own_col];
    if (use_bitmap) {
        const int64_t words = (m + 31) >> 5;
        for (int64_t i = tid; i < words; i += 256) bitmap[i] = 0u;
        __syncthreads();
        for (int64_t f = lo + tid; f < hi; f += 256) {
            const int64_t id = flt_ids[f];
            if (id >= 0 && id < m) atomicOr(&bitmap[id >> 5], 1u << (id & 31));
        }
    }
    int T;
    if (thr_given) {
        T = thr[r];
        __syncthreads();
    } else {
        if (tid == 0) any_bad = 0;
        TopkStream sel{buf, &n_stage};
        sel.reset(tid);
        bool bad = false;
        for (int64_t c0 = 0; c0 < m; c0 += 256) {
            const int64_t c = c0 + tid;
            if (c < m) {
                const float v = row[c];
                bad |= select_non_finite(v);
                if (!select_masked(bitmap, use_bitmap, flt_ids, lo, hi, c)) sel.offer(topk_key((uint32_t)quantise(v) ^ 0x80000000u, c));
            }
            sel.end_of_block(R, c0 + 256 >= m);
        }
        if (bad) any_bad = 1;
        __syncthreads();
        const unsigned long long key = buf[R - 1];
        // fewer than R counted columns: T = -inf; a row with a non-finite score is emitted whole (the exact pass decides it)
        T = (key == 0ull || any_bad) ? INT32_MIN : (int)((uint32_t)(key >> 32) ^ 0x80000000u);
        if (tid == 0) thr[r] = T;
    }
    const long long floor_q = (long long)T - (long long)margin_q;
    const int lane = tid & 63;
    for (int64_t c0 = 0; c0 < m; c0 += 256) {
        const int64_t c = c0 + tid;
        bool pass = false;
        if (c < m && c != own && !select_masked(bitmap, use_bitmap, flt_ids, lo, hi, c)) pass = (long long)quantise(row[c]) >= floor_q;
        const unsigned long long bal = __ballot(pass);
        if (bal) {
            unsigned long long base = 0ull;
            if (lane == 0) base = atomicAdd(count, (unsigned long long)__popcll(bal));
            const uint32_t b_lo = __builtin_amdgcn_readfirstlane((uint32_t)base), b_hi = __builtin_amdgcn_readfirstlane((uint32_t)(base >> 32));
            const unsigned long long pos = (((unsigned long long)b_hi << 32) | b_lo) + (unsigned long long)__popcll(bal & ((1ull << lane) - 1ull));
            if (pass && (int64_t)pos < cap) {
                pairs[2 * pos] = (int32_t)(row_base + r);
                pairs[2 * pos + 1] = (int32_t)c;
            }
        }
    }
}

}  // namespace kge

using namespace kge;

extern "C" int amdkge_discover_select(const float* d_scores, int64_t n, int64_t m, int64_t ld, const int32_t* d_queries, int32_t side,
                                      const int64_t* d_flt_lo, const int64_t* d_flt_hi, const int32_t* d_flt_ids, int32_t R, int32_t margin_q,
                                      int32_t* d_thr, int32_t thr_given, int64_t row_base, int32_t* d_pairs, int64_t cap, int64_t* d_count,
                                      void* stream) {
    if (n < 0 || m < 0 || ld < m || cap < 0 || row_base < 0 || margin_q < 0) return set_error(AMDKGE_EINVAL, "discover_select: bad sizes (ld >= m, cap >= 0, row_base >= 0, margin_q >= 0)");
    if (side != AMDKGE_SIDE_S && side != AMDKGE_SIDE_O) return set_error(AMDKGE_EINVAL, "discover_select: side must be AMDKGE_SIDE_S or AMDKGE_SIDE_O");
    if (R < 1 || (!thr_given && R > TOPK_MAX)) return set_error(AMDKGE_EINVAL, "discover_select: 1 <= R <= 1024 (beyond that the caller supplies the thresholds)");
    if (n > 0x7FFFFFFFll || row_base + n > 0x7FFFFFFFll || m > 0x7FFFFFFFll) return set_error(AMDKGE_EUNSUPPORTED, "discover_select: rows and columns are int32");
    if (!d_count) return set_error(AMDKGE_EINVAL, "discover_select: NULL count");
    if ((d_flt_lo == nullptr) != (d_flt_hi == nullptr) || (d_flt_lo && !d_flt_ids)) return set_error(AMDKGE_EINVAL, "discover_select: the filter is (lo, hi, ids) or three NULLs");
    if (cap > 0 && !d_pairs) return set_error(AMDKGE_EINVAL, "discover_select: NULL pair buffer");
    if (n > 0 && (!d_queries || !d_thr || (m > 0 && !d_scores))) return set_error(AMDKGE_EINVAL, "discover_select: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(d_count, 0, sizeof(int64_t), st);
    if (e != hipSuccess) return set_error_hip(e, "discover_select: hipMemsetAsync");
    if (n == 0) return AMDKGE_OK;
    const int64_t bm_bytes = ((m + 31) / 32) * 4;
    const int use_bitmap = bm_bytes <= SELECT_BITMAP_MAX_BYTES ? 1 : 0;
    const size_t lds = use_bitmap ? (size_t)bm_bytes : 0;
    if (lds > 32 * 1024) {
        static PerDeviceOnce attr;
        if (int rc = ensure_dynamic_lds(attr, {(const void*)discover_select_kernel}, (size_t)SELECT_BITMAP_MAX_BYTES, "discover_select")) return rc;
    }
    hipLaunchKernelGGL(discover_select_kernel, dim3((unsigned)n), dim3(256), lds, st, d_scores, m, ld, d_queries, side == AMDKGE_SIDE_S ? 2 : 0, d_flt_lo,
                       d_flt_hi, d_flt_ids, (int)R, (int)margin_q, d_thr, (int)thr_given, use_bitmap, row_base, d_pairs, cap,
                       (unsigned long long*)d_count);
    return check_launch("discover_select");
}
