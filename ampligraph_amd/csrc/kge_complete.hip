// Batched completion on the device (discovery.query_topn_batch): the per-row top-k selection behind a 1-vs-all score block of
// amdkge_corruption_scores that leaves out the statements already known to be true.  A known completion is EXCLUDED from the
// selection -- it never enters the candidate buffer, so it cannot come back as a filler when fewer than k columns remain --
// instead of being overwritten in the score block: -inf and NaN are legitimate scores there.
#include "kge_topk.h"

namespace kge {

// One workgroup per row: the streaming selection (TopkStream, kge_topk.h) with topk_rows_kernel's key (kge_discovery.hip), so the same
// order, and a membership test in front of the staging buffer.  Only a column whose key beats the current k-th best is looked up: after
// the first merge that is a handful of columns per row, the known facts among them (they score highest), so the usual column costs
// one compare as before.
__global__ __launch_bounds__(256) void topk_rows_excluding_kernel(const float* __restrict__ vals, int64_t m, int64_t ld, const int32_t* __restrict__ col_ids,
                                                                  int64_t id_base, const int64_t* __restrict__ ex_lo, const int64_t* __restrict__ ex_hi,
                                                                  const int32_t* __restrict__ ex_ids, const int32_t* __restrict__ own, int k,
                                                                  int32_t* __restrict__ out_idx, float* __restrict__ out_val) {
    __shared__ unsigned long long buf[TOPK_BUF];
    __shared__ int n_stage;
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const float* row = vals + r * ld;
    const int64_t lo = ex_lo ? ex_lo[r] : 0, hi = ex_lo ? ex_hi[r] : 0;
    const bool has_own = own != nullptr;
    const int64_t own_id = has_own ? (int64_t)own[r] : 0;
    TopkStream sel{buf, &n_stage};
    sel.reset(tid);
    for (int64_t c0 = 0; c0 < m; c0 += 256) {
        const int64_t c = c0 + tid;
        if (c < m)
            sel.offer(topk_key(sortable(row[c]), c), [&] {
                const int64_t id = col_ids ? (int64_t)col_ids[c] : id_base + c;
                return !(has_own && id == own_id) && !sorted_contains(ex_ids, lo, hi, id);
            });
        sel.end_of_block(k, c0 + 256 >= m);
    }
    for (int i = tid; i < k; i += 256) {
        const unsigned long long key = buf[i];
        const bool have = key != 0ull;
        out_idx[r * k + i] = have ? topk_col(key) : -1;
        out_val[r * k + i] = have ? unsortable((uint32_t)(key >> 32)) : -INFINITY;
    }
}

}  // namespace kge

using namespace kge;

extern "C" int amdkge_topk_rows_excluding(const float* d_vals, int64_t n, int64_t m, int64_t ld, const int32_t* d_col_ids, int64_t id_base,
                                          const int64_t* d_ex_lo, const int64_t* d_ex_hi, const int32_t* d_ex_ids, const int32_t* d_own,
                                          int32_t k, int32_t* d_out_idx, float* d_out_val, void* stream) {
    if (n < 0 || m < 0 || ld < m || k < 1 || k > TOPK_MAX) return set_error(AMDKGE_EINVAL, "topk_rows_excluding: bad sizes (1 <= k <= 1024, ld >= m)");
    if ((d_ex_lo == nullptr) != (d_ex_hi == nullptr) || (d_ex_lo == nullptr) != (d_ex_ids == nullptr))
        return set_error(AMDKGE_EINVAL, "topk_rows_excluding: the excluded ids are (lo, hi, ids) or three NULLs");
    // (d_out_idx holds int32 column indices, -1 = missing: a column beyond 2^31 - 1 has no representation)
    if (n > 0x7FFFFFFFll || m > 0x7FFFFFFFll) return set_error(AMDKGE_EUNSUPPORTED, "topk_rows_excluding: rows and columns are int32 (n, m <= 2^31 - 1)");
    if (n == 0) return AMDKGE_OK;
    if (!d_out_idx || !d_out_val || (m > 0 && !d_vals)) return set_error(AMDKGE_EINVAL, "topk_rows_excluding: NULL pointer");
    hipLaunchKernelGGL(topk_rows_excluding_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, d_vals, m, ld, d_col_ids, id_base, d_ex_lo,
                       d_ex_hi, d_ex_ids, d_own, (int)k, d_out_idx, d_out_val);
    return check_launch("topk_rows_excluding");
}
