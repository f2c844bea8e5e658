// Sparse optimizer mode (include/ext/amdkge_sparse.h): the sweep of a shared-negative step over the rows the step can have touched.
//   amdkge_step_rows     : the step's candidate rows -- the ascending unique union of its positives' s and o and its list ids.
//                          Keys -> rocPRIM radix sort (only the bits n_ents needs) -> "first of its value" flags, scanned on the fly
//                          -> emit.  Chosen over an N-bit map: the map's compaction walks N / 32 words every step (16 MB at 2^31 - 1
//                          entities) and the map must be kept zero between calls; the sort's cost depends on the 2B + n_ids keys alone.
//   amdkge_opt_step_rows : opt_row (kge_opt.h, the row body of the whole-table lazy sweep) on the listed rows, one wave per row.
// A gather of whole rows at 16 B per lane, three or four streams per row (g, x and the kind's slots), every row independent: bound by
// HBM on scattered rows of row_floats * 4 bytes, not by the streaming copy rate.
#include <string.h>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "../../include/ext/amdkge_sparse.h"
#include "kge_opt.h"

namespace kge {

// key i of a step: s and o of positive i / 2, then the list ids.  An id outside [0, n_ents) becomes the key n_ents, which sorts
// behind every row and is never emitted.
__global__ void step_keys_kernel(const int32_t* __restrict__ tri, int64_t B, const int32_t* __restrict__ ids, int64_t m, uint32_t n_ents,
                                 uint32_t* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int32_t v = i < 2 * B ? tri[3 * (i >> 1) + 2 * (i & 1)] : ids[i - 2 * B];
    keys[i] = (v >= 0 && (uint32_t)v < n_ents) ? (uint32_t)v : n_ents;
}

// position i of the sorted keys -> 1 where a row id appears for the first time
struct FirstOfRow {
    const uint32_t* k;
    uint32_t n_ents;
    __device__ uint32_t operator()(uint32_t i) const { return (k[i] < n_ents && (i == 0 || k[i] != k[i - 1])) ? 1u : 0u; }
};
using FirstIter = rocprim::transform_iterator<rocprim::counting_iterator<uint32_t>, FirstOfRow, uint32_t>;

__global__ void step_emit_kernel(const uint32_t* __restrict__ k, const uint32_t* __restrict__ pos, int64_t m, uint32_t n_ents, int64_t cap,
                                 int32_t* __restrict__ rows, int64_t* __restrict__ n_rows) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t first = FirstOfRow{k, n_ents}((uint32_t)i), at = pos[i];
    if (first && (int64_t)at < cap) rows[at] = (int32_t)k[i];
    if (i == m - 1) n_rows[0] = (int64_t)at + first;
}

struct StepRowsPlan {
    int64_t off_a, off_b, off_pos, off_tmp, total;   // the walk (the library aligns d_work up itself)
    size_t tmp_bytes;
    unsigned key_bits;
};

static int make_step_rows_plan(int64_t n_ents, int64_t m, StepRowsPlan& p) {
    p.key_bits = 1;
    while (p.key_bits < 32 && (1ull << p.key_bits) <= (uint64_t)n_ents) ++p.key_bits;   // the keys are 0 .. n_ents
    size_t t_sort = 0, t_scan = 0;
    uint32_t* nul = nullptr;
    if (rocprim::radix_sort_keys(nullptr, t_sort, nul, nul, (size_t)m, 0u, p.key_bits, (hipStream_t)0) != hipSuccess) return -1;
    FirstIter flags(rocprim::counting_iterator<uint32_t>(0), FirstOfRow{nul, 0});
    if (rocprim::exclusive_scan(nullptr, t_scan, flags, nul, (uint32_t)0, (size_t)m, rocprim::plus<uint32_t>(), (hipStream_t)0) != hipSuccess) return -1;
    p.tmp_bytes = t_sort > t_scan ? t_sort : t_scan;
    Layout l;
    p.off_a = l.take(m, 4);                     // the keys
    p.off_b = l.take(m, 4);                     // sorted
    p.off_pos = l.take(m, 4);                   // scanned flags: a first occurrence's place in the output
    p.off_tmp = l.take((int64_t)p.tmp_bytes);   // rocPRIM scratch
    p.total = l.any_base(l.next());
    return 0;
}

// the listed-rows sweep: wave w of the grid takes rows[w], rows[w + waves], ...
template <int KIND>
__global__ __launch_bounds__(256) void opt_listed_rows_kernel(OptArgs a, const int32_t* __restrict__ rows, const int64_t* __restrict__ n_rows, int64_t cap,
                                                              int64_t n_table_rows) {
    int64_t n = n_rows[0];
    n = n < 0 ? 0 : (n > cap ? cap : n);
    const int nq = a.row_floats >> 2, lane = threadIdx.x & 63;
    float reg_acc = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += (int64_t)gridDim.x * 4) {
        const int64_t r = (int64_t)__builtin_amdgcn_readfirstlane(rows[i]);
        if (r < 0 || r >= n_table_rows) continue;
        opt_row<KIND>(a, nq, r, lane, reg_acc);
    }
    if (a.reg_loss && a.lam != 0.f) {   // as opt_rows_kernel (kge_opt.hip): the block's four wave totals, one atomic
        __shared__ float red[4];
        const float w = wave_sum(reg_acc);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
        __syncthreads();
        if (threadIdx.x == 0) atomicAdd(a.reg_loss, (double)a.lam * ((double)red[0] + red[1] + red[2] + red[3]));
    }
}

}  // namespace kge

using namespace kge;

static bool step_rows_sizes_ok(int64_t n_ents, int64_t m) { return n_ents >= 1 && n_ents <= 0x7FFFFFFFll && m >= 0 && m <= 0x7FFFFFFFll; }

extern "C" int64_t amdkge_step_rows_workspace_bytes(int64_t n_ents, int64_t n_keys) {
    if (!step_rows_sizes_ok(n_ents, n_keys)) return -1;
    if (n_keys == 0) return 256;
    StepRowsPlan p;
    if (make_step_rows_plan(n_ents, n_keys, p)) return -1;
    return p.total;
}

extern "C" int amdkge_step_rows(int64_t n_ents, const int32_t* d_triples, int64_t B, const int32_t* d_ids, int64_t n_ids, int32_t* d_rows,
                                int64_t cap, int64_t* d_n_rows, void* d_work, void* stream) {
    if (B < 0 || n_ids < 0 || B > 0x3FFFFFFFll || !step_rows_sizes_ok(n_ents, 2 * B + n_ids))
        return set_error(AMDKGE_EINVAL, "step_rows: bad sizes (1 <= n_ents < 2^31, B >= 0, n_ids >= 0, 2 B + n_ids < 2^31)");
    const int64_t m = 2 * B + n_ids;
    if (cap < (m < n_ents ? m : n_ents)) return set_error(AMDKGE_EINVAL, "step_rows: cap must be at least min(2 B + n_ids, n_ents)");
    if (!d_n_rows || (cap > 0 && !d_rows)) return set_error(AMDKGE_EINVAL, "step_rows: NULL d_rows / d_n_rows");
    hipStream_t st = (hipStream_t)stream;
    if (m == 0) {
        if (hipError_t e = hipMemsetAsync(d_n_rows, 0, 8, st)) return set_error_hip(e, "hipMemsetAsync(step_rows count)");
        return AMDKGE_OK;
    }
    if (!d_work || (B > 0 && !d_triples) || (n_ids > 0 && !d_ids)) return set_error(AMDKGE_EINVAL, "step_rows: NULL triples / ids / workspace");
    StepRowsPlan p;
    if (make_step_rows_plan(n_ents, m, p)) return set_error(AMDKGE_EHIP, "step_rows: rocPRIM size query failed");
    char* w = aligned_base(d_work);
    uint32_t* a = (uint32_t*)(w + p.off_a);
    uint32_t* b = (uint32_t*)(w + p.off_b);
    uint32_t* pos = (uint32_t*)(w + p.off_pos);
    void* tmp = w + p.off_tmp;
    const unsigned grid = (unsigned)((m + 255) / 256);
    hipLaunchKernelGGL(step_keys_kernel, dim3(grid), dim3(256), 0, st, d_triples, B, d_ids, m, (uint32_t)n_ents, a);
    if (int rc = check_launch("step_keys")) return rc;
    size_t tb = p.tmp_bytes;
    if (hipError_t e = rocprim::radix_sort_keys(tmp, tb, a, b, (size_t)m, 0u, p.key_bits, st)) return set_error_hip(e, "rocprim::radix_sort_keys(step_rows)");
    tb = p.tmp_bytes;
    FirstIter flags(rocprim::counting_iterator<uint32_t>(0), FirstOfRow{b, (uint32_t)n_ents});
    if (hipError_t e = rocprim::exclusive_scan(tmp, tb, flags, pos, (uint32_t)0, (size_t)m, rocprim::plus<uint32_t>(), st))
        return set_error_hip(e, "rocprim::exclusive_scan(step_rows)");
    hipLaunchKernelGGL(step_emit_kernel, dim3(grid), dim3(256), 0, st, b, pos, m, (uint32_t)n_ents, cap, d_rows, d_n_rows);
    return check_launch("step_emit");
}

extern "C" int amdkge_opt_step_rows(const amdkge_opt* opt, float* d_x, float* d_grad, float* d_slot0, float* d_slot1, int64_t n_table_rows,
                                    const int32_t* d_rows, const int64_t* d_n_rows, int64_t cap, double* d_reg_loss, void* stream) {
    if (int rc = validate_opt(opt)) return rc;
    if (opt->row_floats < 4 || opt->row_floats % 4 != 0)
        return set_error(AMDKGE_EINVAL, "opt_step_rows: needs row_floats = amdkge_row_floats(model) of a padded layout (multiple of 4)");
    if (n_table_rows < 0 || cap < 0) return set_error(AMDKGE_EINVAL, "opt_step_rows: n_table_rows and cap must be >= 0");
    if (!d_x || !d_grad) return set_error(AMDKGE_EINVAL, "opt_step_rows: NULL table / gradient pointer");
    if (opt_nslots(opt->kind) >= 1 && !d_slot0) return set_error(AMDKGE_EINVAL, "opt_step_rows: optimizer slot 0 is NULL");
    if (opt_nslots(opt->kind) == 2 && !d_slot1) return set_error(AMDKGE_EINVAL, "opt_step_rows: optimizer slot 1 is NULL");
    if ((((uintptr_t)d_x | (uintptr_t)d_grad | (uintptr_t)d_slot0 | (uintptr_t)d_slot1) & 15) != 0)
        return set_error(AMDKGE_EINVAL, "opt_step_rows: buffers must be 16-byte aligned");
    if (cap == 0 || n_table_rows == 0) return AMDKGE_OK;
    if (!d_rows || !d_n_rows) return set_error(AMDKGE_EINVAL, "opt_step_rows: NULL d_rows / d_n_rows");
    OptArgs a{};
    a.x = d_x; a.g = d_grad; a.s0 = d_slot0; a.s1 = d_slot1; a.reg_loss = d_reg_loss;
    a.n = n_table_rows * (int64_t)opt->row_floats;
    fill_opt_args(a, opt);
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)((cap + 3) / 4 < 256 * 16 ? (cap + 3) / 4 : 256 * 16);
#define KGE_OPT_LAUNCH_LISTED(KIND) hipLaunchKernelGGL(opt_listed_rows_kernel<KIND>, dim3(grid), dim3(256), 0, st, a, d_rows, d_n_rows, cap, n_table_rows)
    KGE_OPT_DISPATCH(opt->kind, KGE_OPT_LAUNCH_LISTED)
#undef KGE_OPT_LAUNCH_LISTED
    return check_launch("opt_step_rows");
}
