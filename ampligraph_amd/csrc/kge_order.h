// Ordering helpers the kernels share: the order-preserving fp32 key of the per-row selections (kge_topk.h) and the membership test in
// an ascending id range (the id order inside a group of amdkge_filter_build / amdkge_pair_filter_build).
// Depends on <stdint.h> only: hipcc compiles it for both sides (kge_device.h includes it), g++ compiles it for the CPU test
// (tests/csrc/order_check.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KGE_ORDER_FN __host__ __device__ __forceinline__
#else
#define KGE_ORDER_FN inline
#endif

namespace kge {

// order-preserving map fp32 -> uint32 (larger float <=> larger key); NaN sorts below everything
KGE_ORDER_FN uint32_t sortable(float v) {
    if (v != v) return 0u;
    const uint32_t b = __builtin_bit_cast(uint32_t, v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
KGE_ORDER_FN float unsortable(uint32_t k) {
    const uint32_t b = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    return __builtin_bit_cast(float, b);
}

// is `id` in the ascending range ids[lo .. hi)?  I: int for a range staged in LDS, int64_t for one in global memory.  A lower bound
// and one compare: the trip count depends on the range's length only, and nothing leaves the loop early.
template <typename I>
KGE_ORDER_FN bool sorted_contains(const int32_t* __restrict__ ids, I lo, I hi, int64_t id) {
    const I end = hi;
    while (lo < hi) {
        const I mid = lo + ((hi - lo) >> 1);
        if (ids[mid] < id) lo = mid + 1; else hi = mid;
    }
    return lo < end && ids[lo] == id;
}

}  // namespace kge
