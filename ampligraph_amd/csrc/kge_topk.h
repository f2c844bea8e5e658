// The streaming per-row selection's building blocks, shared by amdkge_topk_rows (kge_discovery.hip) and amdkge_discover_select
// (kge_discover.hip): an order-preserving key, and the bitonic merge of the LDS candidate buffer.
#pragma once
#include "kge_host.h"

namespace kge {

constexpr int TOPK_MAX = 1024;          // largest k
constexpr int TOPK_BUF = 2 * TOPK_MAX;  // LDS candidates: the current best TOPK_MAX (sorted) + a staging half

// order-preserving map fp32 -> uint32 (larger float <=> larger key); NaN sorts below everything
__device__ __forceinline__ uint32_t sortable(float v) {
    if (v != v) return 0u;
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float unsortable(uint32_t k) {
    const uint32_t b = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    return __uint_as_float(b);
}

// bitonic sort of buf[0 .. TOPK_BUF) in DESCENDING order by the 64-bit key (256 threads)
__device__ __forceinline__ void sort_desc(unsigned long long* buf, int tid) {
    for (int k = 2; k <= TOPK_BUF; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < TOPK_BUF; i += 256) {
                const int p = i ^ j;
                if (p > i) {
                    const bool desc = (i & k) == 0;
                    const unsigned long long a = buf[i], b = buf[p];
                    if (desc ? (a < b) : (a > b)) { buf[i] = b; buf[p] = a; }
                }
            }
            __syncthreads();
        }
}

}  // namespace kge
