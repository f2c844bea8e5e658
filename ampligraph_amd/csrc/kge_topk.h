// The streaming per-row selection, shared by amdkge_topk_rows (kge_discovery.hip), amdkge_topk_rows_excluding (kge_complete.hip) and
// sweep one of amdkge_discover_select (kge_discover.hip): the 64-bit key, the bitonic merge of the LDS candidate buffer and the loop
// step around them (TopkStream).  A kernel keeps what is its own: how a column's value becomes a key, which columns it skips, what it
// does with the sorted keys.  The order-preserving fp32 key itself (sortable / unsortable) is kge_order.h's.
#pragma once
#include "kge_host.h"

namespace kge {

constexpr int TOPK_MAX = 1024;          // largest k
constexpr int TOPK_BUF = 2 * TOPK_MAX;  // LDS candidates: the current best TOPK_MAX (sorted) + a staging half

// key = 32-bit order key << 32 | ~column: equal values are ordered by LOWER column first, so the result is deterministic (0: no candidate)
__device__ __forceinline__ unsigned long long topk_key(uint32_t ord, int64_t col) {
    return ((unsigned long long)ord << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)col);
}
__device__ __forceinline__ int32_t topk_col(unsigned long long key) { return (int32_t)(0xFFFFFFFFu - (uint32_t)key); }

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

// One workgroup (256 threads) streams a row past its k best keys, 256 columns per block.  Keys at or below the current k-th best
// are dropped as they stream by; survivors collect in the staging half and are merged (one bitonic sort) whenever it fills.
// Every thread makes every call: reset and end_of_block hold the barriers.  Afterwards buf[0 .. k) holds the best keys, descending.
struct TopkStream {
    unsigned long long* buf;   // __shared__ [TOPK_BUF]
    int* n_stage;              // __shared__: keys in the staging half
    int tid = 0;
    unsigned long long kth = 0ull;   // key of the current k-th best (0: fewer than k candidates so far)

    __device__ __forceinline__ void reset(int thread) {
        tid = thread;
        for (int i = tid; i < TOPK_BUF; i += 256) buf[i] = 0ull;
        if (tid == 0) *n_stage = 0;
        kth = 0ull;
        __syncthreads();
    }
    // stage `key` if it beats the k-th best and `admit()` lets it in (asked only then: a caller's lookup runs for the few columns
    // that could enter)
    template <typename Admit>
    __device__ __forceinline__ void offer(unsigned long long key, Admit admit) {
        if (key > kth && admit()) buf[TOPK_MAX + atomicAdd(n_stage, 1)] = key;
    }
    __device__ __forceinline__ void offer(unsigned long long key) {
        offer(key, [] { return true; });
    }
    // behind a block of 256 offers (last: the row's last block): merge when the staging half is (nearly) full or the row has ended
    __device__ __forceinline__ void end_of_block(int k, bool last) {
        __syncthreads();
        if (*n_stage > TOPK_MAX - 256 || last) {
            sort_desc(buf, tid);
            if (tid == 0) *n_stage = 0;
            kth = buf[k - 1];
            __syncthreads();
            for (int i = TOPK_MAX + tid; i < TOPK_BUF; i += 256) buf[i] = 0ull;
            __syncthreads();
        }
    }
};

}  // namespace kge
