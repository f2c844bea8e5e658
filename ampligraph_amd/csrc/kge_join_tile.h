// The 128 x 128 tile of squared euclidean distances between the rows of two dense fp32 matrices, shared by the self-join
// (kge_join.hip: find_duplicates, find_clusters' DBSCAN) and the KMeans assignment (kge_kmeans.hip).
//
// A pair's value is ONE fp32 expression of its two rows, d2 = fma chain over c = 0 .. d-1 of (a_c - b_c)^2 in column order,
// whatever kernel asks for it; (a - b)^2 == (b - a)^2 exactly, so the value does not depend on the side a row is on either.
#pragma once
#include "kge_host.h"

namespace kge {

constexpr int JT = 128;           // rows per tile side
constexpr int JKT = 16;           // columns per LDS stage
constexpr int JLD = JT + 4;       // LDS row pitch (floats)

typedef float jf2 __attribute__((ext_vector_type(2)));

// columns k0 .. k0 + JKT of rows r0 .. r0 + JT -> S[column][row] (rows beyond n repeat row n - 1, columns beyond d are 0 on
// both sides: fma(0, 0, acc) == acc, so the padding leaves every sum as it is).  LD: the pitch of S; a tile side of fewer than JT
// rows (kge_kmeans.hip's narrow centre tiles) is staged by its first 2 * rows threads.
template <bool V4, int LD = JLD>
__device__ __forceinline__ void join_stage(const float* __restrict__ X, int64_t n, int d, int64_t r0, int k0, float (*S)[LD], int tid) {
    const int lrow = tid >> 1, lc = (tid & 1) * 8;
    const int64_t r = r0 + lrow < n ? r0 + lrow : n - 1;
    const float* row = X + r * (int64_t)d;
    float v[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int c = k0 + lc + 4 * h;
        if (V4) {   // d % 4 == 0: a group is either wholly inside the row or wholly beyond it
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < d) t = *reinterpret_cast<const float4*>(row + c);
            v[4 * h] = t.x; v[4 * h + 1] = t.y; v[4 * h + 2] = t.z; v[4 * h + 3] = t.w;
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) v[4 * h + u] = (c + u < d) ? row[c + u] : 0.f;
        }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) S[lc + u][lrow] = v[u];
}

// Squared distances of the thread's 8 x 8 pairs of the tile of rows ra0 .. of XA [na, d] against rows rb0 .. of XB [nb, d] (the
// self-join passes one matrix twice; its diagonal tiles then stage one side only).  Thread (tq, te) = (tid / 16, tid % 16) owns
// A rows ra0 + arow(x) and B rows rb0 + arow(y), arow(v) = v < 4 ? 4 t + v : 64 + 4 t + v - 4 (contiguous 16-byte LDS reads).
// The inner step is the VALU tile of rank_count_kernel<MODE_L1>: a packed subtract forms a - b for two B rows at once (a
// broadcast), and a packed FMA accumulates d * d -- strictly in column order for every pair.
template <bool V4>
__device__ __forceinline__ void join_tile(const float* __restrict__ XA, int64_t na, const float* __restrict__ XB, int64_t nb, int d, int64_t ra0, int64_t rb0,
                                          float (*As)[JLD], float (*Bs)[JLD], jf2 (&acc)[8][4], int tid) {
    const int tq = tid >> 4, te = tid & 15;
    const bool diag = XA == XB && ra0 == rb0;
    float (*B)[JLD] = diag ? As : Bs;
#pragma unroll
    for (int x = 0; x < 8; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) acc[x][y] = jf2{0.f, 0.f};
    for (int k0 = 0; k0 < d; k0 += JKT) {
        __syncthreads();   // the previous stage (or tile) is no longer read
        join_stage<V4>(XA, na, d, ra0, k0, As, tid);
        if (!diag) join_stage<V4>(XB, nb, d, rb0, k0, Bs, tid);
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < JKT; ++kk) {
            const float4 a0 = *reinterpret_cast<const float4*>(&As[kk][tq * 4]), a1 = *reinterpret_cast<const float4*>(&As[kk][64 + tq * 4]);
            const float4 b0 = *reinterpret_cast<const float4*>(&B[kk][te * 4]), b1 = *reinterpret_cast<const float4*>(&B[kk][64 + te * 4]);
            const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            const jf2 bv[4] = {{b0.x, b0.y}, {b0.z, b0.w}, {b1.x, b1.y}, {b1.z, b1.w}};
#pragma unroll
            for (int x = 0; x < 8; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) {
                    const jf2 dd = jf2{av[x], av[x]} - bv[y];
                    acc[x][y] = __builtin_elementwise_fma(dd, dd, acc[x][y]);
                }
        }
    }
}

__device__ __forceinline__ int join_row(int t, int v) { return v < 4 ? 4 * t + v : 64 + 4 * t + v - 4; }
__device__ __forceinline__ float join_val(const jf2 (&acc)[8][4], int x, int v) { return (v & 1) ? acc[x][v >> 1].y : acc[x][v >> 1].x; }
// nearest-row key: non-negative floats order like their bit patterns, so the 64-bit minimum is the smallest distance and,
// among equal distances, the lowest index -- whatever order the atomics arrive in
__device__ __forceinline__ unsigned long long join_key(float v, int64_t idx) {
    return ((unsigned long long)__float_as_uint(v) << 32) | (unsigned long long)(uint32_t)idx;
}
__device__ __forceinline__ unsigned long long umin64(unsigned long long a, unsigned long long b) { return a < b ? a : b; }

}  // namespace kge
