// Exact self-join of a dense fp32 matrix X [n, d] in squared euclidean distance: the device side of find_duplicates
// (the reference's discovery/discovery.py:714-982).  The reference fills a float64 n x n distance_matrix from
// Python for its tolerance bound and runs a full sklearn radius_neighbors pass over all pairs at every bisection step;
// here one pass over the pairs gives every row's nearest other row plus the largest pair distance (amdkge_join_nearest),
// the bisection runs on the host over those n numbers, and a second pass emits the pairs within the chosen radius
// (amdkge_join_radius).
//
// A pair's value is ONE fp32 expression of its two rows, d2 = fma chain over c = 0 .. d-1 of (x_ic - x_jc)^2 in column
// order, computed by the same tile routine in both entry points; (x_i - x_j)^2 == (x_j - x_i)^2 exactly, so the value does
// not depend on which side of the diagonal the pair lands either.  A row's nearest distance and the radius decisions
// therefore agree bit for bit.  The direct form on purpose: the GEMM form |a|^2 + |b|^2 - 2<a,b> cancels for near pairs
// (see pair_dist_kernel in kge_discovery.hip), and near pairs are what duplicate search is about.
//
// find_clusters' DBSCAN (the reference's discovery/discovery.py:546-711 hands the embeddings to sklearn on the host) runs on the
// same tile routine: amdkge_join_dbscan, three passes over the pairs and O(n) state, below the two duplicate kernels.
#include "kge_join_tile.h"

namespace kge {

// (the tile routine -- join_stage, join_tile, join_row, join_val, join_key, umin64 -- lives in kge_join_tile.h)
constexpr int64_t JOIN_MAX_BLOCKS = 65536;   // persistent grid: every block walks tiles blockIdx.x, + gridDim.x, ...

// Tile t of the upper triangle (diagonal included), enumerated column by column: t = tb (tb + 1) / 2 + ta, ta <= tb.
// (t < 2^47 for n = 2^31 - 1: 8 t + 1 is exact in a double; the two loops correct the square root's rounding.)
__device__ __forceinline__ void join_tile_of(int64_t t, int64_t& ta, int64_t& tb) {
    int64_t b = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (b > 0 && b * (b + 1) / 2 > t) --b;
    while ((b + 1) * (b + 2) / 2 <= t) ++b;
    tb = b;
    ta = t - b * (b + 1) / 2;
}

template <bool V4>
__global__ __launch_bounds__(256) void join_nearest_kernel(const float* __restrict__ X, int64_t n, int d, int64_t total,
                                                           unsigned long long* __restrict__ keys, unsigned int* __restrict__ max_bits) {
    __shared__ __attribute__((aligned(16))) float As[JKT][JLD];
    __shared__ __attribute__((aligned(16))) float Bs[JKT][JLD];
    __shared__ unsigned long long red[4][JT];
    const int tid = threadIdx.x, tq = tid >> 4, te = tid & 15, wave = tid >> 6;
    uint32_t mx = 0u;
    for (int64_t t = blockIdx.x; t < total; t += gridDim.x) {
        int64_t ta, tb;
        join_tile_of(t, ta, tb);
        const int64_t ra0 = ta * JT, rb0 = tb * JT;
        jf2 acc[8][4];
        join_tile<V4>(X, n, X, n, d, ra0, rb0, As, Bs, acc, tid);
        const bool diag = ta == tb;
        // A side: the nearest B row of each A row (a diagonal tile holds both orders of its pairs: this side alone covers it)
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            const int64_t ra = ra0 + join_row(tq, x);
            unsigned long long m = ~0ull;
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                const int64_t rb = rb0 + join_row(te, v);
                if (ra < n && rb < n && ra != rb) {
                    const float val = join_val(acc, x, v);
                    m = umin64(m, join_key(val, rb));
                    mx = max(mx, __float_as_uint(val));
                }
            }
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) m = umin64(m, __shfl_xor(m, o, 64));
            if (te == 0 && m != ~0ull) atomicMin(&keys[ra], m);
        }
        if (!diag) {
            // B side: the nearest A row of each B row -- over the thread's 8, the wave's 4 A-row groups, then the 4 waves
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                const int64_t rb = rb0 + join_row(te, v);
                unsigned long long m = ~0ull;
#pragma unroll
                for (int x = 0; x < 8; ++x) {
                    const int64_t ra = ra0 + join_row(tq, x);
                    if (ra < n && rb < n) m = umin64(m, join_key(join_val(acc, x, v), ra));
                }
                m = umin64(m, __shfl_xor(m, 16, 64));
                m = umin64(m, __shfl_xor(m, 32, 64));
                if ((tq & 3) == 0) red[wave][join_row(te, v)] = m;
            }
            __syncthreads();
            if (tid < JT) {
                const unsigned long long m = umin64(umin64(red[0][tid], red[1][tid]), umin64(red[2][tid], red[3][tid]));
                if (m != ~0ull) atomicMin(&keys[rb0 + tid], m);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
    if ((tid & 63) == 0 && mx != 0u) atomicMax(max_bits, mx);
}

__global__ __launch_bounds__(256) void join_keys_kernel(const unsigned long long* __restrict__ keys, int64_t n, float* __restrict__ dist,
                                                        int32_t* __restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = keys[i];
    dist[i] = k == ~0ull ? INFINITY : __uint_as_float((uint32_t)(k >> 32));
    idx[i] = k == ~0ull ? -1 : (int32_t)(uint32_t)k;
}

template <bool V4>
__global__ __launch_bounds__(256) void join_radius_kernel(const float* __restrict__ X, int64_t n, int d, int64_t total, double thr,
                                                          int32_t* __restrict__ pairs, int64_t cap, unsigned long long* __restrict__ count) {
    __shared__ __attribute__((aligned(16))) float As[JKT][JLD];
    __shared__ __attribute__((aligned(16))) float Bs[JKT][JLD];
    const int tid = threadIdx.x, tq = tid >> 4, te = tid & 15;
    for (int64_t t = blockIdx.x; t < total; t += gridDim.x) {
        int64_t ta, tb;
        join_tile_of(t, ta, tb);
        const int64_t ra0 = ta * JT, rb0 = tb * JT;
        jf2 acc[8][4];
        join_tile<V4>(X, n, X, n, d, ra0, rb0, As, Bs, acc, tid);
        // every unordered pair once: i < j (off the diagonal every A row is below every B row); the fp32 value is compared
        // with the double threshold as it is
        uint64_t hit = 0ull;
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            const int64_t ra = ra0 + join_row(tq, x);
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                const int64_t rb = rb0 + join_row(te, v);
                if (rb < n && ra < rb && (double)join_val(acc, x, v) <= thr) hit |= 1ull << (8 * x + v);
            }
        }
        if (hit) {   // one counter update per thread and tile (filter_pairs_kernel's counter-and-capacity pattern)
            unsigned long long pos = atomicAdd(count, (unsigned long long)__popcll(hit));
            for (; hit; hit &= hit - 1ull, ++pos) {
                const int b = __ffsll((unsigned long long)hit) - 1;
                if ((int64_t)pos < cap) {
                    pairs[2 * pos] = (int32_t)(ra0 + join_row(tq, b >> 3));
                    pairs[2 * pos + 1] = (int32_t)(rb0 + join_row(te, b & 7));
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ DBSCAN
// find_clusters' default algorithm as three more passes over the same tiles: a radius self-join (count), a core-point test,
// connected components of the core rows (union) and the border rows' clusters (border).  No pair list: the state is three
// int32 arrays of n.  Every pass takes a pair's d2 from join_tile, so a pair is "within the radius" in all of them or in none.

// bit 8 x + v: the thread's pair (A row x, B row v) lies inside the matrix and has d2 <= thr.  `upper`: only i < j (each
// unordered pair once; off the diagonal every A row is below every B row); otherwise a diagonal tile holds both orders of
// its pairs and the pairs (i, i).
__device__ __forceinline__ uint64_t join_hits(const jf2 (&acc)[8][4], int64_t ra0, int64_t rb0, int64_t n, double thr, int tq, int te, bool upper) {
    uint64_t hit = 0ull;
#pragma unroll
    for (int x = 0; x < 8; ++x) {
        const int64_t ra = ra0 + join_row(tq, x);
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const int64_t rb = rb0 + join_row(te, v);
            if (ra < n && rb < n && (!upper || ra < rb) && (double)join_val(acc, x, v) <= thr) hit |= 1ull << (8 * x + v);
        }
    }
    return hit;
}

// cnt[i] += the rows j of this tile with d2(i, j) <= thr (i itself included, on the diagonal): the thread's 8 x 8 hits are
// summed over the lanes that share a row (A side) or over the wave and then the four waves through LDS (B side), as
// join_nearest_kernel reduces its keys -- one atomic per row and tile.
template <bool V4>
__global__ __launch_bounds__(256) void join_count_kernel(const float* __restrict__ X, int64_t n, int d, int64_t total, double thr, int32_t* __restrict__ cnt) {
    __shared__ __attribute__((aligned(16))) float As[JKT][JLD];
    __shared__ __attribute__((aligned(16))) float Bs[JKT][JLD];
    __shared__ int red[4][JT];
    const int tid = threadIdx.x, tq = tid >> 4, te = tid & 15, wave = tid >> 6;
    for (int64_t t = blockIdx.x; t < total; t += gridDim.x) {
        int64_t ta, tb;
        join_tile_of(t, ta, tb);
        const int64_t ra0 = ta * JT, rb0 = tb * JT;
        jf2 acc[8][4];
        join_tile<V4>(X, n, X, n, d, ra0, rb0, As, Bs, acc, tid);
        const bool diag = ta == tb;
        const uint64_t hit = join_hits(acc, ra0, rb0, n, thr, tq, te, false);
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            int c = __popc((unsigned)(hit >> (8 * x)) & 0xFFu);
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) c += __shfl_xor(c, o, 64);
            if (te == 0 && c) atomicAdd(&cnt[ra0 + join_row(tq, x)], c);
        }
        if (!diag) {
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                int c = __popcll((unsigned long long)(hit & (0x0101010101010101ull << v)));
                c += __shfl_xor(c, 16, 64);
                c += __shfl_xor(c, 32, 64);
                if ((tq & 3) == 0) red[wave][join_row(te, v)] = c;
            }
            __syncthreads();
            if (tid < JT) {
                const int c = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
                if (c) atomicAdd(&cnt[rb0 + tid], c);
            }
        }
    }
}

// core[i] = cnt[i] >= min_samples; every row its own component, no border cluster yet
__global__ __launch_bounds__(256) void join_core_kernel(const int32_t* __restrict__ cnt, int64_t n, int32_t min_samples, uint8_t* __restrict__ core,
                                                        int32_t* __restrict__ parent, int32_t* __restrict__ border) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    core[i] = cnt[i] >= min_samples ? 1 : 0;
    parent[i] = (int32_t)i;
    border[i] = INT32_MAX;
}

// Lock-free union-find over parent[n].  Invariant: parent[x] <= x, and whatever parent[x] has held at any time is an ancestor
// of x from then on -- so a value that another thread has replaced in the meantime is still a correct place to go on from.
// Words shared between workgroups are read with agent-scope loads and changed with atomics only.
__device__ __forceinline__ int32_t uf_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x, with path halving.  x strictly decreases from step to step: at most x steps.
__device__ __forceinline__ int32_t uf_find(int32_t* __restrict__ parent, int32_t x) {
    for (;;) {
        const int32_t p = uf_load(&parent[x]);
        if (p == x) return x;
        const int32_t g = uf_load(&parent[p]);
        if (g == p) return p;
        atomicMin(&parent[x], g);   // (g < p: the minimum keeps parent[x] decreasing whatever order the writers arrive in)
        x = g;
    }
}

// joins the sets of a and b; returns the root the two had when it returned.  The larger root is hooked under the smaller
// one, so a component's root is its lowest row.  A compare-and-swap fails only when another thread has hooked `hi` first;
// it returns hi's new parent, which is below hi: the loop goes on from there, and max(a, b) strictly decreases.
__device__ __forceinline__ int32_t uf_unite(int32_t* __restrict__ parent, int32_t a, int32_t b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return a;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const int32_t old = atomicCAS(&parent[hi], hi, lo);
        if (old == hi) return lo;
        a = old;
        b = lo;
    }
}

// Every hit pair of two core rows joins their components.  Once per tile the 256 threads look up the roots of the tile's
// 128 + 128 rows into LDS (-1: not a core row, or beyond n); a pair whose two roots are equal costs two LDS reads -- in a
// dense tile nearly all of them.  A root in LDS may be out of date; it is still a row of the right component, and uf_unite
// starts with a find.
template <bool V4>
__global__ __launch_bounds__(256) void join_union_kernel(const float* __restrict__ X, int64_t n, int d, int64_t total, double thr,
                                                         const uint8_t* __restrict__ core, int32_t* __restrict__ parent) {
    __shared__ __attribute__((aligned(16))) float As[JKT][JLD];
    __shared__ __attribute__((aligned(16))) float Bs[JKT][JLD];
    __shared__ int rt[2 * JT];
    const int tid = threadIdx.x, tq = tid >> 4, te = tid & 15;
    for (int64_t t = blockIdx.x; t < total; t += gridDim.x) {
        int64_t ta, tb;
        join_tile_of(t, ta, tb);
        const int64_t ra0 = ta * JT, rb0 = tb * JT;
        jf2 acc[8][4];
        join_tile<V4>(X, n, X, n, d, ra0, rb0, As, Bs, acc, tid);
        uint64_t hit = join_hits(acc, ra0, rb0, n, thr, tq, te, true);
        if (!__syncthreads_or(hit != 0ull)) continue;   // most tiles of a sparse matrix: nothing to look up (the barrier also ends the previous tile's reads of rt)
        const bool diag = ta == tb;
        const int64_t row = tid < JT ? ra0 + tid : rb0 + tid - JT;
        rt[tid] = (row < n && !(diag && tid >= JT) && core[row]) ? uf_find(parent, (int32_t)row) : -1;
        __syncthreads();
        const int boff = diag ? 0 : JT;
        for (; hit; hit &= hit - 1ull) {
            const int b = __ffsll((unsigned long long)hit) - 1;
            const int ia = join_row(tq, b >> 3), ib = boff + join_row(te, b & 7);
            const int32_t a = rt[ia], c = rt[ib];
            if (a >= 0 && c >= 0 && a != c) rt[ia] = rt[ib] = uf_unite(parent, a, c);
        }
    }
}

// parent[i] = the root of i (no union runs beside this kernel: the roots are fixed, and every value written is a root)
__global__ __launch_bounds__(256) void join_flatten_kernel(int32_t* __restrict__ parent, const uint8_t* __restrict__ core, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !core[i]) return;
    int32_t x = (int32_t)i;
    for (int32_t p; (p = uf_load(&parent[x])) != x;) x = p;
    __hip_atomic_store(&parent[i], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// border[i] = the lowest root among the core rows within the radius of the non-core row i (there are fewer than min_samples
// of them per row: one atomic per such pair)
template <bool V4>
__global__ __launch_bounds__(256) void join_border_kernel(const float* __restrict__ X, int64_t n, int d, int64_t total, double thr,
                                                          const uint8_t* __restrict__ core, const int32_t* __restrict__ parent, int32_t* __restrict__ border) {
    __shared__ __attribute__((aligned(16))) float As[JKT][JLD];
    __shared__ __attribute__((aligned(16))) float Bs[JKT][JLD];
    __shared__ int rt[2 * JT];
    const int tid = threadIdx.x, tq = tid >> 4, te = tid & 15;
    for (int64_t t = blockIdx.x; t < total; t += gridDim.x) {
        int64_t ta, tb;
        join_tile_of(t, ta, tb);
        const int64_t ra0 = ta * JT, rb0 = tb * JT;
        jf2 acc[8][4];
        join_tile<V4>(X, n, X, n, d, ra0, rb0, As, Bs, acc, tid);
        uint64_t hit = join_hits(acc, ra0, rb0, n, thr, tq, te, true);
        if (!__syncthreads_or(hit != 0ull)) continue;
        const bool diag = ta == tb;
        const int64_t row = tid < JT ? ra0 + tid : rb0 + tid - JT;
        rt[tid] = (row < n && !(diag && tid >= JT) && core[row]) ? parent[row] : -1;
        __syncthreads();
        const int boff = diag ? 0 : JT;
        for (; hit; hit &= hit - 1ull) {
            const int b = __ffsll((unsigned long long)hit) - 1;
            const int ja = join_row(tq, b >> 3), jb = join_row(te, b & 7);
            const int32_t a = rt[ja], c = rt[boff + jb];
            if (a >= 0 && c < 0) atomicMin(&border[rb0 + jb], a);
            if (c >= 0 && a < 0) atomicMin(&border[ra0 + ja], c);
        }
    }
}

// rank[i] = the number of roots (core rows with parent[i] == i) below row i; *n_clusters = the number of roots.  One workgroup
// walks the rows 8192 at a time with a running carry: O(n) reads beside the O(n^2 d) of the passes above.
constexpr int JRANK_PER = 8;
__global__ __launch_bounds__(1024) void join_rank_kernel(const int32_t* __restrict__ parent, const uint8_t* __restrict__ core, int64_t n,
                                                         int32_t* __restrict__ rank, int32_t* __restrict__ n_clusters) {
    __shared__ int wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int carry = 0;
    for (int64_t base = 0; base < n; base += 1024 * JRANK_PER) {
        const int64_t i0 = base + (int64_t)tid * JRANK_PER;
        int f[JRANK_PER], s = 0;
#pragma unroll
        for (int u = 0; u < JRANK_PER; ++u) {
            const int64_t i = i0 + u;
            f[u] = (i < n && core[i] && parent[i] == (int32_t)i) ? 1 : 0;
            s += f[u];
        }
        const int inc = wave_incl_sum_i(s, lane);
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        int below = 0, all = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int v = wsum[k];
            below += k < w ? v : 0;
            all += v;
        }
        int ex = carry + below + inc - s;
#pragma unroll
        for (int u = 0; u < JRANK_PER; ++u) {
            const int64_t i = i0 + u;
            if (i < n) rank[i] = ex;
            ex += f[u];
        }
        carry += all;
        __syncthreads();   // wsum is rewritten by the next round
    }
    if (tid == 0) *n_clusters = carry;
}

// sklearn's numbering: a cluster's label is the rank of its root (its lowest core row) among the roots; a core row takes its
// root's label, a non-core row that of the lowest root within its radius, or -1 (noise)
__global__ __launch_bounds__(256) void join_labels_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ border, const uint8_t* __restrict__ core,
                                                          const int32_t* __restrict__ rank, int64_t n, int32_t* __restrict__ labels) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t r = core[i] ? parent[i] : border[i];
    labels[i] = r == INT32_MAX ? -1 : rank[r];
}

inline int64_t join_tiles(int64_t n) {
    const int64_t nt = (n + JT - 1) / JT;
    return nt * (nt + 1) / 2;
}

// the walks; both use the caller's base as it is.  join_nearest: one 64-bit key per row, at the base; join_dbscan: cnt (later the
// roots' ranks) | parent | border, int32 [n] each
inline int64_t nearest_work_bytes(int64_t n) { Layout l(8); l.take(n, 8); return l.end(); }
struct DbscanLayout { int64_t cnt, parent, border, total; };
inline DbscanLayout dbscan_layout(int64_t n) { Layout l(4); return DbscanLayout{l.take(n, 4), l.take(n, 4), l.take(n, 4), l.end()}; }   // (a braced list is evaluated in order)

}  // namespace kge

using namespace kge;

extern "C" int amdkge_join_nearest(const float* d_x, int64_t n, int32_t d, float* d_dist, int32_t* d_idx, float* d_max, void* d_work, void* stream) {
    if (n < 0 || n > 0x7FFFFFFFll || d < 1) return set_error(AMDKGE_EINVAL, "join_nearest: bad sizes (0 <= n <= 2^31 - 1, d >= 1)");
    if (!d_max || (n > 0 && (!d_x || !d_dist || !d_idx || !d_work))) return set_error(AMDKGE_EINVAL, "join_nearest: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(d_max, 0, sizeof(float), st);
    if (e != hipSuccess) return set_error_hip(e, "join_nearest: hipMemsetAsync");
    if (n == 0) return AMDKGE_OK;
    unsigned long long* keys = (unsigned long long*)d_work;
    e = hipMemsetAsync(keys, 0xFF, (size_t)nearest_work_bytes(n), st);
    if (e != hipSuccess) return set_error_hip(e, "join_nearest: hipMemsetAsync");
    const int64_t total = join_tiles(n);
    const dim3 grid((unsigned)(total < JOIN_MAX_BLOCKS ? total : JOIN_MAX_BLOCKS));
    if (d % 4 == 0 && ((uintptr_t)d_x & 15u) == 0)
        hipLaunchKernelGGL(join_nearest_kernel<true>, grid, dim3(256), 0, st, d_x, n, (int)d, total, keys, (unsigned int*)d_max);
    else
        hipLaunchKernelGGL(join_nearest_kernel<false>, grid, dim3(256), 0, st, d_x, n, (int)d, total, keys, (unsigned int*)d_max);
    int rc = check_launch("join_nearest");
    if (rc != AMDKGE_OK) return rc;
    hipLaunchKernelGGL(join_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, keys, n, d_dist, d_idx);
    return check_launch("join_nearest keys");
}

extern "C" int amdkge_join_radius(const float* d_x, int64_t n, int32_t d, double thr, int32_t* d_pairs, int64_t cap, int64_t* d_count, void* stream) {
    if (n < 0 || n > 0x7FFFFFFFll || d < 1 || cap < 0) return set_error(AMDKGE_EINVAL, "join_radius: bad sizes (0 <= n <= 2^31 - 1, d >= 1, cap >= 0)");
    if (thr != thr) return set_error(AMDKGE_EINVAL, "join_radius: threshold is NaN");
    if (!d_count || (cap > 0 && !d_pairs) || (n > 0 && !d_x)) return set_error(AMDKGE_EINVAL, "join_radius: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(d_count, 0, sizeof(int64_t), st);
    if (e != hipSuccess) return set_error_hip(e, "join_radius: hipMemsetAsync");
    if (n < 2) return AMDKGE_OK;
    const int64_t total = join_tiles(n);
    const dim3 grid((unsigned)(total < JOIN_MAX_BLOCKS ? total : JOIN_MAX_BLOCKS));
    if (d % 4 == 0 && ((uintptr_t)d_x & 15u) == 0)
        hipLaunchKernelGGL(join_radius_kernel<true>, grid, dim3(256), 0, st, d_x, n, (int)d, total, thr, d_pairs, cap, (unsigned long long*)d_count);
    else
        hipLaunchKernelGGL(join_radius_kernel<false>, grid, dim3(256), 0, st, d_x, n, (int)d, total, thr, d_pairs, cap, (unsigned long long*)d_count);
    return check_launch("join_radius");
}

extern "C" int64_t amdkge_join_dbscan_workspace_bytes(int64_t n) {
    if (n < 0 || n > 0x7FFFFFFFll) return -1;
    return dbscan_layout(n).total;
}

extern "C" int amdkge_join_dbscan(const float* d_x, int64_t n, int32_t d, double thr, int32_t min_samples, int32_t* d_labels, uint8_t* d_core,
                                  int32_t* d_n_clusters, void* d_work, void* stream) {
    if (n < 0 || n > 0x7FFFFFFFll || d < 1 || min_samples < 1)
        return set_error(AMDKGE_EINVAL, "join_dbscan: bad sizes (0 <= n <= 2^31 - 1, d >= 1, min_samples >= 1)");
    if (thr != thr) return set_error(AMDKGE_EINVAL, "join_dbscan: threshold is NaN");
    if (!d_n_clusters || (n > 0 && (!d_x || !d_labels || !d_core || !d_work))) return set_error(AMDKGE_EINVAL, "join_dbscan: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        const hipError_t e = hipMemsetAsync(d_n_clusters, 0, sizeof(int32_t), st);
        return e == hipSuccess ? AMDKGE_OK : set_error_hip(e, "join_dbscan: hipMemsetAsync");
    }
    const DbscanLayout wl = dbscan_layout(n);
    char* w = (char*)d_work;
    int32_t *cnt = (int32_t*)(w + wl.cnt), *parent = (int32_t*)(w + wl.parent), *border = (int32_t*)(w + wl.border);
    const hipError_t e = hipMemsetAsync(cnt, 0, (size_t)n * sizeof(int32_t), st);
    if (e != hipSuccess) return set_error_hip(e, "join_dbscan: hipMemsetAsync");
    const int64_t total = join_tiles(n);
    const dim3 grid((unsigned)(total < JOIN_MAX_BLOCKS ? total : JOIN_MAX_BLOCKS)), rows((unsigned)((n + 255) / 256));
    const bool v4 = d % 4 == 0 && ((uintptr_t)d_x & 15u) == 0;
    int rc;
    if (v4) hipLaunchKernelGGL(join_count_kernel<true>, grid, dim3(256), 0, st, d_x, n, (int)d, total, thr, cnt);
    else hipLaunchKernelGGL(join_count_kernel<false>, grid, dim3(256), 0, st, d_x, n, (int)d, total, thr, cnt);
    if ((rc = check_launch("join_dbscan count")) != AMDKGE_OK) return rc;
    hipLaunchKernelGGL(join_core_kernel, rows, dim3(256), 0, st, cnt, n, min_samples, d_core, parent, border);
    if ((rc = check_launch("join_dbscan core")) != AMDKGE_OK) return rc;
    if (v4) hipLaunchKernelGGL(join_union_kernel<true>, grid, dim3(256), 0, st, d_x, n, (int)d, total, thr, d_core, parent);
    else hipLaunchKernelGGL(join_union_kernel<false>, grid, dim3(256), 0, st, d_x, n, (int)d, total, thr, d_core, parent);
    if ((rc = check_launch("join_dbscan union")) != AMDKGE_OK) return rc;
    hipLaunchKernelGGL(join_flatten_kernel, rows, dim3(256), 0, st, parent, d_core, n);
    if ((rc = check_launch("join_dbscan flatten")) != AMDKGE_OK) return rc;
    if (min_samples > 1) {   // (min_samples == 1: every row with a hit, itself included, is a core row -- no border rows)
        if (v4) hipLaunchKernelGGL(join_border_kernel<true>, grid, dim3(256), 0, st, d_x, n, (int)d, total, thr, d_core, parent, border);
        else hipLaunchKernelGGL(join_border_kernel<false>, grid, dim3(256), 0, st, d_x, n, (int)d, total, thr, d_core, parent, border);
        if ((rc = check_launch("join_dbscan border")) != AMDKGE_OK) return rc;
    }
    hipLaunchKernelGGL(join_rank_kernel, dim3(1), dim3(1024), 0, st, parent, d_core, n, cnt, d_n_clusters);
    if ((rc = check_launch("join_dbscan rank")) != AMDKGE_OK) return rc;
    hipLaunchKernelGGL(join_labels_kernel, rows, dim3(256), 0, st, parent, border, d_core, cnt, n, d_labels);
    return check_launch("join_dbscan labels");
}
