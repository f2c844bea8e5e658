// Lloyd's k-means over the rows of a dense fp32 matrix X [n, d]: the device side of discovery.KMeans, the estimator find_clusters'
// documented use (the reference's discovery/discovery.py:614-651 and its tutorials: KMeans(n_clusters=6, n_init=100, max_iter=500))
// runs with.  Everything carries a leading `runs` dimension -- centres [runs, k, d], labels and mind2 [runs, n] --, so the independent
// restarts of one fit advance in lock-step and share every launch: at the sizes of an embedding table a single restart is bound by
// launch latency.
//
// One iteration is four launches:
//   assign    label = argmin_c d2(x_i, C_c) and mind2 per run and row, on the join's tile routine (kge_join_tile.h): d2 is the same
//             declared fp32 fma chain over the columns, the argmin goes through join_key / umin64 (equal distances: the lowest
//             centre).  Also the number of rows whose label changed (an integer atomic) and a partial sum of mind2 per row block.
//   update    per (run, row block, 256-column chunk) the sums of the rows by label, every wave walking its block's rows in row
//             order with one column per lane: partials P[run][block][k][d], no floating-point atomics.  Label histograms -> counts.
//   means     centre = (fp32 sum of the partials over the blocks, in block order) / count; a centre without rows keeps its value.
//   control   shift2 and inertia as fixed-order fp64 sums, n_iter += 1, done = 1 when no label changed (after the first iteration),
//             else done = 2 when shift2 <= tol_abs: sklearn's Lloyd loop.
// Every kernel skips a run whose done != 0, so a call enqueues several iterations with no host round trip.  rows_per_block and every
// summation order depend on n (and k, d) alone: a run's result does not depend on `runs` nor on how its iterations are spread over
// calls -- bit for bit.
#include "kge_join_tile.h"

namespace kge {

constexpr int KM_COLS = 256;      // update: columns per workgroup (64 per wave, one per lane)
constexpr int KM_KR = 32;         // update: centres per pass over the block's rows (KM_KR * KM_COLS floats of LDS = 32 KiB: five workgroups per CU)
constexpr int KM_AHEAD = 8;       // update: rows whose loads are in flight together
constexpr int KM_MAX_Y = 65535;   // grid.y / grid.z bound: the kernels stride over what lies beyond

// rows per update block: a function of n alone (at most 256 blocks of at least 256 rows)
__host__ __device__ inline int64_t km_rows_per_block(int64_t n) {
    const int64_t r = (n + 255) / 256;
    return r > 256 ? r : 256;
}
inline int64_t km_update_blocks(int64_t n) { return n ? (n + km_rows_per_block(n) - 1) / km_rows_per_block(n) : 0; }
inline int64_t km_assign_blocks(int64_t n) { return (n + JT - 1) / JT; }
inline int64_t km_means_blocks(int64_t k, int64_t d) { return (k * d + 255) / 256; }

// the sum of the workgroup's 256 values in a fixed tree: the same bits whatever else runs
__device__ __forceinline__ double km_block_sum(double v, double* sh, int tid) {
    __syncthreads();   // sh is no longer read
    sh[tid] = v;
    __syncthreads();
#pragma unroll
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) sh[tid] += sh[tid + o];
        __syncthreads();
    }
    return sh[0];
}

// centre tile widths: CT centres against JT rows per tile.  CT = 128 is join_tile itself; the narrow tiles keep its staging and its
// chain (a scalar subtract and fma per pair and column, in column order: the same roundings as the packed form) with TC threads
// across the centres, RC centres and RX rows per thread.
template <int CT> struct KmTile {
    static constexpr int TC = CT == 128 ? 16 : CT == 32 ? 8 : 2;
    static constexpr int RC = CT / TC;
    static constexpr int RX = JT / (256 / TC);
};

// skip: 1 = runs with done != 0 (an iteration), 2 = runs with done == 1 (the refresh after a tolerance stop), 0 = none
__device__ __forceinline__ bool km_skipped(const int32_t* __restrict__ state, int run, int skip) {
    if (!state || !skip) return false;
    const int done = state[4 * run + 1];
    return skip == 1 ? done != 0 : done == 1;
}

template <bool V4, int CT>
__global__ __launch_bounds__(256) void kmeans_assign_kernel(const float* __restrict__ X, int64_t n, int d, const float* __restrict__ C, int k, int runs,
                                                            int32_t* __restrict__ labels, float* __restrict__ mind2, const int32_t* __restrict__ state, int skip,
                                                            int32_t* __restrict__ changed_acc, double* __restrict__ inert_part) {
    using T = KmTile<CT>;
    constexpr int TC = T::TC, RC = T::RC, RX = T::RX, BLD = CT + 4;
    __shared__ __attribute__((aligned(16))) float As[JKT][JLD];
    __shared__ __attribute__((aligned(16))) float Bs[JKT][BLD];
    __shared__ float red[JT];
    const int tid = threadIdx.x, tq = tid / TC, te = tid % TC, lane = tid & 63;
    const int64_t r0 = (int64_t)blockIdx.x * JT;
    for (int run = blockIdx.y; run < runs; run += gridDim.y) {
        if (km_skipped(state, run, skip)) continue;   // (the same for the whole workgroup)
        const float* Cr = C + (int64_t)run * k * d;
        unsigned long long m[RX];
#pragma unroll
        for (int x = 0; x < RX; ++x) m[x] = ~0ull;
        for (int c0 = 0; c0 < k; c0 += CT) {
            if constexpr (CT == JT) {
                jf2 acc[8][4];
                join_tile<V4>(X, n, Cr, (int64_t)k, d, r0, (int64_t)c0, As, Bs, acc, tid);
#pragma unroll
                for (int x = 0; x < 8; ++x)
#pragma unroll
                    for (int v = 0; v < 8; ++v) {
                        const int c = c0 + join_row(te, v);
                        if (c < k) m[x] = umin64(m[x], join_key(join_val(acc, x, v), c));
                    }
            } else {
                float acc[RX][RC];
#pragma unroll
                for (int x = 0; x < RX; ++x)
#pragma unroll
                    for (int y = 0; y < RC; ++y) acc[x][y] = 0.f;
                for (int k0 = 0; k0 < d; k0 += JKT) {
                    __syncthreads();   // the previous stage (or tile) is no longer read
                    join_stage<V4>(X, n, d, r0, k0, As, tid);
                    if (tid < 2 * CT) join_stage<V4, BLD>(Cr, (int64_t)k, d, (int64_t)c0, k0, Bs, tid);
                    __syncthreads();
#pragma unroll
                    for (int kk = 0; kk < JKT; ++kk) {
                        float av[RX], bv[RC];
#pragma unroll
                        for (int x = 0; x < RX; ++x) av[x] = As[kk][tq * RX + x];
#pragma unroll
                        for (int y = 0; y < RC; ++y) bv[y] = Bs[kk][te * RC + y];
#pragma unroll
                        for (int x = 0; x < RX; ++x)
#pragma unroll
                            for (int y = 0; y < RC; ++y) {
                                const float dd = av[x] - bv[y];
                                acc[x][y] = __builtin_fmaf(dd, dd, acc[x][y]);
                            }
                    }
                }
#pragma unroll
                for (int x = 0; x < RX; ++x)
#pragma unroll
                    for (int y = 0; y < RC; ++y) {
                        const int c = c0 + te * RC + y;
                        if (c < k) m[x] = umin64(m[x], join_key(acc[x][y], c));
                    }
            }
        }
        // over the TC threads that share a row (neighbouring lanes of one wave)
        int ch = 0;
#pragma unroll
        for (int x = 0; x < RX; ++x) {
            unsigned long long v = m[x];
#pragma unroll
            for (int o = 1; o < TC; o <<= 1) v = umin64(v, __shfl_xor(v, o, 64));
            if (te == 0) {
                const int lrow = CT == JT ? join_row(tq, x) : tq * RX + x;
                const int64_t row = r0 + lrow;
                float val = 0.f;
                if (row < n) {
                    const int32_t lab = (int32_t)(uint32_t)v;
                    val = __uint_as_float((uint32_t)(v >> 32));
                    const int64_t at = (int64_t)run * n + row;
                    ch += labels[at] != lab ? 1 : 0;
                    labels[at] = lab;
                    if (mind2) mind2[at] = val;
                }
                red[lrow] = val;
            }
        }
        if (changed_acc) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) ch += __shfl_xor(ch, o, 64);
            if (lane == 0 && ch) atomicAdd(&changed_acc[run], ch);
        }
        __syncthreads();
        if (inert_part && tid < 64) {   // the block's 128 values in a fixed tree, in fp64
            double s = (double)red[tid] + (double)red[tid + 64];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            if (tid == 0) inert_part[(int64_t)run * gridDim.x + blockIdx.x] = s;
        }
        // (red is written again behind the next run's tile barriers, which wave 0 passes after the reads above)
    }
}

// P[run][b][c][col] = the sum of x[i, col] over the rows i of block b with label c, added in row order.  Each thread owns one column;
// acc[c][column] in LDS is its private, label-indexed accumulator (lanes are columns: no two threads share a word).  counts_acc[run][c]
// += the block's label histogram (chunk 0 only).
__global__ __launch_bounds__(256) void kmeans_update_kernel(const float* __restrict__ X, int64_t n, int d, int k, int runs, int64_t rpb,
                                                            const int32_t* __restrict__ labels, const int32_t* __restrict__ state, float* __restrict__ P,
                                                            int32_t* __restrict__ counts_acc) {
    extern __shared__ __attribute__((aligned(16))) float km_acc[];   // [min(k, KM_KR)][KM_COLS]
    __shared__ int hist[KM_KR];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x, B = gridDim.x;
    const int64_t i0 = b * rpb, i1 = i0 + rpb < n ? i0 + rpb : n;
    const int chunks = (d + KM_COLS - 1) / KM_COLS;
    for (int run = blockIdx.z; run < runs; run += gridDim.z) {
        if (km_skipped(state, run, 1)) continue;
        const int32_t* lab = labels + (int64_t)run * n;
        for (int chunk = blockIdx.y; chunk < chunks; chunk += gridDim.y) {
            const int col = chunk * KM_COLS + tid;
            const bool live = col < d;
            for (int c0 = 0; c0 < k; c0 += KM_KR) {
                const int kr = k - c0 < KM_KR ? k - c0 : KM_KR;
                for (int c = 0; c < kr; ++c) km_acc[c * KM_COLS + tid] = 0.f;
                for (int64_t i = i0; i < i1; i += KM_AHEAD) {
                    int l[KM_AHEAD];
                    float v[KM_AHEAD];
#pragma unroll
                    for (int u = 0; u < KM_AHEAD; ++u) {   // the loads of KM_AHEAD rows first ...
                        const bool in = i + u < i1;
                        l[u] = in ? lab[i + u] : -1;
                        v[u] = in && live ? X[(i + u) * (int64_t)d + col] : 0.f;
                    }
#pragma unroll
                    for (int u = 0; u < KM_AHEAD; ++u) {   // ... then their additions, in row order
                        const unsigned r = (unsigned)(l[u] - c0);
                        if (r < (unsigned)kr) km_acc[r * KM_COLS + tid] += v[u];
                    }
                }
                if (live)
                    for (int c = 0; c < kr; ++c) P[(((int64_t)run * B + b) * k + c0 + c) * d + col] = km_acc[c * KM_COLS + tid];
                if (chunk == 0) {
                    __syncthreads();   // the previous histogram has been read
                    if (tid < KM_KR) hist[tid] = 0;
                    __syncthreads();
                    for (int64_t i = i0 + tid; i < i1; i += 256) {
                        const unsigned r = (unsigned)(lab[i] - c0);
                        if (r < (unsigned)kr) atomicAdd(&hist[r], 1);
                    }
                    __syncthreads();
                    if (tid < kr && hist[tid]) atomicAdd(&counts_acc[(int64_t)run * k + c0 + tid], hist[tid]);
                }
            }
        }
    }
}

// centre[c][col] = (sum over b = 0 .. B-1, in that order, of P[run][b][c][col]) / counts_acc[run][c] -- an IEEE divide; a centre with no
// rows keeps its value.  shift_part[run][block] = the block's sum of (new - old)^2 in fp64.
__global__ __launch_bounds__(256) void kmeans_means_kernel(float* __restrict__ C, int k, int d, int runs, int64_t B, const float* __restrict__ P,
                                                           const int32_t* __restrict__ counts_acc, const int32_t* __restrict__ state, double* __restrict__ shift_part) {
    __shared__ double sh[256];
    const int tid = threadIdx.x;
    const int64_t kd = (int64_t)k * d, e = (int64_t)blockIdx.x * 256 + tid;
    for (int run = blockIdx.y; run < runs; run += gridDim.y) {
        if (km_skipped(state, run, 1)) continue;
        double s2 = 0.0;
        if (e < kd) {
            const float* p = P + (int64_t)run * B * kd + e;
            float sum = 0.f;
            for (int64_t b = 0; b < B; ++b) sum += p[b * kd];
            const int32_t cnt = counts_acc[(int64_t)run * k + e / d];
            const float old = C[(int64_t)run * kd + e];
            const float nw = cnt > 0 ? sum / (float)cnt : old;
            C[(int64_t)run * kd + e] = nw;
            const double df = (double)nw - (double)old;
            s2 = df * df;
        }
        s2 = km_block_sum(s2, sh, tid);
        if (tid == 0) shift_part[(int64_t)run * gridDim.x + blockIdx.x] = s2;
    }
}

// the 256 threads' strided partial sums of v[0 .. m), then the fixed tree: one order for a given m
__device__ __forceinline__ double km_sum_fixed(const double* __restrict__ v, int64_t m, double* sh, int tid) {
    double s = 0.0;
    for (int64_t j = tid; j < m; j += 256) s += v[j];
    return km_block_sum(s, sh, tid);
}

// One workgroup per run: the iteration's bookkeeping (sklearn's Lloyd loop).  state[run] = {n_iter, done, changed, reserved}.
__global__ __launch_bounds__(256) void kmeans_control_kernel(int k, int64_t FB, int64_t NB, double tol_abs, const double* __restrict__ shift_part,
                                                             const double* __restrict__ inert_part, int32_t* __restrict__ counts_acc, int32_t* __restrict__ counts,
                                                             int32_t* __restrict__ changed_acc, int32_t* __restrict__ state, double* __restrict__ inertia) {
    __shared__ double sh[256];
    const int tid = threadIdx.x, run = blockIdx.x;
    if (km_skipped(state, run, 1)) return;
    const double shift2 = km_sum_fixed(shift_part + (int64_t)run * FB, FB, sh, tid);
    const double in = km_sum_fixed(inert_part + (int64_t)run * NB, NB, sh, tid);
    for (int c = tid; c < k; c += 256) {   // the finished iteration's counts stay readable; the accumulators start the next one at 0
        counts[(int64_t)run * k + c] = counts_acc[(int64_t)run * k + c];
        counts_acc[(int64_t)run * k + c] = 0;
    }
    if (tid == 0) {
        const int32_t n_iter = state[4 * run] + 1, changed = changed_acc[run];
        changed_acc[run] = 0;
        state[4 * run] = n_iter;
        state[4 * run + 2] = changed;
        state[4 * run + 1] = (n_iter > 1 && changed == 0) ? 1 : (shift2 <= tol_abs ? 2 : 0);
        inertia[run] = in;
    }
}

// inertia[run] of the labels a refresh has just written (runs with done == 1 keep theirs)
__global__ __launch_bounds__(256) void kmeans_inertia_kernel(int64_t NB, const double* __restrict__ inert_part, const int32_t* __restrict__ state,
                                                             double* __restrict__ inertia) {
    __shared__ double sh[256];
    const int tid = threadIdx.x, run = blockIdx.x;
    if (km_skipped(state, run, 2)) return;
    const double in = km_sum_fixed(inert_part + (int64_t)run * NB, NB, sh, tid);
    if (tid == 0) inertia[run] = in;
}

// workspace, every part on an 8-byte boundary: [counts_acc int32 runs k | changed_acc int32 runs | counts int32 runs k | shift_part f64 runs FB |
//             inert_part f64 runs NB | P f32 runs B k d]
struct KmWork {
    int64_t counts_acc, counts, changed_acc, shift_part, inert_part, P, bytes;
};
inline bool km_layout(int64_t n, int64_t d, int64_t k, int64_t runs, KmWork& w) {
    const int64_t B = km_update_blocks(n), NB = km_assign_blocks(n);
    int64_t kd, rk, FB;
    if (__builtin_mul_overflow(k, d, &kd) || __builtin_mul_overflow(runs, k, &rk)) return false;
    FB = (kd + 255) / 256;
    int64_t rFB, rNB, rB, rBkd;
    if (__builtin_mul_overflow(runs, FB, &rFB) || __builtin_mul_overflow(runs, NB, &rNB) || __builtin_mul_overflow(runs, B, &rB) ||
        __builtin_mul_overflow(rB, kd, &rBkd))
        return false;
    Layout l(8);   // (the caller's base is used as it is)
    w.counts_acc = l.take(rk, 4); w.changed_acc = l.take(runs, 4); w.counts = l.take(rk, 4);
    w.shift_part = l.take(rFB, 8); w.inert_part = l.take(rNB, 8);
    w.P = l.take(rBkd, 4); w.bytes = l.next();
    return w.bytes >= 0;
}

inline bool km_sizes_ok(int64_t n, int32_t d, int32_t k, int32_t runs) { return n >= 0 && n <= 0x7FFFFFFFll && d >= 1 && k >= 1 && runs >= 1; }

// one assignment pass over all runs; the tile width from k
inline int km_launch_assign(const float* d_x, int64_t n, int d, const float* d_centres, int k, int runs, int32_t* d_labels, float* d_mind2,
                            const int32_t* state, int skip, int32_t* changed_acc, double* inert_part, hipStream_t st) {
    const dim3 grid((unsigned)km_assign_blocks(n), (unsigned)(runs < KM_MAX_Y ? runs : KM_MAX_Y));
    const bool v4 = d % 4 == 0 && ((uintptr_t)d_x & 15u) == 0 && ((uintptr_t)d_centres & 15u) == 0;
#define KM_ASSIGN(V4, CT) \
    hipLaunchKernelGGL((kmeans_assign_kernel<V4, CT>), grid, dim3(256), 0, st, d_x, n, d, d_centres, k, runs, d_labels, d_mind2, state, skip, changed_acc, inert_part)
    if (k <= 8) { if (v4) KM_ASSIGN(true, 8); else KM_ASSIGN(false, 8); }
    else if (k <= 32) { if (v4) KM_ASSIGN(true, 32); else KM_ASSIGN(false, 32); }
    else { if (v4) KM_ASSIGN(true, 128); else KM_ASSIGN(false, 128); }
#undef KM_ASSIGN
    return check_launch("kmeans assign");
}

}  // namespace kge

using namespace kge;

extern "C" int64_t amdkge_kmeans_workspace_bytes(int64_t n, int32_t d, int32_t k, int32_t runs) {
    if (!km_sizes_ok(n, d, k, runs)) return -1;
    if (n == 0) return 0;
    KmWork w;
    return km_layout(n, d, k, runs, w) ? w.bytes : -1;
}

extern "C" int amdkge_kmeans_assign(const float* d_x, int64_t n, int32_t d, const float* d_centres, int32_t k, int32_t runs, int32_t* d_labels,
                                    float* d_mind2, void* stream) {
    if (!km_sizes_ok(n, d, k, runs)) return set_error(AMDKGE_EINVAL, "kmeans_assign: bad sizes (0 <= n <= 2^31 - 1, d >= 1, k >= 1, runs >= 1)");
    if (!d_centres || (n > 0 && (!d_x || !d_labels))) return set_error(AMDKGE_EINVAL, "kmeans_assign: NULL pointer");
    if (n == 0) return AMDKGE_OK;
    return km_launch_assign(d_x, n, d, d_centres, k, runs, d_labels, d_mind2, nullptr, 0, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int amdkge_kmeans_lloyd(const float* d_x, int64_t n, int32_t d, float* d_centres, int32_t k, int32_t runs, int32_t iters, double tol_abs,
                                   int32_t* d_labels, float* d_mind2, int32_t* d_state, double* d_inertia, void* d_work, void* stream) {
    if (!km_sizes_ok(n, d, k, runs) || iters < 0)
        return set_error(AMDKGE_EINVAL, "kmeans_lloyd: bad sizes (0 <= n <= 2^31 - 1, d >= 1, k >= 1, runs >= 1, iters >= 0)");
    if (!(tol_abs >= 0.0)) return set_error(AMDKGE_EINVAL, "kmeans_lloyd: tol_abs is NaN or negative");
    if (!d_centres || !d_state || !d_inertia || (n > 0 && (!d_x || !d_labels || !d_mind2 || !d_work))) return set_error(AMDKGE_EINVAL, "kmeans_lloyd: NULL pointer");
    if (n == 0) return AMDKGE_OK;
    KmWork w;
    if (!km_layout(n, d, k, runs, w)) return set_error(AMDKGE_EINVAL, "kmeans_lloyd: the workspace size overflows int64");
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)d_work;
    int32_t* counts_acc = (int32_t*)(base + w.counts_acc);
    int32_t* counts = (int32_t*)(base + w.counts);
    int32_t* changed_acc = (int32_t*)(base + w.changed_acc);
    double* shift_part = (double*)(base + w.shift_part);
    double* inert_part = (double*)(base + w.inert_part);
    float* P = (float*)(base + w.P);
    const int64_t NB = km_assign_blocks(n), B = km_update_blocks(n), FB = km_means_blocks(k, d), rpb = km_rows_per_block(n);
    int rc;
    if (iters == 0) {   // the refresh: labels, mind2 and inertia of the centres as they are, for every run that did not stop on equal labels
        if ((rc = km_launch_assign(d_x, n, d, d_centres, k, runs, d_labels, d_mind2, d_state, 2, nullptr, inert_part, st)) != AMDKGE_OK) return rc;
        hipLaunchKernelGGL(kmeans_inertia_kernel, dim3((unsigned)runs), dim3(256), 0, st, NB, inert_part, d_state, d_inertia);
        return check_launch("kmeans inertia");
    }
    // the accumulators start every call at 0 (a finished iteration leaves them so; a workspace fresh from the allocator does not)
    const hipError_t e = hipMemsetAsync(counts_acc, 0, (size_t)(w.counts - w.counts_acc), st);
    if (e != hipSuccess) return set_error_hip(e, "kmeans_lloyd: hipMemsetAsync");
    const int chunks = (d + KM_COLS - 1) / KM_COLS;
    const dim3 ugrid((unsigned)B, (unsigned)(chunks < KM_MAX_Y ? chunks : KM_MAX_Y), (unsigned)(runs < KM_MAX_Y ? runs : KM_MAX_Y));
    const size_t ulds = (size_t)(k < KM_KR ? k : KM_KR) * KM_COLS * sizeof(float);
    const dim3 mgrid((unsigned)FB, (unsigned)(runs < KM_MAX_Y ? runs : KM_MAX_Y));
    for (int it = 0; it < iters; ++it) {
        if ((rc = km_launch_assign(d_x, n, d, d_centres, k, runs, d_labels, d_mind2, d_state, 1, changed_acc, inert_part, st)) != AMDKGE_OK) return rc;
        hipLaunchKernelGGL(kmeans_update_kernel, ugrid, dim3(256), ulds, st, d_x, n, (int)d, (int)k, (int)runs, rpb, d_labels, d_state, P, counts_acc);
        if ((rc = check_launch("kmeans update")) != AMDKGE_OK) return rc;
        hipLaunchKernelGGL(kmeans_means_kernel, mgrid, dim3(256), 0, st, d_centres, (int)k, (int)d, (int)runs, B, P, counts_acc, d_state, shift_part);
        if ((rc = check_launch("kmeans means")) != AMDKGE_OK) return rc;
        hipLaunchKernelGGL(kmeans_control_kernel, dim3((unsigned)runs), dim3(256), 0, st, (int)k, FB, NB, tol_abs, shift_part, inert_part, counts_acc, counts,
                           changed_acc, d_state, d_inertia);
        if ((rc = check_launch("kmeans control")) != AMDKGE_OK) return rc;
    }
    return AMDKGE_OK;
}
