// The 64 x 64 tile of an exact-fp32 matrix product C = A B, shared by the shared-negative step (kge_train_shared.hip:
// shared_gemm_kernel) and the relation objective (kge_train_relpred.hip: relpred_gemm_kernel).
//
// A workgroup of 256 threads owns the tile; wave wv owns the 32 x 32 quadrant (wv & 1, wv >> 1) of its 2 x 2 in one f32x16
// accumulator of v_mfma_f32_32x32x2_f32.  The operands go through LDS in chunks of PKC along the contraction, both stored
// [contraction][tile row or column] with a pitch of PLD floats: As[kk][m] = A[m0 + m][k0 + kk], Bs[kk][n] = B[k0 + kk][n0 + n].
// Elements past a matrix edge are staged as zeros, so every tile shape is one code path; one wave sums each output in a fixed
// order, so a product is deterministic.
//
// What is here is functions of plain values: which element a thread stages, which operand element a lane feeds, which result a
// register holds.  The loops over them (PSTAGE elements, PKC / 2 matrix instructions between two barriers, 16 registers) stay in
// the two kernels with their sources and sinks: a piece that holds a loop is optimised on its own before it is inlined, and the
// kernels' instruction streams then change (scripts/kernel_isa_digest.py shows it).
#pragma once
#include "kge_train_shared.h"

namespace kge {

constexpr int PT = 64;         // tile edge
static_assert(PT == SHARED_TILE, "the driver counts the tiles");
constexpr int PKC = 32;        // contraction chunk
constexpr int PLD = PT + 1;    // LDS row pitch (floats): a chunk staged along the contraction lands on distinct banks
constexpr int PQ = 32;         // edge of a wave's quadrant
constexpr int PSTAGE = 8;      // elements of a PKC x PT chunk per thread

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- staging: element r < PSTAGE of thread tid is T[kk][x], x the tile row (A) or column (B) ----
// As and Bs are stored alike, so the four forms (A along the contraction or along m, B along the contraction or along n) are two maps.
// the operand is contiguous along the contraction (A[m][kk], B^T[n][kk]): 32 consecutive threads read 32 consecutive floats
__device__ __forceinline__ int product_k_kk(int tid) { return tid & 31; }
__device__ __forceinline__ int product_k_x(int tid, int r) { return (tid >> 5) + 8 * r; }
// the operand is contiguous along the tile's own dimension (A^T[kk][m], B[kk][n]): a wave reads 64 consecutive floats
__device__ __forceinline__ int product_x_x(int tid) { return tid & 63; }
__device__ __forceinline__ int product_x_kk(int tid, int r) { return (tid >> 6) + 4 * r; }

// ---- the matrix loop: one instruction takes two contraction steps ----
// Lane l feeds As[kk + product_kh][quadrant row * PQ + product_in_quad] and Bs[kk + product_kh][quadrant column * PQ +
// product_in_quad] for kk = 0, 2 .. PKC - 2 (lanes 32.. hold the odd step).  The barrier before the loop closes the staging, the
// one behind it keeps the next chunk's staging off the rows still being read.  A kernel asks for the quadrant where it uses it
// and does not keep it in a local: only so does the compiler form the same expressions as for the index written out.
__device__ __forceinline__ int product_quad_row(int wv) { return wv & 1; }
__device__ __forceinline__ int product_quad_col(int wv) { return wv >> 1; }
__device__ __forceinline__ int product_in_quad(int lane) { return lane & 31; }
__device__ __forceinline__ int product_kh(int lane) { return lane >> 5; }

// ---- results: register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31 of the wave's quadrant ----
__device__ __forceinline__ int product_row(int m0, int qr, int lane, int r) { return m0 + qr * PQ + (r & 3) + 8 * (r >> 2) + 4 * product_kh(lane); }
__device__ __forceinline__ int product_col(int n0, int qc, int lane) { return n0 + qc * PQ + product_in_quad(lane); }

// The ComplEx / HolE score of the rows S, P, O (ks units per half as stored, k live) in the reference's own operation order
// (ComplEx.py:58-62, score_unit of kge_device.h: what amdkge_train_fwdbwd computes on an override row), one lane, serially: what
// a product's FWD result is replaced by where an inf in a table made it non-finite.
__device__ __forceinline__ float cplx_reference_score(const float* S, const float* P, const float* O, int ks, int k) {
    float acc = 0.f;
    for (int u = 0; u < k; ++u) {
        const float s0 = S[u], s1 = S[ks + u], p0 = P[u], p1 = P[ks + u], o0 = O[u], o1 = O[ks + u];
        acc += s0 * (p0 * o0 + p1 * o1) + s1 * (p0 * o1 - p1 * o0);
    }
    return acc;
}

}  // namespace kge
