// What the training units share (kge_train.hip; the owner-computes step: kge_train_tiled.hip, kge_train_stage.hip, kge_train_tile.hip,
// kge_train_direct.hip, kge_train_cols.hip): the staging protocol between the forward kernels and the tile passes (StageEntry,
// block-interleaved row ownership, loss partials, hot rows), the forward kernels' arguments, the loss helpers the forward kernel
// shares with the column-sharded kernels, and the LDS sizes the host plans with.
// A training unit includes this header (or one that starts with it) FIRST: see KGE_FAST_ROTATE.
#pragma once

// RotatE's modulus and its reciprocal in the TRAINING kernels use the hardware v_sqrt_f32 / v_rcp_f32 (1 ulp) instead of the
// correctly rounded libm sequences: the fused kernels are bound by exactly these on RotatE (measured 1.26x on the step);
// loss and gradients stay far inside the 1e-5 relative tolerance of the parity tests.  predict() (kge_score.hip) keeps the
// exact forms; the rank kernels have their own rank_sqrt.  Device functions are inlined per kernel, so the two variants of
// score_unit / grad_unit never meet at link time.
// Defined HERE and nowhere else, ahead of this header's own include of kge_device.h.  A unit that had kge_device.h before (by itself or
// through kge_host.h / kge_opt.h) compiled the exact forms: it stops at the static_assert below instead of training with them.
#define KGE_FAST_ROTATE 1

#include "kge_device.h"
#include "kge_host.h"

static_assert(kge::ROTATE_FAST_FORMS, "kge_device.h was included before kge_train_common.h: this unit would train RotatE with the exact sqrt / division forms");

namespace kge {

// one row-gradient contribution, appended by the forward kernel to the bucket of the tile owning row `dest`
struct __attribute__((aligned(16))) StageEntry {
    uint32_t pos;    // positive (index into this launch's batch)
    uint32_t meta;   // role | local row of the tile << 2 [| corruption index << 16: TransE sign codes, see below];
                     // role 0/1 = corruption with object/subject replaced, 2/3 = the positive's own s/o row
    float g;         // dL/dscore * score_sign * score_scale (1 for roles 2, 3)
    uint32_t dest;   // global row id
};

constexpr uint32_t ENTRY_LOCAL_MASK = 0x1FFFu;   // local row (tiles hold at most 4096 rows)
__host__ __device__ __forceinline__ uint32_t entry_local(uint32_t meta) { return (meta >> 2) & ENTRY_LOCAL_MASK; }
// TransE sign codes (one wave per positive).  The gradient of -sum |d| w.r.t. the replaced row is -/+ g sign(d_j): all the
// tile pass needs of corruption j is the SIGN of every unit of d_j = s + p - o, which the forward kernel has in registers when
// it scores the row.  It stores them -- the top byte of each of the lane's four d values packed into one dword, [B][eta][nq]
// dwords -- and the tile pass reads 4 bytes per lane and entry instead of recomputing d_j from three K-float rows (staged
// side copy, relation row, its own row: 2.4 KB per entry at k = 200).  sign(0) = 0 stays exact the slow way: the byte also
// carries the top 7 exponent bits, and an entry with a unit of the model whose |d| is below 2^-125 (zero, or as good as) is
// recomputed by the tile pass in the three-row form.
constexpr int ENTRY_J_SHIFT = 16;                // corruption index (eta <= 65535 when codes are in use)

// Per-block loss partials.  Thousands of blocks adding an fp64 atomic to ONE address serialise at the L2 (measured: 19 of the
// 46 us of a C1 forward kernel, 5 us at C2); spread over LOSS_PARTS cache lines they do not, and a single thread folds the
// partials into the caller's accumulator afterwards (the tile kernel's last workgroup, or loss_fold_kernel on the atomic path).
constexpr int LOSS_PARTS = 64;
constexpr int LOSS_PART_STRIDE = 16;   // doubles

// Hot rows (skewed graphs).  An entity that is the s / o of thousands of positives of one batch would put thousands of entries
// on one row of one tile (one wave adds them one after the other) or, through POS_ATOMIC, thousands of atomic row-adds on the
// same addresses.  Up to HOT_MAX such rows, named by the host, are instead spread over HOT_REPL replica rows: positive i adds
// its s / o gradient row atomically into replica (block index mod HOT_REPL), the owning tile sums the replicas when it flushes
// the row.  Every other row keeps the atomic-free staged path.
// Block-interleaved row ownership of the tile pass: rows are dealt to the tiles in blocks of TILE_RB consecutive rows
// (block b -> tile b % n_tiles).  See tile_backward_kernel.
#ifndef KGE_TILE_RB
#define KGE_TILE_RB 8
#endif
constexpr uint32_t TILE_RB = KGE_TILE_RB;   // (a plan uses fewer when the LDS cannot hold TILE_RB rows: rb = min(TILE_RB, tile_rows))
__host__ __device__ __forceinline__ void tile_of_row(uint32_t row, uint32_t n_tiles, uint32_t rb, uint32_t& tile, uint32_t& local) {
    const uint32_t blk = row / rb;
    tile = blk % n_tiles;
    local = (blk / n_tiles) * rb + row % rb;
}
__host__ __device__ __forceinline__ int64_t row_of_tile(uint32_t tile, uint32_t local, uint32_t n_tiles, uint32_t rb) {
    return ((int64_t)(local / rb) * n_tiles + tile) * rb + local % rb;
}

constexpr int HOT_MAX = 64;
constexpr int HOT_REPL = 16;

struct TrainArgs {
    const float* ent;
    const float* rel;
    const float* rel_cs;     // RotatE, owner-computes path: [R][cos(phase) || sin(phase)] of this step's relation table (rel_phase_kernel);
                             // NULL: the kernel evaluates cos / sin itself (prep_rel)
    const int32_t* triples;
    const int32_t* neg_override;
    float* g_ent;
    float* g_rel;
    double* loss_sum;
    double* loss_parts;      // [LOSS_PARTS] partial sums, 128-byte stride: blocks add here, one thread folds them into loss_sum
    float* pos_scores;
    float* neg_scores;
    int64_t B;
    int eta;
    int k;       // units per half AS STORED (k_pad of the model descriptor, or k for dense rows)
    int K;       // floats per stored row
    int k_live;  // the model's k: units >= k_live of a half are zero padding (only RotatE's gradient needs to know)
    int nq;      // quads per row ( = units / VEC )
    SampleCfg sc;
    ModelConst mc;
    amdkge_loss loss;
    // owner-computes (STAGE) outputs: see kge_train_tiled.hip
    float* stage_rows;       // [B][4][K]: gradient rows of the positive's s and o (unless pos_atomic), then the side rows A, B
    int pos_atomic;          // the positives' own s / o rows go through atomics into g_ent (skewed graphs)
    int sign_off;            // TransE: byte offset of the sign stash in dynamic LDS (see SIGNSTASH in the kernel)
    int ns;                  // staged rows per positive: 4, or 5 in deterministic mode (the relation-row gradient is staged too)
    int det;                 // deterministic mode (AMDKGE_TILED_DETERMINISTIC): no atomics on any gradient
    const uint8_t* hot_map;  // AMDKGE_TILED_HOT_ROWS: byte per entity row, slot + 1 of a hot row, 0 otherwise (NULL: feature off)
    float* hot_buf;          // [HOT_MAX][HOT_REPL][K]: replicas the gradient rows of hot entities are spread over
    uint8_t* touched;        // pos_atomic + lazy optimizer: byte per entity row, set for rows that received an atomic row-add
    uint32_t* sign_codes;    // TransE, one wave per positive: [B][eta][nq] packed sign bytes of d_j (see ENTRY_J_SHIFT); NULL = off
    StageEntry* st_lists;    // [n_tiles][cap] buckets of row-gradient entries, by owning tile
    StageEntry* st_ovf;      // overflow of full buckets
    int* st_counters;        // [(n_tiles + 1) * 32] bucket fill counts (128-byte stride), last = overflow count
    int st_tile_rows, st_n_tiles, st_cap, st_ovf_cap, st_rb;
#ifdef KGE_ABLATE
    int dbg;     // development ablation build only (make EXTRA=-DKGE_ABLATE, env AMDKGE_DEBUG): 1 no neg-row atomics, 2 no s/p/o atomics, 4 no pass 2, 32 no bucket appends, 64 no staged-row stores
#endif
};

// ablation switches exist only in development builds; the release library cannot skip work
#ifdef KGE_ABLATE
#define KGE_DBG(a, bit) (((a).dbg & (bit)) != 0)
#else
#define KGE_DBG(a, bit) false
#endif

// fold the per-block partials into the caller's accumulator and leave them zero (one thread, fixed order)
// (atomic exchanges: the partials may have been written by other CUs of the SAME launch -- the tile kernel's regulariser
// terms -- and must be read from the L2, not from this CU's L1)
// Called by ONE whole wave: lane i takes partial i (LOSS_PARTS == 64), the wave adds them up in a fixed butterfly order.
__device__ __forceinline__ void fold_loss_parts(double* parts, double* loss_sum, int lane, int lane_in_slot = 0) {
    static_assert(LOSS_PARTS == KGE_WAVE, "one partial per lane");
    const unsigned long long old = atomicExch(reinterpret_cast<unsigned long long*>(parts + (size_t)lane * LOSS_PART_STRIDE + lane_in_slot), 0ull);
    double t = __longlong_as_double((long long)old);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    if (lane == 0 && loss_sum && t != 0.0) atomicAdd(loss_sum, t);
}

__device__ __forceinline__ float log_sigmoid(float x) {
    // -softplus(-x), stable on both tails
    return fminf(x, 0.f) - log1pf(expf(-fabsf(x)));
}
__device__ __forceinline__ float sigmoidf(float x) {
    return 1.f / (1.f + expf(-x));
}

// clip_before_exp (loss_functions.py:60-66) = tf.clip_by_value = maximum(minimum(x, 75), -75) built from TensorFlow's NaN-PROPAGATING
// minimum / maximum: a NaN score stays NaN in the loss VALUE.  C's fminf / fmaxf return the other operand instead, which made a NaN
// positive cost a finite eta * log(1 + e^75) = 375 eta.  The GRADIENT through the clip is the exact zero of the
// minimum / maximum masks (less_equal / greater_equal are false for NaN) -- what the `in` range tests beside every clip give.
__device__ __forceinline__ float clip_exp(float x) {
    return (x != x) ? x : fminf(fmaxf(x, -75.f), 75.f);
}
// tf.maximum(h, 0) of the two margin losses (:302-308, :458-464): NaN in the value, zero gradient (greater_equal(NaN, 0) is false)
__device__ __forceinline__ float hinge_nan(float h) {
    return (h != h) ? h : fmaxf(h, 0.f);
}
// A coefficient dL/dscore that a clip or hinge MASK sets to zero.  "Zero coefficient -> no bucket entry for the replaced row" (below,
// STAGE) is valid only while the score's Jacobian is finite: TensorFlow multiplies the exact zero by it, so a positive whose own rows
// hold a NaN hands 0 * NaN = NaN to the replacement rows of its corruptions.  The masked coefficient of a NON-FINITE score (x: the score,
// or the hinge argument it enters) is therefore written as -0.0f: the entry test keeps it (entry_wanted), the tile pass adds (-0) * A --
// NaN exactly where the side row is NaN, nothing elsewhere.  No loss produces -0.0f as a live coefficient.
__device__ __forceinline__ float masked_zero(float x) {
    return (fabsf(x) < INFINITY) ? 0.f : -0.f;
}
// The self-adversarial loss has no mask: its coefficient is COMPUTED, and for a score of -inf (a distance model's corruption that keeps a
// row holding an inf) it is an exact zero -- softmax weight 0 times sigma(-inf) = 0 -- which TensorFlow again multiplies by the Jacobian.
__device__ __forceinline__ float computed_zero(float c, float x) {
    return (c == 0.f) ? masked_zero(x) : c;
}
// coeff: dL/dscore as the loss code left it; g = coeff * score_sign * score_scale.  No entry below fp32's smallest NORMAL number
// (see the forward kernel) unless the coefficient is masked_zero's marker; a NaN coefficient is an entry.
__device__ __forceinline__ bool entry_wanted(float coeff, float g) {
    return !(fabsf(g) < 1.17549435e-38f) || __float_as_uint(coeff) == 0x80000000u;
}

// TransE keeps, per corruption and unit, only sign(s + p - o) for its backward pass (the gradient of |x|): 2 bits per unit,
// one byte per lane and quad, stashed in LDS by the scoring pass so that the replacement rows are read from memory ONCE
// (measured at the C2 shape, k = 200: forward kernel 66.7 -> 54 us).
__host__ __device__ inline size_t sign_stash_bytes(int model, int eta, int CH) {
    return model == AMDKGE_TRANSE ? (size_t)256 * eta * CH : 0;
}

__host__ __device__ inline size_t slot_lds_bytes(int eta, int W) {
    // neg[eta+1], repl[eta+1], keep[eta+1], then (8-byte aligned) part[W][eta+1] (W>1) or perm[eta+1] pairs of (corruption,
    // replacement row) (W==1), dfac[eta+1] (FocusE), rounded to 8 bytes
    const size_t b = (size_t)(eta + 1) * (3 + (W > 1 ? W : 2) + 1) * 4 + 8 + (W > 1 ? 64 * 4 : 0);   // (+ the single-pass cross-wave sums)
    return (b + 7) & ~(size_t)7;
}

template <int W>
__device__ __forceinline__ void slot_sync() {
    if constexpr (W == 1) {
        // single-wave slot: LDS ops of one wave complete in order; only stop compiler reordering
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    } else {
        __syncthreads();
    }
}

}  // namespace kge
