// What the training units share (kge_train.hip; the owner-computes step: kge_train_tiled.hip, kge_train_stage.hip, kge_train_tile.hip,
// kge_train_direct.hip, kge_train_cols.hip): the staging protocol between the forward kernels and the tile passes (StageEntry,
// block-interleaved row ownership, loss partials, hot rows) with its ONE set of writers (stage_draws, stage_side_rows, stage_append:
// used by train_fwdbwd_kernel and by the column-sharded kernels), the forward kernels' arguments, the wave's walk of Loss.__call__
// (WaveWalk; the losses themselves and their NaN / inf rules are in kge_loss.h, which g++ compiles too), and the LDS sizes the host
// plans with.
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
#include "kge_loss.h"

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

// The forward kernel's walk of Loss.__call__ (loss_call, kge_loss.h): one whole wave per positive, lane l takes the scores
// sn[l], sn[l + 64], ... (LDS, sign and scale already applied) and the lanes' partial results meet in wave reductions.
struct WaveWalk {
    float* sn;
    int lane;
    __device__ __forceinline__ int first() const { return lane; }
    __device__ __forceinline__ int stride() const { return KGE_WAVE; }
    __device__ __forceinline__ float load(int j) const { return sn[j]; }
    __device__ __forceinline__ void store(int j, float v) const { sn[j] = v; }
    __device__ __forceinline__ float sum(float v) const { return wave_sum(v); }
    __device__ __forceinline__ float max(float v) const { return wave_max(v); }
};

// coeff: dL/dscore as the loss code left it; g = coeff * score_sign * score_scale.  No entry below fp32's smallest NORMAL number
// (see the forward kernel) unless the coefficient is masked_zero's marker; a NaN coefficient is an entry.
__device__ __forceinline__ bool entry_wanted(float coeff, float g) {
    return !(fabsf(g) < 1.17549435e-38f) || __float_as_uint(coeff) == 0x80000000u;
}

// ---- the writers of the staging protocol: what a forward kernel (train_fwdbwd_kernel<STAGE>, cols_scores_kernel / cols_stage_kernel)
//      hands to tile_backward_kernel, written once ----

// The corruption draws of positive i into LDS (CorruptionGenerationLayerTrain.py:35-94; Philox rows keyed by the global corruption
// row, so every kernel and every GPU of a group draws the same), or the caller's own corruptions.  The threads that share the
// positive take j = first, first + stride, ...
__device__ __forceinline__ void stage_draws(const TrainArgs& a, int64_t i, int ps, int first, int stride, int* sh_keep, int* sh_repl) {
    for (int j = first; j < a.eta; j += stride) {
        int keep, repl;
        if (a.neg_override) {
            const int64_t r = (int64_t)j * a.B + i;
            const int ns = a.neg_override[3 * r + 0], no = a.neg_override[3 * r + 2];
            keep = (ns == ps) ? 1 : 0;
            repl = keep ? no : ns;
        } else {
            draw_corruption(a.sc, i, j, keep, repl);
        }
        sh_keep[j] = keep;
        sh_repl[j] = repl;
    }
}

// The side rows A, B of one quad of a positive (staged rows 2, 3; qa / qb point at the quad, k floats between the halves).
// Trilinear models: d(score)/d(replaced row) does not depend on the replaced row, so the owner only needs g * A (A = d/do (s,p)) or
// g * B (B = d/ds (p,o)).  TransE: copies of s and o (the owner recomputes grad_unit with its own row).
// RotatE: A = s o r (the reference's own first step of s o r - e, RotatE.py:100-101: the object-side entries of the tile pass are
// bit-identical to grad_unit), B = o o conj(r): |e o r - o| = |e - B| as |r| = 1, and d|e o r - o| / de = (e - B) / |e - B| -- one
// side row and the tile's own row per entry, no relation row.  (p holds cos, sin: prep_rel.)
template <int MODEL>
__device__ __forceinline__ void stage_side_rows(const float (&s)[4][ModelTraits<MODEL>::NC], const float (&p)[4][ModelTraits<MODEL>::NC],
                                                const float (&o)[4][ModelTraits<MODEL>::NC], float* qa, float* qb, int k) {
    constexpr int NC = ModelTraits<MODEL>::NC;
    float va[NC][4], vb[NC][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if constexpr (MODEL == AMDKGE_DISTMULT || MODEL == AMDKGE_COMPLEX) {
            float ds[NC], dp[NC], dd[NC];
            grad_unit<MODEL>(s[u], p[u], o[u], 1.f, ds, dp, dd);
#pragma unroll
            for (int h = 0; h < NC; ++h) { va[h][u] = dd[h]; vb[h][u] = ds[h]; }
        } else if constexpr (MODEL == AMDKGE_ROTATE) {
            const float cs = p[u][0], sn = p[u][1];
            va[0][u] = s[u][0] * cs - s[u][1] * sn; va[1][u] = s[u][0] * sn + s[u][1] * cs;
            vb[0][u] = o[u][0] * cs + o[u][1] * sn; vb[1][u] = o[u][1] * cs - o[u][0] * sn;
        } else {
#pragma unroll
            for (int h = 0; h < NC; ++h) { va[h][u] = s[u][h]; vb[h][u] = o[u][h]; }
        }
    }
#pragma unroll
    for (int h = 0; h < NC; ++h) {
        *reinterpret_cast<float4*>(qa + h * k) = make_float4(va[h][0], va[h][1], va[h][2], va[h][3]);
        *reinterpret_cast<float4*>(qb + h * k) = make_float4(vb[h][0], vb[h][1], vb[h][2], vb[h][3]);
    }
}

// One row-gradient entry into the bucket of the tile that owns row `dest` (block-interleaved ownership, see tile_backward_kernel);
// a full bucket spills into the overflow list.  `role`: the StageEntry role, with whatever the caller keeps above the local row
// (local < 4096: below the corruption index of ENTRY_J_SHIFT).
__device__ __forceinline__ void stage_append(const TrainArgs& a, int64_t i, uint32_t role, float g, uint32_t dest) {
    uint32_t tile, local;
    tile_of_row(dest, (uint32_t)a.st_n_tiles, (uint32_t)a.st_rb, tile, local);
    StageEntry* where;
    const int slotpos = atomicAdd(a.st_counters + (size_t)tile * 32, 1);
    if (slotpos < a.st_cap) {
        where = a.st_lists + (size_t)tile * a.st_cap + slotpos;
    } else {
        const int op = atomicAdd(a.st_counters + (size_t)a.st_n_tiles * 32, 1);
        if (op >= a.st_ovf_cap) return;
        where = a.st_ovf + op;
    }
    *where = StageEntry{(uint32_t)i, role | (local << 2), g, dest};   // (one 16-byte store)
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
