// The tile side of the owner-computes step (kge_train_tiled.hip): what its units share.  The tile passes' arguments and LDS geometry
// (kge_train_tile.hip, kge_train_direct.hip; the host plans with them), the compile-time switches that shape their kernels, and the
// launch functions through which kge_train_tiled.hip reaches the kernels of the other units.
#pragma once
#include "kge_train_common.h"
#include "kge_opt.h"

// the lambdas of the tile kernel capture its argument struct by reference: one of them left out of line puts the whole struct
// (and the operand arrays passed to it) into scratch memory -- measured 6x on the TransE instantiation
#ifndef KGE_TILE_INLINE
#define KGE_TILE_INLINE __attribute__((always_inline))
#endif

// 16-byte operand load of the entry loop, as a VALUE.  Written as plain `x = *reinterpret_cast<const float4*>(p)` the RotatE
// tile pass measured 130 us instead of 113: assigned through the reference, the compiler orders the loads of a batch against
// the operand arrays of the previous one (more s_waitcnt, fewer loads in flight).  Found by bisection.
#ifdef KGE_LD4_FN
namespace kge { __device__ __forceinline__ float4 ld4_value(const float* p) { return *reinterpret_cast<const float4*>(p); } }
#define KGE_LD4(p) kge::ld4_value(p)
#else
#define KGE_LD4(p) (false ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(p))
#endif

namespace kge {

constexpr int TILE_THREADS = 1024;
constexpr int TILE_WAVES = TILE_THREADS / 64;
constexpr int TILE_QCAP = 128;                                              // entries of a wave's LDS queue (tile_backward_kernel)
constexpr size_t TILE_QUEUE_BYTES = (size_t)TILE_WAVES * TILE_QCAP * 16;    // 32 KB behind the accumulators
// which instantiations of tile_backward_kernel collect their entries in the LDS queue first (see the kernel); CH = quads per lane
// (rows beyond 2 KB are bandwidth-bound chunk by chunk, and the queue's 32 KB of LDS would shrink their tiles: C5 5 % slower)
__host__ __device__ constexpr bool tile_queued(int model, int CH, int K) {
    return ((model == AMDKGE_TRANSE || model == AMDKGE_ROTATE) && K <= 512) || (model == AMDKGE_DISTMULT && CH == 1);
}
static inline int tile_ch_of(int nq) { return (nq <= 64 || nq > 128) ? 1 : 2; }   // the CH run_tiled picks for the tile kernel

struct TileArgs {
    float* x;                 // entity table (updated in place when g_out == NULL)
    float* s0;                // optimizer slots
    float* s1;
    float* g_ent;             // dense entity gradient buffer
    int apply_update;         // 1: optimizer applied from LDS; 0: g_ent receives the entity gradient (data parallel)
    int pos_atomic;           // g_ent holds the s / o rows of the positives (forward kernel's atomics): fold them in
    int ns;                   // staged rows per positive (4; 5 in deterministic mode)
    int det;                  // deterministic mode: the tile's entries are sorted into a canonical order before they are added
    int sort_cap;             // det: entries the LDS sort buffer holds (a multiple of 64, <= 8192)
    int pos_bits;             // det: bits the positives' indices need (the radix passes of the index sort)
    int own_cache;            // RotatE, queued form: the tile's own live rows are copied into LDS behind the accumulators (see make_plan)
    int lazy;                 // touched-rows optimizer mode (amdkge_opt.lazy): rows without an entry keep their bits
    const uint8_t* hot_map;   // AMDKGE_TILED_HOT_ROWS (see HOT_MAX in kge_train_common.h); NULL = off
    float* hot_buf;
    uint8_t* touched;         // lazy + pos_atomic: rows the forward kernel's atomics touched (read, then cleared here)
    const uint32_t* sign_codes;   // TransE: [B][eta][nq] packed sign bytes written by the forward kernel (see ENTRY_J_SHIFT in kge_train_common.h); NULL = off
    int eta;
    const float* rel;         // live relation table (TransE / RotatE side of the gradient)
    const float* rel_cs;      // RotatE: [R][cos(phase) || sin(phase)] of this step's relation table (rel_phase_kernel)
    const int32_t* triples;
    const float* stage_rows;  // [B][4][K]
    const StageEntry* lists;  // [n_tiles][cap]
    const StageEntry* ovf;    // overflow entries
    int* counters;            // [(n_tiles + 2) * 32]: bucket fills, overflow count, tile ticket (all zero between steps)
    int* status_flag;         // det-sort overflow flag: at a workspace offset that does not depend on the plan (sticky until queried)
    double* loss_parts;       // the forward kernel's per-block loss partials, folded into loss_sum by the first sweep workgroup (without one: by the first LOSS_PARTS tiles)
    double* loss_sum;
    double* reg_loss;
    OptArgs rel_opt;          // fused relation-table sweep (rel_blocks > 0): blocks [n_tiles, n_tiles + rel_blocks)
    int rel_blocks;
    int64_t n_rows;
    int64_t n_rels;
    int k, K, nq;             // stored half width, floats per stored row, quads per half
    int k_live;               // the model's k (RotatE: units behind it are zero padding, see grad_unit)
    int tile_rows, n_tiles, cap, ovf_cap;
    int rb;                   // rows per ownership block (block-interleaved tiles)
    int direct;               // launched as tile_direct_kernel (kge_train_direct.hip)
    int gw;                   // waves that share one row (1: a wave covers the row; 4 / 8: long rows are split over a group of
                              // waves, each lane one quad), rows are owned by wave GROUPS: TILE_WAVES / gw owners per tile
    ModelConst mc;
    OptArgs opt;
#ifdef KGE_ABLATE
    int dbg;                  // development ablation build only: 1024 no flush, 2048 no accumulator zeroing, 4096 no bucket scan, 16384 no sort (det)
                              // (per-load switches in the entry loop were tried: they push its operand arrays to scratch)
#endif
};

// The launches of one step, each in the unit that instantiates its kernels.  `model` is the scoring type (amdkge_model.scoring_type):
// every unit maps it to its own instantiations (KGE_MODEL_DISPATCH).
int run_forward_stage(int model, TrainArgs& f, hipStream_t st);                        // kge_train_stage.hip: F, forward + staging
int run_cols_stage(int model, const TrainArgs& f, float* given, hipStream_t st);       // kge_train_cols.hip: C of the column-sharded step, in F's place
int run_tile_backward(int model, const TileArgs& te, hipStream_t st);                  // kge_train_tile.hip: T, LDS-accumulator tiles
int run_tile_direct(int model, const TileArgs& te, hipStream_t st);                    // kge_train_direct.hip: T, row-direct form (long rows)

}  // namespace kge
