// What the shared-list train units share (kge_train_shared.hip: the matrix-product step of DistMult / ComplEx / HolE;
// kge_train_shared_dist.hip: the distance tiles of TransE / RotatE; kge_train_relpred.hip: the relation objective):
//   shared_step       : THE host driver of a step (defined in kge_train_shared.hip): argument checks, workspace plan, query kernel, per
//                       chunk of the score buffer FWD tiles -> loss stage -> DQ tiles -> DE tiles, chain kernel.  A family (products,
//                       distances) is a SharedFamily: its message prefix, its model test, its tile count along the units and ONE host
//                       function that launches its own kernels -- a __global__ cannot be launched from another unit without relocatable
//                       device code (the kge_train_tiled.h pattern), so the launches live beside their kernels.
//   shared_loss_stage : THE loss stage of one chunk: shared_label_loss_kernel (kge_train_shared_labels.hip) where labels are given, else
//                       the optional shared_mask_kernel, then shared_loss_kernel.  The driver and the relation objective's row loop
//                       both call it; the fill of a masked entry is decided here alone.
//   the workspace plan, the mask's and the labels' arguments with their checks, and shared_model_ok / add_nz.
// The device side of the two matrix-product units, the 64 x 64 fp32 MFMA tile, is kge_product_tile.h (it includes this header).
#pragma once
#include "kge_host.h"
#include "../../include/amdkge_shared_labels.h"

namespace kge {

constexpr int64_t CHUNK_SCORES = 1ll << 24;   // groups are processed in chunks of at most this many scores
constexpr int SHARED_TILE = 64;               // rows of a group / entries of its list per tile, in both families

// the models whose score is a contraction with the replaced row (the product family, the relation objective)
inline bool shared_model_ok(const amdkge_model* m) {
    return m->scoring_type == AMDKGE_DISTMULT || m->scoring_type == AMDKGE_COMPLEX || m->scoring_type == AMDKGE_HOLE;
}
// the chain kernels' row-adds: an exact zero adds nothing (true for NaN)
__device__ __forceinline__ void add_nz(float* p, float v) {
    if (v != 0.f) atomic_add_f32(p, v);
}

// the workspace of a step: Q, dQ [B, K], the positives' raw scores and coefficients [B], the score buffer of one chunk [rows, M]
struct SharedPlan {
    int64_t n_groups, gpc, off_q, off_dq, off_pos, off_cpos, off_s, total;
};
bool shared_plan(const amdkge_model* m, int64_t B, int64_t G, int64_t M, SharedPlan& p);   // false: bad sizes (G is clamped to B)

struct SharedMaskArgs {
    float* S;              // [rows, M]: row r is batch row row0 + r
    int64_t row0, rows, G;
    int M;
    const int32_t* ids;    // [n_groups, M]; not read in IDENTITY mode
    const int32_t* side;   // the six below are indexed by batch row
    const int64_t *s_lo, *s_hi, *o_lo, *o_hi;
    const int32_t *s_ids, *o_ids;
    int identity;
    float fill;            // the buffer holds the plain sums: -inf, or +inf under a negative score scale
    unsigned long long* stats;
};

// the checks the entry points of include/amdkge_shared_mask.h (and of include/amdkge_shared_dist.h) share; fills the part of the
// kernel's arguments that does not depend on the buffer
int shared_mask_args(const char* who, const int32_t* d_neg_ids, const int64_t* d_s_lo, const int64_t* d_s_hi, const int32_t* d_s_ids, const int64_t* d_o_lo,
                     const int64_t* d_o_hi, const int32_t* d_o_ids, int32_t list_mode, int64_t* d_stats, bool ranges_required, SharedMaskArgs& a, bool& masked);

// shared_mask_kernel on a.rows rows of a.S (a wave per row)
int launch_shared_mask(const SharedMaskArgs& a, hipStream_t st);
// shared_loss_kernel: Loss.__call__ on `rows` rows of S [rows, M] (batch rows row0 ...): scores -> dL/d(buffer value) in place, cpos[i],
// the optional score outputs and the loss sum.  `scale` takes a buffer value to a score (HolE's 2/k; -1 for a distance).
int launch_shared_loss(float* S, const float* pos_raw, float* cpos, int64_t row0, int64_t rows, int64_t B, int M, const amdkge_loss& L, float scale, double* loss_sum,
                       float* pos_scores, float* neg_scores, hipStream_t st);


// The labelled loss step (include/amdkge_shared_labels.h; shared_label_loss_kernel, kge_train_shared_labels.hip): labels from the known
// ranges + binary cross-entropy in ONE pass over the buffer, in place of the mask-then-loss pair.
struct SharedLabelArgs {
    float* S;              // [rows, M]: row r is batch row row0 + r; scores in, scale * c out
    int64_t row0, rows, G, B;
    int M;
    const int32_t* ids;    // [n_groups, M]; not read in IDENTITY mode
    const int32_t* side;   // the ranges and the weights are indexed by batch row
    const int64_t *s_lo, *s_hi, *o_lo, *o_hi;
    const int32_t *s_ids, *o_ids;
    int identity;
    float eps, scale;      // label_smoothing; a buffer value times scale is a score
    int mean;
    const float *w_s, *w_o;   // both or neither
    const float* pos_raw;  // [B] or NULL (the kernel alone): the positives' raw scores, for pos_scores only
    float* cpos;           // [B] or NULL: receives exact zeros
    float* pos_scores;     // [B] or NULL
    float* neg_scores;     // [M * B] or NULL: x at row j * B + i
    double* loss_sum;
    unsigned long long* stats;
};

// the checks the three entry points of include/amdkge_shared_labels.h share; fills the part of the kernel's arguments that does not
// depend on the buffer
int shared_label_args(const char* who, const int32_t* d_neg_ids, const int64_t* d_s_lo, const int64_t* d_s_hi, const int32_t* d_s_ids, const int64_t* d_o_lo,
                      const int64_t* d_o_hi, const int32_t* d_o_ids, int32_t list_mode, float label_smoothing, int32_t reduction_mean, const float* d_w_s,
                      const float* d_w_o, int64_t* d_stats, SharedLabelArgs& a);
// shared_label_loss_kernel on a.rows rows of a.S (a wave per row)
int launch_shared_label_loss(const SharedLabelArgs& a, hipStream_t st);

// A step while it runs: its arguments and its carved workspace.  A family's launch function reads the upper part; the loss stage
// reads S, pos_raw, cpos, B, G, M, ids, side, st and the lower part.
struct SharedStep {
    const amdkge_model* m;
    const float *ent, *rel;
    const int32_t *triples, *ids, *side;
    int64_t B, G;
    int M;
    float *g_ent, *g_rel, *Q, *dQ, *pos_raw, *cpos, *S;
    hipStream_t st;
    float scale;                     // a buffer value times scale is a score
    const amdkge_loss* loss;         // not read where labels are given
    const SharedMaskArgs* mask;      // NULL, or the buffer-independent part that shared_mask_args fills
    const SharedLabelArgs* labels;   // NULL, or the buffer-independent part that shared_label_args fills
    double* loss_sum;
    float *pos_scores, *neg_scores;
};
// The loss stage of one chunk (rows batch rows from row0, S holding their scores): labels -> launch_shared_label_loss; else the
// optional mask (fill = the buffer value of a score of -inf: +inf under a negative scale), then launch_shared_loss.
int shared_loss_stage(const SharedStep& s, int64_t row0, int64_t rows);
enum SharedStage { SHARED_QUERY, SHARED_FWD, SHARED_DQ, SHARED_DE, SHARED_CHAIN };
struct SharedFamily {
    const char* who;                          // the prefix of its messages
    bool (*model_ok)(const amdkge_model*);
    const char* wrong_model;                  // what a model of the other family is told
    int (*unit_tiles)(const amdkge_model*);   // tiles along the units of DQ / DE
    // its kernel of `stage` on `blocks` workgroups; FWD / DQ / DE: the groups from g0, tiles_m x tiles_n tiles each
    int (*launch)(const SharedStep& s, SharedStage stage, unsigned blocks, int64_t g0, int tiles_m, int tiles_n);
};
// the step of the five amdkge_train_shared*_fwdbwd entry points (mask, labels: at most one; labels: loss is not read) and their workspace
int shared_step(const SharedFamily& f, const amdkge_model* m, const amdkge_loss* loss, const float* d_ent, const float* d_rel, const int32_t* d_triples, int64_t B, int64_t G,
                int32_t M, const int32_t* d_neg_ids, const int32_t* d_side, float* d_grad_ent, float* d_grad_rel, double* d_loss_sum, float* d_pos_scores,
                float* d_neg_scores, void* d_work, const SharedMaskArgs* mask, const SharedLabelArgs* labels, void* stream);
int64_t shared_step_workspace_bytes(const SharedFamily& f, const amdkge_model* m, int64_t B, int64_t G, int32_t M);

}  // namespace kge
