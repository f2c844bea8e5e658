// What the shared-negative units share (kge_train_shared.hip: the matrix-product step of DistMult / ComplEx / HolE;
// kge_train_shared_dist.hip: the distance tiles of TransE / RotatE): the workspace plan, the mask's arguments and its checks, and the
// launch functions through which the distance unit reaches shared_mask_kernel and shared_loss_kernel, and both reach
// shared_label_loss_kernel (kge_train_shared_labels.hip) -- a __global__ cannot be launched from another unit without relocatable
// device code (the kge_train_tiled.h pattern).
#pragma once
#include "kge_host.h"
#include "../../include/amdkge_shared_labels.h"

namespace kge {

constexpr int64_t CHUNK_SCORES = 1ll << 24;   // groups are processed in chunks of at most this many scores

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

}  // namespace kge
