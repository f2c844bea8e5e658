/* libamdkge -- extension header: SHARED-NEGATIVE TRAINING (one GEMM scores the corruptions of a group of positives).
 *
 * An extension header like include/amdkge_lists.h and include/amdkge_negatives.h: entry points ADDED to ABI version 5 without
 * changing one of amdkge.h's, bound through ampligraph_amd/_ffi.py's SHARED_SIGNATURES table.  amdkge.h does NOT include this
 * header (its text is frozen): a caller includes it by name.  The ABI version stays 5.
 *
 * THE STEP.  A batch of B positives is cut into groups of G consecutive rows (group g = the rows i with i / G == g; the last
 * group may be short), n_groups = ceil(B / G).  Every group shares ONE list of M replacement entities ids[g][0 .. M), every
 * positive i has ONE replaced side[i].  The step is BY DEFINITION the train step of amdkge_train_fwdbwd with eta = M and the
 * override rows
 *     neg[j * B + i] = positive i with its side[i] entity replaced by ids[i / G][j]
 * -- the same loss (Loss.__call__ on the M corruption scores of a positive, "mean" dividing by M, by 2 M for nll), the same
 * gradients; identity corruptions and corruptions that are known statements are kept.  The model's own eta plays no part.
 * What differs is the formulation: with q_i the vector for which score(i, e) = <q_i, e> holds for a replacement e on side[i]
 * (DistMult: s*p or p*o; ComplEx / HolE: the two halves of survey row a9), the G x M scores of a group are one fp32 matrix
 * product Q_g E^T of the group's query vectors with the M gathered rows, and so are both gradients (dQ_g = C_g E and
 * dE = C_g^T Q_g, C = dL/dscore).  A positive then costs 3 row reads and 3 gradient-row adds whatever M is; a group costs M.
 * Only models whose score is such a contraction take part: TransE and RotatE are refused.
 * NaN and inf in the tables follow the definition's rules: a NaN score is a NaN loss, a coefficient that a clip or a hinge zeroes
 * is still multiplied by the score's Jacobian (0 * NaN = NaN), and the padding floats of a padded gradient row are never written.
 * A ComplEx / HolE score that the product makes +-inf is computed again in the reference's operation order, where a * inf - b * inf
 * is NaN although (a - b) * inf is not.  An inf in a positive's own kept row may still become NaN where the definition says +-inf.
 */
#ifndef AMDKGE_SHARED_H
#define AMDKGE_SHARED_H

#include "amdkge.h"
#include "amdkge_negatives.h"   /* the side modes AMDKGE_NEG_SIDE_* */

#ifdef __cplusplus
extern "C" {
#endif

#define AMDKGE_SHARED_MAX_NEGS ((1 << 24) - 1)   /* M: j has the low 24 bits of a counter word to itself */

/* THE DRAW.  Philox4x32-10 with key = (seed_lo, seed_hi); lo / hi = the low / high 32 bits.
 *   ids[g][j]  : x of philox(counter = (g, j | 0xF0 << 24, step_lo, step_hi)),  g = the group's index in the whole batch;
 *                d_pool set:  d_pool[mulhi32(x, pool_n)]       otherwise:  sample_base + mulhi32(x, sample_range)
 *                (mulhi32(a, n) = (a * n) >> 32 on 64-bit integers).
 *   side[i]    : x of philox(counter = (i_lo, i_hi | 0xF1 << 24, step_lo, step_hi)),  i = the positive's row in the whole batch;
 *                AMDKGE_NEG_SIDE_UNIFORM: the subject iff bit 0 of x is 0;  AMDKGE_NEG_SIDE_BERNOULLI: the subject iff
 *                x < d_side_thr[p_i] (amdkge_negatives_side_thresholds);  S_ONLY / O_ONLY: no draw.
 * The side is decided per POSITIVE, not per corruption: that is what lets one product serve a group whose positives are
 * corrupted on different sides.  The top byte of counter word 1 is the DOMAIN TAG: amdkge_sample_corruptions and
 * amdkge_sample_negatives keep a block number <= 10 there, so no stream of this draw coincides with one of theirs.
 * The result is a pure function of (seed, step, g or i, the tables of the call).
 *
 *   d_triples  : int32 [B, 3]; read for AMDKGE_NEG_SIDE_BERNOULLI only (may be NULL otherwise)
 *   d_pool     : NULL, or int32 [pool_n] entity ids, 1 <= pool_n < 2^32; NOT checked against the entity count here.
 *                Without a pool sample_range must be in [1, 2^32) and sample_base >= 0.
 *   d_ids      : int32 [ceil(B / G), M] out
 *   d_side     : int32 [B] out; 1 = the SUBJECT is replaced, 0 = the object
 * Errors (before any launch): AMDKGE_EINVAL for NULL outputs, B < 0, G < 1, M < 1 or > AMDKGE_SHARED_MAX_NEGS, an unknown
 * side_mode, BERNOULLI without d_side_thr or d_triples, a bad pool_n / sample_range.  B == 0: nothing is done. */
int amdkge_sample_shared(const int32_t* d_triples, int64_t B, int64_t G, int32_t M,
                         int64_t sample_base, int64_t sample_range, uint64_t seed, uint64_t step,
                         int32_t side_mode, const uint32_t* d_side_thr, const int32_t* d_pool, int64_t pool_n,
                         int32_t* d_ids, int32_t* d_side, void* stream);

/* Bytes of d_work for a step of this shape, or 0 when the path does not take it: TransE / RotatE, B < 1, G < 1, M out of
 * [1, AMDKGE_SHARED_MAX_NEGS], an invalid model.  The size is bounded in B * M: groups are processed in chunks of at most
 * 2^24 scores (one group at least), so the score buffer never exceeds max(64 MB, 4 G M bytes); the rest is 2 B (K + 1) floats. */
int64_t amdkge_train_shared_workspace_bytes(const amdkge_model* m, int64_t B, int64_t G, int32_t M);

/* Forward + backward of the step above.  The contract of amdkge_train_fwdbwd for the outputs: gradient rows are ADDED to
 * d_grad_ent / d_grad_rel (fp32 atomics, unordered: there is no deterministic mode), the sum of the per-positive losses is
 * ADDED to *d_loss_sum, d_pos_scores [B] / d_neg_scores [M * B] (row j * B + i) are optional outputs (NULL: not written).
 *   d_neg_ids : int32 [ceil(B / G), M], every id in [0, n_ents) -- NOT checked (amdkge_sample_shared's d_ids; an id may
 *               repeat inside a list, between lists, and be a positive's own entity)
 *   d_side    : int32 [B], non-zero = the subject is replaced
 *   d_work    : amdkge_train_shared_workspace_bytes(m, B, G, M) bytes, 4-byte aligned; contents undefined afterwards
 * Errors (before any launch): AMDKGE_EINVAL for an invalid model or loss, NULL pointers, B < 0, G < 1, M out of range;
 * AMDKGE_EUNSUPPORTED for TransE / RotatE (a distance is not a contraction) and FocusE.  B == 0: nothing is done. */
int amdkge_train_shared_fwdbwd(const amdkge_model* m, const amdkge_loss* loss, const float* d_ent, const float* d_rel,
                               const int32_t* d_triples, int64_t B, int64_t G, int32_t M,
                               const int32_t* d_neg_ids, const int32_t* d_side, float* d_grad_ent, float* d_grad_rel,
                               double* d_loss_sum, float* d_pos_scores, float* d_neg_scores, void* d_work, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AMDKGE_SHARED_H */
