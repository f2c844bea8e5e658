/* libamdkge -- extension header: THE RELATION-PREDICTION TRAINING OBJECTIVE (a softmax over the relation table).
 *
 * An extension header like include/amdkge_shared_mask.h: entry points ADDED to ABI version 5 without changing one of amdkge.h's or
 * of another extension header's, bound through ampligraph_amd/_ffi.py's RELATION_OBJECTIVE_SIGNATURES table.  amdkge.h does NOT
 * include this header (its text is frozen): a caller includes it by name.  The ABI version stays 5.
 *
 * THE STEP (Chen et al. 2021, "Relation Prediction as an Auxiliary Training Objective": the term lambda * L(p | s, o)).  For a
 * batch of B positives (s_i, p_i, o_i) and R = m->n_rels the step is BY DEFINITION the train step of amdkge_train_fwdbwd with
 * eta = R on the override rows
 *     neg[j * B + i] = (s_i, j, o_i),   j = 0 .. R - 1
 * -- the same loss (Loss.__call__ on the R scores of a positive; "mean" dividing by R, by 2 R for nll), the same gradients; the
 * identity corruption j == p_i is a row like any other.  The model's own eta plays no part.  What differs is the formulation: the
 * score of DistMult, ComplEx and HolE is linear in the relation row, score(s_i, j, o_i) = <q_i, rel[j]> with the PAIR QUERY
 *     DistMult        : q_i = s * o
 *     ComplEx / HolE  : q_i = [ s_re * o_re + s_im * o_im  ||  s_re * o_im - s_im * o_re ]     (HolE's 2/k scales the sum)
 * so the B x R scores are one fp32 matrix product Q Rel^T over the relation table read in place, and both gradients are matrix
 * products too (dQ = C Rel, dRel = C^T Q, C = dL/dscore).  TransE and RotatE are not linear in the relation row: refused.
 *
 * THE MASK.  With the three range arrays set, the SCORE of (i, j) is replaced by -inf before Loss.__call__ whenever j is in
 *     known_i = d_known[d_lo[i] .. d_hi[i])      (what amdkge_pair_filter_ranges returns for the pairs (s_i, o_i))
 * under the rules of include/amdkge_shared_mask.h for the identity list: ids ascend STRICTLY inside a range; ids >= R are ignored;
 * the empty range leaves the row alone; every loss is defined at -inf (no loss term, an exact-zero coefficient); the divisors do
 * not change; a row whose R entries are ALL known keeps its whole row unmasked and is counted (self_adversarial would otherwise
 * form -inf - (-inf)).  d_stats: NULL, or int64 [2], += (masked entries, rows left unmasked by the exception).
 *
 * THE WEIGHT.  With w = weight (fp32), the step adds w * L to the loss and w times both gradients:
 *   - every coefficient C(i, j) = dL/d(sum of row (i, j)) that Loss.__call__ leaves, and every positive's coefficient c_pos_i, is
 *     multiplied by w ONCE, in fp32, where it is read as an operand of a gradient (C' = fl(w C)); the sums and products behind it
 *     are the unweighted step's, on C';
 *   - the loss is double(w) times the double sum of the positives' fp32 losses, added to *d_loss_sum as one double.
 * w == 0 does nothing and touches nothing (no launch; *d_loss_sum, the gradient tables, the optional outputs, d_stats and the
 * workspace are not written).
 *
 * NaN AND inf follow the project's rule (include/amdkge_shared.h) -- a NaN score is a NaN loss, a coefficient that a clip, a hinge
 * or the mask zeroes is still multiplied by the score's Jacobian (0 * NaN = NaN) -- applied to this step, in which every positive
 * is scored against every relation:
 *   - a non-finite RELATION row j reaches the loss of EVERY positive of the batch (every positive is scored against it, unless j is
 *     masked for it) and the s / o gradient rows of EVERY positive, masked or not (dQ_i = sum_j C'(i, j) rel[j]: C'(i, j) * NaN);
 *     where the loss turns a positive's NaN score into NaN coefficients, those reach every relation gradient row as well;
 *   - a non-finite ENTITY row reaches the loss of the positives that hold it, the gradient rows of those positives' two entities,
 *     and EVERY relation gradient row (dRel[j] = sum_i C'(i, j) q_i with a non-finite q_i, masked or not);
 *   - nothing else is reached: the s / o gradient rows of a positive that does not hold the entity stay finite, and an entity row
 *     that no positive of the batch uses is not written;
 *   - a masked entry is an exact zero times the score's Jacobian.
 * A ComplEx / HolE score that the product makes +-inf or NaN is computed again in the reference's operation order
 * s_re (p_re o_re + p_im o_im) + s_im (p_re o_im - p_im o_re): a * inf - b * inf is NaN although (a - b) * inf is not, and an inf in
 * s or o makes both halves of q infinite, whose product with a relation row is inf - inf although the reference's order has +-inf.
 * The positive's own score is formed in that order from the start.
 * PADDING.  In the stored, padded layout (k_pad > k) the padding floats of a half enter no result and are never written: they are
 * staged as exact zeros whatever they hold.
 * OFFSETS.  A row's offset (its index times the floats of a stored row) is 64-bit.
 */
#ifndef AMDKGE_RELATION_OBJECTIVE_H
#define AMDKGE_RELATION_OBJECTIVE_H

#include "amdkge.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of d_work for a step of B positives, or 0 when the path does not take it: TransE / RotatE, B < 1, an invalid model.
 * Rows are processed in chunks of at most 2^24 scores (one row at least), so the score buffer never exceeds max(64 MB, 4 R bytes);
 * the rest is 2 B (K + 1) floats, B int32 and one double. */
int64_t amdkge_train_relation_workspace_bytes(const amdkge_model* m, int64_t B);

/* Forward + backward of the step above.
 *   weight        : finite and >= 0; exactly 0: nothing is done
 *   d_triples     : int32 [B, 3], every id inside its table -- NOT checked
 *   d_lo, d_hi    : int64 [B]; d_known: int32 -- all three set or all three NULL (NULL: nothing is masked, d_stats is not touched)
 *   d_grad_ent / d_grad_rel : gradient rows are ADDED (fp32 atomics, unordered: there is no deterministic mode)
 *   d_loss_sum    : weight * L is ADDED to *d_loss_sum
 *   d_pos_scores  : NULL, or [B]: the positives' scores (unweighted)
 *   d_rel_scores  : NULL, or [R * B]: the score of (s_i, j, o_i) at row j * B + i, -inf at the masked entries (unweighted)
 *   d_work        : amdkge_train_relation_workspace_bytes(m, B) bytes, 8-byte aligned; contents undefined afterwards
 *   d_stats       : NULL, or int64 [2], += (masked, unmaskable)
 * Errors (before any launch): AMDKGE_EINVAL for an invalid model or loss, a weight that is negative or not finite, B < 0, NULL
 * tables / gradient tables / d_loss_sum, the three range arrays given in part, and with B > 0 and weight > 0 NULL d_triples /
 * d_work; AMDKGE_EUNSUPPORTED for TransE / RotatE (the score is a distance in the relation row) and for a loss that carries FocusE
 * weights.  B == 0: nothing is done. */
int amdkge_train_relation_fwdbwd(const amdkge_model* m, const amdkge_loss* loss, float weight, const float* d_ent,
                                 const float* d_rel, const int32_t* d_triples, int64_t B,
                                 const int64_t* d_lo, const int64_t* d_hi, const int32_t* d_known,
                                 float* d_grad_ent, float* d_grad_rel, double* d_loss_sum, float* d_pos_scores,
                                 float* d_rel_scores, void* d_work, int64_t* d_stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AMDKGE_RELATION_OBJECTIVE_H */
