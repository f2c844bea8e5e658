/* libamdkge -- extension header: SHARED-NEGATIVE TRAINING FOR THE DISTANCE MODELS (TransE, RotatE) on distance tiles.
 *
 * An extension header like include/amdkge_shared.h and include/amdkge_shared_mask.h: entry points ADDED to ABI version 5 without
 * changing one of amdkge.h's, amdkge_shared.h's or amdkge_shared_mask.h's, bound through ampligraph_amd/_ffi.py's
 * SHARED_DIST_SIGNATURES table.  The ABI version stays 5.
 *
 * THE STEP is the one include/amdkge_shared.h defines -- amdkge_train_fwdbwd's step with eta = M on the override rows
 *     neg[j * B + i] = positive i with its side[i] entity replaced by ids[i / G][j]
 * with the draw, the groups and the per-positive side of amdkge_sample_shared, the same five losses and both reductions, identity
 * corruptions kept -- and, with the six range arrays given, the masked step of include/amdkge_shared_mask.h word for word: a known
 * entry scores -inf, a fully known row is kept and counted, d_stats is updated.  amdkge_train_shared_fwdbwd refuses TransE and
 * RotatE because a distance against a shared list is no matrix product.  It is still a TILE: a group's G queries and its M gathered
 * rows are each read once, and the G x M x k work is arithmetic on operands held in LDS and registers.  What this header declares is
 * that arithmetic (u runs over the model's k units; padding units of a stored row are not visited).
 *
 * TransE.   q_i = fp32(s + p) when the object is replaced, q_i = fp32(o - p) when the subject is;  d_iju = fp32(q_iu - e_ju);
 *           score(i, j) = -sum_u |d_iju|.  (The reference's own 1-vs-all rounding order on both sides: |e + (p - o)| equals
 *           |(o - p) - e| bit for bit.)  With sigma = sign(d), sign(0) = 0 and NaN kept, and c_ij = dL/dscore(i, j):
 *               dL/dq_iu = -sum_j c_ij sigma_iju        dL/de_ju = +sum_i c_ij sigma_iju
 * RotatE.   Units are complex; r_i = (cos phi, sin phi) of the positive's relation, phi = fp32(theta / phase_divisor) with the
 *           phase divisor of the whole model (amdkge.h).  q_i = s o r_i when the object is replaced (the reference's form) and
 *           q_i = o o conj(r_i) when the subject is: |e o r - o| = |e - o o conj(r)| because |r| = 1.  THIS IS THE ONE PLACE where
 *           the formulation is not the reference's operation order: in fp32 cos^2 + sin^2 is off by about 1e-7, far inside the
 *           parity bar of 1e-5 that the default (non-deterministic) train mode is held to.  It is what lets one tile serve a
 *           group whose positives are corrupted on different sides.  With z = q - e: score = -sum_u |z_u|, the gradient uses
 *           z / |z| per unit.  A modulus of exactly zero gives NaN, as in the reference and in the per-corruption kernels.
 * Both.     The positive's own score is the same distance to its own replaced-side row.  dL/dq_i goes to the two kept rows of
 *           the positive through the transpose of the query map (RotatE: the phase gradient, divided by the phase divisor, into
 *           the first k floats of the relation row); the replaced row's original gets the positive score's term.
 *           A pair with c_ij == +-0 (a masked entry, a clipped score) adds that zero times sigma / z / |z|: nothing where the
 *           residual is finite, NaN where it is not (0 * NaN = NaN, the reference's rule for every zeroed coefficient:
 *           include/amdkge_shared_mask.h).
 */
#ifndef AMDKGE_SHARED_DIST_H
#define AMDKGE_SHARED_DIST_H

#include "amdkge_shared_mask.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of d_work for a step of this shape, or 0 when the path does not take it: DistMult / ComplEx / HolE (theirs is
 * amdkge_train_shared_workspace_bytes), B < 1, G < 1, M out of [1, AMDKGE_SHARED_MAX_NEGS], an invalid model.  The layout and the
 * bound are amdkge_train_shared_workspace_bytes': chunks of at most 2^24 scores, 2 B (K + 1) floats beside them. */
int64_t amdkge_train_shared_dist_workspace_bytes(const amdkge_model* m, int64_t B, int64_t G, int32_t M);

/* Forward + backward of the step above.  The argument list, the outputs and the error rules are
 * amdkge_train_shared_masked_fwdbwd's: gradient rows are ADDED to d_grad_ent / d_grad_rel (fp32 atomics, unordered: there is no
 * deterministic mode), the loss is ADDED to *d_loss_sum, d_pos_scores [B] / d_neg_scores [M * B] (row j * B + i) are optional and
 * show -inf at masked entries; the six range arrays are all set or all NULL (NULL: the unmasked step; list_mode is still validated,
 * d_stats is not touched).  d_work: amdkge_train_shared_dist_workspace_bytes(m, B, G, M) bytes, 4-byte aligned.
 * The scores are a pure function of the inputs (bitwise equal between runs); the gradients are not.
 * Errors (before any launch): AMDKGE_EINVAL as there; AMDKGE_EUNSUPPORTED for DistMult / ComplEx / HolE (their score is a
 * contraction: use amdkge_train_shared_fwdbwd / amdkge_train_shared_masked_fwdbwd) and for FocusE.  B == 0: nothing is done. */
int amdkge_train_shared_dist_fwdbwd(const amdkge_model* m, const amdkge_loss* loss, const float* d_ent, const float* d_rel,
                                    const int32_t* d_triples, int64_t B, int64_t G, int32_t M,
                                    const int32_t* d_neg_ids, const int32_t* d_side, float* d_grad_ent, float* d_grad_rel,
                                    double* d_loss_sum, float* d_pos_scores, float* d_neg_scores, void* d_work,
                                    const int64_t* d_s_lo, const int64_t* d_s_hi, const int32_t* d_s_ids,
                                    const int64_t* d_o_lo, const int64_t* d_o_hi, const int32_t* d_o_ids,
                                    int32_t list_mode, int64_t* d_stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AMDKGE_SHARED_DIST_H */
