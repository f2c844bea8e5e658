/* libamdkge -- extension header: BATCH REGULARISERS (N3 and per-occurrence Lp on the rows a train step uses).
 *
 * An extension header like include/amdkge_shared.h: one entry point ADDED to ABI version 5 without changing one of amdkge.h's,
 * bound through ampligraph_amd/_ffi.py's BATCH_REG_SIGNATURES table.  amdkge.h does NOT include this header (its text is
 * frozen): a caller includes it by name.  The ABI version stays 5.
 *
 * THE PENALTY.  For a batch of B positives (s_i, p_i, o_i)
 *     R = lambda_e * sum_i sum_u ( n(ent[s_i], u)^p_e + n(ent[o_i], u)^p_e )  +  lambda_r * sum_i sum_u n(rel[p_i], u)^p_r
 * SUMMED over the positives, not averaged -- the data loss is a sum of per-positive losses too -- so a row's weight is the number
 * of times it OCCURS in the batch: a row that occurs twice is penalised twice, also when s_i == o_i.  (amdkge_opt's reg_p /
 * reg_lambda is lambda * sum |x|^p over the WHOLE table, once per step whatever the batch holds.)  Rows of corruptions take no
 * part.  p is 2 or 3; u runs over the model's k live units; n depends on the NORM MODE of the term:
 *   AMDKGE_BATCH_REG_FLOAT   : every float of the row is a unit of its own, n = |x|.  The only mode for TransE and DistMult; for
 *                              ComplEx / HolE / RotatE both halves [re || im] count, 2k floats per row.
 *   AMDKGE_BATCH_REG_MODULUS : a unit is the complex number (re_u, im_u) of the two halves, n = sqrt(re_u^2 + im_u^2).  With
 *                              p = 3 this is the nuclear 3-norm N3 of Lacroix et al. 2018.  ComplEx and HolE: both terms;
 *                              RotatE: the entity term only -- a RotatE relation row holds phases, the modulus of what it stands
 *                              for is 1.
 * THE ARITHMETIC, in fp32 with every rounding where it is written (the unit is compiled with -ffp-contract=off like the rest of
 * the library); c = fp32(p * lambda), formed once on the host:
 *   FLOAT, float x        : a = x * x;  n = |x|;                pen = a (p = 2) | a * n (p = 3);   dx = c * x | (c * n) * x
 *   MODULUS, unit (re,im) : m2 = re * re + im * im;  m = sqrtf(m2);
 *                                                               pen = m2 (p = 2) | m2 * m (p = 3);
 *                                                               f = c | c * m;   dre = f * re;  dim = f * im
 * Nothing is divided: a unit at exactly zero has penalty zero and gradient exactly zero.  dx / dre / dim are ADDED to the float's
 * place in the gradient row (an exact zero adds nothing).
 * THE SUM.  One wave of 64 lanes per positive.  With V = 4 where the stored half width is a multiple of 4 and both table
 * pointers are 16-byte aligned, V = 1 otherwise, lane l owns the units u with (u / V) % 64 == l and walks its groups of V
 * consecutive units in ascending order.  The penalty of a row's group is its units' penalties added in ascending order (in FLOAT
 * mode on a two-half row a unit's penalty is pen(re) + pen(im)); a group adds to the lane's fp32 entity accumulator row s_i's group
 * penalty, then row o_i's, and to its fp32 relation accumulator row p_i's.  The 64 lane values are summed by the tree of
 * wave_sum (lanes at distance 1, 2, 4, 8, then the rows of 16, then the halves).  The positive's penalty is
 * double(lambda_e) * double(E) + double(lambda_r) * double(Rl) of the two wave totals; the positives' penalties are added in
 * double, in no fixed order.
 * NaN AND inf follow the project's rule: a non-finite float makes the penalty non-finite and reaches the gradient of exactly the
 * floats whose formula above reads it -- the float itself; and with MODULUS and p = 3 BOTH components of its unit (f = c * m;
 * inf * 0 = NaN).  With MODULUS and p = 2 the gradient of the partner component, c * im, does not read it and stays finite.  No
 * other unit and no other row is reached.
 * PADDING.  In the stored, padded layout (k_pad > k) the k_pad - k padding floats of a half enter no result and are never written.
 */
#ifndef AMDKGE_BATCH_REG_H
#define AMDKGE_BATCH_REG_H

#include "amdkge.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMDKGE_BATCH_REG_FLOAT 0
#define AMDKGE_BATCH_REG_MODULUS 1

/* Penalty and gradient of the batch regulariser above, between a forward / backward call that leaves dense gradient tables
 * (amdkge_train_fwdbwd, amdkge_train_shared_fwdbwd, ...) and the amdkge_opt_step that consumes them.
 *   d_triples   : int32 [B, 3], every id inside its table -- NOT checked
 *   d_grad_ent  : gradient rows are ADDED (fp32 atomics, unordered: there is no deterministic mode); d_grad_rel likewise
 *   d_reg_sum   : R is ADDED to *d_reg_sum
 *   lambda_ent / lambda_rel : finite and >= 0.  A lambda of exactly 0 switches its term off: its gradient table is not touched and
 *                 may be NULL.  p and norm of a term that is switched off are still validated.
 * All offsets are 64-bit (a row's offset, its index times the floats of a stored row, exceeds 2^31 on large tables).
 * Errors (before any launch): AMDKGE_EINVAL for an invalid model, p outside {2, 3}, an unknown norm, a lambda that is negative or
 * not finite, B < 0, NULL d_ent / d_rel / d_reg_sum, a NULL gradient table whose lambda is not 0, NULL d_triples with B > 0;
 * AMDKGE_EUNSUPPORTED for AMDKGE_BATCH_REG_MODULUS on TransE or DistMult (either term) and on RotatE's relation term.
 * B == 0: nothing is done. */
int amdkge_batch_reg_fwdbwd(const amdkge_model* m, const float* d_ent, const float* d_rel,
                            const int32_t* d_triples, int64_t B,
                            int32_t p_ent, float lambda_ent, int32_t norm_ent,
                            int32_t p_rel, float lambda_rel, int32_t norm_rel,
                            float* d_grad_ent, float* d_grad_rel, double* d_reg_sum, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AMDKGE_BATCH_REG_H */
