/* libamdkge -- extension header: TRAINING NEGATIVE SAMPLERS (filtered, Bernoulli side choice, entity pool).
 *
 * An extension header like include/amdkge_lists.h (see there for why): entry points ADDED to ABI version 5 without changing one of
 * amdkge.h's, bound through ampligraph_amd/_ffi.py's NEG_SIGNATURES table.  amdkge.h includes this header at its end; the ABI
 * version stays 5.  ("Extension headers".)
 *
 * The three train entry points (the fused forward+backward step, the tiled train step, the column-sharded partial scores) take
 * d_neg_override, int32 [(B*eta), 3] with row j*B + i = corruption j of positive i.  amdkge_sample_negatives fills such an array;
 * no train kernel knows about it.
 */
#ifndef AMDKGE_NEGATIVES_H
#define AMDKGE_NEGATIVES_H

#include "amdkge.h"

#ifdef __cplusplus
extern "C" {
#endif

/* side_mode: which element of the positive a corruption replaces */
enum {
    AMDKGE_NEG_SIDE_UNIFORM = 0,    /* the subject iff bit 0 of Philox word x is 0 (amdkge_sample_corruptions' rule) */
    AMDKGE_NEG_SIDE_BERNOULLI = 1,  /* the subject iff x < d_side_thr[p] (Wang et al., TransH, AAAI 2014) */
    AMDKGE_NEG_SIDE_S_ONLY = 2,     /* always the subject */
    AMDKGE_NEG_SIDE_O_ONLY = 3      /* always the object */
};
#define AMDKGE_NEG_MAX_TRIES 32

/* d_out[(B*eta), 3], row j*B + i = corruption j of positive i (amdkge_sample_corruptions' layout), drawn with rejection of known
 * positives, a per-relation side probability and / or a caller's pool of replacement entities.
 *
 * THE DRAW of corruption (i, j).  row = j * b_global + row_offset + i (b_global <= 0: B).  Philox4x32-10 BLOCK b of the row is
 *     (x, y, z, w) = philox(counter = (row_lo, row_hi | b << 24, step_lo, step_hi), key = (seed_lo, seed_hi)),
 * lo / hi = the low / high 32 bits; block 0 is the block of amdkge_sample_corruptions.  eta * b_global must be < 2^56, so that
 * the block number has the top byte of row_hi to itself.
 *   1. The SIDE is decided once, from word x of block 0 (side_mode above), and never redrawn: a redraw of the side after a
 *      rejection would move probability to the side with fewer known statements.
 *   2. TRY t = 0 .. max_tries - 1 takes its replacement from word 1 + t % 3 (y, z, w) of block t / 3:
 *        d_pool set:  d_pool[mulhi32(word, pool_n)]            otherwise:  sample_base + mulhi32(word, sample_range)
 *      (mulhi32(a, n) = (a * n) >> 32 on 64-bit integers).
 *   3. A try is ACCEPTED when the replacement is not in the positive's range of the replaced side: d_s_ids[d_s_lo[i] .. d_s_hi[i])
 *      = the subjects known with the positive's (p, o) when the subject is replaced, d_o_ids[d_o_lo[i] .. d_o_hi[i]) = the objects
 *      known with its (s, p) when the object is replaced.  Ids ascend inside a range (the filter index build's order); an absent
 *      key is the empty range (0, 0): what the filter range lookup returns for both sides.  When the positives themselves are in
 *      the index, a positive's own entity is rejected like every other known one.
 *   4. The first accepted try is the corruption.  If all max_tries tries are rejected, the LAST one is kept.
 *   5. Try 0 with AMDKGE_NEG_SIDE_UNIFORM, no pool and no ranges is amdkge_sample_corruptions' draw: the output is then equal to
 *      that call's bit for bit.
 * The result is a pure function of (seed, step, row, the tables of the call): it depends neither on the launch geometry nor on how
 * a global batch is cut into calls with row_offset / b_global.
 *
 *   d_side_thr : uint32 [n_rels], indexed by the positive's p; required for AMDKGE_NEG_SIDE_BERNOULLI, ignored otherwise
 *   d_pool     : NULL, or int32 [pool_n] entity ids, 1 <= pool_n < 2^32.  The ids are NOT checked here (nor by the train kernels):
 *                the caller validates them against the entity count.  Without a pool sample_range must be in [1, 2^32).
 *   ranges     : d_s_lo, d_s_hi, d_o_lo, d_o_hi int64 [B], d_s_ids, d_o_ids int32: all six set, or all six NULL (no rejection)
 *   max_tries  : 1 .. AMDKGE_NEG_MAX_TRIES
 *   d_stats    : NULL, or int64 [2], += (redraws, exhausted): redraws = the tries after try 0 that were made (a corruption that is
 *                accepted at try t, or exhausts at t = max_tries - 1, adds t); exhausted = the corruptions whose every try was
 *                rejected.  Integer adds: the sums do not depend on the order they arrive in.
 *
 * Errors (before any launch): AMDKGE_EINVAL for a NULL d_out / d_triples, negative B / eta, ranges given in part, max_tries out of
 * range, an unknown side_mode, BERNOULLI without d_side_thr, a pool with pool_n < 1 (or >= 2^32), a bad sample_range without a pool,
 * eta * b_global >= 2^56.  B == 0 or eta == 0: nothing is done. */
int amdkge_sample_negatives(const int32_t* d_triples, int64_t B, int32_t eta,
                            int64_t sample_base, int64_t sample_range, uint64_t seed, uint64_t step,
                            int64_t row_offset, int64_t b_global,
                            int32_t side_mode, const uint32_t* d_side_thr,
                            const int32_t* d_pool, int64_t pool_n,
                            const int64_t* d_s_lo, const int64_t* d_s_hi, const int32_t* d_s_ids,
                            const int64_t* d_o_lo, const int64_t* d_o_hi, const int32_t* d_o_ids,
                            int32_t max_tries, int64_t* d_stats, int32_t* d_out, void* stream);

/* The Bernoulli thresholds of AMDKGE_NEG_SIDE_BERNOULLI from a filter index (the two key arrays the filter index build makes):
 *     d_thr[p] = floor(2^32 * G_po(p) / (G_sp(p) + G_po(p)))          in exact integer arithmetic,
 * G_po(p) = the number of distinct (p, o) groups of relation p, G_sp(p) = the number of its distinct (s, p) groups.  With tph =
 * triples per (s, p) and hpt = triples per (p, o) of the relation this is tph / (tph + hpt), the probability of replacing the
 * subject: a 1-to-N relation mostly has its subject replaced, where a random subject rarely gives a true statement.
 *   d_po_keys : int64 [n_po] ascending, key = p * n_ents + o  (side S of the filter index build)
 *   d_sp_keys : int64 [n_sp], key = s * n_rels + p            (side O), n_sp < 2^31
 *   d_thr     : uint32 [n_rels] out.  A relation with no key in either array gets 0x80000000 (a fair coin).
 * Errors (before any launch): AMDKGE_EINVAL for a NULL d_thr, a NULL key array of non-zero length, negative sizes, n_ents or
 * n_rels < 1 or > 2^31 - 1, n_sp >= 2^31. */
int amdkge_negatives_side_thresholds(const int64_t* d_po_keys, int64_t n_po, const int64_t* d_sp_keys, int64_t n_sp,
                                     int64_t n_ents, int64_t n_rels, uint32_t* d_thr, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AMDKGE_NEGATIVES_H */
