/* libamdkge -- extension header: TYPE-CONSTRAINED negatives and evaluation (per-relation domain / range sets).
 *
 * An extension header like include/amdkge_lists.h (see there for why): entry points ADDED to ABI version 5 without changing one of
 * amdkge.h's, bound through ampligraph_amd/_ffi.py's TYPES_SIGNATURES table.  amdkge.h includes this header at its end; the ABI
 * version stays 5.  ("Extension headers".)
 *
 * A relation's DOMAIN is a set of entities that may stand as its subject, its RANGE a set that may stand as its object (the local
 * closed world of Krompass et al., ISWC 2015, when the sets are the subjects / objects observed with the relation; PyKEEN's and
 * LibKGE's type-constrained negatives; AmpliGraph 1.x's corruption_entities per relation).  Both are held as the CSR of the filter
 * index: ascending relation keys, a start offset per key, one id array with the ids ascending and duplicate-free inside a set.
 * The per-triple range lookup below gives (lo, hi) pairs into that id array; the list-ranking call of amdkge_lists.h takes exactly
 * such pairs as its candidates (type-constrained evaluation needs no kernel of its own), and amdkge_sample_negatives_typed draws
 * a training corruption inside them.
 */
#ifndef AMDKGE_TYPES_H
#define AMDKGE_TYPES_H

#include "amdkge.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The relation sets of the id triples d_triples int32 [m, 3], built on the device: the filter index build with the relation alone as
 * the group key.  Protocol, arrays, workspace (the filter build's workspace function) and limits are that call's.
 *   side     : AMDKGE_SIDE_S -- the DOMAIN CSR, the distinct subjects per relation (group p, value s);
 *              AMDKGE_SIDE_O -- the RANGE CSR, the distinct objects per relation (group p, value o)
 *   d_keys   : int64 [>= n_groups] out, the relations that occur, ascending        (capacity m is always enough)
 *   d_start  : int64 [>= n_groups + 1] out, set g is d_ids[d_start[g] .. d_start[g + 1])
 *   d_ids    : int32 [>= n_unique] out, ascending and duplicate-free inside a set
 *   d_counts : int64 [2] out = (n_groups, n_unique)
 * m == 0: d_start[0] = 0 and d_counts = (0, 0), nothing else is touched.
 * Errors: AMDKGE_EINVAL for a bad side, NULL pointers, negative sizes or m >= 2^32; AMDKGE_EUNSUPPORTED when n_rels * n_ents^2 does
 * not fit the packed 64-bit sort keys (the shared plan's limit). */
int amdkge_relation_sets_build(const int32_t* d_triples, int64_t m, int32_t side, int64_t n_ents, int64_t n_rels,
                               int64_t* d_keys, int64_t* d_start, int32_t* d_ids, int64_t* d_counts, void* d_work, void* stream);

/* Triple i of d_triples int32 [n, 3] gets (d_lo[i], d_hi[i]) = the range of ITS RELATION's set in the id array of a relation-set CSR
 * (d_keys int64 [n_keys] ascending, d_start int64 [n_keys + 1]) -- the domain and the range CSR are looked up the same way, their
 * key is the relation.  When the relation is absent from d_keys, or its set holds fewer than min_size ids, the triple gets the
 * FALLBACK range (fb_lo, fb_hi) instead: (0, 0) = "unconstrained" for the typed sampler, the range of an appended 0 .. N-1 block
 * for evaluation.  This lookup is the one place the min_size rule lives.
 * Errors: AMDKGE_EINVAL for negative n / n_keys / min_size, fb_lo < 0 or fb_hi < fb_lo, a NULL d_triples / d_lo / d_hi with n > 0,
 * NULL d_keys / d_start with n_keys > 0.  n == 0: nothing is done. */
int amdkge_relation_sets_ranges(const int64_t* d_keys, const int64_t* d_start, int64_t n_keys, const int32_t* d_triples, int64_t n,
                                int64_t min_size, int64_t fb_lo, int64_t fb_hi, int64_t* d_lo, int64_t* d_hi, void* stream);

/* The sampler of include/amdkge_negatives.h, amdkge_sample_negatives, with the replacement drawn INSIDE THE POSITIVE'S OWN CANDIDATE SET.  Every
 * argument of that call, in its order, then the candidate ranges, then the stream:
 *   d_cs_lo, d_cs_hi : int64 [B], d_cs_ids int32 -- positive i's subject candidates are d_cs_ids[d_cs_lo[i] .. d_cs_hi[i])
 *   d_co_lo, d_co_hi : int64 [B], d_co_ids int32 -- its object candidates; all six set, or all six NULL
 *   (a range holds fewer than 2^32 ids; what amdkge_relation_sets_ranges returns on a relation-set CSR.  The ids are NOT checked here:
 *   the caller validates them against the entity count, as it does a pool's.)
 *
 * THE DRAW of corruption (i, j).  row = j * b_global + row_offset + i (b_global <= 0: B).  Philox4x32-10 BLOCK b of the row is
 *     (x, y, z, w) = philox(counter = (row_lo, row_hi | b << 24, step_lo, step_hi), key = (seed_lo, seed_hi)),
 * lo / hi = the low / high 32 bits; eta * b_global must be < 2^56.
 *   1. The SIDE is decided once, from word x of block 0 (side_mode of amdkge_negatives.h), and never redrawn.
 *   2. Take the decided side's candidate range [lo, hi) of positive i.  TRY t = 0 .. max_tries - 1 takes its replacement from word
 *      1 + t % 3 (y, z, w) of block t / 3:
 *        hi > lo  :  ids[lo + mulhi32(word, hi - lo)]                                  (ids = d_cs_ids or d_co_ids)
 *        hi == lo (or the six candidate arrays NULL): the UNTYPED rule of amdkge_sample_negatives,
 *                    d_pool set:  d_pool[mulhi32(word, pool_n)]       otherwise:  sample_base + mulhi32(word, sample_range)
 *      (mulhi32(a, n) = (a * n) >> 32 on 64-bit integers).  A corruption drawn by the untyped rule adds 1 to `untyped`.
 *   3. A try is ACCEPTED when the replacement is not in the positive's FILTER range of the replaced side (d_s_* / d_o_*, as in
 *      amdkge_sample_negatives).
 *   4. The first accepted try is the corruption.  If all max_tries tries are rejected, the LAST one is kept.
 * The result is a pure function of (seed, step, row, the tables of the call): it depends neither on the launch geometry nor on how
 * a global batch is cut into calls with row_offset / b_global.  Two identities hold bit for bit:
 *   a. with the six candidate arrays NULL the output is amdkge_sample_negatives' (and untyped += B * eta);
 *   b. with every candidate range being the ascending ids 0 .. N-1 the output is amdkge_sample_negatives' with no pool,
 *      sample_base = 0, sample_range = N.
 *
 *   d_stats : NULL, or int64 [3], += (redraws, exhausted, untyped); redraws and exhausted as in amdkge_sample_negatives.
 *
 * Errors (before any launch): those of amdkge_sample_negatives -- a pool or a valid sample_range is required even when every range
 * is typed --, and AMDKGE_EINVAL for candidate arrays given in part.  B == 0 or eta == 0: nothing is done. */
int amdkge_sample_negatives_typed(const int32_t* d_triples, int64_t B, int32_t eta,
                                  int64_t sample_base, int64_t sample_range, uint64_t seed, uint64_t step,
                                  int64_t row_offset, int64_t b_global,
                                  int32_t side_mode, const uint32_t* d_side_thr,
                                  const int32_t* d_pool, int64_t pool_n,
                                  const int64_t* d_s_lo, const int64_t* d_s_hi, const int32_t* d_s_ids,
                                  const int64_t* d_o_lo, const int64_t* d_o_hi, const int32_t* d_o_ids,
                                  int32_t max_tries, int64_t* d_stats, int32_t* d_out,
                                  const int64_t* d_cs_lo, const int64_t* d_cs_hi, const int32_t* d_cs_ids,
                                  const int64_t* d_co_lo, const int64_t* d_co_hi, const int32_t* d_co_ids, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AMDKGE_TYPES_H */
