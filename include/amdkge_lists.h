/* libamdkge -- extension header: ranking against PER-TRIPLE candidate lists.
 *
 * Why a second header: include/amdkge.h is the frozen declaration set of ABI version 5 -- its entry points are bound one for one by
 * ampligraph_amd/_ffi.py's SIGNATURES table, and each has a guard-band case.  Entry points ADDED to that ABI without changing any
 * existing one are declared in extension headers such as this one (bound through _ffi.py's EXT_SIGNATURES), which include
 * amdkge.h for the types and which amdkge.h includes at its end, so that a client still needs one #include.  The ABI version
 * stays 5: a client built against amdkge.h alone keeps working, and one that needs the entry points below can test for them with
 * dlsym.  ("Extension headers".)
 */
#ifndef AMDKGE_LISTS_H
#define AMDKGE_LISTS_H

#include "amdkge.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Ranks against per-triple candidate lists: sampled negatives (ogbl-wikikg2 ships 500 heads and 500 tails per test triple),
 * re-ranking the output of a first retrieval stage, type-constrained evaluation.  The counts / filter / compose steps of get_ranks
 * (AbstractScoringLayer.py:156-422) with the candidate set of amdkge_rank_counts replaced by a list per triple.
 *
 *   d_ent, n_ents : the entity table and its number of rows; d_rel: the relation table (stored layout, as everywhere)
 *   d_triples     : int32 [n, 3]
 *   side          : AMDKGE_SIDE_S | AMDKGE_SIDE_O -- which element the candidates replace
 *   candidates    : triple i's candidates are the table rows d_cand_ids[d_cand_lo[i] .. d_cand_hi[i]) -- a CSR when lo = off[i],
 *                   hi = off[i + 1]; a dense [n, C] block when lo = i * C, hi = (i + 1) * C.  EVERY OCCURRENCE is a candidate of its
 *                   own (a repeated id counts twice, as in amdkge_rank_counts' d_ent_ids).  An id outside [0, n_ents) is NOT a
 *                   candidate and its row is never dereferenced: ragged lists may be padded with -1.
 *   max_len       : an upper bound of hi - lo the caller knows.  It only plans the launch: a longer list is still walked
 *                   completely.  max_len == 0 or n == 0: nothing is done.
 *   d_counts      : int32 [n, 2], += (#candidates with q(pos) < q(cand), #candidates with q(pos) == q(cand)), q = the quantised
 *                   score int32(score * 1000) of amdkge_rank_counts, through the same accumulation chain: a list that is the id
 *                   range 0 .. n_ents - 1 gives amdkge_rank_counts' counts, bit for bit.
 *   filter        : d_flt_lo, d_flt_hi, d_flt_ids are all set or all NULL.  Triple i's known positives are
 *                   d_flt_ids[d_flt_lo[i] .. d_flt_hi[i]), ASCENDING inside a range: what the filter index build and its range
 *                   lookup produce.  d_sub int32 [n] (may be NULL without a filter), += the number of candidate occurrences whose
 *                   id is in that range and whose quantised score is >= q(pos) -- always ">=", whatever the tie strategy
 *                   (AbstractScoringLayer.py:292-303).  The rank-compose call on (d_counts, d_sub) then gives the rank: on
 *                   duplicate-free lists the reference's evaluate(x[i], entities_subset = list i, use_filter = ...) rank.
 *                   DUPLICATES: a known positive listed twice is subtracted twice here (each occurrence was also counted
 *                   twice), where the reference, whose subset is a set, subtracts it once.
 *   d_scores      : NULL, or float parallel to d_cand_ids: position p gets the un-quantised score of its (triple, entity) -- the
 *                   bits the 1-vs-all corruption-score call gives that pair --, -inf where the id is no candidate.  Positions
 *                   outside every [lo, hi) are not written.
 *   d_work        : amdkge_rank_lists_workspace_bytes(m, n) bytes (= the rank workspace of n triples; like it, aligned up by the library)
 *
 * Errors: AMDKGE_EINVAL before any launch for a NULL pointer, a negative size, a filter given in part, a bad side;
 * AMDKGE_EUNSUPPORTED for RotatE's exact mode on rows that are not stored padded (k_pad = the padded k), as the filter pass. */
int64_t amdkge_rank_lists_workspace_bytes(const amdkge_model* m, int64_t n);
int amdkge_rank_lists(const amdkge_model* m, const float* d_ent, const float* d_rel, int64_t n_ents,
                      const int32_t* d_triples, int64_t n, int32_t side,
                      const int64_t* d_cand_lo, const int64_t* d_cand_hi, const int32_t* d_cand_ids, int64_t max_len,
                      const int64_t* d_flt_lo, const int64_t* d_flt_hi, const int32_t* d_flt_ids,
                      int32_t* d_counts, int32_t* d_sub, float* d_scores, void* d_work, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AMDKGE_LISTS_H */
