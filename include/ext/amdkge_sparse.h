/* libamdkge -- extension header: SPARSE OPTIMIZER MODE (the sweep of a shared-negative step over the rows the step can touch).
 *
 * Three entry points ADDED to ABI version 5 without changing one of amdkge.h's, bound through ampligraph_amd/_ffi.py's ABI_EXT
 * table.  The headers directly under include/ are a closed set; this one lives under include/ext/ and a caller includes it by name
 * ("ext/amdkge_sparse.h").  The ABI version stays 5.
 *
 * WHY.  A shared-negative step (include/amdkge_shared.h, amdkge_shared_mask.h, amdkge_shared_dist.h) adds gradient to at most
 * 2 * B + n_groups * M entity rows, and ends in amdkge_opt_step, which walks the whole [N, K] table: densely, or with opt->lazy row
 * by row -- but also then it reads the whole gradient table to find the rows that are not zero.  The two calls below never walk
 * anything of size N * K: the first names the rows the step CAN have touched, the second sweeps those rows and nothing else.
 *
 * THE CANDIDATE SET of a step: the ascending, duplicate-free union of the subjects s_i and the objects o_i of the step's B positives
 * and the n_ids entity ids of its lists (every group's list; for a list that all groups share, one copy of it).  Every entity row
 * the step's backward call, a batch regulariser (amdkge_batch_reg.h) and the relation-prediction term
 * (amdkge_relation_objective.h) add gradient to is a candidate; a candidate need not have received any.
 *
 * THE SWEEP of a list of rows is amdkge_opt_step with opt->lazy restricted to the listed rows: per listed row, one wave reads the
 * gradient row; a row whose fp32 gradient row is entirely zero is left alone (x, the slots and the regulariser are not read); any
 * other row goes float by float through the update rule and the whole-table LP terms of the descriptor exactly as in
 * amdkge_opt_step, its gradient row is reset to zero and lambda * sum |x|^p (+ the second term) of its floats before the update
 * is added to *d_reg_loss.  The arithmetic per float is that of amdkge_opt_step bit for bit: on a list that holds every row whose
 * gradient is not zero, x, both slots and the gradient table end with the bits amdkge_opt_step with lazy = 1 over the whole table
 * gives them; *d_reg_loss is a sum of the same terms in no fixed order.  A row that is NOT listed keeps every bit, its gradient
 * row included.
 * So a training loop that sweeps every step's candidate set keeps the gradient table all-zero between steps without anybody
 * clearing N rows.
 */
#ifndef AMDKGE_SPARSE_H
#define AMDKGE_SPARSE_H

#include "../amdkge.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of d_work amdkge_step_rows needs for n_keys = 2 * B + n_ids keys over a table of n_ents rows (a function of both sizes
 * only; > 0); -1 for n_ents outside [1, 2^31 - 1] or n_keys outside [0, 2^31 - 1]. */
int64_t amdkge_step_rows_workspace_bytes(int64_t n_ents, int64_t n_keys);

/* The candidate set: d_rows[0 .. n) = the ascending unique union of { s_i, o_i : i < B } and d_ids[0 .. n_ids), d_n_rows[0] = n.
 * A radix sort of the 2 * B + n_ids keys (only the bits n_ents needs) and a compaction: the cost does not depend on n_ents, no
 * table is read, nothing is synchronised with the host.
 *   d_triples : int32 [B, 3] (columns s, p, o; p is not read); may be NULL when B == 0
 *   d_ids     : int32 [n_ids]; may be NULL when n_ids == 0
 *   d_rows    : int32 [cap], entries at and beyond n are not written;  d_n_rows : int64 [1]
 *   d_work    : amdkge_step_rows_workspace_bytes(n_ents, 2 * B + n_ids) bytes, contents undefined before and after; it may start
 *               anywhere (the library aligns it up to 256 bytes itself, the size includes that slack)
 * An id outside [0, n_ents) is an argument error of the caller that cannot be seen from the host: it is skipped and never used as
 * an index.  B == 0 and n_ids == 0: n = 0.
 * Errors (before any launch): AMDKGE_EINVAL for n_ents outside [1, 2^31 - 1], B < 0, n_ids < 0, 2 * B + n_ids > 2^31 - 1,
 * cap < min(2 * B + n_ids, n_ents) (n can be that large), NULL d_rows with cap > 0, NULL d_n_rows, and with 2 * B + n_ids > 0 NULL
 * d_work, NULL d_triples with B > 0, NULL d_ids with n_ids > 0. */
int amdkge_step_rows(int64_t n_ents, const int32_t* d_triples, int64_t B, const int32_t* d_ids, int64_t n_ids,
                     int32_t* d_rows, int64_t cap, int64_t* d_n_rows, void* d_work, void* stream);

/* The sweep of the rows d_rows[0 .. d_n_rows[0]) of ONE table of n_table_rows rows of opt->row_floats floats each.
 *   opt        : as for amdkge_opt_step; opt->row_floats is required (a multiple of 4, >= 4: the padded layout), opt->lazy is
 *                ignored -- the sweep is row-wise whatever it says
 *   d_x, d_grad, d_slot0, d_slot1 : the WHOLE table, its gradient and its optimizer slots (those the kind keeps; NULL otherwise),
 *                16-byte aligned
 *   d_rows     : int32 [cap], STRICTLY ASCENDING in [0, d_n_rows[0]) -- a row listed twice would be swept by two waves at once.
 *                A listed id outside [0, n_table_rows) is skipped.  Entries at and beyond d_n_rows[0] are never read.
 *   d_n_rows   : int64 [1], read on the device (a count above cap is taken as cap, a negative one as 0); cap sizes the grid
 *   d_reg_loss : NULL or double [1], the regulariser value of the swept rows is ADDED
 * One wave per listed row, grid-stride; every offset is 64-bit (a row's offset, its id times row_floats, passes 2^31 on large
 * tables).  Nothing of the table besides the listed rows is read or written.
 * Errors (before any launch): those of amdkge_opt_step's descriptor checks; AMDKGE_EINVAL for row_floats that is not a multiple of 4
 * or < 4, n_table_rows < 0, cap < 0, NULL d_x / d_grad, a NULL slot the kind keeps, buffers that are not 16-byte aligned, and with
 * cap > 0 NULL d_rows / d_n_rows.  cap == 0 or n_table_rows == 0: nothing is done. */
int amdkge_opt_step_rows(const amdkge_opt* opt, float* d_x, float* d_grad, float* d_slot0, float* d_slot1, int64_t n_table_rows,
                         const int32_t* d_rows, const int64_t* d_n_rows, int64_t cap, double* d_reg_loss, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AMDKGE_SPARSE_H */
