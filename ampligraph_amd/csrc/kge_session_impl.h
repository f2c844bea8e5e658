// Private to the session translation units (kge_session.hip, kge_session_group.hip): the state behind the opaque handle and the one
// copy of every building block a step or a rank call is composed of (bodies in kge_session.hip).
#pragma once
#include <vector>

#include "kge_opt.h"

#define KGE_HIP(call, what) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return kge::set_error_hip(e_, what); } while (0)
#define KGE_RC(call) do { const int rc_ = (call); if (rc_ != AMDKGE_OK) return rc_; } while (0)
#define KGE_HIDDEN __attribute__((visibility("hidden")))

struct amdkge_session {
    amdkge_session_config cfg;   // cfg.model.k_pad = amdkge_padded_k(k): the session owns the tables and stores them padded
    int K = 0;                   // floats per DENSE row (what the host hands over and gets back)
    int Ks = 0;                  // floats per STORED row
    hipStream_t st = nullptr;
    float* tab[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // AMDKGE_TABLE_* order
    float* g_ent = nullptr;
    float* g_rel = nullptr;
    double* acc = nullptr;          // [data loss, regulariser loss]
    void* twork = nullptr;          // owner-computes workspace (zero-filled when (re)allocated): session_twork / session_drop_twork only
    int64_t twork_bytes = 0;
    void* buf[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // growable scratch
    int64_t buf_bytes[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t step = 0;
    int64_t iteration = 0;
    std::vector<int32_t> hot_ids;   // AMDKGE_TILED_HOT_ROWS: declared hot rows, (re)applied whenever the workspace is (re)allocated
    bool hot_dirty = false;
    bool screen_ran = false;        // the last amdkge_session_rank went through the int8 screening pass
    int32_t screen_stats[2] = {0, 0};   // its {rechecked pairs, fell back to the exact kernel} (last side)
};

inline bool is_entity_table(int t) { return t == AMDKGE_TABLE_ENT || t == AMDKGE_TABLE_ENT_SLOT0 || t == AMDKGE_TABLE_ENT_SLOT1; }
// get_ranks wants this side (AMDKGE_SIDE_*) for corrupt_side (AMDKGE_CORRUPT_*)
inline bool rank_side_wanted(int side, int32_t corrupt_side) { return side == AMDKGE_SIDE_S ? corrupt_side != AMDKGE_CORRUPT_O : corrupt_side != AMDKGE_CORRUPT_S; }

// ---- building blocks of a step ------------------------------------------------------------------------------------------------------
// host triples against tables of n_ents / n_rels rows: AMDKGE_EINVAL "<who>: triple <i> has ..." for the first one outside
KGE_HIDDEN int session_check_triples(const int32_t* t, int64_t n, int64_t n_ents, int64_t n_rels, const char* who);
// the workspace size the owner-computes pair reports for model `m` and batch b (0: shapes the pair does not cover); s->twork is grown
// (zero-filled, the hot-row map marked for re-application) when it is smaller.  session_drop_twork: after a failed launch the
// bookkeeping may be dirty -- start from a fresh zeroed buffer next time.
KGE_HIDDEN int session_twork(amdkge_session* s, const amdkge_model* m, int64_t b, int64_t* need);
KGE_HIDDEN void session_drop_twork(amdkge_session* s);
// the loss descriptor of a step without FocusE weights: FocusE off
inline amdkge_loss session_step_loss(const amdkge_session* s) {
    amdkge_loss loss = s->cfg.loss;
    loss.focus_nonlinearity = AMDKGE_FOCUS_OFF; loss.d_focus_w = nullptr;
    return loss;
}
// ... of a step or share of b positives: host FocusE weights focus_w[lo, lo + b) ride in scratch slot 1; none: as above
// (`whose` names the owner of the loss in the message for weights given to a loss without a non-linearity)
KGE_HIDDEN int session_step_loss(amdkge_session* s, const float* focus_w, int64_t lo, int64_t b, const char* who, const char* whose, amdkge_loss* out);
// the gradient kernels of a share of b device triples on the model `m` the kernels should see: the owner-computes pair where it covers
// the shape (apply_update = 1: the complete step, optimizer included; 0: gradients only, null slot tables), else the atomic
// forward/backward (gradients only either way -- the caller sweeps); *tiled (optional) tells which ran.  Hot rows are (re)applied when flags carry
// AMDKGE_TILED_HOT_ROWS.  A failed launch drops the workspace.
KGE_HIDDEN int session_share_kernels(amdkge_session* s, const amdkge_model* m, const amdkge_loss* loss, const amdkge_opt* opt, const int32_t* d_tri, int64_t b,
                                     int64_t sample_range, uint64_t step, int64_t row_offset, int64_t b_global, const int32_t* d_neg_override,
                                     int32_t apply_update, int32_t flags, double* d_loss, double* d_reg, bool* tiled);
// the dense sweep with whatever the gradient buffers hold: n_rows rows of the entity table (none: skipped), then the relation table
// with the optimizer derived for it; the regulariser terms go to d_reg_ent / d_reg_rel
KGE_HIDDEN int session_dense_sweep(amdkge_session* s, const amdkge_opt* opt, int64_t n_rows, double* d_reg_ent, double* d_reg_rel);
// n ranks of a chunk from d_ranks (as amdkge_rank_compose left them for corrupt_side) to the host; synchronises.  s+o: the two 0-based
// sides are summed, then +1 (ScoringBasedEmbeddingModel.py:1459-1463,1684)
KGE_HIDDEN int session_ranks_to_host(amdkge_session* s, const int32_t* d_ranks, int64_t n, int32_t corrupt_side, int32_t* ranks_out);

// The three phases of a data-parallel step on one replica (kge_session.hip; used by the session group): gradients of the
// replica's share of a global batch (nothing is updated), the dense sweep over both tables with whatever the gradient
// buffers then hold, and the read-back of the loss accumulators (synchronises; counts the step).
KGE_HIDDEN int amdkge_session_grad_step(amdkge_session* s, const int32_t* triples, int64_t b, const float* focus_w, int64_t row_offset, int64_t b_global);
KGE_HIDDEN int amdkge_session_apply_step(amdkge_session* s);
KGE_HIDDEN int amdkge_session_finish_step(amdkge_session* s, double (&h)[2]);

// Evaluation pieces shared with the session group (kge_session.hip): one side's counts + filter subtractions for device-resident
// triples against candidate rows [ent_lo, ent_hi) of the model `m` the kernels should see (d_counts3_out: int32 [n, 2] counts then
// [n] subtractions, in the session's scratch, valid until its next rank call), and the host-side validation of a filter CSR.
KGE_HIDDEN int amdkge_session_count_side(amdkge_session* s, const amdkge_model* m, const int32_t* d_tri, int64_t n, int32_t side,
                                         const int64_t* off, const int32_t* ids, int64_t id_shift, int64_t id_limit,
                                         const int32_t* d_ent_ids, const int32_t* d_subset_pos, int64_t ent_lo, int64_t ent_hi,
                                         int32_t** d_counts3_out);
KGE_HIDDEN int amdkge_session_scratch(amdkge_session* s, int slot, int64_t bytes, void** out);   // growable scratch slot (contents undefined)
KGE_HIDDEN int amdkge_session_check_filter(const int64_t* off, const int32_t* ids, int64_t n, int64_t n_ents, const char* who);

// The column-sharded step on one replica (kge_session.hip; session group with AMDKGE_GROUP_COLS): A -- the slice's partial score sums of
// the whole batch into the session's score buffer (device pointer returned; the group sums the buffers over the replicas); B + C --
// loss on the complete sums, then backward / merge / optimizer on the slice (amdkge_session_finish_step reads the accumulators).
KGE_HIDDEN int amdkge_session_cols_scores(amdkge_session* s, const int32_t* triples, int64_t B, float** d_scores_out);
KGE_HIDDEN int amdkge_session_cols_apply(amdkge_session* s, int64_t B);
