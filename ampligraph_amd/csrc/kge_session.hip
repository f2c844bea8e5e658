// Session layer of the C ABI (include/amdkge.h): an opaque handle that owns the HBM-resident state of one model and
// drives the device-pointer entry points with HOST buffers in and out, so that a host without torch (the reference's
// numpy-level Python through ctypes) can train, score and rank.  Pure composition: every computation is one of the entry
// points of the other translation units.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kge_group_staging.h"
#include "kge_session_impl.h"

using namespace kge;

namespace {

int64_t table_rows(const amdkge_session* s, int t) { return is_entity_table(t) ? s->cfg.model.n_ents : s->cfg.model.n_rels; }

// scratch slot `i` with at least `bytes` bytes (contents undefined)
int scratch(amdkge_session* s, int i, int64_t bytes, void** out) {
    if (bytes > s->buf_bytes[i]) {
        if (s->buf[i]) KGE_HIP(hipFree(s->buf[i]), "hipFree(scratch)");
        s->buf[i] = nullptr; s->buf_bytes[i] = 0;
        KGE_HIP(hipMalloc(&s->buf[i], (size_t)bytes), "hipMalloc(scratch)");
        s->buf_bytes[i] = bytes;
    }
    *out = s->buf[i];
    return AMDKGE_OK;
}

int upload(amdkge_session* s, int slot, const void* host, int64_t bytes, void** d) {
    KGE_RC(scratch(s, slot, bytes > 0 ? bytes : 16, d));
    if (bytes > 0) KGE_HIP(hipMemcpyAsync(*d, host, (size_t)bytes, hipMemcpyHostToDevice, s->st), "hipMemcpyAsync(H2D)");
    return AMDKGE_OK;
}

amdkge_opt step_opt(const amdkge_session* s) {
    amdkge_opt opt = s->cfg.opt;
    opt.iteration = s->iteration + 1;
    return opt;
}

__global__ void gather_rows_kernel(const float* src, const int32_t* ids, int64_t n, int K, float* dst) {
    const int64_t r = blockIdx.x;
    const float* row = src + (int64_t)ids[r] * K;
    for (int c = threadIdx.x; c < K; c += blockDim.x) dst[r * K + c] = row[c];
}

}  // namespace

// ---- building blocks of a step (kge_session_impl.h) -----------------------------------------------------------------------
// ids arrive from the host and are checked, O(n) on host memory, before anything is uploaded (kge_group_staging.h)
int session_check_triples(const int32_t* t, int64_t n, int64_t n_ents, int64_t n_rels, const char* who) {
    const int64_t i = first_bad_triple(t, n, n_ents, n_rels);
    if (i < 0) return AMDKGE_OK;
    static thread_local char msg[160];
    snprintf(msg, sizeof(msg), "%s: triple %lld has an entity / relation id outside the tables", who, (long long)i);
    return set_error(AMDKGE_EINVAL, msg);
}

int session_twork(amdkge_session* s, const amdkge_model* m, int64_t b, int64_t* need) {
    *need = amdkge_train_tiled_workspace_bytes(m, b, s->cfg.eta);
    if (*need <= s->twork_bytes) return AMDKGE_OK;
    if (s->twork) KGE_HIP(hipFree(s->twork), "hipFree(twork)");
    s->twork = nullptr; s->twork_bytes = 0;
    KGE_HIP(hipMalloc(&s->twork, (size_t)*need), "hipMalloc(twork)");
    KGE_HIP(hipMemsetAsync(s->twork, 0, (size_t)*need, s->st), "hipMemsetAsync(twork)");
    s->twork_bytes = *need;
    s->hot_dirty = !s->hot_ids.empty();
    return AMDKGE_OK;
}

void session_drop_twork(amdkge_session* s) {
    if (s->twork) (void)hipFree(s->twork);
    s->twork = nullptr; s->twork_bytes = 0;
}

int session_step_loss(amdkge_session* s, const float* focus_w, int64_t lo, int64_t b, const char* who, const char* whose, amdkge_loss* out) {
    *out = session_step_loss(s);
    if (!focus_w) return AMDKGE_OK;
    if (!s->cfg.loss.focus_nonlinearity) {
        static thread_local char msg[160];
        snprintf(msg, sizeof(msg), "%s: FocusE weights given but the %s's loss has focus_nonlinearity == 0", who, whose);
        return set_error(AMDKGE_EINVAL, msg);
    }
    void* d_fw;
    KGE_RC(upload(s, 1, focus_w + lo, b * (int64_t)sizeof(float), &d_fw));
    out->focus_nonlinearity = s->cfg.loss.focus_nonlinearity;
    out->d_focus_w = (const float*)d_fw;
    return AMDKGE_OK;
}

int session_share_kernels(amdkge_session* s, const amdkge_model* m, const amdkge_loss* loss, const amdkge_opt* opt, const int32_t* d_tri, int64_t b,
                          int64_t sample_range, uint64_t step, int64_t row_offset, int64_t b_global, const int32_t* d_neg_override,
                          int32_t apply_update, int32_t flags, double* d_loss, double* d_reg, bool* tiled) {
    int64_t need = 0;
    KGE_RC(session_twork(s, m, b, &need));
    if (tiled) *tiled = need > 0;
    if (need <= 0)   // shapes the pair does not cover
        return amdkge_train_fwdbwd(m, loss, s->tab[0], s->tab[1], d_tri, b, s->cfg.eta, 0, sample_range, s->cfg.seed, step, row_offset, b_global,
                                   d_neg_override, s->g_ent, s->g_rel, d_loss, nullptr, nullptr, s->st);
    if ((flags & AMDKGE_TILED_HOT_ROWS) && s->hot_dirty) {
        void* d_hot;
        KGE_RC(upload(s, 6, s->hot_ids.data(), (int64_t)(s->hot_ids.size() * sizeof(int32_t)), &d_hot));   // (scratch slot of its own)
        KGE_RC(amdkge_train_tiled_set_hot_rows(m, s->twork, (const int32_t*)d_hot, (int32_t)s->hot_ids.size(), s->st));
        s->hot_dirty = false;
    }
    float* const* t = s->tab;
    const int rc = amdkge_train_step_tiled(m, loss, opt, t[0], t[1], apply_update ? t[2] : nullptr, apply_update ? t[3] : nullptr,
                                           apply_update ? t[4] : nullptr, apply_update ? t[5] : nullptr, apply_update ? s->cfg.rel_reg_lambda : 0.f,
                                           d_tri, b, s->cfg.eta, 0, sample_range, s->cfg.seed, step, row_offset, b_global, d_neg_override,
                                           s->g_ent, s->g_rel, apply_update, flags, d_loss, d_reg, nullptr, nullptr, s->twork, s->st);
    if (rc != AMDKGE_OK) session_drop_twork(s);
    return rc;
}

int session_dense_sweep(amdkge_session* s, const amdkge_opt* opt, int64_t n_rows, double* d_reg_ent, double* d_reg_rel) {
    if (n_rows > 0) KGE_RC(amdkge_opt_step(opt, s->tab[0], s->g_ent, s->tab[2], s->tab[3], n_rows * (int64_t)s->Ks, d_reg_ent, s->st));
    amdkge_opt orel = *opt;
    orel.reg_lambda = s->cfg.rel_reg_lambda;
    if (opt->rel_reg_p > 0) orel.reg_p = opt->rel_reg_p;
    orel.reg2_p = opt->rel_reg2_p; orel.reg2_lambda = opt->rel_reg2_lambda;
    return amdkge_opt_step(&orel, s->tab[1], s->g_rel, s->tab[4], s->tab[5], s->cfg.model.n_rels * (int64_t)s->Ks, d_reg_rel, s->st);
}

int session_ranks_to_host(amdkge_session* s, const int32_t* d_ranks, int64_t n, int32_t corrupt_side, int32_t* ranks_out) {
    const bool sum = corrupt_side == AMDKGE_CORRUPT_S_PLUS_O;
    const size_t cols = (sum || corrupt_side == AMDKGE_CORRUPT_S_O) ? 2 : 1;
    std::vector<int32_t> h(sum ? (size_t)2 * n : 0);
    KGE_HIP(hipMemcpyAsync(sum ? h.data() : ranks_out, d_ranks, (size_t)n * cols * sizeof(int32_t), hipMemcpyDeviceToHost, s->st), "hipMemcpyAsync(D2H)");
    KGE_HIP(hipStreamSynchronize(s->st), "hipStreamSynchronize");
    for (int64_t i = 0; sum && i < n; ++i) ranks_out[i] = h[(size_t)i] + h[(size_t)(n + i)] - 1;
    return AMDKGE_OK;
}

extern "C" void amdkge_session_destroy(amdkge_session* s) {
    if (!s) return;
    (void)hipSetDevice(s->cfg.device);
    if (s->st) (void)hipStreamSynchronize(s->st);
    for (float* p : s->tab) if (p) (void)hipFree(p);
    if (s->g_ent) (void)hipFree(s->g_ent);
    if (s->g_rel) (void)hipFree(s->g_rel);
    if (s->acc) (void)hipFree(s->acc);
    session_drop_twork(s);
    for (void* p : s->buf) if (p) (void)hipFree(p);
    if (s->st) (void)hipStreamDestroy(s->st);
    delete s;
}

extern "C" int amdkge_session_create(const amdkge_session_config* cfg, amdkge_session** out) try {
    if (!cfg || !out) return set_error(AMDKGE_EINVAL, "session_create: NULL argument");
    *out = nullptr;
    KGE_RC(validate_model(&cfg->model));
    if (cfg->loss.kind < 0 || cfg->loss.kind > AMDKGE_LOSS_MULTICLASS_NLL) return set_error(AMDKGE_EINVAL, "session_create: unknown loss kind");
    amdkge_opt o = cfg->opt;
    o.iteration = 1;
    KGE_RC(validate_opt(&o));
    if (cfg->eta < 1) return set_error(AMDKGE_EINVAL, "session_create: eta must be >= 1");
    KGE_HIP(hipSetDevice(cfg->device), "hipSetDevice");
    amdkge_session* s = new amdkge_session();
    s->cfg = *cfg;
    s->cfg.loss.d_focus_w = nullptr;
    s->cfg.model.k_pad = amdkge_padded_k(cfg->model.k);   // every k gets the 16-byte kernels; hosts only ever see dense rows
    s->K = amdkge_internal_k(cfg->model.scoring_type, cfg->model.k);
    s->Ks = row_floats(&s->cfg.model);
    s->cfg.opt.row_floats = s->Ks;   // touched-rows mode (cfg.opt.lazy) sweeps whole stored rows
    const int64_t ne = cfg->model.n_ents * (int64_t)s->Ks, nr = cfg->model.n_rels * (int64_t)s->Ks;
    const int nslots = opt_nslots(cfg->opt.kind);
    auto fail = [&](int rc) { amdkge_session_destroy(s); return rc; };
    hipError_t e = hipStreamCreate(&s->st);
    if (e != hipSuccess) return fail(set_error_hip(e, "hipStreamCreate"));
    auto alloc = [&](float** p, int64_t n, float fill) -> int {
        hipError_t e2 = hipMalloc((void**)p, (size_t)n * sizeof(float));
        if (e2 != hipSuccess) return set_error_hip(e2, "hipMalloc(table)");
        uint32_t bits; memcpy(&bits, &fill, 4);
        e2 = hipMemsetD32Async((hipDeviceptr_t)*p, (int)bits, (size_t)n, s->st);
        return e2 == hipSuccess ? AMDKGE_OK : set_error_hip(e2, "hipMemsetD32Async");
    };
    // Keras legacy Adagrad starts its accumulator at 0.1; every other state tensor at 0
    const float fill0 = cfg->opt.kind == AMDKGE_OPT_ADAGRAD ? 0.1f : 0.f;
    int rc = alloc(&s->tab[AMDKGE_TABLE_ENT], ne, 0.f);
    if (!rc) rc = alloc(&s->tab[AMDKGE_TABLE_REL], nr, 0.f);
    if (!rc) rc = alloc(&s->g_ent, ne, 0.f);
    if (!rc) rc = alloc(&s->g_rel, nr, 0.f);
    if (!rc && nslots >= 1) rc = alloc(&s->tab[AMDKGE_TABLE_ENT_SLOT0], ne, fill0);
    if (!rc && nslots >= 1) rc = alloc(&s->tab[AMDKGE_TABLE_REL_SLOT0], nr, fill0);
    if (!rc && nslots == 2) rc = alloc(&s->tab[AMDKGE_TABLE_ENT_SLOT1], ne, 0.f);
    if (!rc && nslots == 2) rc = alloc(&s->tab[AMDKGE_TABLE_REL_SLOT1], nr, 0.f);
    if (rc) return fail(rc);
    e = hipMalloc((void**)&s->acc, 2 * sizeof(double));
    if (e != hipSuccess) return fail(set_error_hip(e, "hipMalloc(acc)"));
    e = hipStreamSynchronize(s->st);
    if (e != hipSuccess) return fail(set_error_hip(e, "hipStreamSynchronize"));
    *out = s;
    return AMDKGE_OK;
} KGE_CATCH("session_create")

extern "C" int amdkge_session_set_rows(amdkge_session* s, int32_t table, int64_t row0, int64_t nrows, const float* host) try {
    if (!s || table < 0 || table > 5 || !s->tab[table]) return set_error(AMDKGE_EINVAL, "session_set_rows: no such table (optimizer without that state tensor?)");
    if (row0 < 0 || nrows < 0 || row0 + nrows > table_rows(s, table)) return set_error(AMDKGE_EINVAL, "session_set_rows: rows outside the table");
    if (nrows == 0) return AMDKGE_OK;
    if (!host) return set_error(AMDKGE_EINVAL, "session_set_rows: NULL host buffer");
    KGE_HIP(hipSetDevice(s->cfg.device), "hipSetDevice");
    void* d_dense;
    KGE_RC(upload(s, 1, host, nrows * s->K * (int64_t)sizeof(float), &d_dense));
    KGE_RC(amdkge_pack_rows(&s->cfg.model, (const float*)d_dense, nrows, s->tab[table] + row0 * s->Ks, s->st));
    KGE_HIP(hipStreamSynchronize(s->st), "hipStreamSynchronize");
    return AMDKGE_OK;
} KGE_CATCH("session_set_rows")

extern "C" int amdkge_session_get_rows(amdkge_session* s, int32_t table, const int32_t* ids, int64_t row0, int64_t nrows, float* host) try {
    if (!s || table < 0 || table > 5 || !s->tab[table]) return set_error(AMDKGE_EINVAL, "session_get_rows: no such table (optimizer without that state tensor?)");
    if (nrows < 0) return set_error(AMDKGE_EINVAL, "session_get_rows: nrows must be >= 0");
    if (nrows == 0) return AMDKGE_OK;
    if (!host) return set_error(AMDKGE_EINVAL, "session_get_rows: NULL host buffer");
    KGE_HIP(hipSetDevice(s->cfg.device), "hipSetDevice");
    const float* src;
    if (ids) {
        const int64_t rows = table_rows(s, table);
        for (int64_t i = 0; i < nrows; ++i)
            if (ids[i] < 0 || ids[i] >= rows) return set_error(AMDKGE_EINVAL, "session_get_rows: row id outside the table");
        void *d_ids, *d_tmp;
        KGE_RC(upload(s, 0, ids, nrows * (int64_t)sizeof(int32_t), &d_ids));
        KGE_RC(scratch(s, 1, nrows * s->Ks * (int64_t)sizeof(float), &d_tmp));
        hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)nrows), dim3(256), 0, s->st, s->tab[table], (const int32_t*)d_ids, nrows, s->Ks, (float*)d_tmp);
        KGE_RC(check_launch("gather_rows"));
        src = (const float*)d_tmp;
    } else {
        if (row0 < 0 || row0 + nrows > table_rows(s, table)) return set_error(AMDKGE_EINVAL, "session_get_rows: rows outside the table");
        src = s->tab[table] + row0 * s->Ks;
    }
    void* d_dense;
    KGE_RC(scratch(s, 7, nrows * s->K * (int64_t)sizeof(float), &d_dense));
    KGE_RC(amdkge_unpack_rows(&s->cfg.model, src, nrows, (float*)d_dense, s->st));
    KGE_HIP(hipMemcpyAsync(host, d_dense, (size_t)nrows * s->K * sizeof(float), hipMemcpyDeviceToHost, s->st), "hipMemcpyAsync(D2H)");
    KGE_HIP(hipStreamSynchronize(s->st), "hipStreamSynchronize");
    return AMDKGE_OK;
} KGE_CATCH("session_get_rows")

extern "C" int amdkge_session_train_step(amdkge_session* s, const int32_t* triples, int64_t B, const float* focus_w, double* loss_out) try {
    if (!s || B < 0) return set_error(AMDKGE_EINVAL, "session_train_step: bad arguments");
    if (loss_out) *loss_out = 0.0;
    if (B == 0) return AMDKGE_OK;   // (the reference never produces an empty batch; nothing happens, no step is counted)
    if (!triples) return set_error(AMDKGE_EINVAL, "session_train_step: NULL triples");
    KGE_RC(session_check_triples(triples, B, s->cfg.model.n_ents, s->cfg.model.n_rels, "session_train_step"));
    KGE_HIP(hipSetDevice(s->cfg.device), "hipSetDevice");
    const amdkge_model* m = &s->cfg.model;
    void* d_tri;
    KGE_RC(upload(s, 0, triples, B * 3 * (int64_t)sizeof(int32_t), &d_tri));
    amdkge_loss loss;
    KGE_RC(session_step_loss(s, focus_w, 0, B, "session_train_step", "session", &loss));
    const amdkge_opt opt = step_opt(s);
    KGE_HIP(hipMemsetAsync(s->acc, 0, 2 * sizeof(double), s->st), "hipMemsetAsync");
    const int32_t step_flags = s->cfg.flags | (s->hot_ids.empty() ? 0 : AMDKGE_TILED_HOT_ROWS);
    bool tiled = false;
    KGE_RC(session_share_kernels(s, m, &loss, &opt, (const int32_t*)d_tri, B, m->n_ents, s->step, 0, 0, nullptr, 1, step_flags, s->acc, s->acc + 1, &tiled));
    if (!tiled) {   // the atomic forward/backward left gradients: dense sweeps
        KGE_RC(session_dense_sweep(s, &opt, m->n_ents, s->acc + 1, s->acc + 1));
    } else if (step_flags & AMDKGE_TILED_DETERMINISTIC) {   // a tile beyond its sort buffer fell back to arrival order: say so
        int32_t st_flag = 0;
        KGE_RC(amdkge_train_tiled_status(m, B, s->cfg.eta, step_flags, s->twork, &st_flag, s->st));
        if (st_flag) {
            s->step += 1; s->iteration += 1;   // the step itself was carried out
            return set_error(AMDKGE_EUNSUPPORTED, "session_train_step: deterministic mode -- a tile received more entries than its sort buffer holds (a very hot row); this step's sums were not all added in canonical order");
        }
    }
    double h[2] = {0.0, 0.0};
    KGE_HIP(hipMemcpyAsync(h, s->acc, sizeof(h), hipMemcpyDeviceToHost, s->st), "hipMemcpyAsync(D2H)");
    KGE_HIP(hipStreamSynchronize(s->st), "hipStreamSynchronize");
    s->step += 1;
    s->iteration += 1;
    if (loss_out) *loss_out = h[0] + h[1];
    return AMDKGE_OK;
} KGE_CATCH("session_train_step")

// ---- data-parallel phases of a step (session group) ----------------------------------------------------------------------
int amdkge_session_grad_step(amdkge_session* s, const int32_t* triples, int64_t b, const float* focus_w, int64_t row_offset, int64_t b_global) {
    if (!s || b < 0 || (b > 0 && !triples)) return set_error(AMDKGE_EINVAL, "session_grad_step: bad arguments");
    KGE_RC(session_check_triples(triples, b, s->cfg.model.n_ents, s->cfg.model.n_rels, "session_grad_step"));
    KGE_HIP(hipSetDevice(s->cfg.device), "hipSetDevice");
    KGE_HIP(hipMemsetAsync(s->acc, 0, 2 * sizeof(double), s->st), "hipMemsetAsync");
    if (b == 0) return AMDKGE_OK;   // (a replica without a share: its zero gradients still take part in the sum)
    const amdkge_model* m = &s->cfg.model;
    void* d_tri;
    KGE_RC(upload(s, 0, triples, b * 3 * (int64_t)sizeof(int32_t), &d_tri));
    amdkge_loss loss;
    KGE_RC(session_step_loss(s, focus_w, 0, b, "session_grad_step", "session", &loss));
    const amdkge_opt opt = step_opt(s);
    const int32_t flags = s->cfg.flags & (AMDKGE_TILED_POS_ATOMIC | AMDKGE_TILED_DETERMINISTIC | AMDKGE_TILED_DET_WIDE_SORT);   // (hot-row replicas: single-GPU steps only)
    return session_share_kernels(s, m, &loss, &opt, (const int32_t*)d_tri, b, m->n_ents, s->step, row_offset, b_global, nullptr, 0, flags, s->acc, s->acc + 1, nullptr);
}

int amdkge_session_apply_step(amdkge_session* s) {
    if (!s) return set_error(AMDKGE_EINVAL, "session_apply_step: NULL session");
    KGE_HIP(hipSetDevice(s->cfg.device), "hipSetDevice");
    const amdkge_opt opt = step_opt(s);
    return session_dense_sweep(s, &opt, s->cfg.model.n_ents, s->acc + 1, s->acc + 1);
}

int amdkge_session_finish_step(amdkge_session* s, double (&h)[2]) {
    h[0] = h[1] = 0.0;
    if (!s) return set_error(AMDKGE_EINVAL, "session_finish_step: NULL session");
    KGE_HIP(hipSetDevice(s->cfg.device), "hipSetDevice");
    KGE_HIP(hipMemcpyAsync(h, s->acc, sizeof(h), hipMemcpyDeviceToHost, s->st), "hipMemcpyAsync(D2H)");
    KGE_HIP(hipStreamSynchronize(s->st), "hipStreamSynchronize");
    s->step += 1;
    s->iteration += 1;
    return AMDKGE_OK;
}

// ---- column-sharded phases of a step (session group, AMDKGE_GROUP_COLS): this session holds a column slice of every row ----------
// A: the slice's partial score sums of the WHOLE batch into the session's score buffer (scratch slot 2), left on the device
int amdkge_session_cols_scores(amdkge_session* s, const int32_t* triples, int64_t B, float** d_scores_out) {
    if (!s || B < 1 || !triples || !d_scores_out) return set_error(AMDKGE_EINVAL, "session_cols_scores: bad arguments");
    KGE_RC(session_check_triples(triples, B, s->cfg.model.n_ents, s->cfg.model.n_rels, "session_group_train_step"));
    KGE_HIP(hipSetDevice(s->cfg.device), "hipSetDevice");
    void *d_tri, *d_sc;
    KGE_RC(upload(s, 0, triples, B * 3 * (int64_t)sizeof(int32_t), &d_tri));
    KGE_RC(scratch(s, 2, B * (int64_t)(1 + s->cfg.eta) * (int64_t)sizeof(float), &d_sc));
    KGE_HIP(hipMemsetAsync(s->acc, 0, 2 * sizeof(double), s->st), "hipMemsetAsync");
    const amdkge_model* m = &s->cfg.model;
    KGE_RC(amdkge_cols_partial_scores(m, s->tab[0], s->tab[1], (const int32_t*)d_tri, B, s->cfg.eta, 0, m->n_ents, s->cfg.seed, s->step, 0, 0, nullptr,
                                      (float*)d_sc, s->st));
    *d_scores_out = (float*)d_sc;
    return AMDKGE_OK;
}

// B + C: loss on the complete sums the group left in the score buffer, then backward / merge / optimizer on the slice
int amdkge_session_cols_apply(amdkge_session* s, int64_t B) {
    if (!s || B < 1) return set_error(AMDKGE_EINVAL, "session_cols_apply: bad arguments");
    KGE_HIP(hipSetDevice(s->cfg.device), "hipSetDevice");
    const amdkge_model* m = &s->cfg.model;
    float* d_sc = (float*)s->buf[2];
    void* d_tri = s->buf[0];
    const amdkge_loss loss = session_step_loss(s);   // (FocusE is not offered for column-sharded groups)
    KGE_RC(amdkge_cols_loss(m, &loss, d_sc, B, s->cfg.eta, s->acc, s->st));
    const amdkge_opt opt = step_opt(s);
    int64_t need = 0;
    KGE_RC(session_twork(s, m, B, &need));
    if (need <= 0) return set_error(AMDKGE_EUNSUPPORTED, "session_group_train_step: the column-sharded step needs the owner-computes pair for this slice shape");
    const int rc = amdkge_train_step_tiled(m, &loss, &opt, s->tab[0], s->tab[1], s->tab[2], s->tab[3], s->tab[4], s->tab[5], s->cfg.rel_reg_lambda,
                                           (const int32_t*)d_tri, B, s->cfg.eta, 0, m->n_ents, s->cfg.seed, s->step, 0, 0, nullptr, s->g_ent, s->g_rel, 1,
                                           AMDKGE_TILED_GIVEN_COEFFS, s->acc, s->acc + 1, d_sc, d_sc + B, s->twork, s->st);
    if (rc != AMDKGE_OK) session_drop_twork(s);
    return rc;
}

extern "C" int amdkge_session_score(amdkge_session* s, const int32_t* triples, int64_t n, float* scores_out) try {
    if (!s || n < 0) return set_error(AMDKGE_EINVAL, "session_score: bad arguments");
    if (n == 0) return AMDKGE_OK;
    if (!triples || !scores_out) return set_error(AMDKGE_EINVAL, "session_score: NULL buffer");
    KGE_RC(session_check_triples(triples, n, s->cfg.model.n_ents, s->cfg.model.n_rels, "session_score"));
    KGE_HIP(hipSetDevice(s->cfg.device), "hipSetDevice");
    void *d_tri, *d_sc;
    KGE_RC(upload(s, 0, triples, n * 3 * (int64_t)sizeof(int32_t), &d_tri));
    KGE_RC(scratch(s, 1, n * (int64_t)sizeof(float), &d_sc));
    KGE_RC(amdkge_score(&s->cfg.model, s->tab[0], s->tab[1], (const int32_t*)d_tri, n, (float*)d_sc, s->st));
    KGE_HIP(hipMemcpyAsync(scores_out, d_sc, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s->st), "hipMemcpyAsync(D2H)");
    KGE_HIP(hipStreamSynchronize(s->st), "hipStreamSynchronize");
    return AMDKGE_OK;
} KGE_CATCH("session_score")

int amdkge_session_scratch(amdkge_session* s, int slot, int64_t bytes, void** out) { return scratch(s, slot, bytes, out); }

// One side of get_ranks for n DEVICE-resident triples on this session's stream: d_counts3 = int32 [n, 2] counts (zeroed here, then
// += by the count pass) followed by int32 [n] filter subtractions.  `m` is the model the kernels see (a row-sharded group passes its
// local index space: shard + scratch rows); candidates are rows [ent_lo, ent_hi) of the table (or of d_ent_ids); filter ids come as a
// HOST CSR and, when id_limit > 0, are uploaded in a shard's local numbering: ids[f] - id_shift if that lies in [0, id_limit), else
// id_limit itself -- a row beyond the candidates, which the filter kernel drops (the partition rule, AbstractScoringLayer.py:280-288;
// with an entities subset its position entry must be -1).  Callers have validated ids and offsets.
int amdkge_session_count_side(amdkge_session* s, const amdkge_model* m, const int32_t* d_tri, int64_t n, int32_t side,
                              const int64_t* off, const int32_t* ids, int64_t id_shift, int64_t id_limit, const int32_t* d_ent_ids,
                              const int32_t* d_subset_pos, int64_t ent_lo, int64_t ent_hi, int32_t** d_counts3_out) {
    void *d_work, *d_counts, *d_off = nullptr, *d_ids = nullptr;
    KGE_RC(scratch(s, 1, amdkge_rank_workspace_bytes(m, n), &d_work));
    KGE_RC(scratch(s, 2, n * 3 * (int64_t)sizeof(int32_t), &d_counts));   // counts [n,2] + sub [n]
    int32_t* d_sub = (int32_t*)d_counts + 2 * n;
    KGE_HIP(hipMemsetAsync(d_counts, 0, (size_t)n * 3 * sizeof(int32_t), s->st), "hipMemsetAsync");
    // DistMult / ComplEx / HolE: the int8 screening pass + exact recheck (kge_rank_screen.hip) -- the counts of amdkge_rank_counts,
    // bit for bit, at about twice its rate; TransE / RotatE: their exact early exit (kge_rank_tile.hip, kge_rank_early.h) through the same workspace.
    // Beyond SCREEN_MAX (huge candidate ranges) or when the library sees nothing to gain (screen_need == 0: tiny problems) the
    // call is the plain amdkge_rank_counts.
    void* d_screen = nullptr;
    const int64_t screen_need = amdkge_rank_screen_workspace_bytes(m, n, ent_hi - ent_lo);
    const int64_t SCREEN_MAX = (int64_t)8 << 30;
    int64_t screen_bytes = 0;
    if (screen_need > 0 && screen_need <= SCREEN_MAX) {
        KGE_RC(scratch(s, 7, screen_need, &d_screen));
        screen_bytes = screen_need;
        // the statistics words (rechecked pairs, fell back, ...) are written only by the passes that run: small problems inside a
        // non-zero workspace take the plain kernel and would leave stale bytes to amdkge_session_screen_stats
        KGE_HIP(hipMemsetAsync(d_screen, 0, 256, s->st), "hipMemsetAsync(screen stats)");
    }
    KGE_RC(amdkge_rank_counts_screened(m, s->tab[0], s->tab[1], d_tri, n, side, d_ent_ids, ent_lo, ent_hi, (int32_t*)d_counts,
                                       d_work, d_screen, screen_bytes, s->st));
    s->screen_ran = d_screen != nullptr;
    if (off) {
        KGE_RC(upload(s, 4, off, (n + 1) * (int64_t)sizeof(int64_t), &d_off));
        if (id_limit <= 0) {
            KGE_RC(upload(s, 5, ids, off[n] * (int64_t)sizeof(int32_t), &d_ids));
        } else {
            std::vector<int32_t> local((size_t)off[n]);
            for (int64_t f = 0; f < off[n]; ++f) {
                const int64_t v = (int64_t)ids[f] - id_shift;
                local[(size_t)f] = (int32_t)((v < 0 || v >= id_limit) ? id_limit : v);
            }
            KGE_RC(upload(s, 5, local.data(), off[n] * (int64_t)sizeof(int32_t), &d_ids));
            KGE_HIP(hipStreamSynchronize(s->st), "hipStreamSynchronize");   // `local` leaves scope
        }
        KGE_RC(amdkge_rank_filter(m, s->tab[0], s->tab[1], d_tri, n, side, (const int64_t*)d_off, (const int64_t*)d_off + 1,
                                  (const int32_t*)d_ids, d_subset_pos, ent_lo, ent_hi, d_sub, d_work, s->st));
    }
    *d_counts3_out = (int32_t*)d_counts;
    return AMDKGE_OK;
}

int amdkge_session_check_filter(const int64_t* off, const int32_t* ids, int64_t n, int64_t n_ents, const char* who) {
    static thread_local char msg[160];
    if (!off) return AMDKGE_OK;
    if (off[0] < 0) { snprintf(msg, sizeof(msg), "%s: negative filter offset", who); return set_error(AMDKGE_EINVAL, msg); }
    for (int64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) { snprintf(msg, sizeof(msg), "%s: filter offsets must be non-decreasing", who); return set_error(AMDKGE_EINVAL, msg); }
    if (off[n] > 0 && !ids) { snprintf(msg, sizeof(msg), "%s: filter offsets without ids", who); return set_error(AMDKGE_EINVAL, msg); }
    for (int64_t f = 0; f < off[n]; ++f)
        if (ids[f] < 0 || ids[f] >= n_ents) { snprintf(msg, sizeof(msg), "%s: filter id outside the entity table", who); return set_error(AMDKGE_EINVAL, msg); }
    return AMDKGE_OK;
}

extern "C" int amdkge_session_rank(amdkge_session* s, const int32_t* triples, int64_t n, const int64_t* fs_off, const int32_t* fs_ids,
                                   const int64_t* fo_off, const int32_t* fo_ids, const int32_t* ent_subset, int64_t n_subset,
                                   int32_t corrupt_side, int32_t strategy, int32_t* ranks_out) try {
    if (!s || n < 0 || corrupt_side < AMDKGE_CORRUPT_S || corrupt_side > AMDKGE_CORRUPT_S_PLUS_O)
        return set_error(AMDKGE_EINVAL, "session_rank: bad arguments (corrupt_side must be AMDKGE_CORRUPT_*)");
    if (strategy < 0 || strategy > 2) return set_error(AMDKGE_EINVAL, "session_rank: unknown ranking strategy");
    if (n == 0) return AMDKGE_OK;
    if (!triples || !ranks_out) return set_error(AMDKGE_EINVAL, "session_rank: NULL buffer");
    if (n_subset < 0 || (n_subset > 0 && !ent_subset)) return set_error(AMDKGE_EINVAL, "session_rank: bad entities subset");
    KGE_RC(session_check_triples(triples, n, s->cfg.model.n_ents, s->cfg.model.n_rels, "session_rank"));
    const amdkge_model* m = &s->cfg.model;
    KGE_RC(amdkge_session_check_filter(fs_off, fs_ids, n, m->n_ents, "session_rank"));
    KGE_RC(amdkge_session_check_filter(fo_off, fo_ids, n, m->n_ents, "session_rank"));
    KGE_HIP(hipSetDevice(s->cfg.device), "hipSetDevice");
    void *d_tri, *d_ranks, *d_sel = nullptr;
    KGE_RC(upload(s, 0, triples, n * 3 * (int64_t)sizeof(int32_t), &d_tri));
    KGE_RC(scratch(s, 3, n * 2 * (int64_t)sizeof(int32_t), &d_ranks));
    const int32_t* d_ent_ids = nullptr;
    const int32_t* d_subset_pos = nullptr;
    int64_t ent_hi = m->n_ents;
    if (n_subset > 0) {   // entities_subset: candidate list + id -> position table (kge_group_staging.h)
        std::vector<int32_t> lst, pos;
        if (!stage_subset(ent_subset, n_subset, m->n_ents, 0, m->n_ents, m->n_ents, lst, pos)) return set_error(AMDKGE_EINVAL, "session_rank: subset id outside the entity table");
        KGE_RC(scratch(s, 6, (n_subset + m->n_ents) * (int64_t)sizeof(int32_t), &d_sel));
        KGE_HIP(hipMemcpyAsync(d_sel, lst.data(), (size_t)n_subset * sizeof(int32_t), hipMemcpyHostToDevice, s->st), "hipMemcpyAsync(H2D)");
        KGE_HIP(hipMemcpyAsync((int32_t*)d_sel + n_subset, pos.data(), (size_t)m->n_ents * sizeof(int32_t), hipMemcpyHostToDevice, s->st), "hipMemcpyAsync(H2D)");
        KGE_HIP(hipStreamSynchronize(s->st), "hipStreamSynchronize");   // the host lists leave scope below
        d_ent_ids = (const int32_t*)d_sel;
        d_subset_pos = (const int32_t*)d_sel + n_subset;
        ent_hi = n_subset;
    }
    const bool two_cols = corrupt_side == AMDKGE_CORRUPT_S_O;
    int col = 0;
    for (int side = AMDKGE_SIDE_S; side <= AMDKGE_SIDE_O; ++side) {
        if (!rank_side_wanted(side, corrupt_side)) continue;
        const int64_t* off = (side == AMDKGE_SIDE_S) ? fs_off : fo_off;
        const int32_t* ids = (side == AMDKGE_SIDE_S) ? fs_ids : fo_ids;
        int32_t* d_counts = nullptr;
        KGE_RC(amdkge_session_count_side(s, m, (const int32_t*)d_tri, n, side, off, ids, 0, 0, d_ent_ids, d_subset_pos, 0, ent_hi, &d_counts));
        KGE_RC(amdkge_rank_compose(d_counts, off ? d_counts + 2 * n : nullptr, n, strategy, (int32_t*)d_ranks + (two_cols ? col : col * n), two_cols ? 2 : 1, s->st));
        ++col;
    }
    s->screen_stats[0] = s->screen_stats[1] = 0;
    if (s->screen_ran) {   // (of the LAST side counted: the workspace is reused per side)
        KGE_HIP(hipMemcpyAsync(s->screen_stats, s->buf[7], sizeof(s->screen_stats), hipMemcpyDeviceToHost, s->st), "hipMemcpyAsync(D2H)");
    }
    return session_ranks_to_host(s, (const int32_t*)d_ranks, n, corrupt_side, ranks_out);
} KGE_CATCH("session_rank")

extern "C" int amdkge_session_screen_stats(const amdkge_session* s, int32_t* ran, int64_t* rechecked_pairs, int32_t* fell_back) try {
    if (!s) return set_error(AMDKGE_EINVAL, "session_screen_stats: NULL session");
    if (ran) *ran = s->screen_ran ? 1 : 0;
    if (rechecked_pairs) *rechecked_pairs = s->screen_ran ? (int64_t)s->screen_stats[0] : 0;
    if (fell_back) *fell_back = s->screen_ran ? s->screen_stats[1] : 0;
    return AMDKGE_OK;
} KGE_CATCH("session_screen_stats")

extern "C" int amdkge_session_set_hot_rows(amdkge_session* s, const int32_t* ids, int32_t n) try {
    if (!s || n < 0 || n > 64 || (n > 0 && !ids)) return set_error(AMDKGE_EINVAL, "session_set_hot_rows: bad arguments (at most 64 rows)");
    for (int32_t i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= s->cfg.model.n_ents) return set_error(AMDKGE_EINVAL, "session_set_hot_rows: row id outside the entity table");
    KGE_HIP(hipSetDevice(s->cfg.device), "hipSetDevice");
    s->hot_ids.assign(ids, ids + n);
    if (n == 0 && s->twork) KGE_RC(amdkge_train_tiled_set_hot_rows(&s->cfg.model, s->twork, nullptr, 0, s->st));   // clear the map
    s->hot_dirty = n > 0;
    return AMDKGE_OK;
} KGE_CATCH("session_set_hot_rows")
