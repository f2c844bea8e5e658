// Fused training forward+backward for gfx950: lookup (a1) + negative sampling (a3) + scoring
// (a4-a8) + loss (a12-a16) + gradient scatter, one launch per batch.  Replaces the TF graph of
// ScoringBasedEmbeddingModel.train_step (/root/reference/ampligraph/latent_features/models/
// ScoringBasedEmbeddingModel.py:370-429) up to (not including) optimizer.apply_gradients.
//
// Mapping: one "slot" of W wave64s owns one positive and its eta corruptions.  Each lane owns CH
// "quads" of VEC consecutive units of the embedding row; the positive's s, p, o quads and their
// gradient accumulators stay in VGPRs for the whole slot, replacement rows are streamed (16-byte
// coalesced loads) twice: once for the scores, once (L2-hot) for the gradients.  Score reductions
// are DPP wave reductions (+ one LDS hop when W > 1); the loss and dL/dscore of all eta corruptions
// are evaluated by the wave itself, so nothing but row gradients leaves the CU.  Row gradients are
// accumulated in registers per distinct row (s, p, o: one atomic row-add each per positive; every
// replacement row: one atomic row-add) with hardware fp32 atomics into the dense gradient buffers.
#include <stdlib.h>
#include <mutex>
#include <unordered_map>

#include "kge_train_kernel.h"

namespace kge {

// ------------------------------------------------------------------------------------------------
// stand-alone sampler (materialises what the fused kernel draws; a3)
// ------------------------------------------------------------------------------------------------
__global__ void sample_kernel(const int32_t* triples, int64_t B, int eta, SampleCfg sc, int32_t* out) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= B * eta) return;
    const int j = (int)(r / B);
    const int64_t i = r % B;
    int keep, repl;
    draw_corruption(sc, i, j, keep, repl);
    const int s = triples[3 * i], p = triples[3 * i + 1], o = triples[3 * i + 2];
    out[3 * r + 0] = keep ? s : repl;
    out[3 * r + 1] = p;
    out[3 * r + 2] = keep ? repl : o;
}

__global__ void loss_fold_kernel(double* parts, double* loss_sum) {
    fold_loss_parts(parts, loss_sum, threadIdx.x);   // one wave
}

// Scratch of the atomic path (it has no workspace argument): LOSS_PARTS partial sums, zero between calls.  One buffer per LOSS
// ACCUMULATOR -- keyed by (device, d_loss_sum): two engines or sessions that train on different streams of one GPU have their
// own accumulators, hence their own partials (a buffer shared per device let their kernels and fold launches mix sums, ADVICE
// r2), and the same address on ANOTHER GPU is another accumulator, whose partials must live on that GPU.  Calls
// that share an accumulator are ordered by their caller anyway.  Thread-safe.  A buffer is 8 KB and is NEVER freed behind a
// caller's back (the wholesale eviction of round 3 could free a buffer another host thread had just been handed and
// not yet launched on): a host that hands over fresh accumulators without end is stopped at LOSS_PARTS_MAX entries with
// AMDKGE_ENOMEM and told to call amdkge_release_scratch(), which synchronises every device with entries and frees them -- at a
// point of the caller's choosing, when no call of its own is in flight.
namespace {
struct PartsKey {
    int dev; const void* p;
    bool operator==(const PartsKey& o) const { return dev == o.dev && p == o.p; }
};
struct PartsHash { size_t operator()(const PartsKey& k) const { return std::hash<const void*>()(k.p) ^ ((size_t)k.dev * 0x9E3779B97F4A7C15ull); } };
constexpr size_t LOSS_PARTS_MAX = 1024;
std::mutex g_parts_mu;
std::unordered_map<PartsKey, double*, PartsHash> g_parts;

void release_parts_locked() {
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (auto& kv : g_parts) {
        (void)hipSetDevice(kv.first.dev);
        (void)hipDeviceSynchronize();   // (a launch that still reads the partials may be in flight)
        (void)hipFree(kv.second);
    }
    g_parts.clear();
    (void)hipSetDevice(cur);
}
}  // namespace

void release_loss_parts() {   // (kge::, called by amdkge_release_scratch)
    std::lock_guard<std::mutex> lk(g_parts_mu);
    release_parts_locked();
}

static double* loss_parts_for(const void* d_loss_sum) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(g_parts_mu);
    auto it = g_parts.find(PartsKey{dev, d_loss_sum});
    if (it != g_parts.end()) return it->second;
    if (g_parts.size() >= LOSS_PARTS_MAX) return nullptr;   // (the caller reports it: see the comment above)
    double* p = nullptr;
    const size_t bytes = (size_t)LOSS_PARTS * LOSS_PART_STRIDE * sizeof(double);
    if (hipMalloc((void**)&p, bytes) != hipSuccess) return nullptr;
    if (hipMemset(p, 0, bytes) != hipSuccess) { (void)hipFree(p); return nullptr; }
    try {
        g_parts.emplace(PartsKey{dev, d_loss_sum}, p);
    } catch (...) {   // (host allocation of the registry node: nothing may cross the C ABI)
        (void)hipFree(p);
        return nullptr;
    }
    return p;
}

template <int MODEL, int VEC, int W>
static int launch_train_w(TrainArgs& a, int CH, hipStream_t st) {
    const int slots = 4 / W;
    size_t shmem = (size_t)slots * slot_lds_bytes(a.eta, W) + slots * sizeof(double) + (VEC == 4 ? 4 * (size_t)a.K * 4 : 0);
    a.sign_off = (int)shmem;
    if (VEC == 4) shmem += sign_stash_bytes(MODEL, a.eta, CH);
    if (shmem > 150 * 1024) return set_error(AMDKGE_EUNSUPPORTED, "train: eta too large for the LDS score buffer");
    const unsigned grid = (unsigned)((a.B + slots - 1) / slots);
#define KGE_LAUNCH(CC) do { \
        if (shmem > 64 * 1024) { \
            static PerDeviceOnce attr;   /* one per instantiation */ \
            if (int rc = ensure_dynamic_lds(attr, {(const void*)train_fwdbwd_kernel<MODEL, VEC, W, CC>}, 160 * 1024, "train_fwdbwd")) return rc; \
        } \
        hipLaunchKernelGGL((train_fwdbwd_kernel<MODEL, VEC, W, CC>), dim3(grid), dim3(256), shmem, st, a); } while (0)
    switch (CH) {
        case 1: KGE_LAUNCH(1); break;
        case 2: KGE_LAUNCH(2); break;
        case 4: KGE_LAUNCH(4); break;
        default: KGE_LAUNCH(8); break;
    }
#undef KGE_LAUNCH
    return check_launch("train_fwdbwd");
}

// Slot geometry.  A lane owns CH "quads" of VEC consecutive units at quad index ts + c*64*W, so with
// VEC == 1 every wave-instruction (load or atomic) covers 64 consecutive floats = two full 128-byte
// lines.  Measured on MI355X (scripts/atomic_bench.hip): fp32 atomics retire ~10.4 G cache-line
// operations/s whatever the number of dwords per line, so the 16-byte-per-lane layout (8 active
// dwords per line) makes the gradient scatter 4.4x slower than the lane-contiguous one.
template <int MODEL, int VEC>
static int launch_train_mv(TrainArgs& a, hipStream_t st) {
    int W = 1;
    while (W < 4 && (a.nq + 64 * W - 1) / (64 * W) > 8) W *= 2;
    int ch = (a.nq + 64 * W - 1) / (64 * W);
    if (ch > 8) return set_error(AMDKGE_EUNSUPPORTED, "train: embedding row too long for the compiled slot geometries (k > 2048)");
    int CH = 1;
    while (CH < ch) CH *= 2;
    if (W == 1) return launch_train_w<MODEL, VEC, 1>(a, CH, st);
    if (W == 2) return launch_train_w<MODEL, VEC, 2>(a, CH, st);
    return launch_train_w<MODEL, VEC, 4>(a, CH, st);
}

template <int MODEL>
static int launch_train_m(TrainArgs& a, hipStream_t st) {
    const int units = a.k;  // units per row: k floats (real models) or k complex pairs
    // 16-byte loads + LDS-transposed scatter when one wave covers the row with <= 2 quads per lane.  Rows of up to 128 units
    // stay on the one-unit-per-lane geometry: with 13 ... 32 quads most lanes of the 16-byte form idle through the whole
    // per-row instruction stream, and the scalar form needs no transposition for its atomics (C1: 29.1 -> 26.8 us per step,
    // TransE k = 100: 110.9 -> 106.5)
    if (units % 4 == 0 && units <= 512 && units > 128 && !KGE_DBG(a, 16)) { a.nq = units / 4; return launch_train_w<MODEL, 4, 1>(a, a.nq <= 64 ? 1 : 2, st); }
    a.nq = units;
    return launch_train_mv<MODEL, 1>(a, st);
}

}  // namespace kge

using namespace kge;

extern "C" int amdkge_sample_corruptions(const int32_t* d_triples, int64_t B, int32_t eta, int64_t sample_base,
                                         int64_t sample_range, uint64_t seed, uint64_t step, int64_t row_offset,
                                         int64_t b_global, int32_t* d_out, void* stream) {
    if (B < 0 || eta < 0 || !d_out || (B > 0 && !d_triples)) return set_error(AMDKGE_EINVAL, "sample: bad arguments");
    if (sample_range <= 0 || sample_range > 0xFFFFFFFFll) return set_error(AMDKGE_EINVAL, "sample: sample_range must be in [1, 2^32)");
    if (B == 0 || eta == 0) return AMDKGE_OK;
    SampleCfg sc{sample_base, (uint32_t)sample_range, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step,
                 (uint32_t)(step >> 32), row_offset, b_global > 0 ? b_global : B};
    const int64_t n = B * eta;
    hipLaunchKernelGGL(sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_triples, B, eta, sc, d_out);
    return check_launch("sample_corruptions");
}

extern "C" int amdkge_train_fwdbwd(const amdkge_model* m, const amdkge_loss* loss, const float* d_ent, const float* d_rel,
                                   const int32_t* d_triples, int64_t B, int32_t eta, int64_t sample_base,
                                   int64_t sample_range, uint64_t seed, uint64_t step, int64_t row_offset,
                                   int64_t b_global, const int32_t* d_neg_override, float* d_grad_ent,
                                   float* d_grad_rel, double* d_loss_sum, float* d_pos_scores, float* d_neg_scores,
                                   void* stream) {
    if (int rc = validate_model(m)) return rc;
    if (!loss || loss->kind < 0 || loss->kind > AMDKGE_LOSS_MULTICLASS_NLL) return set_error(AMDKGE_EINVAL, "train: unknown loss kind");
    if (loss->focus_nonlinearity < AMDKGE_FOCUS_OFF || loss->focus_nonlinearity > AMDKGE_FOCUS_SOFTPLUS || (loss->focus_nonlinearity && !loss->d_focus_w))
        return set_error(AMDKGE_EINVAL, "train: bad FocusE settings (unknown non-linearity or NULL weights)");
    if (!d_ent || !d_rel || !d_grad_ent || !d_grad_rel || !d_loss_sum) return set_error(AMDKGE_EINVAL, "train: null table / gradient / loss pointer");
    if (B < 0 || eta < 1) return set_error(AMDKGE_EINVAL, "train: B must be >= 0 and eta >= 1");
    if (B == 0) return AMDKGE_OK;
    if (!d_triples) return set_error(AMDKGE_EINVAL, "train: null triples");
    if (!d_neg_override && (sample_range <= 0 || sample_range > 0xFFFFFFFFll || sample_base < 0 ||
                            sample_base + sample_range > m->n_ents))
        return set_error(AMDKGE_EINVAL, "train: sampling range outside the entity table");
    TrainArgs a{};
    a.ent = d_ent; a.rel = d_rel; a.triples = d_triples; a.neg_override = d_neg_override;
    a.g_ent = d_grad_ent; a.g_rel = d_grad_rel; a.loss_sum = d_loss_sum;
    a.pos_scores = d_pos_scores; a.neg_scores = d_neg_scores;
    a.B = B; a.eta = eta; a.k = stored_k(m); a.K = row_floats(m); a.k_live = m->k;
    a.sc = SampleCfg{sample_base, (uint32_t)sample_range, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step,
                     (uint32_t)(step >> 32), row_offset, b_global > 0 ? b_global : B};
    a.mc = model_const(m);
    a.loss = *loss;
#ifdef KGE_ABLATE
    { const char* e = getenv("AMDKGE_DEBUG"); a.dbg = e ? atoi(e) : 0; }
#endif
    hipStream_t st = (hipStream_t)stream;
    a.loss_parts = loss_parts_for(d_loss_sum);
    if (!a.loss_parts) return set_error(AMDKGE_ENOMEM, "train: cannot allocate the loss scratch (or 1 024 distinct loss accumulators are already registered: amdkge_release_scratch() frees the library's scratch of finished jobs)");
    int rc;
#define KGE_RUN(MODEL) rc = launch_train_m<MODEL>(a, st)
    KGE_MODEL_DISPATCH(m->scoring_type, KGE_RUN)
#undef KGE_RUN
    if (rc) return rc;
    hipLaunchKernelGGL(loss_fold_kernel, dim3(1), dim3(64), 0, st, a.loss_parts, d_loss_sum);
    return check_launch("loss_fold");
}
