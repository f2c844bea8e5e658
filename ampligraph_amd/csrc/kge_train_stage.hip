// F of the owner-computes step (kge_train_tiled.hip): the STAGE = true instantiations of the fused forward kernel
// (kge_train_kernel.h) -- 4 models x 4 slot geometries x the deterministic variant -- and their launch.
#include "kge_train_kernel.h"
#include "kge_train_tiled.h"

namespace kge {

template <int MODEL, int W, int CHF, bool DET>
static int launch_forward_v(TrainArgs& f, hipStream_t st) {
    constexpr int slots = 4 / W;
    // LDS: per-slot score / id arrays, per-slot loss, and the transpose rows of emit_row (one per wave, or one per
    // workgroup when a positive spans the whole workgroup)
    size_t shmem = (size_t)slots * slot_lds_bytes(f.eta, W) + slots * sizeof(double) + (W == 1 ? 4 : 1) * (size_t)f.K * 4;
    f.sign_off = (int)shmem;
    if (W != 1 || CHF != 1) shmem += sign_stash_bytes(MODEL, f.eta, CHF);   // (one wave per positive, one quad per lane: TransE takes the single-pass form, no stash)
    if (forward_spo_lds(MODEL, true, W, CHF)) shmem += (size_t)FWD_WAVES * 3 * f.K * 4;   // the waves' copies of s, p, o (behind the transpose rows: no stash in this geometry)
    if (shmem > 64 * 1024) {
        static PerDeviceOnce attr;
        if (int rc = ensure_dynamic_lds(attr, {(const void*)train_fwdbwd_kernel<MODEL, 4, W, CHF, true, DET>}, 160 * 1024, "train_forward_stage")) return rc;
    }
    unsigned grid = KGE_DBG(f, 8192) ? 0u : (unsigned)((f.B + slots - 1) / slots);   // (ablation 8192: no forward launch)
    if (forward_persistent(MODEL, true, W)) {
        // persistent waves: no more blocks than the device holds at once
        static ResidentBlocks resident;
        int cap = 0;
        if (int rc = resident_blocks(resident, (const void*)train_fwdbwd_kernel<MODEL, 4, W, CHF, true, DET>, 256, shmem, "train_forward_stage", cap)) return rc;
        if (grid > (unsigned)cap) grid = (unsigned)cap;
    }
    if (grid) hipLaunchKernelGGL((train_fwdbwd_kernel<MODEL, 4, W, CHF, true, DET>), dim3(grid), dim3(256), shmem, st, f);
    return check_launch("train_forward_stage");
}
template <int MODEL, int W, int CHF>
static int launch_forward(TrainArgs& f, hipStream_t st) {
    return f.det ? launch_forward_v<MODEL, W, CHF, true>(f, st) : launch_forward_v<MODEL, W, CHF, false>(f, st);
}

// Rows of up to 128 quads: one wave per positive (1 or 2 quads per lane); longer rows (k <= 2048): the four waves of a workgroup
// share one positive.
template <int MODEL>
static int forward_by_width(TrainArgs& f, hipStream_t st) {
    if (f.nq <= 64) return launch_forward<MODEL, 1, 1>(f, st);
    if (f.nq <= 128) return launch_forward<MODEL, 1, 2>(f, st);
    if (f.nq <= 256) return launch_forward<MODEL, 4, 1>(f, st);
    return launch_forward<MODEL, 4, 2>(f, st);
}

int run_forward_stage(int model, TrainArgs& f, hipStream_t st) {
#define KGE_RUN(MODEL) return forward_by_width<MODEL>(f, st)
    KGE_MODEL_DISPATCH(model, KGE_RUN)
#undef KGE_RUN
}

}  // namespace kge
