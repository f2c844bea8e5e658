// Host-side helpers shared by the translation units of libamdkge: error reporting that never
// throws across the C ABI, argument validation, per-model constants.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <exception>
#include <initializer_list>
#include <new>

#include "../../include/amdkge.h"
#include "kge_device.h"
#include "kge_layout.h"
#include "kge_once.h"

namespace kge {

int set_error(int code, const char* msg);            // stores a thread-local message, returns code
int set_error_hip(hipError_t e, const char* where);  // AMDKGE_EHIP with hipGetErrorString
int check_launch(const char* kernel_name);           // hipGetLastError() after a launch

// Raises the dynamic-LDS limit of `kernels` to `bytes` on the calling thread's current device, once per device (kge_once.h).  Every
// kernel that is launched with more than 64 KB of dynamic LDS goes through this in front of its launch.  The first failure is
// reported as "hipFuncSetAttribute(<what>): <HIP's message>", and the device stays unmarked.
inline int ensure_dynamic_lds(PerDeviceOnce& once, std::initializer_list<const void*> kernels, size_t bytes, const char* what) {
    hipError_t err = hipSuccess;
    const bool ok = once.run([] { int dev = 0; return hipGetDevice(&dev) == hipSuccess ? dev : 0; },
                             [&] {
                                 for (const void* f : kernels)
                                     if ((err = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes)) != hipSuccess) return false;
                                 return true;
                             });
    if (ok) return AMDKGE_OK;
    char where[96];
    snprintf(where, sizeof(where), "hipFuncSetAttribute(%s)", what);
    return set_error_hip(err, where);
}

// How many blocks of a PERSISTENT kernel the calling thread's current device holds at once: compute units x
// hipOccupancyMaxActiveBlocksPerMultiprocessor at the launch's dynamic LDS size.  One object per kernel instantiation; the answers are
// kept per device ordinal (mod 64, as PerDeviceOnce) and LDS size, RESIDENT_SIZES sizes per device (a process that trains two models,
// or one with two values of eta, alternates between two), each in one 64-bit word next to the size it belongs to -- threads on
// different devices share the object, and a step whose shape was seen before asks nothing.  A fifth size takes the place of an older
// one (and is asked again when that one returns).  Neither query touches a stream: both are safe while a graph is being captured.
constexpr int RESIDENT_SIZES = 4;
struct ResidentBlocks {
    unsigned long long slot[64][RESIDENT_SIZES] = {};   // (dynamic LDS bytes + 1) << 32 | blocks; 0: free
};
inline int resident_blocks(ResidentBlocks& r, const void* kernel, int block_threads, size_t dyn_lds, const char* what, int& blocks) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    unsigned long long* words = r.slot[dev & 63];
    int put = (int)((dyn_lds >> 3) % RESIDENT_SIZES);   // (all taken: the size's own place)
    for (int e = RESIDENT_SIZES - 1; e >= 0; --e) {
        const unsigned long long have = __atomic_load_n(&words[e], __ATOMIC_ACQUIRE);
        if ((have >> 32) == (unsigned long long)dyn_lds + 1) { blocks = (int)(have & 0xFFFFFFFFull); return AMDKGE_OK; }
        if (have == 0) put = e;
    }
    unsigned long long& word = words[put];
    int per_cu = 0, cus = 0;
    char where[96];
    if (hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block_threads, dyn_lds); e != hipSuccess) {
        snprintf(where, sizeof(where), "hipOccupancyMaxActiveBlocksPerMultiprocessor(%s)", what);
        return set_error_hip(e, where);
    }
    if (hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev); e != hipSuccess) {
        snprintf(where, sizeof(where), "hipDeviceGetAttribute(%s)", what);
        return set_error_hip(e, where);
    }
    if (per_cu < 1 || cus < 1) {
        snprintf(where, sizeof(where), "%s: the device holds no block of this kernel with %zu bytes of LDS", what, dyn_lds);
        return set_error(AMDKGE_EINVAL, where);
    }
    blocks = per_cu * cus;
    __atomic_store_n(&word, ((unsigned long long)dyn_lds + 1) << 32 | (unsigned)blocks, __ATOMIC_RELEASE);
    return AMDKGE_OK;
}

// The session layers allocate on the host (staging vectors, the per-device threads of a group, the registries): those can throw,
// the C ABI cannot.  Their entry points are function-try-blocks closed by KGE_CATCH("name").
#define KGE_CATCH(NAME)                                                                                              \
    catch (const std::bad_alloc&) { return kge::set_error(AMDKGE_ENOMEM, NAME ": out of host memory"); }             \
    catch (const std::exception& e) { return kge::set_error(AMDKGE_EINVAL, e.what()); }                              \
    catch (...) { return kge::set_error(AMDKGE_EINVAL, NAME ": unexpected C++ exception"); }

inline int validate_model(const amdkge_model* m) {
    if (!m) return set_error(AMDKGE_EINVAL, "model descriptor is NULL");
    if (m->scoring_type < AMDKGE_TRANSE || m->scoring_type > AMDKGE_ROTATE)
        return set_error(AMDKGE_EINVAL, "unknown scoring_type (expected TransE/DistMult/ComplEx/HolE/RotatE)");
    if (m->k <= 0) return set_error(AMDKGE_EINVAL, "k must be positive");
    if (m->k_pad != 0 && m->k_pad < m->k) return set_error(AMDKGE_EINVAL, "k_pad must be 0 (dense rows) or >= k");
    if (m->k_full != 0 && m->k_full < m->k) return set_error(AMDKGE_EINVAL, "k_full must be 0 (the model is whole) or >= k (the model is a column slice of a k_full-unit model)");
    if (m->n_ents <= 0 || m->n_rels <= 0)
        return set_error(AMDKGE_EINVAL, "entity / relation table sizes must be positive (model not built?)");
    if (m->n_ents > 0x7FFFFFFFll || m->n_rels > 0x7FFFFFFFll)
        return set_error(AMDKGE_EINVAL, "row ids are int32: tables are limited to 2^31-1 rows");
    return AMDKGE_OK;
}

// units per half AS STORED (include/amdkge.h "STORED row layout") and floats per stored row
inline int stored_k(const amdkge_model* m) { return m->k_pad > 0 ? m->k_pad : m->k; }
inline int row_floats(const amdkge_model* m) { return internal_k_of(m->scoring_type, stored_k(m)); }

inline ModelConst model_const(const amdkge_model* m) {
    ModelConst mc;
    mc.score_scale = 1.f;
    mc.score_sign = 1.f;
    mc.phase_div = 1.f;
    if (m->scoring_type == AMDKGE_TRANSE || m->scoring_type == AMDKGE_ROTATE) mc.score_sign = -1.f;
    // (a column slice -- amdkge_model.k_full -- scores with the constants of the WHOLE model: its sums are partial sums of that one)
    const double kf = m->k_full > 0 ? (double)m->k_full : (double)m->k;
    if (m->scoring_type == AMDKGE_HOLE) mc.score_scale = (float)(2.0 / kf);  // HolE.py:45
    if (m->scoring_type == AMDKGE_ROTATE) {
        const double R = m->max_rel_size > 0 ? (double)m->max_rel_size : 1.0;           // RotatE.py:87-94
        const double embedding_range = sqrt(6.0 / (2.0 * kf * R));                      // RotatE.py:95
        mc.phase_div = (float)(embedding_range / 3.14159265358979323846);               // :96 (pi from math)
    }
    return mc;
}

}  // namespace kge
