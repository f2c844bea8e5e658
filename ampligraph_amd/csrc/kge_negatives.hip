// Training negative samplers (include/amdkge_negatives.h): corruptions drawn with rejection of known positives, a per-relation
// (Bernoulli) side probability and / or a caller's pool of replacement entities, written as the [(B*eta), 3] override array the
// train entry points take.  The draw is DEFINED in the header; tests/negatives_ref.py restates it in numpy.
//   negatives_typed_kernel (include/amdkge_types.h) is the same body with the replacement of a try read from the positive's own
//   candidate range (a relation's domain / range set): negatives_body<TYPED>.
//   negatives_kernel : a thread owns ONE positive i (its triple and its four range bounds are loaded once, into registers) and
//                      walks corruptions j = blockIdx.y, blockIdx.y + gridDim.y, ...  Lanes are consecutive positives, so every
//                      load of the positives' arrays and every store of output row r = j * B + i is a run of consecutive addresses.
//                      The host picks gridDim.y: all eta corruptions in parallel while that is what fills the device (a C2 batch is
//                      200 k rows), several per thread on batches that fill it anyway -- the result does not depend on the split.
//   Divergence       : try 0 runs for every lane with the three words block 0 already holds; the retry loop is entered by the lanes
//                      whose try was rejected, and the wave leaves it when its last lane is accepted.  On real graphs a rejection is
//                      rare (a uniform entity is a known one with probability range length / N), so most waves never run a
//                      second Philox block; the dense test graphs, where most lanes retry, only cost more iterations.
//   Membership       : sorted_contains (kge_order.h), a lower bound in global memory: a hub's range of thousands of ids is ~12
//                      dependent loads, a typical range of a handful 2 - 3.  No LDS (nothing is shared between lanes), no scratch, 8 waves per SIMD.
//   Stats            : per-thread counts, one wave reduction at the end, one 64-bit integer atomic per wave and counter (none when
//                      the wave made no redraw): order-free.
//   side_thresholds  : G_po from two lower bounds per relation in the ascending (p, o) keys, G_sp from an integer histogram of
//                      key % n_rels that is accumulated in d_thr itself and replaced by the threshold in place.
#include "kge_host.h"

namespace kge {

struct NegArgs {
    const int32_t* triples;
    int64_t B;
    int eta;
    SampleCfg sc;
    int side_mode;
    const uint32_t* side_thr;
    const int32_t* pool;   // NULL: sample_base + mulhi(word, range)
    uint32_t pool_n;
    const int64_t* s_lo;   // all six NULL: no rejection
    const int64_t* s_hi;
    const int32_t* s_ids;
    const int64_t* o_lo;
    const int64_t* o_hi;
    const int32_t* o_ids;
    int max_tries;
    unsigned long long* stats;
    int32_t* out;
    const int64_t* cs_lo;  // negatives_typed_kernel only; all six NULL: every corruption is drawn by the untyped rule
    const int64_t* cs_hi;
    const int32_t* cs_ids;
    const int64_t* co_lo;
    const int64_t* co_hi;
    const int32_t* co_ids;
};

// The body of both kernels.  TYPED: a try takes its replacement from the positive's own candidate range of the decided side
// (include/amdkge_types.h) -- one dependent 4-byte load per try -- where that range is not empty; everything else (side, words, blocks,
// rejection, the kept last try, the output row) is the one code.  The four candidate bounds are loaded once, with the filter bounds.
template <bool TYPED>
__device__ __forceinline__ void negatives_body(const NegArgs& a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < a.B;   // (no early return: every lane takes part in the wave reduction at the end)
    int redraws = 0, exhausted = 0, untyped = 0;
    if (live) {
        const int s = a.triples[3 * i], p = a.triples[3 * i + 1], o = a.triples[3 * i + 2];
        int64_t slo = 0, shi = 0, olo = 0, ohi = 0;
        if (a.s_ids) { slo = a.s_lo[i]; shi = a.s_hi[i]; olo = a.o_lo[i]; ohi = a.o_hi[i]; }
        int64_t cslo = 0, cshi = 0, colo = 0, cohi = 0;
        if (TYPED && a.cs_ids) { cslo = a.cs_lo[i]; cshi = a.cs_hi[i]; colo = a.co_lo[i]; cohi = a.co_hi[i]; }
        const uint32_t thr = a.side_mode == AMDKGE_NEG_SIDE_BERNOULLI ? a.side_thr[p] : 0u;
        for (int j = blockIdx.y; j < a.eta; j += gridDim.y) {
            const uint64_t row = (uint64_t)j * (uint64_t)a.sc.b_global + (uint64_t)(a.sc.row_offset + i);
            const uint32_t row_lo = (uint32_t)row, row_hi = (uint32_t)(row >> 32);
            u32x4 blk = philox4x32_10(row_lo, row_hi, a.sc.step_lo, a.sc.step_hi, a.sc.seed_lo, a.sc.seed_hi);
            bool subj;   // decided once, from block 0
            switch (a.side_mode) {
                case AMDKGE_NEG_SIDE_BERNOULLI: subj = blk.x < thr; break;
                case AMDKGE_NEG_SIDE_S_ONLY: subj = true; break;
                case AMDKGE_NEG_SIDE_O_ONLY: subj = false; break;
                default: subj = (blk.x & 1u) == 0u; break;
            }
            const int32_t* ids = subj ? a.s_ids : a.o_ids;
            const int64_t lo = subj ? slo : olo, hi = subj ? shi : ohi;
            // the candidate range of the decided side: cand == nullptr is the untyped rule
            const int32_t* cand = nullptr;
            uint32_t cand_n = 0;
            if (TYPED) {
                const int64_t clo = subj ? cslo : colo, chi = subj ? cshi : cohi;
                if (chi > clo) { cand = (subj ? a.cs_ids : a.co_ids) + clo; cand_n = (uint32_t)(chi - clo); }
                else ++untyped;
            }
            // the three replacement words of the current block, rotated so that the try at hand reads w0 (an index into the block
            // would make the compiler park it in LDS)
            uint32_t w0 = blk.y, w1 = blk.z, w2 = blk.w;
            int repl = 0, t = 0;
            for (;;) {
                if (TYPED && cand) repl = cand[__umulhi(w0, cand_n)];
                else repl = a.pool ? a.pool[__umulhi(w0, a.pool_n)] : (int)(a.sc.base + (int64_t)__umulhi(w0, a.sc.range));
                if (!(ids && hi > lo && sorted_contains<int64_t>(ids, lo, hi, repl))) break;   // accepted
                if (t + 1 == a.max_tries) { ++exhausted; break; }                               // the last try is kept
                ++t;
                if (t % 3 == 0) {
                    blk = philox4x32_10(row_lo, row_hi | ((uint32_t)(t / 3) << 24), a.sc.step_lo, a.sc.step_hi, a.sc.seed_lo, a.sc.seed_hi);
                    w0 = blk.y; w1 = blk.z; w2 = blk.w;
                } else {
                    w0 = w1; w1 = w2;
                }
            }
            redraws += t;
            const int64_t r = (int64_t)j * a.B + i;
            a.out[3 * r + 0] = subj ? repl : s;
            a.out[3 * r + 1] = p;
            a.out[3 * r + 2] = subj ? o : repl;
        }
    }
    if (!a.stats) return;   // (uniform over the grid)
    const int rd = wave_sum_i(redraws), ex = wave_sum_i(exhausted), ut = TYPED ? wave_sum_i(untyped) : 0;
    if ((threadIdx.x & 63) == 0) {
        if (rd) atomicAdd(&a.stats[0], (unsigned long long)rd);
        if (ex) atomicAdd(&a.stats[1], (unsigned long long)ex);
        if (TYPED && ut) atomicAdd(&a.stats[2], (unsigned long long)ut);
    }
}

__global__ __launch_bounds__(256) void negatives_kernel(NegArgs a) { negatives_body<false>(a); }

// amdkge_sample_negatives_typed (include/amdkge_types.h): negatives_kernel with the replacement of a try read from the positive's
// candidate set.  Four more bounds in registers, no LDS, no scratch.
__global__ __launch_bounds__(256) void negatives_typed_kernel(NegArgs a) { negatives_body<true>(a); }

// histogram of the (s, p) groups over their relation, into thr (zero on entry)
__global__ __launch_bounds__(256) void neg_sp_hist_kernel(const int64_t* sp_keys, int64_t n_sp, int64_t n_rels, uint32_t* thr) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n_sp; q += stride) {
        const int64_t key = sp_keys[q];
        if (key >= 0) atomicAdd(&thr[key % n_rels], 1u);
    }
}

// first position of ascending keys[0 .. n) that holds a value >= v
__device__ __forceinline__ int64_t lower_bound_i64(const int64_t* keys, int64_t n, int64_t v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void neg_thresholds_kernel(const int64_t* po_keys, int64_t n_po, int64_t n_ents, int64_t n_rels, uint32_t* thr) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_rels) return;
    const uint64_t g_sp = thr[p];
    const uint64_t g_po = (uint64_t)(lower_bound_i64(po_keys, n_po, (p + 1) * n_ents) - lower_bound_i64(po_keys, n_po, p * n_ents));
    // both counts are < 2^31: g_po << 32 is exact in 64 bits.  A relation present on one side only (two indexes of different
    // data) would give 0 or 2^32: it is clamped to the representable end.
    uint64_t v = 0x80000000ull;
    if (g_sp + g_po) v = (g_po << 32) / (g_sp + g_po);
    thr[p] = v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v;
}

}  // namespace kge

using namespace kge;

static int neg_error(const char* who, const char* what) {
    char msg[200];
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return set_error(AMDKGE_EINVAL, msg);
}

// the checks and the launch behind both sampler entry points; typed: amdkge_sample_negatives_typed (the six candidate arrays count,
// d_stats has a third word)
static int sample_negatives_run(const char* who, bool typed, const int32_t* d_triples, int64_t B, int32_t eta, int64_t sample_base,
                                int64_t sample_range, uint64_t seed, uint64_t step, int64_t row_offset, int64_t b_global, int32_t side_mode,
                                const uint32_t* d_side_thr, const int32_t* d_pool, int64_t pool_n, const int64_t* d_s_lo, const int64_t* d_s_hi,
                                const int32_t* d_s_ids, const int64_t* d_o_lo, const int64_t* d_o_hi, const int32_t* d_o_ids, int32_t max_tries,
                                int64_t* d_stats, int32_t* d_out, const int64_t* d_cs_lo, const int64_t* d_cs_hi, const int32_t* d_cs_ids,
                                const int64_t* d_co_lo, const int64_t* d_co_hi, const int32_t* d_co_ids, void* stream) {
    if (B < 0 || eta < 0 || row_offset < 0) return neg_error(who, "negative size");
    if (!d_out || (B > 0 && !d_triples)) return neg_error(who, "NULL pointer");
    if (side_mode < AMDKGE_NEG_SIDE_UNIFORM || side_mode > AMDKGE_NEG_SIDE_O_ONLY) return neg_error(who, "unknown side_mode");
    if (side_mode == AMDKGE_NEG_SIDE_BERNOULLI && !d_side_thr) return neg_error(who, "AMDKGE_NEG_SIDE_BERNOULLI needs d_side_thr");
    if (max_tries < 1 || max_tries > AMDKGE_NEG_MAX_TRIES) return neg_error(who, "max_tries must be in [1, 32]");
    const int nrng = (d_s_lo ? 1 : 0) + (d_s_hi ? 1 : 0) + (d_s_ids ? 1 : 0) + (d_o_lo ? 1 : 0) + (d_o_hi ? 1 : 0) + (d_o_ids ? 1 : 0);
    if (nrng != 0 && nrng != 6) return neg_error(who, "the six range arrays are given together or not at all");
    const int ncand = (d_cs_lo ? 1 : 0) + (d_cs_hi ? 1 : 0) + (d_cs_ids ? 1 : 0) + (d_co_lo ? 1 : 0) + (d_co_hi ? 1 : 0) + (d_co_ids ? 1 : 0);
    if (ncand != 0 && ncand != 6) return neg_error(who, "the six candidate arrays are given together or not at all");
    if (d_pool && (pool_n < 1 || pool_n > 0xFFFFFFFFll)) return neg_error(who, "a pool needs pool_n in [1, 2^32)");
    if (!d_pool && (sample_range <= 0 || sample_range > 0xFFFFFFFFll)) return neg_error(who, "sample_range must be in [1, 2^32)");
    const int64_t bg = b_global > 0 ? b_global : B;
    if (bg > 0 && (int64_t)eta >= ((1ll << 56) + bg - 1) / bg) return neg_error(who, "eta * b_global must be < 2^56");
    if (B == 0 || eta == 0) return AMDKGE_OK;
    NegArgs a{};
    a.triples = d_triples; a.B = B; a.eta = eta;
    a.sc = SampleCfg{sample_base, d_pool ? 1u : (uint32_t)sample_range, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step, (uint32_t)(step >> 32), row_offset, bg};
    a.side_mode = side_mode; a.side_thr = d_side_thr; a.pool = d_pool; a.pool_n = d_pool ? (uint32_t)pool_n : 0u;
    a.s_lo = d_s_lo; a.s_hi = d_s_hi; a.s_ids = d_s_ids; a.o_lo = d_o_lo; a.o_hi = d_o_hi; a.o_ids = d_o_ids;
    a.max_tries = max_tries; a.stats = reinterpret_cast<unsigned long long*>(d_stats); a.out = d_out;
    a.cs_lo = d_cs_lo; a.cs_hi = d_cs_hi; a.cs_ids = d_cs_ids; a.co_lo = d_co_lo; a.co_hi = d_co_hi; a.co_ids = d_co_ids;
    // grid.x: 256 positives per workgroup; grid.y: enough corruption lanes for ~1024 workgroups (4 waves per SIMD of the 256 CUs)
    // when the call has that many rows, the rest of a thread's corruptions in its loop
    const int64_t bx = (B + 255) / 256;
    if (bx > 0x7FFFFFFFll) {
        char msg[200];
        snprintf(msg, sizeof(msg), "%s: too many positives for one launch; split them", who);
        return set_error(AMDKGE_EUNSUPPORTED, msg);
    }
    int64_t by = (1024 + bx - 1) / bx;
    if (by > eta) by = eta;
    if (by > 65535) by = 65535;
    if (typed) hipLaunchKernelGGL(negatives_typed_kernel, dim3((unsigned)bx, (unsigned)by), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(negatives_kernel, dim3((unsigned)bx, (unsigned)by), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch(who);
}

extern "C" int amdkge_sample_negatives(const int32_t* d_triples, int64_t B, int32_t eta, int64_t sample_base, int64_t sample_range,
                                       uint64_t seed, uint64_t step, int64_t row_offset, int64_t b_global, int32_t side_mode,
                                       const uint32_t* d_side_thr, const int32_t* d_pool, int64_t pool_n,
                                       const int64_t* d_s_lo, const int64_t* d_s_hi, const int32_t* d_s_ids,
                                       const int64_t* d_o_lo, const int64_t* d_o_hi, const int32_t* d_o_ids,
                                       int32_t max_tries, int64_t* d_stats, int32_t* d_out, void* stream) {
    return sample_negatives_run("sample_negatives", false, d_triples, B, eta, sample_base, sample_range, seed, step, row_offset, b_global, side_mode,
                                d_side_thr, d_pool, pool_n, d_s_lo, d_s_hi, d_s_ids, d_o_lo, d_o_hi, d_o_ids, max_tries, d_stats, d_out,
                                nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int amdkge_sample_negatives_typed(const int32_t* d_triples, int64_t B, int32_t eta, int64_t sample_base, int64_t sample_range,
                                             uint64_t seed, uint64_t step, int64_t row_offset, int64_t b_global, int32_t side_mode,
                                             const uint32_t* d_side_thr, const int32_t* d_pool, int64_t pool_n,
                                             const int64_t* d_s_lo, const int64_t* d_s_hi, const int32_t* d_s_ids,
                                             const int64_t* d_o_lo, const int64_t* d_o_hi, const int32_t* d_o_ids,
                                             int32_t max_tries, int64_t* d_stats, int32_t* d_out,
                                             const int64_t* d_cs_lo, const int64_t* d_cs_hi, const int32_t* d_cs_ids,
                                             const int64_t* d_co_lo, const int64_t* d_co_hi, const int32_t* d_co_ids, void* stream) {
    return sample_negatives_run("sample_negatives_typed", true, d_triples, B, eta, sample_base, sample_range, seed, step, row_offset, b_global,
                                side_mode, d_side_thr, d_pool, pool_n, d_s_lo, d_s_hi, d_s_ids, d_o_lo, d_o_hi, d_o_ids, max_tries, d_stats, d_out,
                                d_cs_lo, d_cs_hi, d_cs_ids, d_co_lo, d_co_hi, d_co_ids, stream);
}

extern "C" int amdkge_negatives_side_thresholds(const int64_t* d_po_keys, int64_t n_po, const int64_t* d_sp_keys, int64_t n_sp,
                                                int64_t n_ents, int64_t n_rels, uint32_t* d_thr, void* stream) {
    if (n_po < 0 || n_sp < 0 || n_sp > 0x7FFFFFFFll || n_ents < 1 || n_rels < 1 || n_ents > 0x7FFFFFFFll || n_rels > 0x7FFFFFFFll)
        return set_error(AMDKGE_EINVAL, "negatives_side_thresholds: bad sizes");
    if (!d_thr || (n_po > 0 && !d_po_keys) || (n_sp > 0 && !d_sp_keys)) return set_error(AMDKGE_EINVAL, "negatives_side_thresholds: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    if (hipError_t e = hipMemsetAsync(d_thr, 0, (size_t)n_rels * sizeof(uint32_t), st)) return set_error_hip(e, "negatives_side_thresholds: hipMemsetAsync");
    if (n_sp > 0) {
        int64_t blocks = (n_sp + 255) / 256;
        if (blocks > 2048) blocks = 2048;
        hipLaunchKernelGGL(neg_sp_hist_kernel, dim3((unsigned)blocks), dim3(256), 0, st, d_sp_keys, n_sp, n_rels, d_thr);
        if (int rc = check_launch("negatives_sp_hist")) return rc;
    }
    hipLaunchKernelGGL(neg_thresholds_kernel, dim3((unsigned)((n_rels + 255) / 256)), dim3(256), 0, st, d_po_keys, n_po, n_ents, n_rels, d_thr);
    return check_launch("negatives_side_thresholds");
}
