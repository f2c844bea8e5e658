// KvsAll on the shared step (include/amdkge_shared_labels.h): the loss step that labels a row's entries from its known range and applies
// binary cross-entropy with logits, in ONE pass over the score buffer -- each score is read once and its coefficient written once, where
// the softmax sibling runs shared_mask_kernel and then shared_loss_kernel over the same buffer.  The header's text DEFINES the arithmetic;
// tests/shared_labels_ref.py restates it in numpy.
//   shared_label_loss_kernel : a wave per row (the grid cap of shared_loss_kernel), lanes stride over j in chunks of 64.
//       GIVEN lists    : a lane looks ids[g][j] up in the row's range (sorted_contains: the mask kernel's search, one per entry).
//       IDENTITY lists : ids[g][j] == j, and both j and the range ascend, so the range is walked ONCE beside the chunks.  The wave holds a
//                        window of 64 of the range's ids in a register (every id is loaded once, by one lane); the ids of the window
//                        that fall into the current chunk [j0, j0 + 64) are a run of its lanes, their bits 1 << (id - j0) are OR-ed over
//                        the wave into a 64-bit word, and lane l reads its label from bit l.  A chunk without a known id -- nearly all
//                        of them -- costs one compare of the window's next id against j0 + 64.  Nothing is written and read back: a
//                        "store y = 0 everywhere, then patch the known places" would have one lane read what another lane of the wave
//                        has just stored to global memory, without a fence.
//       The loss partials are fp32 per lane, one wave_sum per row, a double per wave, one fp64 atomic per workgroup: shared_loss_kernel's
//       scheme.  Row offsets are 64-bit.
// The three entry points of the header: the kernel alone lives here, the two steps live with run_shared / run_shared_dist in their units
// and reach the kernel through launch_shared_label_loss (kge_train_shared.h).
#include "kge_train_shared.h"
#include <string>

namespace kge {

__device__ __forceinline__ unsigned long long wave_or_u64(unsigned long long v) {
    unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo |= (unsigned)__shfl_xor((int)lo, o, 64);
        hi |= (unsigned)__shfl_xor((int)hi, o, 64);
    }
    return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(256) void shared_label_loss_kernel(SharedLabelArgs a) {
    __shared__ double s_loss[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float t0 = a.eps / (float)a.M, t1 = (1.f - a.eps) + t0;
    const float red = a.mean ? (float)a.M : 1.f;
    double tot = 0.0;
    int64_t n_lab = 0, n_none = 0;   // (lane 0's are the wave's totals)
    for (int64_t r = (int64_t)blockIdx.x * 4 + wv; r < a.rows; r += (int64_t)gridDim.x * 4) {   // (wave-uniform)
        const int64_t i = a.row0 + r;
        const bool subj = a.side[i] != 0;
        const int64_t lo = subj ? a.s_lo[i] : a.o_lo[i], hi = subj ? a.s_hi[i] : a.o_hi[i];
        const int32_t* __restrict__ kid = subj ? a.s_ids : a.o_ids;
        const int32_t* __restrict__ gid = a.identity ? nullptr : a.ids + (i / a.G) * a.M;
        const float w = a.w_s ? (subj ? a.w_s[i] : a.w_o[i]) : 1.f;
        const float wr = w / red;
        float* s = a.S + r * a.M;
        // IDENTITY: the window kid[wbase .. wbase + 64) in idv, pos = the first id of the range not yet consumed
        int64_t pos = lo, wbase = lo;
        int idv = 0;
        if (a.identity && lo < hi && wbase + lane < hi) idv = kid[wbase + lane];
        float acc = 0.f;
        int cnt = 0;
        for (int j0 = 0; j0 < a.M; j0 += 64) {   // (wave-uniform)
            const int j = j0 + lane;
            const bool in = j < a.M;
            bool y;
            if (a.identity) {
                unsigned long long bits = 0ull;
                while (pos < hi) {   // (wave-uniform: pos, wbase and the ballot are)
                    if (pos >= wbase + 64) {   // the window is used up: the next 64 ids
                        wbase = pos;
                        if (wbase + lane < hi) idv = kid[wbase + lane];
                    }
                    const int64_t at = wbase + lane;
                    const bool mine = at >= pos && at < hi && (int64_t)idv < (int64_t)j0 + 64;   // ascending: a run of lanes from pos
                    const unsigned long long run = __ballot(mine);
                    if (run == 0ull) break;
                    bits |= wave_or_u64(mine && idv >= j0 ? 1ull << (idv - j0) : 0ull);   // (an id below j0 can only be negative: ignored)
                    pos += __popcll(run);
                    if (pos < wbase + 64) break;   // the window's next id lies beyond this chunk
                }
                y = (bits >> lane) & 1ull;
            } else {
                y = in && lo < hi && sorted_contains<int64_t>(kid, lo, hi, gid[j]);
            }
            if (in) {
                const float x = a.scale * s[j];
                if (a.neg_scores) a.neg_scores[(int64_t)j * a.B + i] = x;
                const float t = y ? t1 : t0;
                const float e = expf(-fabsf(x));
                const float relu = x < 0.f ? 0.f : x;               // keeps a NaN
                acc += (relu - t * x) + log1pf(e);
                const float sig = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
                s[j] = (wr * (sig - t)) * a.scale;
                cnt += y ? 1 : 0;
            }
        }
        const float per = wr * wave_sum(acc);
        cnt = wave_sum_i(cnt);
        if (lane == 0) {
            if (a.cpos) a.cpos[i] = 0.f;
            if (a.pos_scores) a.pos_scores[i] = a.scale * a.pos_raw[i];
            tot += (double)per;
            n_lab += cnt;
            n_none += cnt == 0 ? 1 : 0;
        }
    }
    if (lane == 0) s_loss[wv] = tot;
    __syncthreads();
    if (tid == 0) {
        const double t = s_loss[0] + s_loss[1] + s_loss[2] + s_loss[3];
        if (t != 0.0) atomicAdd(a.loss_sum, t);   // (true for NaN)
    }
    if (a.stats && lane == 0) {
        if (n_lab) atomicAdd(&a.stats[0], (unsigned long long)n_lab);
        if (n_none) atomicAdd(&a.stats[1], (unsigned long long)n_none);
    }
}

int launch_shared_label_loss(const SharedLabelArgs& a, hipStream_t st) {
    int64_t lb = (a.rows + 3) / 4;
    if (lb > 2048) lb = 2048;
    hipLaunchKernelGGL(shared_label_loss_kernel, dim3((unsigned)lb), dim3(256), 0, st, a);
    return check_launch("shared_label_loss");
}

int shared_label_args(const char* who, const int32_t* d_neg_ids, const int64_t* d_s_lo, const int64_t* d_s_hi, const int32_t* d_s_ids, const int64_t* d_o_lo,
                      const int64_t* d_o_hi, const int32_t* d_o_ids, int32_t list_mode, float label_smoothing, int32_t reduction_mean, const float* d_w_s,
                      const float* d_w_o, int64_t* d_stats, SharedLabelArgs& a) {
    const std::string w(who);
    if (!d_s_lo || !d_s_hi || !d_s_ids || !d_o_lo || !d_o_hi || !d_o_ids) return set_error(AMDKGE_EINVAL, (w + ": the six range arrays are all required (labels need them)").c_str());
    if (list_mode != AMDKGE_SHARED_LIST_GIVEN && list_mode != AMDKGE_SHARED_LIST_IDENTITY) return set_error(AMDKGE_EINVAL, (w + ": unknown list_mode").c_str());
    if (list_mode == AMDKGE_SHARED_LIST_GIVEN && !d_neg_ids) return set_error(AMDKGE_EINVAL, (w + ": AMDKGE_SHARED_LIST_GIVEN needs d_neg_ids").c_str());
    if (!(label_smoothing >= 0.f && label_smoothing < 1.f)) return set_error(AMDKGE_EINVAL, (w + ": label_smoothing must be in [0, 1)").c_str());   // (NaN fails both)
    if ((d_w_s != nullptr) != (d_w_o != nullptr)) return set_error(AMDKGE_EINVAL, (w + ": d_w_s and d_w_o are given together or not at all").c_str());
    a = SharedLabelArgs{};
    a.s_lo = d_s_lo; a.s_hi = d_s_hi; a.s_ids = d_s_ids; a.o_lo = d_o_lo; a.o_hi = d_o_hi; a.o_ids = d_o_ids;
    a.identity = list_mode == AMDKGE_SHARED_LIST_IDENTITY;
    a.eps = label_smoothing; a.mean = reduction_mean ? 1 : 0; a.scale = 1.f;
    a.w_s = d_w_s; a.w_o = d_w_o;
    a.stats = reinterpret_cast<unsigned long long*>(d_stats);
    return AMDKGE_OK;
}

}  // namespace kge

using namespace kge;

extern "C" int amdkge_shared_label_loss(float* d_scores, int64_t row0, int64_t rows, int64_t G, int32_t M, const int32_t* d_neg_ids, const int32_t* d_side,
                                        const int64_t* d_s_lo, const int64_t* d_s_hi, const int32_t* d_s_ids, const int64_t* d_o_lo, const int64_t* d_o_hi,
                                        const int32_t* d_o_ids, int32_t list_mode, float label_smoothing, int32_t reduction_mean, float scale, const float* d_w_s,
                                        const float* d_w_o, double* d_loss_sum, int64_t* d_stats, void* stream) {
    if (row0 < 0 || rows < 0 || G < 1 || M < 1 || M > AMDKGE_SHARED_MAX_NEGS) return set_error(AMDKGE_EINVAL, "shared_label_loss: bad sizes (row0 >= 0, rows >= 0, G >= 1, 1 <= M < 2^24)");
    if (!d_scores || !d_side || !d_loss_sum) return set_error(AMDKGE_EINVAL, "shared_label_loss: NULL scores / sides / loss pointer");
    if (!(scale != 0.f) || !isfinite(scale)) return set_error(AMDKGE_EINVAL, "shared_label_loss: scale must be finite and not zero");
    SharedLabelArgs a;
    if (int rc = shared_label_args("shared_label_loss", d_neg_ids, d_s_lo, d_s_hi, d_s_ids, d_o_lo, d_o_hi, d_o_ids, list_mode, label_smoothing, reduction_mean, d_w_s,
                                   d_w_o, d_stats, a)) return rc;
    if (rows == 0) return AMDKGE_OK;
    a.S = d_scores; a.row0 = row0; a.rows = rows; a.G = G; a.B = row0 + rows; a.M = M; a.ids = d_neg_ids; a.side = d_side; a.scale = scale; a.loss_sum = d_loss_sum;
    return launch_shared_label_loss(a, (hipStream_t)stream);
}
