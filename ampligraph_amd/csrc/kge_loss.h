// Loss.__call__ (loss_functions.py:185-225 and the five _apply_loss bodies) for one positive and its eta corruptions: the ONE
// definition of the five losses, of their reduction divisor, of the clip range and of every NaN / inf rule.  Written over a "walk"
// of the corruption scores, so that the forward kernel (one wave per positive, scores in LDS: WaveWalk, kge_train_common.h) and the
// column-sharded loss kernel (one thread per positive, scores B floats apart: SerialWalk below) run the same operations in the same
// order -- the build keeps -ffp-contract=off, every rounding happens where it is written.
// Depends on include/amdkge.h and <math.h> only: hipcc compiles it for both sides, g++ compiles it for the CPU test
// (tests/csrc/loss_check.cpp).
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/amdkge.h"

#if defined(__HIPCC__)
#define KGE_LOSS_FN __host__ __device__ __forceinline__
#else
#define KGE_LOSS_FN inline
#endif

namespace kge {

KGE_LOSS_FN float log_sigmoid(float x) {
    // -softplus(-x), stable on both tails
    return fminf(x, 0.f) - log1pf(expf(-fabsf(x)));
}
KGE_LOSS_FN float sigmoidf(float x) {
    return 1.f / (1.f + expf(-x));
}

// the divisor of the reduction over the corruptions (:211-225): the number of terms for "mean", 1 for "sum".  `per_corruption`: 2 for
// nll, which takes its mean over the concatenated (2 eta, B) tensor of positive and corruption terms (:380-382)
KGE_LOSS_FN float loss_red(const amdkge_loss& L, float feta, float per_corruption = 1.f) {
    return L.reduction_mean ? per_corruption * feta : 1.f;
}

// clip_before_exp (loss_functions.py:60-66) = tf.clip_by_value = maximum(minimum(x, 75), -75) built from TensorFlow's NaN-PROPAGATING
// minimum / maximum: a NaN score stays NaN in the loss VALUE.  C's fminf / fmaxf return the other operand instead, which made a NaN
// positive cost a finite eta * log(1 + e^75) = 375 eta.  The GRADIENT through the clip is the exact zero of the
// minimum / maximum masks (less_equal / greater_equal are false for NaN) -- what in_clip gives beside every clip.
KGE_LOSS_FN float clip_exp(float x) {
    return (x != x) ? x : fminf(fmaxf(x, -75.f), 75.f);
}
KGE_LOSS_FN bool in_clip(float x) {
    return (x >= -75.f) && (x <= 75.f);
}
// tf.maximum(h, 0) of the two margin losses (:302-308, :458-464): NaN in the value, zero gradient (greater_equal(NaN, 0) is false)
KGE_LOSS_FN float hinge_nan(float h) {
    return (h != h) ? h : fmaxf(h, 0.f);
}
// A coefficient dL/dscore that a clip or hinge MASK sets to zero.  "Zero coefficient -> no bucket entry for the replaced row" (the
// forward kernel, STAGE) is valid only while the score's Jacobian is finite: TensorFlow multiplies the exact zero by it, so a positive
// whose own rows hold a NaN hands 0 * NaN = NaN to the replacement rows of its corruptions.  The masked coefficient of a NON-FINITE score
// (x: the score, or the hinge argument it enters) is therefore written as -0.0f: the entry test keeps it (entry_wanted), the tile pass
// adds (-0) * A -- NaN exactly where the side row is NaN, nothing elsewhere.  No loss produces -0.0f as a live coefficient.
KGE_LOSS_FN float masked_zero(float x) {
    return (fabsf(x) < INFINITY) ? 0.f : -0.f;
}
// The self-adversarial loss has no mask: its coefficient is COMPUTED, and for a score of -inf (a distance model's corruption that keeps a
// row holding an inf) it is an exact zero -- softmax weight 0 times sigma(-inf) = 0 -- which TensorFlow again multiplies by the Jacobian.
KGE_LOSS_FN float computed_zero(float c, float x) {
    return (c == 0.f) ? masked_zero(x) : c;
}

// Loss.__call__ for one positive with score P: the corruption scores of the walk are replaced by dL/dneg; returns the per-sample loss
// and dL/dpos.  A walk `w` gives the indices it owns (j = w.first(); j < eta; j += w.stride()), w.load(j) / w.store(j, v), and
// w.sum(v) / w.max(v), which combine the partial results of all the walks that share the positive (the identity for one thread, a
// wave reduction for WaveWalk: every lane gets the results).
template <class Walk>
KGE_LOSS_FN void loss_call(const amdkge_loss& L, float P, int eta, const Walk& w, float& per, float& dP) {
    const float feta = (float)eta;
    float red = loss_red(L, feta);
    switch (L.kind) {
        case AMDKGE_LOSS_PAIRWISE: {  // loss_functions.py:302-308
            float acc = 0.f, cnt = 0.f;
            for (int j = w.first(); j < eta; j += w.stride()) {
                const float h = L.margin - P + w.load(j);
                const bool act = h >= 0.f;
                acc += hinge_nan(h);
                cnt += act ? 1.f : 0.f;
                w.store(j, act ? 1.f / red : masked_zero(h));
            }
            per = w.sum(acc) / red;
            dP = -w.sum(cnt) / red;
        } break;
        case AMDKGE_LOSS_NLL: {  // :376-382 (clip at :60-66)
            red = loss_red(L, feta, 2.f);
            const float Pc = clip_exp(P);
            float acc = 0.f;
            for (int j = w.first(); j < eta; j += w.stride()) {
                const float n = w.load(j);
                const float nc = clip_exp(n);
                acc += logf(1.f + expf(nc));
                w.store(j, in_clip(n) ? sigmoidf(nc) / red : masked_zero(n));
            }
            per = (feta * logf(1.f + expf(-Pc)) + w.sum(acc)) / red;
            dP = in_clip(P) ? -feta * sigmoidf(-Pc) / red : 0.f;
        } break;
        case AMDKGE_LOSS_ABSOLUTE_MARGIN: {  // :458-464
            float acc = 0.f;
            for (int j = w.first(); j < eta; j += w.stride()) {
                const float h = L.margin + w.load(j);
                acc += hinge_nan(h);
                w.store(j, (h >= 0.f) ? 1.f / red : masked_zero(h));
            }
            per = (w.sum(acc) - feta * P) / red;
            dP = -feta / red;
        } break;
        case AMDKGE_LOSS_SELF_ADVERSARIAL: {  // :556-574 (softmax NOT stop-gradiented)
            float mx = -INFINITY;
            for (int j = w.first(); j < eta; j += w.stride()) mx = fmaxf(mx, L.alpha * w.load(j));
            mx = w.max(mx);
            float se = 0.f;
            for (int j = w.first(); j < eta; j += w.stride()) se += expf(L.alpha * w.load(j) - mx);
            se = w.sum(se);
            float lb = 0.f;
            for (int j = w.first(); j < eta; j += w.stride()) {
                const float n = w.load(j);
                const float wt = expf(L.alpha * n - mx) / se;
                lb += wt * log_sigmoid(-n - L.margin);
            }
            const float lbar = w.sum(lb);
            for (int j = w.first(); j < eta; j += w.stride()) {
                const float n = w.load(j);
                const float wt = expf(L.alpha * n - mx) / se;
                const float ell = log_sigmoid(-n - L.margin);
                w.store(j, computed_zero((wt * sigmoidf(n + L.margin) - L.alpha * wt * (ell - lbar)) / red, n));
            }
            per = -log_sigmoid(L.margin + P) - lbar / red;
            dP = -sigmoidf(-(L.margin + P));
        } break;
        default: {  // AMDKGE_LOSS_MULTICLASS_NLL :647-654
            const float eP = expf(clip_exp(P));
            float acc = 0.f;
            for (int j = w.first(); j < eta; j += w.stride()) acc += expf(clip_exp(w.load(j)));
            const float Z = w.sum(acc) / red + eP;
            for (int j = w.first(); j < eta; j += w.stride()) {
                const float n = w.load(j);
                w.store(j, in_clip(n) ? expf(clip_exp(n)) / Z / red : masked_zero(n));
            }
            per = -logf(eP / Z);
            dP = in_clip(P) ? -1.f + eP / Z : 0.f;
        } break;
    }
}

// One thread (or the CPU) walks all eta scores of a positive, which sit B floats apart: corruption j at nj[j * B].  The scores are the
// plain sums of the score kernels; the walk applies the reference's last rounding: reduce_sum, then negate (TransE / RotatE) or
// scale (HolE).
struct SerialWalk {
    float* nj;
    int64_t B;
    float sgn_scale;
    KGE_LOSS_FN int first() const { return 0; }
    KGE_LOSS_FN int stride() const { return 1; }
    KGE_LOSS_FN float load(int j) const { return sgn_scale * nj[(int64_t)j * B]; }
    KGE_LOSS_FN void store(int j, float v) const { nj[(int64_t)j * B] = v; }
    KGE_LOSS_FN float sum(float v) const { return v; }
    KGE_LOSS_FN float max(float v) const { return v; }
};

}  // namespace kge
