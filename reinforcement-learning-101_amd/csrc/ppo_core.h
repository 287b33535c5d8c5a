// ppo_core.h — compute_ppo_losses' per-row arithmetic and the scalars formed
// from the sums (ppo_loss.hip has the notebook's lines and the derivation of the
// gradients).  Shared by dd_ppo_losses' kernels and the fused PPO update
// (ppo_fused.hip), so both produce the same bits.
#pragma once

#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "dronestep.h"

namespace dd {
namespace ppo {

// One thread's, block's or the batch's sums; += is the tree's node.  min and
// max carry a NaN ratio on, as torch.min / torch.max do.
struct Part {
    double surr, sq, ent, r, clipped;
    float rmin, rmax;
    __device__ __forceinline__ Part& operator+=(const Part& b) {
        surr += b.surr;
        sq += b.sq;
        ent += b.ent;
        r += b.r;
        clipped += b.clipped;
        rmin = (b.rmin < rmin || b.rmin != b.rmin) ? b.rmin : rmin;
        rmax = (b.rmax > rmax || b.rmax != b.rmax) ? b.rmax : rmax;
        return *this;
    }
};

// The sums of no row.
__device__ __forceinline__ Part no_rows() { return {0.0, 0.0, 0.0, 0.0, 0.0, INFINITY, -INFINITY}; }

__device__ __forceinline__ float ratio_of(float lp, float old) { return (float)exp((double)(lp - old)); }

// One row's clipped surrogate: the ratio, whether it left [lo, hi], the two
// surrogates.
struct Surrogate {
    float rf;
    bool outside;
    double r, A, s1, s2;
    __device__ __forceinline__ double smaller() const { return s2 < s1 ? s2 : s1; }
    // d total_loss / d new_log_prob over m rows: the clipped branch taken (or tied with A == 0)
    // outside the range passes no gradient
    __device__ __forceinline__ double grad(double md) const { return !(s1 < s2) && outside ? 0.0 : -A * r / md; }
};

__device__ __forceinline__ Surrogate surrogate_of(float log_prob, float old_log_prob, float advantage, float lo,
                                                  float hi) {
    const float rf = ratio_of(log_prob, old_log_prob);
    const float cf = rf < lo ? lo : rf > hi ? hi : rf;  // torch.clamp: a NaN stays
    const double r = rf, A = advantage;
    return {rf, rf < lo || rf > hi, r, A, r * A, (double)cf * A};
}

// grad_logits[k][j]: g = Surrogate::grad, on = the given action's bit j, pf =
// the actor's probability of factor j.
__device__ __forceinline__ float grad_logit_of(double g, bool on, float pf, double entropy_coef, double md) {
    double v = pf != pf ? (double)pf : 0.0;  // outside clamp_probs' range: 0 (NaN stays)
    if (pf >= FLT_EPSILON && pf <= 1.0f - FLT_EPSILON) {
        const double p = pf, a = on ? 1.0 : 0.0;
        v = g * (a - p) + entropy_coef / (3.0 * md) * (log(p) - log1p(-p)) * (p * (1.0 - p));
    }
    return (float)v;
}

// grad_values[k] from dv = v_k - R_k.
__device__ __forceinline__ float grad_value_of(double value_coef, double dv, double md) {
    return (float)(value_coef * 2.0 * dv / md);
}

// The scalars from the batch's sums.
__device__ __forceinline__ double policy_loss_of(const Part& t, double md) { return -(t.surr / md); }
__device__ __forceinline__ double value_loss_of(double sq, double md) { return sq / md; }
__device__ __forceinline__ double entropy_of(const Part& t, double md) { return t.ent / (3.0 * md); }
__device__ __forceinline__ double total_loss_of(double policy, double value, double entropy, double entropy_coef,
                                                double value_coef) {
    return policy + value_coef * value - entropy_coef * entropy;
}
// torch.std's default (unbiased) from the sum of squared deviations from the mean
__device__ __forceinline__ double ratio_std_of(double ss, int64_t m) {
    return m < 2 ? __builtin_nan("") : sqrt(ss / (double)(m - 1));
}

}  // namespace ppo
}  // namespace dd
