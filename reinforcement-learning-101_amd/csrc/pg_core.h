// pg_core.h — the row arithmetic of the score-function loss and the one-step
// TD loss (pg_loss.hip has the notebooks' lines and the derivation), shared by
// pg_loss.hip's launch kernels (dd_pg_losses, dd_td_losses) and the one-step
// actor-critic frame loop (ac_fused.hip), so both leave the same bits: the sums'
// parts, a row's contribution to them, the scalars from the totals, and a row's
// gradient at its network's output.  Every product and sum in double on the
// float32 inputs.
#pragma once

#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

namespace dd {
namespace pg {

struct PgPart {
    double s, cnt;
    __device__ __forceinline__ PgPart& operator+=(const PgPart& b) {
        s += b.s;
        cnt += b.cnt;
        return *this;
    }
};

struct TdPart {
    double sq, v2, cnt;
    __device__ __forceinline__ TdPart& operator+=(const TdPart& b) {
        sq += b.sq;
        v2 += b.v2;
        cnt += b.cnt;
        return *this;
    }
};

// ---- the score-function loss: -(log_prob w).mean() ------------------------------
__device__ __forceinline__ PgPart pg_row(float log_prob, float weight) {
    return {(double)log_prob * (double)weight, 1.0};
}

__device__ __forceinline__ double pg_loss_of(const PgPart& t) { return -(t.s / t.cnt); }

// d loss / d lp of an active row
__device__ __forceinline__ double pg_grad_of(float weight, double cnt) { return -((double)weight / cnt); }

// d loss / d z_j from g = d loss / d lp, the action bit and the probability
__device__ __forceinline__ float pg_grad_logit_of(double g, uint32_t bit, float pf) {
    double v = pf != pf ? (double)pf : 0.0;  // outside clamp_probs' range: 0 (NaN stays)
    if (pf >= FLT_EPSILON && pf <= 1.0f - FLT_EPSILON) v = g * ((double)bit - (double)pf);
    return (float)v;
}

// ---- the one-step TD loss --------------------------------------------------------
// The unrounded TD target and error of a row; gamma as float32, widened.
__device__ __forceinline__ void td_row_of(double v, double vn, double r, double d, double gamma, double* target,
                                          double* delta) {
    *target = r + (gamma * vn) * (1.0 - d);
    *delta = *target - v;
}

__device__ __forceinline__ TdPart td_part_of(double delta, double v) { return {delta * delta, v * v, 1.0}; }

__device__ __forceinline__ double td_mse_of(const TdPart& t) { return t.sq / t.cnt; }
__device__ __forceinline__ double td_reg_of(const TdPart& t, double value_reg) { return value_reg * (t.v2 / t.cnt); }

// d critic_loss / d v of an active row
__device__ __forceinline__ float td_grad_value_of(double delta, double v, double value_reg, double cnt) {
    return (float)((-2.0 * delta + 2.0 * value_reg * v) / cnt);
}

}  // namespace pg
}  // namespace dd
