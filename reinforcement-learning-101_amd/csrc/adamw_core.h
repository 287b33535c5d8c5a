// adamw_core.h — dd_adamw_step's per-element arithmetic and its step scalars
// (adamw.hip has the formula and its order of operations).  Shared with the
// fused PPO update (ppo_fused.hip), so both produce the same bits.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dronestep.h"

namespace dd {
namespace adamw {

// the fourteen tensors' first elements in the flat buffer (DDMlpParams' order)
constexpr int oW0 = 0, oB0 = oW0 + 128 * 15, oG1 = oB0 + 128, oE1 = oG1 + 128;
constexpr int oW3 = oE1 + 128, oB3 = oW3 + 128 * 128, oG4 = oB3 + 128, oE4 = oG4 + 128;
constexpr int oW6 = oE4 + 128, oB6 = oW6 + 64 * 128, oG7 = oB6 + 64, oE7 = oG7 + 64;
constexpr int oW9 = oE7 + 64;
__host__ __device__ constexpr int params_of(int k) { return oW9 + 65 * k; }

struct Args {
    double lr, beta1, beta2, eps;
    double decay, omb1, omb2;  // 1 - lr wd, 1 - beta1, 1 - beta2
};

inline bool is_rate(double x) { return __builtin_isfinite(x) && x >= 0.0; }

// A DDAdamWHyper the entry points accept, and its Args.
inline bool hyper_ok(const DDAdamWHyper& h) {
    return is_rate(h.lr) && is_rate(h.eps) && is_rate(h.weight_decay) && is_rate(h.beta1) && is_rate(h.beta2) &&
           h.beta1 < 1.0 && h.beta2 < 1.0;
}
inline Args args_of(const DDAdamWHyper& h) {
    return {h.lr, h.beta1, h.beta2, h.eps, 1.0 - h.lr * h.weight_decay, 1.0 - h.beta1, 1.0 - h.beta2};
}

// This step's scalars from the running products beta1^(t-1), beta2^(t-1).
struct Step {
    double b1t, b2t, step_size, root;
};
__device__ __forceinline__ Step step_of(const Args& a, double beta1_t, double beta2_t) {
    const double b1t = beta1_t * a.beta1, b2t = beta2_t * a.beta2;
    return {b1t, b2t, a.lr / (1.0 - b1t), sqrt(1.0 - b2t)};
}

// One element's new p, m, v from the float32 p, g, m, v.
__device__ __forceinline__ void element(const Args& a, const Step& s, float p, float g, float m, float v, float& pn,
                                        float& mn, float& vn) {
    const double gd = (double)g;
    const double pd = (double)p * a.decay;
    const double md = a.beta1 * (double)m + a.omb1 * gd;
    const double vd = a.beta2 * (double)v + a.omb2 * (gd * gd);
    pn = (float)(pd - s.step_size * (md / (sqrt(vd) / s.root + a.eps)));
    mn = (float)md;
    vn = (float)vd;
}

// The flat parameter buffer as a DDMlpParams.
__host__ __device__ inline DDMlpParams params_view(const float* q, int out_dim, float ln_eps) {
    return {q + oW0, q + oB0, q + oG1, q + oE1, q + oW3, q + oB3, q + oG4, q + oE4, q + oW6,
            q + oB6, q + oG7, q + oE7, q + oW9, q + oW9 + 64 * out_dim, out_dim, ln_eps};
}

}  // namespace adamw
}  // namespace dd
