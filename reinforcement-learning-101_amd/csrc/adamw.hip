// adamw.hip — dd_adamw_step / dd_adamw_init: torch.optim.AdamW on one network's
// flat parameter buffer, the training cell's `policy_optimizer.step();
// critic_optimizer.step()` (Actor_Critic_PPO.ipynb, PHASE 3).
//
// Per element, in double from the float32 p, g, m, v, in this order (the
// library is built with -ffp-contract=off; tests/adamw_ref.py restates it):
//   pd = p decay                       decay = 1 - lr wd     (host, once)
//   md = beta1 m + omb1 g              omb1  = 1 - beta1     (host, once)
//   vd = beta2 v + omb2 (g g)          omb2  = 1 - beta2     (host, once)
//   b1t' = b1t beta1,  b2t' = b2t beta2                      (the running products)
//   step_size = lr / (1 - b1t'),  root = sqrt(1 - b2t')
//   pn = pd - step_size (md / (sqrt(vd) / root + eps))
// and p = (float)pn, m = (float)md, v = (float)vd: one rounding each.  The f64
// divide and square root are correctly rounded, so NumPy gives the same bits.
//
// The network is 27,456 + 65 K floats, so one block of 1,024 threads holds the
// whole step: 28 candidates of each of p, m, v per thread in registers, then
// (DD_MLP_F16X3 only) the block's verdict on the candidate parameters by the
// rules MlpNet applies to a state_dict on the host, then the commit.  A
// refused step writes the status bit and nothing else.  The verdict is a
// maximum over a fixed tree and an or; no atomics, nothing depends on timing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dronestep.h"
#include "adamw_core.h"
#include "launch.h"

namespace dd {
namespace adamw {

constexpr int kThreads = 1024;
constexpr int kPer = 28;  // 28 x 1,024 = 28,672 >= 27,651 (the actor)
static_assert(params_of(3) == 27651 && params_of(1) == 27521 && params_of(3) <= kPer * kThreads, "flat layout");

// The f16x3 forward's operand ranges (delivery_drone_amd/policy.py _validated).
constexpr float kWeightLimit = 65504.0f / 32;  // hidden weights: centred and x16 they must stay in f16
constexpr double kRoot128 = 0x1.6a09e667f3bcdp+3, kRoot64 = 8.0;  // sqrt(rows)
constexpr int kMaxima = 7;  // |gamma|, |beta| of the three LayerNorms, and the "refuse" flag

__device__ __forceinline__ bool layer_norm_fits(float gamma_max, float beta_max, double root) {
    const double bound = (double)gamma_max * root * (1.0 + 0x1p-8) + (double)beta_max;
    return bound < 128.0;
}

template <bool kCheck>
__global__ __launch_bounds__(kThreads) void step_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v,
                                                        DDAdamWState* __restrict__ st, int n, Args a) {
    const int tid = threadIdx.x;
    const int64_t step = st->step;
    const int32_t status = st->status;
    const Step now = step_of(a, st->beta1_t, st->beta2_t);

    float cp[kPer], cm[kPer], cv[kPer];
    float top[kMaxima] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const int e = i * kThreads + tid;
        cp[i] = cm[i] = cv[i] = 0.0f;
        if (e < n) {
            element(a, now, p[e], g[e], m[e], v[e], cp[i], cm[i], cv[i]);
            if constexpr (!kCheck) {  // nothing can refuse the step: each thread owns its elements
                p[e] = cp[i];
                m[e] = cm[i];
                v[e] = cv[i];
            } else {
                const float c = cp[i], mag = __builtin_fabsf(c);
                const bool hidden = e < oB0 || (e >= oW3 && e < oB3) || (e >= oW6 && e < oB6);
                if (hidden && !(mag < kWeightLimit)) top[6] = 1.0f;  // too large, inf or NaN
                const int first[6] = {oG1, oE1, oG4, oE4, oG7, oE7};
                const int last[6] = {oE1, oW3, oE4, oW6, oE7, oW9};
#pragma unroll
                for (int k = 0; k < 6; ++k)
                    if (e >= first[k] && e < last[k]) {
                        if (c != c) top[6] = 1.0f;  // a NaN maximum fails the bound, as torch's max() carries it
                        top[k] = __builtin_fmaxf(top[k], mag);
                    }
            }
        }
    }

    bool commit = true;
    if constexpr (kCheck) {
        __shared__ float sh[kMaxima][kThreads];
#pragma unroll
        for (int k = 0; k < kMaxima; ++k) sh[k][tid] = top[k];
        __syncthreads();
        for (int half = kThreads / 2; half > 0; half >>= 1) {
            if (tid < half) {
#pragma unroll
                for (int k = 0; k < kMaxima; ++k) sh[k][tid] = __builtin_fmaxf(sh[k][tid], sh[k][tid + half]);
            }
            __syncthreads();
        }
        commit = sh[6][0] == 0.0f && layer_norm_fits(sh[0][0], sh[1][0], kRoot128) &&
                 layer_norm_fits(sh[2][0], sh[3][0], kRoot128) && layer_norm_fits(sh[4][0], sh[5][0], kRoot64);
    }
    __syncthreads();  // every thread has read the state block

    if (commit) {
        if constexpr (kCheck) {
#pragma unroll
            for (int i = 0; i < kPer; ++i) {
                const int e = i * kThreads + tid;
                if (e < n) {
                    p[e] = cp[i];
                    m[e] = cm[i];
                    v[e] = cv[i];
                }
            }
        }
        if (tid == 0) {
            st->step = step + 1;
            st->beta1_t = now.b1t;
            st->beta2_t = now.b2t;
        }
    } else if (tid == 0) {
        st->status = status | DD_ADAMW_REFUSED;
    }
}

__global__ __launch_bounds__(256) void init_kernel(float* __restrict__ m, float* __restrict__ v, int64_t count,
                                                   DDAdamWState* __restrict__ st) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < count) {
        m[e] = 0.0f;
        v[e] = 0.0f;
    }
    if (e == 0) {
        st->step = 0;
        st->beta1_t = 1.0;
        st->beta2_t = 1.0;
        st->status = 0;
        st->_pad = 0;
    }
}

}  // namespace adamw
}  // namespace dd

extern "C" {

int64_t dd_adamw_state_bytes(void) { return (int64_t)sizeof(DDAdamWState); }

int dd_adamw_init(float* exp_avg, float* exp_avg_sq, int64_t count, DDAdamWState* state, void* stream) {
    if (!state || count < 0 || count > (int64_t)1 << 40) return hipErrorInvalidValue;
    if (count > 0 && (!exp_avg || !exp_avg_sq)) return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(state) & 7u) return hipErrorInvalidValue;
    const int64_t blocks = count > 0 ? (count + 255) / 256 : 1;
    hipLaunchKernelGGL(dd::adamw::init_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       exp_avg, exp_avg_sq, count, state);
    return dd::finish();
}

int dd_adamw_step(const DDAdamWHyper* hyper, const DDAdamWIO* io, void* stream) {
    using namespace dd::adamw;
    if (!hyper || !io) return hipErrorInvalidValue;
    if (!io->params || !io->grads || !io->exp_avg || !io->exp_avg_sq || !io->state) return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(io->state) & 7u) return hipErrorInvalidValue;
    if (io->out_dim != 1 && io->out_dim != 3) return hipErrorInvalidValue;
    if (io->compute != DD_MLP_F32 && io->compute != DD_MLP_F16X3) return hipErrorInvalidValue;
    if (!hyper_ok(*hyper)) return hipErrorInvalidValue;
    if (io->packed && ((reinterpret_cast<uintptr_t>(io->packed) & 15u) || !(io->ln_eps > 0.0f)))
        return hipErrorInvalidValue;
    const int n = params_of(io->out_dim);
    const Args a = args_of(*hyper);
    hipStream_t s = static_cast<hipStream_t>(stream);
    dd::with_bool(io->compute == DD_MLP_F16X3, [&](auto check) {
        hipLaunchKernelGGL(step_kernel<decltype(check)::value>, dim3(1), dim3(kThreads), 0, s, io->params, io->grads,
                           io->exp_avg, io->exp_avg_sq, io->state, n, a);
    });
    const int e = dd::finish();
    if (e != 0 || !io->packed) return e;
    const DDMlpParams net = params_view(io->params, io->out_dim, io->ln_eps);
    return dd_mlp_pack(&net, io->compute, io->packed, stream);
}

}  // extern "C"
