// gae_core.h — one frame of compute_gae's recursion
// (Actor_Critic_PPO.ipynb:733-787), shared by the rectangular scan
// (env_ops.hip gae_kernel) and the ragged one (train_batch.hip).
//
// Float32 throughout, in the notebook's operation order: torch evaluates
// `gamma * values[t + 1]` with gamma rounded to float32 (g), `gamma * lambda_`
// in Python doubles before that rounding (gl), and each product with the mask
// left to right:
//   delta = rewards[t] + gamma * values[t + 1] * mask - values[t]
//   gae   = delta + gamma * lambda_ * mask * gae
// The units that include this are built with -ffp-contract=off, so no product
// is fused into the following sum.
#pragma once

#include <hip/hip_runtime.h>

namespace dd {

// mask = 1 - done[t].  Updates and returns the running gae.
__device__ __forceinline__ float gae_frame(float r, float v, float v_next, float mask, float g, float gl,
                                           float& gae) {
    const float delta = (r + (g * v_next) * mask) - v;
    gae = delta + (gl * mask) * gae;
    return gae;
}

}  // namespace dd
