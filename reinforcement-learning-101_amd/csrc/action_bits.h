// action_bits.h — a batch row's given action as dd_step's bitmask, for the
// loss units that score given actions (ppo_loss.hip, pg_loss.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dronestep.h"

namespace dd {

// Row k's given action as dd_step's bitmask (DDMlpEvalIO's two formats).
__device__ __forceinline__ uint32_t given_bits(const void* actions, int32_t fmt, int64_t k) {
    if (fmt == DD_ACT_BITMASK) return static_cast<const uint8_t*>(actions)[k] & 7u;
    const float* a = static_cast<const float*>(actions) + k * 3;
    return (a[0] != 0.0f ? 1u : 0u) | (a[1] != 0.0f ? 2u : 0u) | (a[2] != 0.0f ? 4u : 0u);
}

}  // namespace dd
