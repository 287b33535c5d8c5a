// policy_tile.h — the 32-drone wave tile of the fused actor + frame loops
// (policy_rollout.hip, policy_eval.hip): which observation columns a lane half
// holds, the [32, 15] row slice a wave stores through LDS, and the next
// frame's policy input.  Lane (c, h) of a wave holds drone c in both halves h
// (mlp_core.h's MFMA layout).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dronestep.h"
#include "frame.h"
#include "mlp_core.h"

namespace dd {
namespace prl {

using mlp::kCols;
using mlp::kPacked;
using mlp::kThreads;
using mlp::kWaves;
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kRowFloats = kCols * DD_OBS_DIM;  // one wave's [32, 15] observation slice: 480 floats
constexpr size_t kLdsBytes = (size_t)(kPacked + kWaves * kRowFloats) * sizeof(float);
static_assert(kPacked % 4 == 0 && kRowFloats % 4 == 0, "16-byte aligned LDS slices");

// Observation column `col` of layer 1's B operand for lane half h: column
// 8h + q (f16x3: one k-step of 16) or 2q + h (f32: k-steps of 2).
template <bool kSplit>
__device__ __forceinline__ constexpr int in_col(int q, int h) {
    return kSplit ? 8 * h + q : 2 * q + h;
}

// A wave's [rows, 15] observation slice, assembled in LDS from the lanes'
// columns, stored at dst (16-byte stores when aligned).
template <bool kSplit>
__device__ __forceinline__ void store_rows(float* slice, const float (&x)[8], int c, int h, int rows, float* dst,
                                           bool aligned) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int col = in_col<kSplit>(q, h);
        if (col < DD_OBS_DIM) slice[c * DD_OBS_DIM + col] = x[q];
    }
    __syncwarp();
    const int nf = rows * DD_OBS_DIM;
    if (aligned) {
        const int nv = nf >> 2;
        const f32x4* src4 = reinterpret_cast<const f32x4*>(slice);
        f32x4* dst4 = reinterpret_cast<f32x4*>(dst);
        for (int k = lane; k < nv; k += 64) __builtin_nontemporal_store(src4[k], &dst4[k]);
        for (int k = (nv << 2) + lane; k < nf; k += 64) __builtin_nontemporal_store(slice[k], &dst[k]);
    } else {
        for (int k = lane; k < nf; k += 64) __builtin_nontemporal_store(slice[k], &dst[k]);
    }
    __syncwarp();  // the slice is rewritten next frame
}

// The next frame's policy input: observation row of the frame's (unrounded)
// state as dd_step writes it, this lane half's 8 columns of it.
template <bool kRef, bool kGuard, bool kSplit>
__device__ __forceinline__ void next_input(const Consts& k, const Lane& s, int h, float (&x)[8]) {
    double v[13];
    observe_values<kGuard>(k, s, v);
    float o[16];
    write_obs_row(v, s.status, o);
    o[15] = 0.0f;
#pragma unroll
    for (int q = 0; q < 8; ++q) x[q] = h ? o[in_col<kSplit>(q, 1)] : o[in_col<kSplit>(q, 0)];
}

}  // namespace prl
}  // namespace dd
