// launch.h — the host side's small shared pieces: tile and chunk arithmetic,
// which notebook reward a call asks for, the action byte width and the
// storage-width dispatch of the C ABI's entry points (step.hip, rollout.hip,
// env_ops.hip, policy_rollout.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dronestep.h"
#include "lane_io.h"

namespace dd {

inline int64_t tiles_of(int64_t n) { return (n + kBlock - 1) / kBlock; }

// The notebook reward a call asks for (frame.h kShape*): REINFORCE's by its
// mode, PPO's when the history pointer is set, else none.
inline int shape_of(int32_t shaped_mode, const void* shaped_hist, const void* shaped_reward) {
    if (shaped_mode == DD_SHAPED_REINFORCE) return kShapeReinforce;
    return shaped_hist || shaped_reward ? kShapePpo : kShapeNone;
}

// Bytes of one lane's action in a caller's buffer (DD_ACT_PHILOX: none, the
// kernel draws it).
__host__ __device__ constexpr int64_t action_bytes(int fmt) {
    return fmt == DD_ACT_F32X3 ? 12 : fmt == DD_ACT_U8X3 ? 3 : fmt == DD_ACT_BITMASK ? 1 : 0;
}

// fn(first, len) for every launch's run of lanes: at most kChunk each, so a
// lane's byte offset fits 32 bits (lane_io.h).
template <typename F>
void for_each_chunk(int64_t n, F fn) {
    for (int64_t first = 0; first < n; first += kChunk) fn(first, n - first < kChunk ? n - first : kChunk);
}

// fn(T{}) with T the storage width of a DDState's precision:
// with_storage(st->precision, [&](auto tag) { using T = decltype(tag); ... }).
template <typename F>
void with_storage(int32_t precision, F fn) {
    if (precision == DD_F32) fn(float{});
    else fn(double{});
}

inline int finish() { return (int)hipGetLastError(); }

}  // namespace dd
