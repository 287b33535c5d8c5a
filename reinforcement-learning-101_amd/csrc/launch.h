// launch.h — the host side's small shared pieces: tile and chunk arithmetic,
// which notebook reward a call asks for (and the checks the loops' entry
// points make of it), the action byte width, and the dispatch from run-time
// values (storage width, action format, reward shape, flags) to the kernels'
// template arguments: with_storage, with_value, with_bool.  For the C ABI's
// entry points (step.hip, rollout.hip, env_ops.hip, policy_rollout.hip,
// policy_mlp.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

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

// shape_of for the loops (dd_rollout, dd_policy_rollout_sampled), or -1 for
// arguments they both refuse: an unknown shaped_mode, one engine output
// without the other, engine outputs without a notebook reward.
inline int loop_shape(int32_t shaped_mode, const void* shaped_hist, const void* engine_reward,
                      const void* engine_done) {
    if (shaped_mode != DD_SHAPED_PPO && shaped_mode != DD_SHAPED_REINFORCE) return -1;
    if ((engine_reward != nullptr) != (engine_done != nullptr)) return -1;
    const int shape = shape_of(shaped_mode, shaped_hist, nullptr);
    return engine_reward && shape == kShapeNone ? -1 : shape;
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

// Run-time values to template arguments.  Each returns what fn returns.
// fn(T{}) with T the storage width of a DDState's precision:
// with_storage(st->precision, [&](auto tag) { using T = decltype(tag); ... }).
template <typename F>
auto with_storage(int32_t precision, F fn) {
    if (precision == DD_F32) return fn(float{});
    return fn(double{});
}

// fn(std::integral_constant<int, V>{}) for the listed V that equals v; the last
// one listed stands for every other value (a switch's default):
// with_value<kShapeNone, kShapePpo, kShapeReinforce>(shape, [&](auto sh) { f<decltype(sh)::value>(); }).
template <int kFirst, int... kRest, typename F>
auto with_value(int v, F fn) {
    if constexpr (sizeof...(kRest) == 0) {
        return fn(std::integral_constant<int, kFirst>{});
    } else {
        if (v == kFirst) return fn(std::integral_constant<int, kFirst>{});
        return with_value<kRest...>(v, fn);
    }
}

// fn(std::true_type{}) or fn(std::false_type{})
template <typename F>
auto with_bool(bool v, F fn) {
    if (v) return fn(std::true_type{});
    return fn(std::false_type{});
}

inline int finish() { return (int)hipGetLastError(); }

}  // namespace dd
