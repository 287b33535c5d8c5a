// policy_eval.hip — the notebooks' evaluate_policy with the reward's
// components kept (Actor_Critic_PPO.ipynb's evaluate_policy / evaluate_policy_simple
// / plot_accumulated_rewards, Policy_Gradients.ipynb's "Eval" cells), as ONE
// launch for `frames` frames:
//
//   for each frame k:   probs  = actor(state)
//                       a      = DDSampling's selection (temperature / greedy)
//                       next_state, done = DroneGame.step(a)       (sticky done)
//                       reward = calc_reward(next_state, prev_state=state)
//                       accumulated[key] += reward[key]    for the eight keys
//
// The loop is policy_rollout.hip's evaluation path (weights in LDS, one wave
// per 32-drone tile, mlp_core.h's actor, frame.h's checked frame, the exact
// observation quotients), in a translation unit of its own: the collection
// kernel there sits at its register cap and its device code is hashed into
// dd_build_info().  What differs:
//   * calc_reward's eight values (frame.h *_reward_parts) instead of their sum;
//     each is rounded to the storage width T, as the stored reward is, and added
//     in double to the lane's eight sums under DDEpisodeStats' rule (while no
//     frame has ended the lane's episode, the ending frame included);
//   * the PPO shape's prev_state is the state the actor saw, ONE frame back (the
//     notebook's evaluation), carried between launches in prev_dist; the
//     collection loop's two-frame shaped_hist is neither read nor written;
//   * sticky done only, and no timeout penalty (the notebooks' evaluation just
//     stops).
// Registers: the actor's MFMA tiles take the wave's register budget (two waves
// per SIMD: 256 VGPRs), and what a lane carries across them was spilled to
// scratch.  So the lane's state waits in a 3 KB LDS slice per wave while the
// actor runs (park / unpark), and the eight sums are a read-modify-write of
// the caller's [8][N] array once per frame (8 x 16 bytes per drone-frame, L2
// resident) instead of 16 VGPRs.  The kernel metadata of every instantiation
// is in DESIGN.md §4.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "dronestep.h"
#include "frame.h"
#include "lane_io.h"
#include "launch.h"
#include "mlp_core.h"
#include "policy_tile.h"

namespace dd {
namespace pev {

using prl::f32x4;
using prl::in_col;
using prl::kCols;
using prl::kLdsBytes;
using prl::kPacked;
using prl::kRowFloats;
using prl::kThreads;
using prl::kWaves;
constexpr int kParts = DD_REWARD_PARTS;
// A wave's parked lane state: [kParkSlots][32] doubles, slot-major (a lane's 8-byte accesses are conflict-free)
constexpr int kParkSlots = 15;
constexpr int kParkDoubles = kParkSlots * kCols;
constexpr size_t kEvalLdsBytes = kLdsBytes + (size_t)kWaves * kParkDoubles * sizeof(double);
static_assert(kLdsBytes % 8 == 0, "the parked doubles start 8-byte aligned");
static_assert(kEvalLdsBytes <= 160 * 1024, "gfx950: 160 KB of LDS per workgroup");

struct Args {
    Consts k;              // runtime constants (switches, spawn; physics when !kRef)
    const float* obs0;
    float* obs_final;
    float* obs;
    uint8_t* actions;
    float* log_prob;
    char* reward;          // [frames][n] of T: slot 7 of the frame (nullable)
    uint8_t* done;
    float* probs_used;     // [frames][n][3] or null
    double* ep_return;     // DDEpisodeStats: all four
    int32_t* ep_steps;
    uint8_t* ep_status;
    void* ep_fuel;
    double* sum;           // DDRewardParts: [8][n]
    double* prev_dist;     // [n] (PPO shape) or null
    char* per_frame;       // [frames][8][n] of T or null
    uint64_t seed;
    int64_t step;
    int64_t n;
    int32_t frames;
    int32_t shape;         // kShapePpo / kShapeReinforce (frame.h)
    int32_t rows_aligned;  // every frame's obs rows start 16-byte aligned (obs aligned, n % 4 == 0)
    int32_t final_aligned; // obs_final 16-byte aligned
    int32_t mode;          // DD_SAMPLE_* (uniform: one branch per frame)
    float temperature;
};

// DDEpisodeStats of a lane, carried across the launch's frames.
struct Episode {
    double ret, fuel;
    int32_t steps;
    uint32_t status;
};

// The lane's state across the actor: lane half 0 stores it, both halves load it back.
__device__ __forceinline__ void park(double* slot, int c, int h, const Lane& s, double prev, const Episode& e) {
    if (h == 0) {
        slot[0 * kCols + c] = s.x; slot[1 * kCols + c] = s.y; slot[2 * kCols + c] = s.vx; slot[3 * kCols + c] = s.vy;
        slot[4 * kCols + c] = s.angle; slot[5 * kCols + c] = s.omega; slot[6 * kCols + c] = s.fuel;
        slot[7 * kCols + c] = s.px; slot[8 * kCols + c] = s.py; slot[9 * kCols + c] = s.total;
        slot[10 * kCols + c] = prev;
        slot[11 * kCols + c] = __builtin_bit_cast(double, ((uint64_t)(uint32_t)s.steps << 32) | s.status);
        slot[12 * kCols + c] = e.ret;
        slot[13 * kCols + c] = e.fuel;
        slot[14 * kCols + c] = __builtin_bit_cast(double, ((uint64_t)(uint32_t)e.steps << 32) | e.status);
    }
    __syncwarp();
}

__device__ __forceinline__ void unpark(const double* slot, int c, Lane& s, double& prev, Episode& e) {
    s.x = slot[0 * kCols + c]; s.y = slot[1 * kCols + c]; s.vx = slot[2 * kCols + c]; s.vy = slot[3 * kCols + c];
    s.angle = slot[4 * kCols + c]; s.omega = slot[5 * kCols + c]; s.fuel = slot[6 * kCols + c];
    s.px = slot[7 * kCols + c]; s.py = slot[8 * kCols + c]; s.total = slot[9 * kCols + c];
    prev = slot[10 * kCols + c];
    const uint64_t w = __builtin_bit_cast(uint64_t, slot[11 * kCols + c]);
    s.status = (uint32_t)w;
    s.steps = (int32_t)(w >> 32);
    e.ret = slot[12 * kCols + c];
    e.fuel = slot[13 * kCols + c];
    const uint64_t u = __builtin_bit_cast(uint64_t, slot[14 * kCols + c]);
    e.status = (uint32_t)u;
    e.steps = (int32_t)(u >> 32);
    __syncwarp();  // the slice is rewritten next frame
}

template <typename T, bool kSplit, bool kRef>
__global__ __launch_bounds__(kThreads) void policy_eval_kernel(const float* __restrict__ packed, Args p, Soa<T> a) {
    extern __shared__ f32x4 lds4[];
    float* lds = reinterpret_cast<float*>(lds4);
    for (int i = threadIdx.x; i < kPacked / 4; i += kThreads)
        lds4[i] = mlp::packed_fragment(reinterpret_cast<const f32x4*>(packed), i,
                                       mlp::pack_tag(kSplit ? DD_MLP_F16X3 : DD_MLP_F32, 3));
    __syncthreads();  // the only block barrier: waves run their frames independently

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
    const int64_t d0 = ((int64_t)blockIdx.x * kWaves + wave) * kCols;
    if (d0 >= p.n) return;
    const int rows = (int)min((int64_t)kCols, p.n - d0);
    const bool live = c < rows;
    const bool writer = live && h == 0;  // one lane per drone stores its outputs
    const int64_t d = live ? d0 + c : p.n - 1;  // lanes past n shadow the last drone
    float* slice = lds + kPacked + wave * kRowFloats;
    double* slot = reinterpret_cast<double*>(lds + kPacked + kWaves * kRowFloats) + wave * kParkDoubles;
    const DDConfig& sw = p.k.c;
    const Consts& k = kRef ? kRefConsts : p.k;
    constexpr bool kGuard = !kRef && std::is_same<T, double>::value;
    const bool ppo = p.shape == kShapePpo;
    const int64_t env = a.env_id_base + d;

    Lane s;
    load_lane<false>(a, d, s);  // (no re-spawn here: the lane's episode counter is neither read nor written)
    double prev = ppo ? p.prev_dist[d] : 0.0;  // prev_state.distance_to_platform: the state the actor saw
    float x[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int col = in_col<kSplit>(q, h);
        x[q] = col < DD_OBS_DIM ? p.obs0[d * DD_OBS_DIM + col] : 0.0f;
    }
    Episode ep;
    ep.ret = p.ep_return[d];
    ep.fuel = (double)static_cast<const T*>(p.ep_fuel)[d];
    ep.steps = p.ep_steps[d];
    ep.status = p.ep_status[d];

    for (int f = 0; f < p.frames; ++f) {
        const int64_t fo = (int64_t)f * p.n;  // frame offset of [frames][n] buffers
        if (p.obs) prl::store_rows<kSplit>(slice, x, c, h, rows, p.obs + (fo + d0) * DD_OBS_DIM, p.rows_aligned);

        // the actor and DDSampling's action selection (dd_mlp_forward_sampled)
        float z[3];
        park(slot, c, h, s, prev, ep);
        mlp::mlp_body<3, kSplit, false>(lds, lane, x, z);  // serial schedule
        unpark(slot, c, s, prev, ep);
        float prob[3];
        mlp::actor_probs(z, prob);
        uint32_t act;
        float lp;
        float used[3];
        mlp::actor_select(p.mode, z, prob, p.temperature, (uint64_t)env, (uint64_t)(p.step + f), p.seed, used, act, lp);
        if (writer) {
            if (p.probs_used) {
#pragma unroll
                for (int j = 0; j < 3; ++j) __builtin_nontemporal_store(used[j], &p.probs_used[(fo + d) * 3 + j]);
            }
            if (p.actions) __builtin_nontemporal_store((uint8_t)act, &p.actions[fo + d]);
            if (p.log_prob) __builtin_nontemporal_store(lp, &p.log_prob[fo + d]);
        }

        // the frame (dd_step), sticky done (game_engine.py:107-111)
        const bool was_done = (s.status & DD_ST_DONE) != 0;
        if (was_done) {
            measure(s);
        } else {
            frame_checked<kRef, true>(k, sw, act, s);
        }
        double v[13];
        observe_values<kGuard, true>(k, s, v);  // calc_reward's doubles: exact quotients
        double parts[kParts];
        if (ppo) {
            notebook_reward_parts(v, s.status, prev, parts);
        } else {
            reinforce_reward_parts(v, s.status, parts);
        }
        prev = was_done ? prev : v[9];  // the next frame's prev_state is this frame's (unrounded) state
        T stored[kParts];  // as written: rounded to the storage width; zeros once the lane is done
#pragma unroll
        for (int j = 0; j < kParts; ++j) stored[j] = was_done ? (T)0 : (T)parts[j];
        const bool ep_done = (s.status & DD_ST_DONE) != 0;
        if (writer) {
            if (p.reward) __builtin_nontemporal_store(stored[7], reinterpret_cast<T*>(p.reward) + fo + d);
            if (p.done) __builtin_nontemporal_store((uint8_t)(ep_done ? 1 : 0), p.done + fo + d);
            if (p.per_frame) {
                T* pf = reinterpret_cast<T*>(p.per_frame) + fo * kParts + d;
#pragma unroll
                for (int j = 0; j < kParts; ++j) __builtin_nontemporal_store(stored[j], pf + (int64_t)j * p.n);
            }
        }
        prl::next_input<kRef, kGuard, kSplit>(k, s, h, x);  // from the unrounded frame, like dd_step's obs
        quantize<T, kRef>(s);
        // the lane's first episode, counted once: only while no frame has ended it
        if (!(ep.status & DD_ST_DONE)) {
            ep.ret += (double)stored[7];  // the stored values, in frame order
            if (writer) {
#pragma unroll
                for (int j = 0; j < kParts; ++j) p.sum[(int64_t)j * p.n + d] += (double)stored[j];
            }
            ep.steps += 1;
            ep.fuel = (double)(T)s.fuel;
            if (ep_done) ep.status = s.status | DD_ST_DONE;
        }
    }

    if (p.obs_final) prl::store_rows<kSplit>(slice, x, c, h, rows, p.obs_final + d0 * DD_OBS_DIM, p.final_aligned);
    if (writer) {
        store_lane<false>(a, d, s);
        if (ppo) p.prev_dist[d] = prev;
        p.ep_return[d] = ep.ret;
        p.ep_steps[d] = ep.steps;
        p.ep_status[d] = (uint8_t)ep.status;
        static_cast<T*>(p.ep_fuel)[d] = (T)ep.fuel;
    }
}

template <typename T, bool kSplit, bool kRef>
hipError_t launch(const float* packed, const Args& p, const Soa<T>& a, hipStream_t s) {
    // the LDS image exceeds the 64 KB default; per device, so set on every launch
    const hipError_t e = hipFuncSetAttribute((const void*)policy_eval_kernel<T, kSplit, kRef>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEvalLdsBytes);
    if (e != hipSuccess) return e;
    const int64_t tiles = (p.n + kCols - 1) / kCols;
    const unsigned blocks = (unsigned)((tiles + kWaves - 1) / kWaves);  // one wave per 32-drone tile
    hipLaunchKernelGGL((policy_eval_kernel<T, kSplit, kRef>), dim3(blocks), dim3(kThreads), kEvalLdsBytes, s, packed, p,
                       a);
    return hipGetLastError();
}

}  // namespace pev
}  // namespace dd

extern "C" int dd_policy_evaluate_parts(const DDConfig* cfg, const DDState* st, const float* packed, int32_t compute,
                                        const DDPolicyRolloutIO* io, const DDSampling* sampling,
                                        const DDEpisodeStats* stats, const DDRewardParts* parts, int64_t n,
                                        void* stream) {
    if (!cfg || !io || !dd::state_ok(st) || n < 0 || io->frames < 0) return hipErrorInvalidValue;
    if (sampling) {
        if (sampling->mode != DD_SAMPLE_BERNOULLI && sampling->mode != DD_SAMPLE_TEMPERED &&
            sampling->mode != DD_SAMPLE_GREEDY)
            return hipErrorInvalidValue;
        if (sampling->mode == DD_SAMPLE_TEMPERED && !(sampling->temperature > 0.0f && isfinite(sampling->temperature)))
            return hipErrorInvalidValue;
    }
    // the statistics carry the episode's end: all four
    if (!stats || !stats->ep_return || !stats->ep_steps || !stats->ep_status || !stats->ep_fuel)
        return hipErrorInvalidValue;
    if (compute != DD_MLP_F32 && compute != DD_MLP_F16X3) return hipErrorInvalidValue;
    const int shape = dd::loop_shape(io->shaped_mode, io->shaped_hist, io->engine_reward, io->engine_done);
    if (shape < 0 || shape == dd::kShapeNone) return hipErrorInvalidValue;  // the engine's reward has no components
    if (io->engine_reward) return hipErrorInvalidValue;                     // not written by this call
    if (!parts || !parts->sum) return hipErrorInvalidValue;
    if (shape == dd::kShapePpo && !parts->prev_dist) return hipErrorInvalidValue;
    if (cfg->auto_reset) return hipErrorInvalidValue;  // one episode per lane, sticky done
    if (n == 0) return hipSuccess;
    if (!packed || !io->obs0) return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(packed) & 15u) return hipErrorInvalidValue;  // read as 16-byte fragments
    if (io->frames == 0 && io->obs_final == nullptr) return hipSuccess;
    dd::pev::Args p{};
    p.k = dd::make_consts(*cfg);
    p.obs0 = io->obs0;
    p.obs_final = io->obs_final;
    p.obs = io->obs;
    p.actions = io->actions;
    p.log_prob = io->log_prob;
    p.reward = static_cast<char*>(io->reward);
    p.done = io->done;
    p.probs_used = sampling ? sampling->probs_used : nullptr;
    p.ep_return = stats->ep_return;
    p.ep_steps = stats->ep_steps;
    p.ep_status = stats->ep_status;
    p.ep_fuel = stats->ep_fuel;
    p.sum = parts->sum;
    p.prev_dist = shape == dd::kShapePpo ? parts->prev_dist : nullptr;
    p.per_frame = static_cast<char*>(parts->per_frame);
    p.seed = io->seed;
    p.step = io->step;
    p.n = n;
    p.frames = io->frames;
    p.shape = shape;
    p.rows_aligned = (reinterpret_cast<uintptr_t>(io->obs) & 15u) == 0 && (n & 3) == 0;
    p.final_aligned = (reinterpret_cast<uintptr_t>(io->obs_final) & 15u) == 0;
    p.mode = sampling ? sampling->mode : DD_SAMPLE_BERNOULLI;
    p.temperature = sampling ? sampling->temperature : 1.0f;
    const bool ref = dd::uses_reference_physics(*cfg);
    const hipStream_t s = (hipStream_t)stream;
    return (int)dd::with_bool(st->precision == DD_F64, [&](auto f64) {
        using T = std::conditional_t<decltype(f64)::value, double, float>;
        return dd::with_bool(compute == DD_MLP_F16X3, [&](auto split) {
            return dd::with_bool(ref, [&](auto r) {
                return dd::pev::launch<T, decltype(split)::value, decltype(r)::value>(packed, p, dd::soa_of<T>(*st, 0),
                                                                                      s);
            });
        });
    });
}
