// policy_rollout.hip — collect_episodes_ppo (reference Actor_Critic_PPO.ipynb:
// 797-917) with the actor in the loop, as ONE launch for `frames` frames:
//
//   for each frame k:   obs[k] = observation (policy input)
//                       probs  = actor(obs[k])                   :851-855
//                       a, lp  = Bernoulli(probs).sample / .log_prob(a).sum   :857-859
//                       reward[k], done[k] = DroneGame.step(a)   (game_engine.py:95-138,
//                                            notebook reward + max_steps optional:
//                                            PPO's, or REINFORCE's for collect_episodes,
//                                            Policy_Gradients.ipynb:528-598)
//
// The two kernels it replaces (dd_mlp_forward + dd_step per frame) each pay a
// launch, the actor re-reads its 111 KB of packed parameters into every CU's
// LDS per call, and the observation makes an HBM round trip between them.
// Here a block of 8 waves (2 per SIMD, one block per CU: the parameters fill
// 111 KB of the 160 KB LDS) loads the parameters once and each wave carries
// its 32 drones through every frame with their state in registers:
//
//   * the network is mlp_core.h's mlp_body, the exact code of dd_mlp_forward,
//     so probabilities, samples and log-probabilities are bit-identical;
//   * the frame is frame.h's, the exact code of dd_step / dd_rollout, rounded
//     to the storage width after every frame as dd_step stores it;
//   * a wave tile is 32 drones (the MFMA's N) on 64 lanes: lane (c, h) holds
//     drone c in both halves h.  Both halves step the drone (the same
//     instructions either way) and each keeps the 8 observation columns that
//     are its B operands of the next frame's first layer, so the observation
//     never leaves the registers between frames; the [32, 15] rows a frame
//     records leave through a 1.9 KB LDS slice per wave as 16-byte stores.
//
// Bytes per drone-frame: obs 60 + action 1 + log-prob 4 + reward 4 + done 1
// (the state is read and written once per launch).  The work is the actor's
// (26.7k multiply-adds per drone-frame on the MFMA + LayerNorm on the VALU,
// which a gfx950 SIMD does not overlap); the frame adds ~3 % to a wave's
// cycles (SQ counters).
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
namespace prl {

struct Args {
    Consts k;              // runtime constants (switches, spawn; physics when !kRef)
    const float* obs0;
    float* obs_final;
    float* obs;
    uint8_t* actions;
    float* log_prob;
    char* reward;          // [frames][n] of T
    uint8_t* done;
    double* shaped_hist;   // [2][n] (notebook reward mode) or null
    char* engine_reward;
    uint8_t* engine_done;
    uint64_t seed;
    int64_t step;
    int64_t n;
    int32_t frames;
    int32_t max_steps;
    int32_t shape;         // kShapeNone / kShapePpo / kShapeReinforce (frame.h)
    int32_t rows_aligned;  // every frame's obs rows start 16-byte aligned (obs aligned, n % 4 == 0)
    int32_t final_aligned; // obs_final 16-byte aligned
};

// dd_policy_rollout_sampled's launch: Args, DDSampling and DDEpisodeStats.  A
// type of its own: the kernel is a template over its argument type, so the
// evaluation kernels (policy_rollout_kernel<..., EvalArgs>) are instantiations
// apart, and the collection kernel (<..., Args>: DD_SAMPLE_BERNOULLI, no
// statistics, every per-frame buffer), which sits at its register cap
// (mlp_core.h), compiles to the instructions it had before the evaluation
// existed.  With statistics, reward, done, actions and log_prob may be null.
struct EvalArgs : Args {
    int32_t mode;          // DD_SAMPLE_* (uniform: one branch per frame)
    float temperature;
    float* probs_used;     // [frames][n][3] or null
    double* ep_return;     // DDEpisodeStats: all four or none
    int32_t* ep_steps;
    uint8_t* ep_status;
    void* ep_fuel;
};

// dd_policy_rollout_population's launch: the lanes [0, n) are `members` groups
// of lanes_per_member lanes, group g driven by packed_table[g].  A block
// belongs to one group (blocks_per_member blocks each) and loads that group's
// image; its tiles end at the group's end.  Everything indexed by lane keeps
// its global index.  Again a type of its own, so the kernels above stay the
// instantiations they were.
struct PopArgs : EvalArgs {
    const float* const* packed_table;  // device, [members]
    int64_t lanes_per_member;
    int32_t members;
    int32_t blocks_per_member;         // ceil(lanes_per_member / (kWaves * kCols))
};

// A wave's first lane, and the end of the lanes its block's network drives: one batch ...
__device__ __forceinline__ int64_t first_lane(const Args& p, int wave) {
    return ((int64_t)blockIdx.x * kWaves + wave) * kCols;
}
__device__ __forceinline__ int64_t lanes_end(const Args& p) { return p.n; }
// ... or group g = block / blocks_per_member, whose tiles count from its lane g * L
__device__ __forceinline__ int64_t first_lane(const PopArgs& p, int wave) {
    const unsigned g = blockIdx.x / (unsigned)p.blocks_per_member;
    return (int64_t)g * p.lanes_per_member +
           ((int64_t)(blockIdx.x % (unsigned)p.blocks_per_member) * kWaves + wave) * kCols;
}
__device__ __forceinline__ int64_t lanes_end(const PopArgs& p) {
    return (int64_t)(blockIdx.x / (unsigned)p.blocks_per_member + 1) * p.lanes_per_member;
}

template <typename T, bool kSplit, bool kRef, typename P>
__global__ __launch_bounds__(kThreads) void policy_rollout_kernel(const float* __restrict__ packed, P p,
                                                                  Soa<T> a) {
    constexpr bool kEval = std::is_base_of<EvalArgs, P>::value;
    constexpr bool kPop = std::is_same<P, PopArgs>::value;
    extern __shared__ f32x4 lds4[];
    float* lds = reinterpret_cast<float*>(lds4);
    if constexpr (kPop) packed = p.packed_table[blockIdx.x / (unsigned)p.blocks_per_member];  // the group's image
    for (int i = threadIdx.x; i < kPacked / 4; i += kThreads)
        lds4[i] = mlp::packed_fragment(reinterpret_cast<const f32x4*>(packed), i,
                                       mlp::pack_tag(kSplit ? DD_MLP_F16X3 : DD_MLP_F32, 3));
    __syncthreads();  // the only block barrier: waves run their frames independently

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
    const int64_t d0 = first_lane(p, wave);
    if (d0 >= lanes_end(p)) return;
    const int rows = (int)min((int64_t)kCols, lanes_end(p) - d0);
    const bool live = c < rows;
    const bool writer = live && h == 0;  // one lane per drone stores its per-frame outputs
    const int64_t d = live ? d0 + c : lanes_end(p) - 1;  // lanes past the end shadow the last drone (of the group)
    float* slice = lds + kPacked + wave * kRowFloats;
    const DDConfig& sw = p.k.c;
    const Consts& k = kRef ? kRefConsts : p.k;
    constexpr bool kGuard = !kRef && std::is_same<T, double>::value;
    const bool shaped = p.shape != kShapeNone;
    const bool ppo = p.shape == kShapePpo;
    const int64_t env = a.env_id_base + d;

    Lane s;
    load_lane(a, d, s);
    double h0 = 0.0, h1 = 0.0;  // the notebook reward's two-frame distance history
    if (ppo) load_hist(p.shaped_hist, p.n, d, h0, h1);
    float x[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int col = in_col<kSplit>(q, h);
        x[q] = col < DD_OBS_DIM ? p.obs0[d * DD_OBS_DIM + col] : 0.0f;
    }
    // DDEpisodeStats of this lane, in registers across the launch's frames
    double ep_return = 0.0, ep_fuel = 0.0;
    int32_t ep_steps = 0;
    uint32_t ep_status = 0;
    bool stats = false;
    if constexpr (kEval) {
        stats = p.ep_return != nullptr;
        if (stats) {
            ep_return = p.ep_return[d];
            ep_steps = p.ep_steps[d];
            ep_status = p.ep_status[d];
            ep_fuel = (double)static_cast<const T*>(p.ep_fuel)[d];
        }
    }

    for (int f = 0; f < p.frames; ++f) {
        const int64_t fo = (int64_t)f * p.n;  // frame offset of [frames][n] buffers
        if (p.obs) store_rows<kSplit>(slice, x, c, h, rows, p.obs + (fo + d0) * DD_OBS_DIM, p.rows_aligned);

        // the actor and the collection loop's sampling (dd_mlp_forward)
        float z[3];
        mlp::mlp_body<3, kSplit, false>(lds, lane, x, z);  // serial schedule: the frame holds the registers
        float prob[3];
        mlp::actor_probs(z, prob);
        uint32_t act;
        float lp;
        if constexpr (kEval) {  // DDSampling's action selection (mlp_core.h actor_select)
            float used[3];
            mlp::actor_select(p.mode, z, prob, p.temperature, (uint64_t)env, (uint64_t)(p.step + f), p.seed, used, act,
                              lp);
            if (writer && p.probs_used) {
#pragma unroll
                for (int j = 0; j < 3; ++j) __builtin_nontemporal_store(used[j], &p.probs_used[(fo + d) * 3 + j]);
            }
        } else {
            mlp::actor_sample(prob, (uint64_t)env, (uint64_t)(p.step + f), p.seed, act, lp);
        }
        if (writer) {
            if (p.actions) __builtin_nontemporal_store((uint8_t)act, &p.actions[fo + d]);
            if (p.log_prob) __builtin_nontemporal_store(lp, &p.log_prob[fo + d]);
        }

        // the frame (dd_step / dd_rollout)
        const bool was_done = (s.status & DD_ST_DONE) != 0;
        double reward;
        if (sw.auto_reset) {  // next-step reset: the frame's result is discarded for a done lane
            reward = frame_checked<kRef, true>(k, sw, act, s);
            if (__ballot(was_done)) {
                if (was_done) {
                    spawn(sw, k.c.max_fuel, env, s);
                    reward = 0.0;
                }
            }
        } else if (was_done) {  // sticky done (game_engine.py:107-111)
            measure(s);
            reward = 0.0;
        } else {
            reward = frame_checked<kRef, true>(k, sw, act, s);
        }
        T* rew = reinterpret_cast<T*>(p.reward) + fo + d;
        uint8_t* dn = p.done + fo + d;
        T ep_rew = (T)0;       // the frame's stored reward and done flag, for the statistics
        bool ep_done = false;
        if (shaped) {  // dd_step's notebook path (PPO: the history in h0 / h1)
            double v[13];
            observe_values<kGuard, true>(k, s, v);  // the notebook reward's doubles: exact quotients
            double sr;
            const bool sd = shaped_tail(v, s, ppo, was_done, sw.auto_reset && was_done, p.max_steps, h0, h1, sr);
            if constexpr (kEval) {
                ep_rew = (T)sr;
                ep_done = sd;
            }
            if (writer) {
                if (!kEval || p.reward) __builtin_nontemporal_store((T)sr, rew);
                if (!kEval || p.done) __builtin_nontemporal_store((uint8_t)(sd ? 1 : 0), dn);
                if (p.engine_reward) {
                    __builtin_nontemporal_store((T)reward, reinterpret_cast<T*>(p.engine_reward) + fo + d);
                    __builtin_nontemporal_store((uint8_t)((s.status & DD_ST_DONE) ? 1 : 0), p.engine_done + fo + d);
                }
            }
        } else {
            if constexpr (kEval) {
                ep_rew = (T)reward;
                ep_done = (s.status & DD_ST_DONE) != 0;
            }
            if (writer) {
                if (!kEval || p.reward) __builtin_nontemporal_store((T)reward, rew);
                if (!kEval || p.done) __builtin_nontemporal_store((uint8_t)((s.status & DD_ST_DONE) ? 1 : 0), dn);
            }
        }
        next_input<kRef, kGuard, kSplit>(k, s, h, x);  // from the unrounded frame, like dd_step's obs
        quantize<T, kRef>(s);
        if constexpr (kEval) {
            // the lane's first episode, counted once: only while no frame has ended it
            if (stats && !(ep_status & DD_ST_DONE)) {
                ep_return += (double)ep_rew;  // the stored value, in frame order
                ep_steps += 1;
                ep_fuel = (double)(T)s.fuel;
                if (ep_done) ep_status = s.status | DD_ST_DONE;
            }
        }
    }

    if (p.obs_final) store_rows<kSplit>(slice, x, c, h, rows, p.obs_final + d0 * DD_OBS_DIM, p.final_aligned);
    if (writer) {
        store_lane(a, d, s);
        if (ppo) store_hist(p.shaped_hist, p.n, d, h0, h1);
        if constexpr (kEval) {
            if (stats) {
                p.ep_return[d] = ep_return;
                p.ep_steps[d] = ep_steps;
                p.ep_status[d] = (uint8_t)ep_status;
                static_cast<T*>(p.ep_fuel)[d] = (T)ep_fuel;
            }
        }
    }
}

template <typename T, bool kSplit, bool kRef, typename P>
hipError_t launch(const float* packed, const P& p, const Soa<T>& a, hipStream_t s) {
    // the LDS image exceeds the 64 KB default; per device, so set on every launch
    const hipError_t e = hipFuncSetAttribute((const void*)policy_rollout_kernel<T, kSplit, kRef, P>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes);
    if (e != hipSuccess) return e;
    const int64_t tiles = (p.n + kCols - 1) / kCols;
    unsigned blocks = (unsigned)((tiles + kWaves - 1) / kWaves);  // one wave per 32-drone tile
    if constexpr (std::is_same<P, PopArgs>::value) blocks = (unsigned)p.members * (unsigned)p.blocks_per_member;
    hipLaunchKernelGGL((policy_rollout_kernel<T, kSplit, kRef, P>), dim3(blocks), dim3(kThreads), kLdsBytes, s,
                       packed, p, a);
    return hipGetLastError();
}

// The kernel for a state's storage width, the actor's arithmetic and the physics (launch.h).  The width
// through with_bool, not with_storage: double first keeps the unit's kernels in the order they had (the
// order of instantiation is the order of the device code, which policy_rollout_isa hashes).
template <typename P>
hipError_t launch_for(const DDState& st, int32_t compute, bool ref, const float* packed, const P& p, hipStream_t s) {
    return with_bool(st.precision == DD_F64, [&](auto f64) {
        using T = std::conditional_t<decltype(f64)::value, double, float>;
        return with_bool(compute == DD_MLP_F16X3, [&](auto split) {
            return with_bool(ref, [&](auto r) {
                return launch<T, decltype(split)::value, decltype(r)::value>(packed, p, soa_of<T>(st, 0), s);
            });
        });
    });
}

}  // namespace prl
}  // namespace dd

extern "C" int dd_policy_rollout(const DDConfig* cfg, const DDState* st, const float* packed, int32_t compute,
                                 const DDPolicyRolloutIO* io, int64_t n, void* stream) {
    return dd_policy_rollout_sampled(cfg, st, packed, compute, io, nullptr, nullptr, n, stream);
}

// dd_policy_rollout_sampled (table == nullptr: one network, `packed`) and
// dd_policy_rollout_population (table: the groups' images; `packed` unused).
static int rollout_checked(const DDConfig* cfg, const DDState* st, const float* packed,
                           const float* const* table, int32_t members, int64_t lanes_per_member, int32_t compute,
                           const DDPolicyRolloutIO* io, const DDSampling* sampling, const DDEpisodeStats* stats,
                           int64_t n, void* stream) {
    if (!cfg || !io || !dd::state_ok(st) || n < 0 || io->frames < 0) return hipErrorInvalidValue;
    int64_t blocks_per_member = 0;
    if (table) {  // the groups tile [0, n) exactly; the grid is members * blocks_per_member blocks
        if ((reinterpret_cast<uintptr_t>(table) & 7u) || members < 1 || lanes_per_member < 1)
            return hipErrorInvalidValue;
        // members * lanes_per_member == n, without the product
        if (n > 0 && (n % lanes_per_member != 0 || n / lanes_per_member != members)) return hipErrorInvalidValue;
        constexpr int64_t kBlockLanes = dd::prl::kWaves * dd::prl::kCols;
        blocks_per_member = lanes_per_member / kBlockLanes + (lanes_per_member % kBlockLanes != 0);
        if (n > 0 && blocks_per_member * members > INT32_MAX) return hipErrorInvalidValue;
    }
    if (sampling) {
        if (sampling->mode != DD_SAMPLE_BERNOULLI && sampling->mode != DD_SAMPLE_TEMPERED &&
            sampling->mode != DD_SAMPLE_GREEDY)
            return hipErrorInvalidValue;
        if (sampling->mode == DD_SAMPLE_TEMPERED && !(sampling->temperature > 0.0f && isfinite(sampling->temperature)))
            return hipErrorInvalidValue;
    }
    bool with_stats = false;
    if (stats) {  // all four, or none (= no statistics)
        const int set = (stats->ep_return != nullptr) + (stats->ep_steps != nullptr) + (stats->ep_status != nullptr) +
                        (stats->ep_fuel != nullptr);
        if (set != 0 && set != 4) return hipErrorInvalidValue;
        with_stats = set == 4;
    }
    if (compute != DD_MLP_F32 && compute != DD_MLP_F16X3) return hipErrorInvalidValue;
    const int shape = dd::loop_shape(io->shaped_mode, io->shaped_hist, io->engine_reward, io->engine_done);
    if (shape < 0) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    // the per-frame buffers are optional only next to the statistics
    if ((!table && !packed) || !io->obs0 || (io->frames > 0 && !with_stats && (!io->reward || !io->done)))
        return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(packed) & 15u) return hipErrorInvalidValue;  // read as 16-byte fragments
    if (io->frames == 0 && io->obs_final == nullptr) return hipSuccess;
    dd::prl::Args p{};
    p.k = dd::make_consts(*cfg);
    p.obs0 = io->obs0;
    p.obs_final = io->obs_final;
    p.obs = io->obs;
    p.actions = io->actions;
    p.log_prob = io->log_prob;
    p.reward = static_cast<char*>(io->reward);
    p.done = io->done;
    p.shaped_hist = io->shaped_hist;
    p.engine_reward = static_cast<char*>(io->engine_reward);
    p.engine_done = io->engine_done;
    p.seed = io->seed;
    p.step = io->step;
    p.n = n;
    p.frames = io->frames;
    p.max_steps = io->max_steps;
    p.shape = shape;
    p.rows_aligned = (reinterpret_cast<uintptr_t>(io->obs) & 15u) == 0 && (n & 3) == 0;
    p.final_aligned = (reinterpret_cast<uintptr_t>(io->obs_final) & 15u) == 0;
    const bool ref = dd::uses_reference_physics(*cfg);
    const hipStream_t s = (hipStream_t)stream;
    // the plain Bernoulli draw with no probs_used and no statistics is the collection kernel
    const bool eval = with_stats || (sampling && (sampling->mode != DD_SAMPLE_BERNOULLI || sampling->probs_used));
    if (!eval && !table) return (int)dd::prl::launch_for(*st, compute, ref, packed, p, s);
    if (table) {
        // A tile starts at lane g * L + 32 k: its rows are 16-byte aligned only if L % 4 == 0 (then n % 4 == 0
        // too).  One group starts at lane 0, as dd_policy_rollout_sampled's tiles do.
        const bool lanes4 = (lanes_per_member & 3) == 0;
        p.rows_aligned = p.rows_aligned && lanes4;
        p.final_aligned = p.final_aligned && (lanes4 || members == 1);
    }
    dd::prl::PopArgs q{};
    static_cast<dd::prl::Args&>(q) = p;
    q.mode = sampling ? sampling->mode : DD_SAMPLE_BERNOULLI;
    q.temperature = sampling ? sampling->temperature : 1.0f;
    q.probs_used = sampling ? sampling->probs_used : nullptr;
    if (with_stats) {
        q.ep_return = stats->ep_return;
        q.ep_steps = stats->ep_steps;
        q.ep_status = stats->ep_status;
        q.ep_fuel = stats->ep_fuel;
    }
    if (!table) return (int)dd::prl::launch_for<dd::prl::EvalArgs>(*st, compute, ref, packed, q, s);
    q.packed_table = table;
    q.lanes_per_member = lanes_per_member;
    q.members = members;
    q.blocks_per_member = (int32_t)blocks_per_member;
    return (int)dd::prl::launch_for(*st, compute, ref, nullptr, q, s);
}

extern "C" int dd_policy_rollout_sampled(const DDConfig* cfg, const DDState* st, const float* packed,
                                         int32_t compute, const DDPolicyRolloutIO* io, const DDSampling* sampling,
                                         const DDEpisodeStats* stats, int64_t n, void* stream) {
    return rollout_checked(cfg, st, packed, nullptr, 1, n, compute, io, sampling, stats, n, stream);
}

extern "C" int dd_policy_rollout_population(const DDConfig* cfg, const DDState* st, const float* const* packed_table,
                                            int32_t members, int64_t lanes_per_member, int32_t compute,
                                            const DDPolicyRolloutIO* io, const DDSampling* sampling,
                                            const DDEpisodeStats* stats, int64_t n, void* stream) {
    if (!packed_table) return hipErrorInvalidValue;
    return rollout_checked(cfg, st, nullptr, packed_table, members, lanes_per_member, compute, io, sampling, stats, n,
                           stream);
}
