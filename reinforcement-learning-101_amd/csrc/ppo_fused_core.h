// ppo_fused_core.h — one workgroup's walk over a learner's minibatch epochs:
// the device code of dd_ppo_update_fused (ppo_fused.hip has the design and the
// contract) shared with dd_ppo_update_population (ppo_fused_population.hip),
// which runs the same walk for every member of a population, so both leave the
// same bits.  The phases after a step's head gradient (backward_norm,
// clip_adamw, repack) are functions of their own: dd_actor_critic_train
// (ac_fused.hip) runs them inside its frame loop, dd_reinforce_train
// (reinforce_fused.hip) the last two after its own backward.  Both also take
// load_image here, reinforce_fused.hip load_row, and all three member-table
// entries (ppo_fused_population.hip, ac_fused.hip, reinforce_fused.hip) the
// host section's clip_of, the check that no two owners share a buffer (Owned,
// owned_of / owned_apart, shared_between_owners) and launch_with_table.
//
// learn<K, Rows> is parameterised on where a minibatch's rows come from:
//   DirectRows  rows [first, first + rows) of the columns as the caller laid
//               them out, first = epoch epoch_stride + i size (ppo_fused.hip).
//   a staged source (ppo_fused_population.hip) gathers the minibatch's rows
//               into a stage of its own at begin() and serves them from there.
// A source gives begin<kActor>(epoch, i, rows) at the top of a minibatch (all
// threads call it; LDS is free then), which returns the minibatch's view:
// states() (its [rows][15], row 0 first), bits(d), old_log_prob(d),
// advantage(d) and ret(d) of its row d.
//
// Memory the block rewrites and reads again (parameters, moments, gradients,
// the two packed images, the head gradient, a source's stage): same-workgroup
// traffic through the CU's own vector L1, ordered by __syncthreads() (which
// drains the stores); no agent-scope fence.  None of it is read through a
// const __restrict__ pointer, so no load of it can become a scalar or
// read-only load (the scalar cache is not coherent with vector stores).
//
// LDS: the forward's packed image (109 KB) and the backward's transposition
// buffers (136 KB) take turns in one region; the per-row forward outputs and the
// reductions' scratch follow it.  154 KB, one block per CU.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "action_bits.h"
#include "adamw_core.h"
#include "batch_core.h"
#include "dronestep.h"
#include "launch.h"
#include "mlp_backward_core.h"
#include "mlp_core.h"
#include "ppo_core.h"

namespace dd {
namespace fused {

using mlp::f32x4;
using mlpbwd::kFinishBlocks;
using mlpbwd::kPackedB;
using mlpbwd::kTileRows;
using ppo::Part;

static_assert(kTileRows == DD_PPO_FUSED_ROWS, "a minibatch is one backward row tile");
static_assert(kBlock == 4 * 64 && kTileRows == 4 * mlp::kCols, "four waves, 32 rows each");
static_assert(mlp::kLdsBytes <= mlpbwd::kLdsB, "the forward image fits the backward's LDS");

constexpr int kRowFloats = 8;  // a row's forward outputs: log_prob, entropy, probs[3] (actor); value (critic)
constexpr size_t kRowsAt = mlpbwd::kLdsB;
constexpr size_t kRedAt = kRowsAt + kTileRows * kRowFloats * sizeof(float);
constexpr size_t kNormAt = kRedAt + kBlock * sizeof(Part);
constexpr size_t kLds = kNormAt + kBlock * sizeof(double);
static_assert(kRowsAt % 16 == 0 && kRedAt % 8 == 0 && kNormAt % 8 == 0, "alignment");
static_assert(kLds <= 160 * 1024, "LDS of one CU");

// Workspace per network: the backward's packed weight images, the minibatch's
// gradient at the network's output.
constexpr int kHeadFloats = kTileRows * 4;
constexpr int64_t kNetWorkspace = (int64_t)(kPackedB + kHeadFloats) * (int64_t)sizeof(float);
static_assert(kNetWorkspace % 16 == 0, "16-byte weight fragments");

struct Net {
    float* params;
    float* grads;
    float* exp_avg;
    float* exp_avg_sq;
    DDAdamWState* state;
    float* packed;
    float* image;  // workspace: mlpbwd's packed images
    float* head;   // workspace: grad_logits [rows][3] or grad_values [rows]
    adamw::Args opt;
    float ln_eps;
};

struct Args {
    Net net[2];  // actor, critic
    const float* states;
    const void* actions;
    const float* old_log_probs;
    const float* advantages;
    const float* returns;
    int64_t epoch_stride;
    int32_t action_format, num_epochs, m, size, steps;
    float lo, hi;  // the clip range, as float32
    double entropy_coef, value_coef, max_norm;
    bool clip;
    double* logs;
};

// The rows as the caller laid them out: epoch e's batch at e epoch_stride.
struct DirectRows {
    const Args& a;
    struct At {
        const Args& a;
        const int64_t first;
        __device__ __forceinline__ const float* states() const { return a.states + first * DD_OBS_DIM; }
        __device__ __forceinline__ uint32_t bits(int d) const {
            return given_bits(a.actions, a.action_format, first + d);
        }
        __device__ __forceinline__ float old_log_prob(int d) const { return a.old_log_probs[first + d]; }
        __device__ __forceinline__ float advantage(int d) const { return a.advantages[first + d]; }
        __device__ __forceinline__ float ret(int d) const { return a.returns[first + d]; }
    };
    template <bool kActor>
    __device__ __forceinline__ At begin(int epoch, int i, int) const {
        return {a, (int64_t)epoch * a.epoch_stride + (int64_t)i * a.size};
    }
};

// dd_mlp_pack's shared quantities (mlp_core.h pack_f32_at), from the LDS table.
constexpr int kMeans = 15 + 128 + 128 + 3;  // the columns of w0, w3, w6; b0, b3, b6
struct PackTable {
    const double* mean;
    const float* scale;
    __device__ double weight_mean(int base, int col) const {
        return mean[(base == mlp::kA1 ? 0 : base == mlp::kA2 ? 15 : 143) + col];
    }
    __device__ double bias_mean(int L) const { return mean[271 + L]; }
    __device__ float act_scale(int L) const { return scale[L]; }
};

// The batch's total as dd_ppo_losses forms it when block 0 holds every row:
// block 0's block_sum, then stat_total over (that partial, nothing, ...).
template <typename V>
__device__ __forceinline__ V stat_sum(V v, V nothing, V* sh) {
    const V partial = block_sum<V>(v, sh);
    V mine = threadIdx.x == 0 ? partial : nothing;
    mine += nothing;  // part[t] + part[t + kBlock]
    return block_sum<V>(mine, sh);
}

// A network's packed image into LDS (all threads; a barrier follows at the caller).
__device__ __forceinline__ void load_image(const float* packed, float* lds) {
    f32x4* lds4 = reinterpret_cast<f32x4*>(lds);
    const f32x4* src4 = reinterpret_cast<const f32x4*>(packed);
    for (int j = threadIdx.x; j < mlp::kPacked / 4; j += kBlock) lds4[j] = src4[j];
}

// Layer 1's B operand of a [15] row for this lane half: the row's columns
// 2q + h, zero past column 14 and for a dead row.
__device__ __forceinline__ void load_row(const float* row, bool live, int h, float (&x)[8]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int col = 2 * q + h;
        x[q] = live && col < DD_OBS_DIM ? row[col] : 0.0f;
    }
}

// ---- one step's phases after the head gradient is written ---------------------
// learn's, and ac_fused.hip's (the one-step actor-critic frame loop): every
// thread of the block calls each, in this order.  LDS as learn lays it out.

// A network's step count and running beta products, in registers between the
// block's steps (the state block is written after every step).
struct Running {
    int64_t step;
    double beta1_t, beta2_t;
};

__device__ __forceinline__ Running running_of(const Net& n) {
    return {n.state->step, n.state->beta1_t, n.state->beta2_t};
}

// dd_mlp_backward of one row tile into n.grads (the weight images, then the
// tile; n.head holds the head gradient of `rows` rows of `states`), and the
// norm before clipping.  Starts with writes to workspace only, so the head
// gradient needs no barrier of its own before the call.
template <int K>
__device__ __forceinline__ double backward_norm(const Net& n, const DDMlpParams& p, const float* states, int rows,
                                                float* lds) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    double* redd = reinterpret_cast<double*>(reinterpret_cast<char*>(lds) + kRedAt);
    double* normp = reinterpret_cast<double*>(reinterpret_cast<char*>(lds) + kNormAt);
    constexpr int kCount = adamw::params_of(K);
    for (int idx = tid; idx < kPackedB; idx += kBlock) n.image[idx] = mlpbwd::packed_value(p, idx);
    __syncthreads();  // the images and the head gradient are written
    mlpbwd::backward_block<K>(p, states, n.head, rows, n.image, n.grads, 0, 1, lds);
    __syncthreads();  // the gradient is written; LDS is free again

    for (int b = wave; b < kFinishBlocks; b += kBlock / 64) {
        double sq[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = b * kBlock + 64 * j + lane;
            sq[j] = 0.0;
            if (e < kCount) {
                const float f = (float)(0.0 + (double)n.grads[e]);  // the finish's sum from 0.0
                n.grads[e] = f;
                sq[j] = (double)f * (double)f;
            }
        }
        const double s = wave_block_sum(sq);
        if (lane == 0) normp[b] = s;
    }
    __syncthreads();
    return sqrt(block_sum<double>(tid < kFinishBlocks ? normp[tid] : 0.0, redd));
}

// clip_grad_norm_ on n.grads, then the AdamW step: each thread reads and writes
// its own elements.  Ends with the new parameters written.
template <int K>
__device__ __forceinline__ void clip_adamw(const Net& n, bool clip, double max_norm, double norm, Running& run) {
    const int tid = threadIdx.x;
    constexpr int kCount = adamw::params_of(K);
    const double coef = clip ? mlpbwd::clip_coef(max_norm, norm) : 1.0;
    const bool scale = !(coef == 1.0);  // a NaN factor scales, as clip_grad_norm_'s does
    const adamw::Step now = adamw::step_of(n.opt, run.beta1_t, run.beta2_t);
    for (int e = tid; e < kCount; e += kBlock) {
        float g = n.grads[e];
        if (scale) {
            g = (float)((double)g * coef);
            n.grads[e] = g;
        }
        float pn, mn, vn;
        adamw::element(n.opt, now, n.params[e], g, n.exp_avg[e], n.exp_avg_sq[e], pn, mn, vn);
        n.params[e] = pn;
        n.exp_avg[e] = mn;
        n.exp_avg_sq[e] = vn;
    }
    run.step += 1;
    run.beta1_t = now.b1t;
    run.beta2_t = now.b2t;
    if (tid == 0) {
        n.state->step = run.step;
        n.state->beta1_t = run.beta1_t;
        n.state->beta2_t = run.beta2_t;
    }
    __syncthreads();  // the new parameters are written
}

// dd_mlp_pack of the new parameters into n.packed.  Ends with the image
// written and the table (the reductions' scratch) free again.
__device__ __forceinline__ void repack(const Net& n, const DDMlpParams& p, float* lds) {
    const int tid = threadIdx.x;
    double* redd = reinterpret_cast<double*>(reinterpret_cast<char*>(lds) + kRedAt);
    float* scales = reinterpret_cast<float*>(redd + kMeans);
    for (int task = tid; task < kMeans + 3; task += kBlock) {
        if (task < 15) redd[task] = mlp::column_mean(p.w0, 128, DD_OBS_DIM, task);
        else if (task < 143) redd[task] = mlp::column_mean(p.w3, 128, 128, task - 15);
        else if (task < 271) redd[task] = mlp::column_mean(p.w6, 64, 128, task - 143);
        else if (task < kMeans) redd[task] = mlp::column_mean(task == 271 ? p.b0 : task == 272 ? p.b3 : p.b6,
                                                              task == 273 ? 64 : 128, 1, 0);
        else if (task == kMeans) scales[0] = mlp::act_scale_of(p.ln1_w, p.ln1_b, 128);
        else if (task == kMeans + 1) scales[1] = mlp::act_scale_of(p.ln4_w, p.ln4_b, 128);
        else scales[2] = mlp::act_scale_of(p.ln7_w, p.ln7_b, 64);
    }
    __syncthreads();
    const PackTable table = {redd, scales};
    for (int j = tid; j < mlp::kPacked; j += kBlock) n.packed[j] = mlp::pack_f32_at(p, j, table);
    __syncthreads();  // the image is written; the table is free again
}

// Where learn writes its logs: a learner's own [DD_PPO_FUSED_LOGS][num_epochs]
// [steps] block at a.logs.  dd_ppo_train gives a layout of its own.
struct DenseLogs {
    __device__ __forceinline__ double* entry(const Args& a, int epoch, int i) const {
        return a.logs + (int64_t)epoch * a.steps + i;
    }
    __device__ __forceinline__ int64_t row(const Args& a) const { return (int64_t)a.num_epochs * a.steps; }
};

template <int K, typename Rows, typename Logs = DenseLogs>
__device__ __forceinline__ void learn(const Args& a, const Net& n, const Rows& src, float* lds, Logs at_logs = {}) {
    constexpr bool kActor = K == 3;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, c = lane & 31;
    float* rowbuf = reinterpret_cast<float*>(reinterpret_cast<char*>(lds) + kRowsAt);
    Part* red = reinterpret_cast<Part*>(reinterpret_cast<char*>(lds) + kRedAt);
    double* redd = reinterpret_cast<double*>(red);
    const DDMlpParams p = adamw::params_view(n.params, K, n.ln_eps);
    Running run = running_of(n);

    for (int epoch = 0; epoch < a.num_epochs; ++epoch) {
        for (int i = 0; i < a.steps; ++i) {
            const int rows = min(a.size, a.m - i * a.size);
            const auto at = src.template begin<kActor>(epoch, i, rows);
            const float* states = at.states();
            const double md = (double)rows;

            // ---- forward: the packed image into LDS, a wave per 32 rows --------------
            load_image(n.packed, lds);
            __syncthreads();
            if (wave * mlp::kCols < rows) {
                const int d = wave * mlp::kCols + c;
                const bool live = d < rows;
                float x[8], z[K];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int k = 2 * q + h;  // layer 1's B operand: the row's columns 2q + h, zero past column 14
                    x[q] = live && k < DD_OBS_DIM ? states[d * DD_OBS_DIM + k] : 0.0f;
                }
                mlp::mlp_body<K, false>(lds, lane, x, z);
                if (live && h == 0) {
                    if constexpr (kActor) {
                        float prob[3], lp, ent;
                        mlp::actor_probs(z, prob);
                        mlp::actor_evaluate(prob, at.bits(d), lp, ent);
                        rowbuf[d * kRowFloats + 0] = lp;
                        rowbuf[d * kRowFloats + 1] = ent;
#pragma unroll
                        for (int j = 0; j < 3; ++j) rowbuf[d * kRowFloats + 2 + j] = prob[j];
                    } else {
                        rowbuf[d * kRowFloats] = z[0];
                    }
                }
            }
            __syncthreads();

            // ---- losses: thread k has row k ------------------------------------------
            double* entry = at_logs.entry(a, epoch, i);
            const int64_t log_row = at_logs.row(a);
            if constexpr (kActor) {
                Part acc = ppo::no_rows();
                float rf = 0.0f;
                if (tid < rows) {
                    const float* out = rowbuf + tid * kRowFloats;
                    const ppo::Surrogate s = ppo::surrogate_of(out[0], at.old_log_prob(tid), at.advantage(tid), a.lo,
                                                               a.hi);
                    Part row = {s.smaller(), 0.0, (double)out[1], s.r, s.outside ? 1.0 : 0.0, s.rf, s.rf};
                    acc += row;
                    rf = s.rf;
                    const double g = s.grad(md);
                    const uint32_t bits = at.bits(tid);
#pragma unroll
                    for (int j = 0; j < 3; ++j)
                        n.head[tid * 3 + j] = ppo::grad_logit_of(g, (bits >> j) & 1u, out[2 + j], a.entropy_coef, md);
                }
                const Part t = stat_sum<Part>(acc, ppo::no_rows(), red);
                const double mean = t.r / md;
                double dev = 0.0;
                if (tid < rows) {
                    const double d = (double)rf - mean;
                    dev += d * d;
                }
                const double ss = stat_sum<double>(dev, 0.0, redd);
                if (tid == 0) {
                    entry[DD_PPO_POLICY_LOSS * log_row] = ppo::policy_loss_of(t, md);
                    entry[DD_PPO_ENTROPY * log_row] = ppo::entropy_of(t, md);
                    entry[DD_PPO_RATIO_MEAN * log_row] = mean;
                    entry[DD_PPO_RATIO_MIN * log_row] = (double)t.rmin;
                    entry[DD_PPO_RATIO_MAX * log_row] = (double)t.rmax;
                    entry[DD_PPO_RATIO_STD * log_row] = ppo::ratio_std_of(ss, rows);
                    entry[DD_PPO_CLIPPED_FRAC * log_row] = t.clipped / md;
                }
            } else {
                double sq = 0.0;
                if (tid < rows) {
                    const double dv = (double)rowbuf[tid * kRowFloats] - (double)at.ret(tid);
                    sq += dv * dv;
                    n.head[tid] = ppo::grad_value_of(a.value_coef, dv, md);
                }
                const double total = stat_sum<double>(sq, 0.0, redd);
                if (tid == 0) entry[DD_PPO_VALUE_LOSS * log_row] = ppo::value_loss_of(total, md);
            }

            // ---- backward, the norm before clipping, clip, AdamW, re-pack ---------------
            const double norm = backward_norm<K>(n, p, states, rows, lds);
            if (tid == 0) entry[(kActor ? DD_PPO_POLICY_GRAD_NORM : DD_PPO_CRITIC_GRAD_NORM) * log_row] = norm;
            clip_adamw<K>(n, a.clip, a.max_norm, norm, run);
            repack(n, p, lds);
        }
    }
}

// total_loss of one step from the two blocks' rows (count: a log row's entries).
__device__ __forceinline__ void total_of(double* logs, int64_t count, int64_t j, double entropy_coef,
                                         double value_coef) {
    logs[DD_PPO_TOTAL_LOSS * count + j] =
        ppo::total_loss_of(logs[DD_PPO_POLICY_LOSS * count + j], logs[DD_PPO_VALUE_LOSS * count + j],
                           logs[DD_PPO_ENTROPY * count + j], entropy_coef, value_coef);
}

// ---- host: what the entries refuse, the kernels' view of one learner, the member-table launch ----
inline bool net_ok(const DDPpoFusedNet& n) {
    if (!n.params || !n.grads || !n.exp_avg || !n.exp_avg_sq || !n.state || !n.packed) return false;
    if ((reinterpret_cast<uintptr_t>(n.state) & 7u) || (reinterpret_cast<uintptr_t>(n.packed) & 15u)) return false;
    return n.ln_eps > 0.0f && adamw::hyper_ok(n.hyper);
}

inline Net net_of(const DDPpoFusedNet& n, char* workspace) {
    float* image = reinterpret_cast<float*>(workspace);
    return {n.params, n.grads, n.exp_avg, n.exp_avg_sq, n.state, n.packed, image, image + kPackedB,
            adamw::args_of(n.hyper), n.ln_eps};
}

// Whether clip_grad_norm_ runs for a max_grad_norm (a NaN one is refused by the entries).
inline bool clip_of(double max_grad_norm) { return max_grad_norm > 0.0 && __builtin_isfinite(max_grad_norm); }

// A buffer of a network, for the entries' check that no two owners share one.
// The owner is the member where a member's own networks may overlap
// (dd_ppo_update_population), or a number of the buffer's own where nothing
// may (dd_actor_critic_train, dd_reinforce_train).
struct Owned {
    uintptr_t first, last;  // [first, last)
    int32_t owner;
};

// The six buffers of a K-output network, all `owner`'s.
inline void owned_of(const DDPpoFusedNet& n, int k, int32_t owner, std::vector<Owned>& out) {
    const uintptr_t floats = (uintptr_t)adamw::params_of(k) * sizeof(float);
    const float* flat[4] = {n.params, n.grads, n.exp_avg, n.exp_avg_sq};
    for (const float* p : flat) out.push_back({(uintptr_t)p, (uintptr_t)p + floats, owner});
    out.push_back({(uintptr_t)n.state, (uintptr_t)n.state + sizeof(DDAdamWState), owner});
    out.push_back({(uintptr_t)n.packed, (uintptr_t)n.packed + (uintptr_t)mlp::kPacked * sizeof(float), owner});
}

// The same with an owner per buffer, counted on from `next`: any overlap is one between owners.
inline void owned_apart(const DDPpoFusedNet& n, int k, int32_t& next, std::vector<Owned>& out) {
    const size_t from = out.size();
    owned_of(n, k, 0, out);
    for (size_t i = from; i < out.size(); ++i) out[i].owner = next++;
}

// Whether buffers of two different owners overlap.
inline bool shared_between_owners(std::vector<Owned>& v) {
    std::sort(v.begin(), v.end(), [](const Owned& x, const Owned& y) { return x.first < y.first; });
    // of the ranges seen so far: the furthest end, and the furthest end among the other owners' ranges
    uintptr_t end1 = 0, end2 = 0;
    int32_t owner1 = -1;
    for (const Owned& r : v) {
        if (r.owner != owner1 ? r.first < end1 : r.first < end2) return true;
        if (r.owner == owner1) {
            end1 = std::max(end1, r.last);
        } else if (r.last > end1) {
            end2 = end1;
            end1 = r.last;
            owner1 = r.owner;
        } else {
            end2 = std::max(end2, r.last);
        }
    }
    return false;
}

// The tail of a member-table launch: the table into the head of the workspace
// on the stream, then `blocks` workgroups of `kernel` with the fused LDS, each
// reading its own entry.  Returns after the launch; the caller ends with finish().
template <typename M, typename... P, typename... A>
hipError_t launch_with_table(void (*kernel)(const M*, P...), const std::vector<M>& table, void* workspace,
                             unsigned blocks, hipStream_t s, const A&... args) {
    // from pageable memory the copy has left `table` when the call returns
    hipError_t e = hipMemcpyAsync(workspace, table.data(), table.size() * sizeof(M), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    // the LDS exceeds the 64 KB default; the attribute is per device, so it is set on every launch
    e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), kLds, s, static_cast<const M*>(workspace), args...);
    return hipSuccess;
}

// One learner's batch and coefficients.
struct Learner {
    const DDPpoFusedNet& actor;
    const DDPpoFusedNet& critic;
    const float* states;
    const void* actions;
    const float* old_log_probs;
    const float* advantages;
    const float* returns;
    double* logs;
    int32_t action_format;
    int64_t m;
    double clip_epsilon, entropy_coef, value_coef, max_grad_norm;
};

// dd_ppo_update_fused's refusals that concern one learner (include/dronestep.h).
inline bool learner_ok(const Learner& l) {
    if (!net_ok(l.actor) || !net_ok(l.critic)) return false;
    if (!l.states || !l.actions || !l.old_log_probs || !l.advantages || !l.returns || !l.logs) return false;
    if (l.action_format != DD_ACT_BITMASK && l.action_format != DD_ACT_F32X3) return false;
    if (l.m < 1 || l.m >= (int64_t)1 << 31) return false;
    if (!(l.clip_epsilon >= 0.0) || !__builtin_isfinite(l.clip_epsilon)) return false;
    if (!__builtin_isfinite(l.entropy_coef) || !__builtin_isfinite(l.value_coef)) return false;
    return l.max_grad_norm == l.max_grad_norm;
}

// The kernels' arguments for a checked learner: size rows a minibatch, steps
// minibatches an epoch; the two networks' workspaces at ws_actor and ws_critic.
inline Args args_of(const Learner& l, int32_t num_epochs, int64_t size, int64_t steps, int64_t epoch_stride,
                    char* ws_actor, char* ws_critic) {
    Args a = {};
    a.net[0] = net_of(l.actor, ws_actor);
    a.net[1] = net_of(l.critic, ws_critic);
    a.states = l.states;
    a.actions = l.actions;
    a.old_log_probs = l.old_log_probs;
    a.advantages = l.advantages;
    a.returns = l.returns;
    a.epoch_stride = epoch_stride;
    a.action_format = l.action_format;
    a.num_epochs = num_epochs;
    a.m = (int32_t)l.m;
    a.size = (int32_t)size;
    a.steps = (int32_t)steps;
    a.lo = (float)(1.0 - l.clip_epsilon);
    a.hi = (float)(1.0 + l.clip_epsilon);
    a.entropy_coef = l.entropy_coef;
    a.value_coef = l.value_coef;
    a.max_norm = l.max_grad_norm;
    a.clip = clip_of(l.max_grad_norm);
    a.logs = l.logs;
    return a;
}

}  // namespace fused
}  // namespace dd
