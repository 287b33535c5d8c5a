// ppo_fused.hip — dd_ppo_update_fused: the PPO notebook's `for epoch: for
// minibatch:` loop (Actor_Critic_PPO.ipynb, PHASE 3) in one launch, for
// minibatches of at most one dd_mlp_backward row tile (128 rows) and
// DD_MLP_F32 networks.
//
// Why one launch is possible.  A minibatch of at most 128 rows is one row tile:
// its forward (four 32-row wave tiles), its loss sums, its backward tile, the
// gradient norm and the AdamW step all fit one workgroup, so nothing needs a
// grid-wide barrier.  And total_loss = policy_loss + value_coef value_loss -
// entropy_coef entropy separates: the actor's gradient depends on the actor
// alone, the critic's on the critic.  So the grid is two workgroups of 256
// threads, block 0 the actor and block 1 the critic, that never talk to each
// other; each walks the epochs' minibatches in order and keeps its parameters,
// moments, packed forward image and backward weight images up to date as it
// goes.  total_loss, the one number that needs both, is formed by a second,
// tiny kernel from the two blocks' log rows.
//
// The contract is bit equality with the multi-launch path (dd_mlp_evaluate_actions
// / dd_mlp_forward, dd_ppo_losses, dd_mlp_backward, dd_adamw_step with its
// dd_mlp_pack), so every phase runs that path's own device code from its header
// (mlp_core.h, ppo_core.h, mlp_backward_core.h, adamw_core.h, batch_core.h) in
// that path's order, for a grid of which one block has rows:
//   * forward: mlp_body on the wave's 32 rows, from the packed image copied
//     into LDS; a wave's arithmetic does not depend on the block around it.
//   * loss sums: dd_ppo_losses gives block 0 every row (thread k row k) and
//     sums its kStatBlocks partials, all but the first the sum of no row, in
//     stat_total's tree: block_sum, then block_sum again over (partial, nothing,
//     nothing, ...).
//   * backward: backward_block on tile 0.  dd_mlp_backward's finish adds block
//     0's partial and 255 zero partials in double and rounds once: the partial
//     itself, with a negative zero turned positive (0.0 + x).
//   * norm: dd_mlp_backward sums the squares over 109 blocks of 256 elements
//     (block_sum) and then the 109 partials (block_sum).  Here a wave stands for
//     one of the 109 blocks at a time (wave_block_sum: the same tree, no
//     barrier), then one real block_sum.
//   * AdamW: adamw_core.h's element; the step count and the running products
//     stay in registers from one minibatch to the next and are written to the
//     state block after every step.
//   * re-pack: pack_f32_at with the column means and LayerNorm scales, which
//     dd_mlp_pack computes again for every element, computed once per column
//     (the same additions in the same order) into an LDS table.
//
// Memory the block rewrites and reads again (parameters, moments, gradients,
// the two packed images, the head gradient): same-workgroup traffic through the
// CU's own vector L1, ordered by __syncthreads() (which drains the stores); no
// agent-scope fence.  None of it is read through a const __restrict__ pointer,
// so no load of it can become a scalar or read-only load (the scalar cache is
// not coherent with vector stores); the kernel's only scalar loads are of its
// arguments.
//
// LDS: the forward's packed image (109 KB) and the backward's transposition
// buffers (136 KB) take turns in one region; the per-row forward outputs and the
// reductions' scratch follow it.  154 KB, one block per CU.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

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

template <int K>
__device__ __forceinline__ void learn(const Args& a, const Net& n, float* lds) {
    constexpr bool kActor = K == 3;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, c = lane & 31;
    float* rowbuf = reinterpret_cast<float*>(reinterpret_cast<char*>(lds) + kRowsAt);
    Part* red = reinterpret_cast<Part*>(reinterpret_cast<char*>(lds) + kRedAt);
    double* redd = reinterpret_cast<double*>(red);
    double* normp = reinterpret_cast<double*>(reinterpret_cast<char*>(lds) + kNormAt);
    const DDMlpParams p = adamw::params_view(n.params, K, n.ln_eps);
    constexpr int kCount = adamw::params_of(K);
    int64_t step = n.state->step;
    double beta1_t = n.state->beta1_t, beta2_t = n.state->beta2_t;

    for (int epoch = 0; epoch < a.num_epochs; ++epoch) {
        for (int i = 0; i < a.steps; ++i) {
            const int rows = min(a.size, a.m - i * a.size);
            const int64_t first = (int64_t)epoch * a.epoch_stride + (int64_t)i * a.size;
            const float* states = a.states + first * DD_OBS_DIM;
            const double md = (double)rows;

            // ---- forward: the packed image into LDS, a wave per 32 rows --------------
            {
                f32x4* lds4 = reinterpret_cast<f32x4*>(lds);
                const f32x4* src4 = reinterpret_cast<const f32x4*>(n.packed);
                for (int j = tid; j < mlp::kPacked / 4; j += kBlock) lds4[j] = src4[j];
            }
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
                        mlp::actor_evaluate(prob, given_bits(a.actions, a.action_format, first + d), lp, ent);
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
            double* entry = a.logs + (int64_t)epoch * a.steps + i;
            const int64_t log_row = (int64_t)a.num_epochs * a.steps;
            if constexpr (kActor) {
                Part acc = ppo::no_rows();
                float rf = 0.0f;
                if (tid < rows) {
                    const float* out = rowbuf + tid * kRowFloats;
                    const ppo::Surrogate s = ppo::surrogate_of(out[0], a.old_log_probs[first + tid],
                                                               a.advantages[first + tid], a.lo, a.hi);
                    Part row = {s.smaller(), 0.0, (double)out[1], s.r, s.outside ? 1.0 : 0.0, s.rf, s.rf};
                    acc += row;
                    rf = s.rf;
                    const double g = s.grad(md);
                    const uint32_t bits = given_bits(a.actions, a.action_format, first + tid);
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
                    const double dv = (double)rowbuf[tid * kRowFloats] - (double)a.returns[first + tid];
                    sq += dv * dv;
                    n.head[tid] = ppo::grad_value_of(a.value_coef, dv, md);
                }
                const double total = stat_sum<double>(sq, 0.0, redd);
                if (tid == 0) entry[DD_PPO_VALUE_LOSS * log_row] = ppo::value_loss_of(total, md);
            }

            // ---- backward: the weight images, then the one tile ------------------------
            for (int idx = tid; idx < kPackedB; idx += kBlock) n.image[idx] = mlpbwd::packed_value(p, idx);
            __syncthreads();  // the images and the head gradient are written
            mlpbwd::backward_block<K>(p, states, n.head, rows, n.image, n.grads, 0, 1, lds);
            __syncthreads();  // the gradient is written; LDS is free again

            // ---- the norm before clipping ----------------------------------------------
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
            const double norm = sqrt(block_sum<double>(tid < kFinishBlocks ? normp[tid] : 0.0, redd));
            if (tid == 0) entry[(kActor ? DD_PPO_POLICY_GRAD_NORM : DD_PPO_CRITIC_GRAD_NORM) * log_row] = norm;
            const double coef = a.clip ? mlpbwd::clip_coef(a.max_norm, norm) : 1.0;
            const bool scale = !(coef == 1.0);  // a NaN factor scales, as clip_grad_norm_'s does

            // ---- AdamW: each thread reads and writes its own elements ---------------------
            const adamw::Step now = adamw::step_of(n.opt, beta1_t, beta2_t);
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
            step += 1;
            beta1_t = now.b1t;
            beta2_t = now.b2t;
            if (tid == 0) {
                n.state->step = step;
                n.state->beta1_t = beta1_t;
                n.state->beta2_t = beta2_t;
            }
            __syncthreads();  // the new parameters are written

            // ---- re-pack the forward image ---------------------------------------------------
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
    }
}

__global__ __launch_bounds__(kBlock) void update_kernel(Args a) {
    extern __shared__ f32x4 lds4[];
    float* lds = reinterpret_cast<float*>(lds4);
    if (blockIdx.x == 0) learn<3>(a, a.net[0], lds);
    else learn<1>(a, a.net[1], lds);
}

// total_loss of every step from the two blocks' rows.
__global__ __launch_bounds__(kBlock) void total_kernel(double* __restrict__ logs, int64_t count, double entropy_coef,
                                                       double value_coef) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j < count)
        logs[DD_PPO_TOTAL_LOSS * count + j] =
            ppo::total_loss_of(logs[DD_PPO_POLICY_LOSS * count + j], logs[DD_PPO_VALUE_LOSS * count + j],
                               logs[DD_PPO_ENTROPY * count + j], entropy_coef, value_coef);
}

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

}  // namespace fused
}  // namespace dd

extern "C" {

int64_t dd_ppo_update_fused_workspace(void) { return 2 * dd::fused::kNetWorkspace; }

int dd_ppo_update_fused(const DDPpoFusedIO* io, void* workspace, void* stream) {
    using namespace dd::fused;
    if (!io || !workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u)) return hipErrorInvalidValue;
    if (!net_ok(io->actor) || !net_ok(io->critic)) return hipErrorInvalidValue;
    if (!io->states || !io->actions || !io->old_log_probs || !io->advantages || !io->returns || !io->logs)
        return hipErrorInvalidValue;
    if (io->action_format != DD_ACT_BITMASK && io->action_format != DD_ACT_F32X3) return hipErrorInvalidValue;
    if (io->m < 1 || io->m >= (int64_t)1 << 31 || io->num_epochs < 1) return hipErrorInvalidValue;
    if (io->minibatch_size < 1 || io->minibatch_size > DD_PPO_FUSED_ROWS) return hipErrorInvalidValue;
    if (io->epoch_stride < 0 || (io->epoch_stride > 0 && io->epoch_stride < io->m)) return hipErrorInvalidValue;
    if (!(io->clip_epsilon >= 0.0) || !__builtin_isfinite(io->clip_epsilon)) return hipErrorInvalidValue;
    if (!__builtin_isfinite(io->entropy_coef) || !__builtin_isfinite(io->value_coef)) return hipErrorInvalidValue;
    if (io->max_grad_norm != io->max_grad_norm) return hipErrorInvalidValue;
    const int64_t size = io->minibatch_size;
    const int64_t steps = io->drop_last ? io->m / size : (io->m + size - 1) / size;
    if (steps < 1) return hipErrorInvalidValue;

    Args a = {};
    a.net[0] = net_of(io->actor, static_cast<char*>(workspace));
    a.net[1] = net_of(io->critic, static_cast<char*>(workspace) + kNetWorkspace);
    a.states = io->states;
    a.actions = io->actions;
    a.old_log_probs = io->old_log_probs;
    a.advantages = io->advantages;
    a.returns = io->returns;
    a.epoch_stride = io->epoch_stride;
    a.action_format = io->action_format;
    a.num_epochs = io->num_epochs;
    a.m = (int32_t)io->m;
    a.size = (int32_t)size;
    a.steps = (int32_t)steps;
    a.lo = (float)(1.0 - io->clip_epsilon);
    a.hi = (float)(1.0 + io->clip_epsilon);
    a.entropy_coef = io->entropy_coef;
    a.value_coef = io->value_coef;
    a.max_norm = io->max_grad_norm;
    a.clip = io->max_grad_norm > 0.0 && __builtin_isfinite(io->max_grad_norm);
    a.logs = io->logs;

    hipStream_t s = static_cast<hipStream_t>(stream);
    // the LDS exceeds the 64 KB default; the attribute is per device, so it is set on every launch
    const hipError_t e = hipFuncSetAttribute((const void*)update_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)kLds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(update_kernel, dim3(2), dim3(dd::kBlock), kLds, s, a);
    const int64_t count = (int64_t)io->num_epochs * steps;
    hipLaunchKernelGGL(total_kernel, dim3((unsigned)dd::tiles_of(count)), dim3(dd::kBlock), 0, s, io->logs, count,
                       io->entropy_coef, io->value_coef);
    return dd::finish();
}

}  // extern "C"
