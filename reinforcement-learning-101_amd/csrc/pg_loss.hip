// pg_loss.hip — the elementwise loss stages of the two notebooks that learn
// from a score-function loss: Policy_Gradients.ipynb (REINFORCE) and
// Actor_Critic_Basic.ipynb (one-step TD actor-critic), from per-row network
// outputs, with the gradient of each loss at its network's output.  The
// networks themselves are dd_mlp_evaluate_actions (log_prob, probs of the given
// actions) and dd_mlp_forward on the critic (values, next_values); the backward
// is dd_mlp_backward.  As ppo_loss.hip: kStatBlocks blocks of kBlock rows
// (batch_core.h) place every row in the reduction tree by m alone, the same
// bits on every run and every device; no atomics.
//
// The notebooks, line by line (torch float32; here every product and sum is in
// double on the float32 inputs, each output rounded to float32 once):
//   loss = -(log_probs_tensor * advantages).mean()          Policy_Gradients, the training cell
//   actor_loss = -(batch_data['log_probs'] * td_errors.detach()).mean()      Actor_Critic_Basic
//       one stage for both, dd_pg_losses: loss = -sum(lp_i w_i) / cnt, w the
//       normalised advantage or the detached TD error.
//   td_targets = (batch_data['rewards'] + bellman_gamma * next_values * (1 - batch_data['dones']))
//       gamma rounded to float32, as torch multiplies a float32 tensor by a
//       Python number: (gamma v') (1 - d), then r + that.
//   td_errors = td_targets - values
//       from the unrounded target; td_errors[] is its one rounding, and that
//       float32 is what the actor stage takes as w (the notebook's detached tensor).
//   critic_loss = (td_errors ** 2).mean()
//   value_reg = 0.01 * (values ** 2).mean()
//   critic_loss = critic_loss + value_reg
//
// The gradients autograd leaves at the actor's pre-Sigmoid outputs z and at the
// critic's value v (next_values is under no_grad):
//   d loss / d lp_i = -w_i / cnt, and d lp_i / d z_ik = a_ik - p_ik for p_ik in
//       [FLT_EPSILON, 1 - FLT_EPSILON], else 0 (clamp_probs passes no gradient
//       there; a NaN p stays NaN): ppo_loss.hip's derivation.
//   grad_logits[i][k] = -(w_i / cnt) (a_ik - p_ik)
//   grad_values[i] = (-2 delta_i + 2 value_reg v_i) / cnt
//
// The mask.  active[i] == 0 takes row i out of every mean: its inputs are not
// read, its gradient rows are exactly 0 (so it adds nothing to a dW of
// dd_mlp_backward), its td_targets and td_errors are 0.  cnt, the number of
// active rows, is counted on the device with the sums.  cnt == 0: the scalars
// are NaN (torch's mean over nothing) and every gradient row is 0.
//
// The row arithmetic (the parts, a row's contribution, the scalars from the
// totals, a row's gradient) is pg_core.h's, shared with the actor-critic frame
// loop (ac_fused.hip), which must leave these kernels' bits.
//
// Two launches each: the per-row work and kStatBlocks partial sums; then every
// block adds the partials in the same tree (as ppo_dev_kernel re-totals the
// mean) for cnt, block 0 writes result[], and all write the gradient rows.

#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "action_bits.h"
#include "batch_core.h"
#include "dronestep.h"
#include "launch.h"
#include "pg_core.h"

namespace dd {
namespace pg {

__device__ __forceinline__ bool is_active(const uint8_t* __restrict__ active, int64_t k) {
    return !active || active[k] != 0;
}

// The unrounded TD target and error of row k.
__device__ __forceinline__ void td_row(const DDTdLossIO& io, double gamma, int64_t k, double* target, double* delta) {
    td_row_of(io.values[k], io.next_values[k], io.rewards[k], io.dones[k], gamma, target, delta);
}

__global__ __launch_bounds__(kBlock) void pg_rows_kernel(DDPgLossIO io, int64_t m, PgPart* __restrict__ part) {
    __shared__ PgPart sh[kBlock];
    PgPart acc = {0.0, 0.0};
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < m; k += (int64_t)kStatBlocks * kBlock) {
        if (!is_active(io.active, k)) continue;
        acc += pg_row(io.log_prob[k], io.weights[k]);
    }
    acc = block_sum<PgPart>(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// One block without grad_logits, kStatBlocks with it.
__global__ __launch_bounds__(kBlock) void pg_finish_kernel(DDPgLossIO io, int64_t m, const PgPart* __restrict__ part) {
    __shared__ PgPart sh[kBlock];
    const PgPart t = stat_total(part, sh);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        io.result[DD_PG_LOSS] = pg_loss_of(t);
        io.result[DD_PG_COUNT] = t.cnt;
    }
    if (!io.grad_logits) return;
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < m; k += (int64_t)kStatBlocks * kBlock) {
        float out[3] = {0.0f, 0.0f, 0.0f};
        if (is_active(io.active, k)) {
            const double g = pg_grad_of(io.weights[k], t.cnt);
            const uint32_t bits = given_bits(io.actions, io.action_format, k);
#pragma unroll
            for (int j = 0; j < 3; ++j) out[j] = pg_grad_logit_of(g, (bits >> j) & 1u, io.probs[k * 3 + j]);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) io.grad_logits[k * 3 + j] = out[j];
    }
}

__global__ __launch_bounds__(kBlock) void td_rows_kernel(DDTdLossIO io, int64_t m, double gamma,
                                                         TdPart* __restrict__ part) {
    __shared__ TdPart sh[kBlock];
    TdPart acc = {0.0, 0.0, 0.0};
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < m; k += (int64_t)kStatBlocks * kBlock) {
        double target = 0.0, delta = 0.0;
        if (is_active(io.active, k)) {
            td_row(io, gamma, k, &target, &delta);
            acc += td_part_of(delta, io.values[k]);
        }
        io.td_targets[k] = (float)target;
        io.td_errors[k] = (float)delta;
    }
    acc = block_sum<TdPart>(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// One block without grad_values, kStatBlocks with it.
__global__ __launch_bounds__(kBlock) void td_finish_kernel(DDTdLossIO io, int64_t m, double gamma,
                                                           const TdPart* __restrict__ part) {
    __shared__ TdPart sh[kBlock];
    const TdPart t = stat_total(part, sh);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const double mse = td_mse_of(t), reg = td_reg_of(t, io.value_reg);
        io.result[DD_TD_CRITIC_LOSS] = mse + reg;
        io.result[DD_TD_MSE] = mse;
        io.result[DD_TD_VALUE_REG] = reg;
        io.result[DD_TD_COUNT] = t.cnt;
    }
    if (!io.grad_values) return;
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < m; k += (int64_t)kStatBlocks * kBlock) {
        float gv = 0.0f;
        if (is_active(io.active, k)) {
            double target, delta;
            td_row(io, gamma, k, &target, &delta);
            gv = td_grad_value_of(delta, io.values[k], io.value_reg, t.cnt);
        }
        io.grad_values[k] = gv;
    }
}

inline bool workspace_ok(const void* workspace) {
    return workspace && !(reinterpret_cast<uintptr_t>(workspace) & 7u);
}

}  // namespace pg
}  // namespace dd

extern "C" {

int64_t dd_pg_loss_workspace(void) { return dd::kStatBlocks * (int64_t)sizeof(dd::pg::PgPart); }

int dd_pg_losses(const DDPgLossIO* io, int64_t m, void* workspace, void* stream) {
    if (!io || m <= 0 || !dd::pg::workspace_ok(workspace)) return hipErrorInvalidValue;
    if (!io->log_prob || !io->weights || !io->result) return hipErrorInvalidValue;
    if (io->action_format != DD_ACT_BITMASK && io->action_format != DD_ACT_F32X3) return hipErrorInvalidValue;
    if (io->grad_logits && (!io->probs || !io->actions)) return hipErrorInvalidValue;
    hipStream_t s = static_cast<hipStream_t>(stream);
    dd::pg::PgPart* part = static_cast<dd::pg::PgPart*>(workspace);
    hipLaunchKernelGGL(dd::pg::pg_rows_kernel, dim3(dd::kStatBlocks), dim3(dd::kBlock), 0, s, *io, m, part);
    hipLaunchKernelGGL(dd::pg::pg_finish_kernel, dim3(io->grad_logits ? dd::kStatBlocks : 1), dim3(dd::kBlock), 0, s,
                       *io, m, (const dd::pg::PgPart*)part);
    return dd::finish();
}

int64_t dd_td_loss_workspace(void) { return dd::kStatBlocks * (int64_t)sizeof(dd::pg::TdPart); }

int dd_td_losses(const DDTdLossIO* io, int64_t m, void* workspace, void* stream) {
    if (!io || m <= 0 || !dd::pg::workspace_ok(workspace)) return hipErrorInvalidValue;
    if (!io->values || !io->next_values || !io->rewards || !io->dones || !io->td_targets || !io->td_errors ||
        !io->result)
        return hipErrorInvalidValue;
    if (!__builtin_isfinite(io->gamma) || !__builtin_isfinite(io->value_reg)) return hipErrorInvalidValue;
    hipStream_t s = static_cast<hipStream_t>(stream);
    dd::pg::TdPart* part = static_cast<dd::pg::TdPart*>(workspace);
    const double gamma = (double)(float)io->gamma;
    hipLaunchKernelGGL(dd::pg::td_rows_kernel, dim3(dd::kStatBlocks), dim3(dd::kBlock), 0, s, *io, m, gamma, part);
    hipLaunchKernelGGL(dd::pg::td_finish_kernel, dim3(io->grad_values ? dd::kStatBlocks : 1), dim3(dd::kBlock), 0, s,
                       *io, m, gamma, (const dd::pg::TdPart*)part);
    return dd::finish();
}

}  // extern "C"
