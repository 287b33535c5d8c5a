// ppo_loss.hip — compute_ppo_losses (Actor_Critic_PPO.ipynb, the cell after
// collect_episodes_ppo, :927-988) from per-row network outputs: the clipped
// surrogate, the value loss, the entropy bonus, the ratio statistics the
// training cell logs every epoch, and the gradient of total_loss at the two
// networks' outputs.  The networks themselves are dd_mlp_evaluate_actions
// (log_prob, entropy, probs of the given actions) and dd_mlp_forward on the
// critic (values); this unit is the elementwise stage after them.
//
// A stage of its own, not an epilogue of the MFMA kernel: the forward launches
// one block per CU, so partial sums taken there would be grouped by the
// device's CU count; kStatBlocks blocks of kBlock rows (batch_core.h) place
// every row in the tree by m alone, the same bits on every device, at tens of
// bytes per row next to a compute-bound forward.
//
// The notebook, line by line (torch float32; here every product and sum is in
// double on the float32 inputs, where a product of two floats is exact):
//   ratio = torch.exp(new_log_probs - old_log_probs)              (:957)
//       the difference in float32; exp in double rounded to float32 once, a
//       correctly rounded expf but for double rounding (within torch's own
//       expf error, and the same bits on every device and in NumPy)
//   surr1 = ratio * advantages                                    (:960)
//   surr2 = torch.clamp(ratio, 1 - eps, 1 + eps) * advantages     (:961)
//       the bounds as float32, as torch compares a float32 tensor with a
//       Python number
//   policy_loss = -torch.min(surr1, surr2).mean()                 (:962)
//   value_loss = ((values - returns) ** 2).mean()                 (:966)
//   entropy = dist.entropy().mean()     over the [m, 3] factors   (:954)
//   total_loss = policy_loss + value_coef * value_loss - entropy_coef * entropy   (:969)
//   ratio_stats: mean, min, max, std (unbiased), clipped_frac     (:973-979)
//
// The gradient of total_loss that autograd leaves at the critic's output v and
// at the actor's pre-Sigmoid outputs z (p = Sigmoid(z), dp/dz = p (1 - p)):
//   d total / d v_i = value_coef 2 (v_i - R_i) / m.
//   d total / d new_log_prob_i = g_i = -(d min(surr1, surr2)_i / d r_i) r_i / m
//       (d r / d lp = r).  torch.min passes the gradient to the smaller
//       operand and splits it between equal ones; clamp passes it inside its
//       range, bounds included.  So d min / d r is A_i when surr1 < surr2 (the
//       unclipped branch), A_i again when r_i lies in [1 - eps, 1 + eps] (then
//       surr1 == surr2 and the two halves add up to A_i), and 0 otherwise (the
//       clipped branch is the smaller, or a tie outside the range, which needs
//       A_i == 0):  g_i = -A_i r_i / m  if r_i A_i < clip(r_i) A_i or 1 - eps <=
//       r_i <= 1 + eps, else 0.
//   d new_log_prob_i / d z_ik = a_ik - p_ik: log_prob is -BCE-with-logits of l
//       = logit(pc) against a, d / d l = a - Sigmoid(l) = a - pc, d l / d pc =
//       1 / (pc (1 - pc)), and pc = clamp_probs(p) passes the gradient only for
//       p in [FLT_EPSILON, 1 - FLT_EPSILON], where pc = p.
//   d (-entropy_coef entropy) / d z_ik = entropy_coef / (3 m) logit(p_ik) p_ik
//       (1 - p_ik): Bernoulli.entropy is BCE-with-logits of l against p; through
//       l the derivative is Sigmoid(l) - p = 0, through the target p it is -l.
//   A factor whose p lies outside [FLT_EPSILON, 1 - FLT_EPSILON] contributes
//   0.  (The notebook's own clamp(1e-8, 1 - 1e-8) is the identity on that
//   range.)
//   grad_logits[i][k] = g_i (a_ik - p_ik) + entropy_coef / (3 m) logit(p_ik) p_ik (1 - p_ik).
//
// Three launches: per-row work and kStatBlocks partial sums; the mean ratio
// (every block adds the partials in the same tree) and the partial sums of
// squared deviations from it; one block that writes result[].  No atomics.

#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "action_bits.h"
#include "batch_core.h"
#include "dronestep.h"
#include "launch.h"
#include "ppo_core.h"

namespace dd {
namespace ppo {

__global__ __launch_bounds__(kBlock) void ppo_rows_kernel(DDPpoLossIO io, int64_t m, float lo, float hi,
                                                          Part* __restrict__ part) {
    __shared__ Part sh[kBlock];
    Part acc = no_rows();
    const double md = (double)m;
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < m; k += (int64_t)kStatBlocks * kBlock) {
        const Surrogate s = surrogate_of(io.log_prob[k], io.old_log_prob[k], io.advantages[k], lo, hi);
        const double dv = (double)io.values[k] - (double)io.returns[k];
        Part row = {s.smaller(), dv * dv, (double)io.entropy[k], s.r, s.outside ? 1.0 : 0.0, s.rf, s.rf};
        acc += row;
        if (io.ratio) io.ratio[k] = s.rf;
        if (io.grad_values) io.grad_values[k] = grad_value_of(io.value_coef, dv, md);
        if (io.grad_logits) {
            const double g = s.grad(md);
            const uint32_t bits = given_bits(io.actions, io.action_format, k);
#pragma unroll
            for (int j = 0; j < 3; ++j)
                io.grad_logits[k * 3 + j] = grad_logit_of(g, (bits >> j) & 1u, io.probs[k * 3 + j], io.entropy_coef, md);
        }
    }
    acc = block_sum<Part>(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

__global__ __launch_bounds__(kBlock) void ppo_dev_kernel(const float* __restrict__ log_prob,
                                                         const float* __restrict__ old_log_prob, int64_t m,
                                                         const Part* __restrict__ part,
                                                         double* __restrict__ part_ss) {
    __shared__ Part sh[kBlock];
    __shared__ double shd[kBlock];
    const double mean = stat_total(part, sh).r / (double)m;
    double s = 0.0;
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < m; k += (int64_t)kStatBlocks * kBlock) {
        const double d = (double)ratio_of(log_prob[k], old_log_prob[k]) - mean;
        s += d * d;
    }
    s = block_sum<double>(s, shd);
    if (threadIdx.x == 0) part_ss[blockIdx.x] = s;
}

__global__ __launch_bounds__(kBlock) void ppo_finish_kernel(const Part* __restrict__ part,
                                                            const double* __restrict__ part_ss, int64_t m,
                                                            double entropy_coef, double value_coef,
                                                            double* __restrict__ result) {
    __shared__ Part sh[kBlock];
    __shared__ double shd[kBlock];
    const Part t = stat_total(part, sh);
    const double ss = stat_total(part_ss, shd);
    if (threadIdx.x != 0) return;
    const double md = (double)m;
    const double policy = policy_loss_of(t, md), value = value_loss_of(t.sq, md), entropy = entropy_of(t, md);
    result[DD_PPO_TOTAL_LOSS] = total_loss_of(policy, value, entropy, entropy_coef, value_coef);
    result[DD_PPO_POLICY_LOSS] = policy;
    result[DD_PPO_VALUE_LOSS] = value;
    result[DD_PPO_ENTROPY] = entropy;
    result[DD_PPO_RATIO_MEAN] = t.r / md;
    result[DD_PPO_RATIO_MIN] = (double)t.rmin;
    result[DD_PPO_RATIO_MAX] = (double)t.rmax;
    result[DD_PPO_RATIO_STD] = ratio_std_of(ss, m);
    result[DD_PPO_CLIPPED_FRAC] = t.clipped / md;
}

}  // namespace ppo
}  // namespace dd

extern "C" {

int64_t dd_ppo_loss_workspace(void) { return dd::kStatBlocks * (int64_t)(sizeof(dd::ppo::Part) + sizeof(double)); }

int dd_ppo_losses(const DDPpoLossIO* io, int64_t m, void* workspace, void* stream) {
    if (!io || m <= 0 || !workspace || (reinterpret_cast<uintptr_t>(workspace) & 7u)) return hipErrorInvalidValue;
    if (!io->log_prob || !io->entropy || !io->values || !io->old_log_prob || !io->advantages || !io->returns ||
        !io->result)
        return hipErrorInvalidValue;
    if (!(io->clip_epsilon >= 0.0) || !__builtin_isfinite(io->clip_epsilon)) return hipErrorInvalidValue;
    if (io->action_format != DD_ACT_BITMASK && io->action_format != DD_ACT_F32X3) return hipErrorInvalidValue;
    if (io->grad_logits && (!io->probs || !io->actions)) return hipErrorInvalidValue;
    hipStream_t s = static_cast<hipStream_t>(stream);
    dd::ppo::Part* part = static_cast<dd::ppo::Part*>(workspace);
    double* part_ss = reinterpret_cast<double*>(part + dd::kStatBlocks);
    const float lo = (float)(1.0 - io->clip_epsilon), hi = (float)(1.0 + io->clip_epsilon);
    hipLaunchKernelGGL(dd::ppo::ppo_rows_kernel, dim3(dd::kStatBlocks), dim3(dd::kBlock), 0, s, *io, m, lo, hi, part);
    hipLaunchKernelGGL(dd::ppo::ppo_dev_kernel, dim3(dd::kStatBlocks), dim3(dd::kBlock), 0, s, io->log_prob,
                       io->old_log_prob, m, (const dd::ppo::Part*)part, part_ss);
    hipLaunchKernelGGL(dd::ppo::ppo_finish_kernel, dim3(1), dim3(dd::kBlock), 0, s, (const dd::ppo::Part*)part,
                       (const double*)part_ss, m, io->entropy_coef, io->value_coef, io->result);
    return dd::finish();
}

}  // extern "C"
