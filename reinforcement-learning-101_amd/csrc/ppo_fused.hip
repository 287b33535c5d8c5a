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
// The walk itself, its memory-ordering rule and its LDS plan are in
// ppo_fused_core.h (learn<K, Rows>), shared with the population update
// (ppo_fused_population.hip); this unit instantiates it on DirectRows, the rows
// as the caller laid them out.  The kernel's only scalar loads are of its
// arguments.
#include "ppo_fused_core.h"

namespace dd {
namespace fused {

__global__ __launch_bounds__(kBlock) void update_kernel(Args a) {
    extern __shared__ f32x4 lds4[];
    float* lds = reinterpret_cast<float*>(lds4);
    if (blockIdx.x == 0) learn<3>(a, a.net[0], DirectRows{a}, lds);
    else learn<1>(a, a.net[1], DirectRows{a}, lds);
}

// total_loss of every step from the two blocks' rows.
__global__ __launch_bounds__(kBlock) void total_kernel(double* __restrict__ logs, int64_t count, double entropy_coef,
                                                       double value_coef) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j < count) total_of(logs, count, j, entropy_coef, value_coef);
}

}  // namespace fused
}  // namespace dd

extern "C" {

int64_t dd_ppo_update_fused_workspace(void) { return 2 * dd::fused::kNetWorkspace; }

int dd_ppo_update_fused(const DDPpoFusedIO* io, void* workspace, void* stream) {
    using namespace dd::fused;
    if (!io || !workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u)) return hipErrorInvalidValue;
    const Learner l = {io->actor, io->critic, io->states, io->actions, io->old_log_probs, io->advantages, io->returns,
                       io->logs, io->action_format, io->m, io->clip_epsilon, io->entropy_coef, io->value_coef,
                       io->max_grad_norm};
    if (!learner_ok(l) || io->num_epochs < 1) return hipErrorInvalidValue;
    if (io->minibatch_size < 1 || io->minibatch_size > DD_PPO_FUSED_ROWS) return hipErrorInvalidValue;
    if (io->epoch_stride < 0 || (io->epoch_stride > 0 && io->epoch_stride < io->m)) return hipErrorInvalidValue;
    const int64_t size = io->minibatch_size;
    const int64_t steps = io->drop_last ? io->m / size : (io->m + size - 1) / size;
    if (steps < 1) return hipErrorInvalidValue;

    const Args a = args_of(l, io->num_epochs, size, steps, io->epoch_stride, static_cast<char*>(workspace),
                           static_cast<char*>(workspace) + kNetWorkspace);
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
