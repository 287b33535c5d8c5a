// ppo_fused_population.hip — dd_ppo_update_population: the fused PPO update
// (ppo_fused.hip) for every learner of a population in one launch.
//
// The two workgroups of a fused update never talk to each other, and those of
// different learners have nothing to say to each other either: the grid is 2 P
// workgroups of 256 threads, block b the network b & 1 (0 actor, 1 critic) of
// member b >> 1, each running ppo_fused_core.h's learn<K> on its own member,
// with that member's batch, coefficients and step count.  No block waits on
// another, so nothing assumes co-residency: at one block per CU (the LDS), the
// blocks past the card's CUs start when a CU is free.  A second small kernel
// forms every member's total_loss.
//
// The members' descriptors do not fit kernel arguments: the host lays out one
// Member per learner (learn's Args and the shuffle key), uploads the table into
// the head of the workspace on the stream, and each block reads its own.  The
// kernels never write the table, so its loads may be scalar loads.
//
// Staged rows.  The single update reads num_epochs shuffled copies of the batch
// that the caller laid out; here the batch stays as it is.  At the top of
// minibatch i of epoch e the block gathers the minibatch's rows, source row
// perm(i size + k; m, seed, epoch + e) (shuffle_core.h) or i size + k without
// shuffle, into its stage in the workspace: states [128][15], the action as the
// three bits given_bits returns, old_log_probs, advantages, returns (a block
// fills the columns its network reads), moved as 32-bit words.  Forward, losses
// and backward_block then read the stage: the same rows the shuffled copy would
// hold at [first, first + rows), so the same bits.  The stage is memory the
// block writes and reads again: ppo_fused_core.h's rule holds for it (ordered by
// __syncthreads(), never behind a const __restrict__ pointer; every load of it
// has a per-lane address).
#include <algorithm>
#include <vector>

#include "ppo_fused_core.h"
#include "shuffle_core.h"

namespace dd {
namespace fused {

// One block's stage.
constexpr int kStageStates = 0;                                  // float    [128][15]
constexpr int kStageBits = kStageStates + kTileRows * DD_OBS_DIM;  // uint32_t [128]
constexpr int kStageOld = kStageBits + kTileRows;                // float    [128] each
constexpr int kStageAdv = kStageOld + kTileRows;
constexpr int kStageRet = kStageAdv + kTileRows;
constexpr int kStageWords = kStageRet + kTileRows;
constexpr int64_t kBlockWorkspace = kNetWorkspace + (int64_t)kStageWords * 4;
static_assert(kBlockWorkspace % 16 == 0, "every block's images are 16-byte aligned");

struct alignas(16) Member {
    Args a;  // states .. returns: the unshuffled batch; epoch_stride unused
    uint64_t seed, epoch;
    int32_t shuffle;
};
static_assert(sizeof(Member) % 16 == 0, "the blocks' workspaces follow the table");

inline int64_t table_bytes(int64_t members) { return members * (int64_t)sizeof(Member); }

struct StagedRows {
    const Args& a;
    const uint64_t seed, epoch;
    const bool shuffle;
    uint32_t* stage;  // workspace: kStageWords words
    uint32_t* from;   // LDS: the minibatch's source rows, kTileRows words

    struct At {
        uint32_t* stage;
        __device__ __forceinline__ const float* states() const {
            return reinterpret_cast<const float*>(stage + kStageStates);
        }
        __device__ __forceinline__ uint32_t bits(int d) const { return stage[kStageBits + d]; }
        __device__ __forceinline__ float old_log_prob(int d) const { return __uint_as_float(stage[kStageOld + d]); }
        __device__ __forceinline__ float advantage(int d) const { return __uint_as_float(stage[kStageAdv + d]); }
        __device__ __forceinline__ float ret(int d) const { return __uint_as_float(stage[kStageRet + d]); }
    };

    template <bool kActor>
    __device__ __forceinline__ At begin(int epoch_index, int i, int rows) const {
        const int tid = threadIdx.x;
        if (tid < rows) {  // rows <= kTileRows
            const uint32_t j = (uint32_t)(i * a.size + tid);  // < m
            const uint32_t s =
                shuffle ? shuffle::perm(j, shuffle::key_of(a.m, seed, epoch + (uint64_t)epoch_index)) : j;  // < m
            from[tid] = s;
            if constexpr (kActor) {
                stage[kStageBits + tid] = given_bits(a.actions, a.action_format, s);
                stage[kStageOld + tid] = reinterpret_cast<const uint32_t*>(a.old_log_probs)[s];
                stage[kStageAdv + tid] = reinterpret_cast<const uint32_t*>(a.advantages)[s];
            } else {
                stage[kStageRet + tid] = reinterpret_cast<const uint32_t*>(a.returns)[s];
            }
        }
        __syncthreads();
        const uint32_t* src = reinterpret_cast<const uint32_t*>(a.states);
        for (int idx = tid; idx < rows * DD_OBS_DIM; idx += kBlock) {
            const int r = idx / DD_OBS_DIM, c = idx - r * DD_OBS_DIM;
            stage[kStageStates + idx] = src[(uint64_t)from[r] * DD_OBS_DIM + (uint32_t)c];
        }
        __syncthreads();  // the stage is written; `from` is free again
        return {stage};
    }
};

__global__ __launch_bounds__(kBlock) void population_kernel(const Member* __restrict__ table, char* workspace) {
    extern __shared__ f32x4 lds4[];
    float* lds = reinterpret_cast<float*>(lds4);
    const Member mb = table[blockIdx.x >> 1];
    const int k = blockIdx.x & 1;
    uint32_t* stage = reinterpret_cast<uint32_t*>(workspace + (int64_t)blockIdx.x * kBlockWorkspace + kNetWorkspace);
    uint32_t* from = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(lds) + kRedAt);
    const StagedRows src = {mb.a, mb.seed, mb.epoch, mb.shuffle != 0, stage, from};
    if (k == 0) learn<3>(mb.a, mb.a.net[0], src, lds);
    else learn<1>(mb.a, mb.a.net[1], src, lds);
}
static_assert(kTileRows * sizeof(uint32_t) <= kBlock * sizeof(Part), "the source rows fit the reductions' scratch");

// total_loss of every member's every step: blockIdx.y the member.
__global__ __launch_bounds__(kBlock) void population_total_kernel(const Member* __restrict__ table) {
    const Args& a = table[blockIdx.y].a;
    const int64_t count = (int64_t)a.num_epochs * a.steps;
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j < count) total_of(a.logs, count, j, a.entropy_coef, a.value_coef);
}

}  // namespace fused
}  // namespace dd

extern "C" {

int64_t dd_ppo_update_population_workspace(int32_t members) {
    using namespace dd::fused;
    if (members < 1) return 0;
    return table_bytes(members) + 2 * (int64_t)members * kBlockWorkspace;
}

int dd_ppo_update_population(const DDPpoPopulationIO* io, void* workspace, void* stream) {
    using namespace dd::fused;
    if (!io || !workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u)) return hipErrorInvalidValue;
    if (!io->table || io->members < 1 || io->num_epochs < 1) return hipErrorInvalidValue;
    if (io->minibatch_size < 1 || io->minibatch_size > DD_PPO_FUSED_ROWS) return hipErrorInvalidValue;
    const int32_t members = io->members;
    char* blocks = static_cast<char*>(workspace) + table_bytes(members);
    std::vector<Member> table((size_t)members);
    std::vector<Owned> owned;
    owned.reserve((size_t)members * 12);
    int64_t most = 0;  // the longest log row
    for (int32_t p = 0; p < members; ++p) {
        const DDPpoPopulationMember& mb = io->table[p];
        const Learner l = {mb.actor, mb.critic, mb.states, mb.actions, mb.old_log_probs, mb.advantages, mb.returns,
                           mb.logs, mb.action_format, mb.m, mb.clip_epsilon, mb.entropy_coef, mb.value_coef,
                           mb.max_grad_norm};
        if (!learner_ok(l)) return hipErrorInvalidValue;
        if (io->drop_last && mb.m < io->minibatch_size) return hipErrorInvalidValue;  // no minibatch
        const int64_t size = std::min<int64_t>(io->minibatch_size, mb.m);  // as the single call is given it
        const int64_t steps = io->drop_last ? mb.m / size : (mb.m + size - 1) / size;
        table[p].a = args_of(l, io->num_epochs, size, steps, 0, blocks + (int64_t)(2 * p) * kBlockWorkspace,
                             blocks + (int64_t)(2 * p + 1) * kBlockWorkspace);
        table[p].seed = mb.shuffle_seed;
        table[p].epoch = mb.shuffle_epoch;
        table[p].shuffle = mb.shuffle ? 1 : 0;
        most = std::max(most, (int64_t)io->num_epochs * steps);
        owned_of(mb.actor, 3, p, owned);
        owned_of(mb.critic, 1, p, owned);
    }
    if (shared_between_owners(owned)) return hipErrorInvalidValue;  // a member's own networks may share

    hipStream_t s = static_cast<hipStream_t>(stream);
    const hipError_t e = launch_with_table(population_kernel, table, workspace, 2u * (unsigned)members, s, blocks);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(population_total_kernel, dim3((unsigned)dd::tiles_of(most), (unsigned)members),
                       dim3(dd::kBlock), 0, s, static_cast<const Member*>(workspace));
    return dd::finish();
}

}  // extern "C"
