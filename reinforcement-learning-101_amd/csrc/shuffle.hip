// shuffle.hip — dd_shuffle_indices / dd_shuffle_rows: the keyed permutation of
// a training batch's rows behind ppo_update's shuffled minibatch epochs
// ("Shuffle collected data into minibatches", Actor_Critic_PPO.ipynb).
//
// perm(j) is stateless (include/dronestep.h has the definition; shuffle_core.h
// the device code and the key's set-up).  Each thread computes perm for its own
// row once and keeps it for every column: no sort, no atomics, no workspace,
// and the result does not depend on the launch geometry.
//
// A block of kBlock threads owns kBlock consecutive destination rows.
//   [m] columns   a gathered load per thread and a coalesced store.
//   actions [m][3] three gathered loads per thread into an LDS tile that
//                 leaves as coalesced 4-byte stores.
//   states [m][15] the 60-byte source rows (4-byte aligned only, anywhere in
//                 the batch) are gathered into an LDS tile, fifteen lanes per
//                 row, the tile laid out in the destination's 16-byte phase;
//                 it leaves as 16-byte stores on the destination's own
//                 16-byte grid, with 4-byte stores at the two ragged ends
//                 (batch_core.h's gather tile, in one dimension).
// Rows are moved as 32-bit words, never as floats: NaN payloads keep their bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "batch_core.h"
#include "dronestep.h"
#include "launch.h"
#include "shuffle_core.h"

namespace dd {
namespace shuffle {

constexpr int kRowWords = kBlock * DD_OBS_DIM;  // one block's states
constexpr int kPerThread = DD_OBS_DIM;          // words of the tile each thread gathers
constexpr int kActWords = kBlock * 3;

__global__ __launch_bounds__(kBlock) void indices_kernel(int32_t* __restrict__ out, Key key) {
    const uint32_t j = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (j < key.m) out[j] = (int32_t)perm(j, key);
}

// The block's states: rows' source rows into the tile (kFull: all kBlock rows
// exist, so every trip count is a constant and the fifteen loads of a thread
// are in flight together).
template <bool kFull>
__device__ __forceinline__ void states_in(const uint32_t* __restrict__ src, const uint32_t* perm_s, uint32_t* tile,
                                          int cnt) {
    const int tid = (int)threadIdx.x;
    uint32_t v[kPerThread];
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
        const int idx = tid + i * kBlock;
        v[i] = 0;
        if (kFull || idx < cnt) {
            const int r = idx / DD_OBS_DIM, c = idx - r * DD_OBS_DIM;
            v[i] = src[(uint64_t)perm_s[r] * DD_OBS_DIM + (uint32_t)c];
        }
    }
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
        const int idx = tid + i * kBlock;
        if (kFull || idx < cnt) tile[idx] = v[i];
    }
}

// kAct: the bytes of one row's action (0: no actions column)
template <int kAct>
__global__ __launch_bounds__(kBlock) void rows_kernel(DDShuffleIO io, Key key) {
    __shared__ __attribute__((aligned(16))) uint32_t tile_s[kRowWords + 4];  // + room for the destination's 16-byte phase
    __shared__ uint32_t perm_s[kBlock];
    __shared__ uint32_t act_s[kAct == 12 ? kActWords : 1];
    const int tid = (int)threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * kBlock;  // the block's first destination row
    const int64_t left = (int64_t)key.m - r0;
    const int rows = left < kBlock ? (int)left : kBlock;
    const int64_t row = r0 + tid;

    uint32_t p = 0;
    if (tid < rows) {
        p = perm((uint32_t)row, key);
        if (io.indices) io.indices[row] = (int32_t)p;
        if (io.old_log_probs)
            reinterpret_cast<uint32_t*>(io.old_log_probs_out)[row] = reinterpret_cast<const uint32_t*>(io.old_log_probs)[p];
        if (io.advantages)
            reinterpret_cast<uint32_t*>(io.advantages_out)[row] = reinterpret_cast<const uint32_t*>(io.advantages)[p];
        if (io.returns)
            reinterpret_cast<uint32_t*>(io.returns_out)[row] = reinterpret_cast<const uint32_t*>(io.returns)[p];
        if constexpr (kAct == 1) {
            static_cast<uint8_t*>(io.actions_out)[row] = static_cast<const uint8_t*>(io.actions)[p];
        } else if constexpr (kAct == 12) {
            const uint32_t* a = static_cast<const uint32_t*>(io.actions) + (uint64_t)p * 3;
            act_s[tid * 3 + 0] = a[0];
            act_s[tid * 3 + 1] = a[1];
            act_s[tid * 3 + 2] = a[2];
        }
    }
    perm_s[tid] = p;
    __syncthreads();

    if constexpr (kAct == 12) {
        uint32_t* dst = static_cast<uint32_t*>(io.actions_out) + r0 * 3;
        for (int idx = tid; idx < rows * 3; idx += kBlock) dst[idx] = act_s[idx];
    }
    if (!io.states) return;  // uniform over the grid

    const int cnt = rows * DD_OBS_DIM;
    const int a = obs_phase(io.states_out, r0 * DD_OBS_DIM);  // the tile sits in the destination's 16-byte phase
    uint32_t* tile = tile_s + a;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(io.states);
    if (rows == kBlock) states_in<true>(src, perm_s, tile, cnt);
    else states_in<false>(src, perm_s, tile, cnt);
    __syncthreads();

    uint32_t* dst = reinterpret_cast<uint32_t*>(io.states_out) + r0 * DD_OBS_DIM;
    const int head = min((4 - a) & 3, cnt);  // words before the destination's first 16-byte boundary
    const int nv = (cnt - head) >> 2;
    const int tail0 = head + (nv << 2);      // and after its last
    for (int k = tid; k < nv; k += kBlock) {
        const int e0 = head + (k << 2);      // tile + e0 and dst + e0 are both 16-byte aligned
        __builtin_nontemporal_store(*reinterpret_cast<const u32x4*>(tile + e0), reinterpret_cast<u32x4*>(dst + e0));
    }
    if (tid < head) {
        dst[tid] = tile[tid];
    } else if (tid < head + (cnt - tail0)) {
        const int e = tail0 + (tid - head);
        dst[e] = tile[e];
    }
}

inline bool size_ok(int64_t m) { return m >= 0 && m < (int64_t)1 << 31; }

struct Range {
    uintptr_t first;
    uint64_t bytes;
};
inline bool overlap(const Range& x, const Range& y) {
    return x.bytes && y.bytes && x.first < y.first + y.bytes && y.first < x.first + x.bytes;
}

}  // namespace shuffle
}  // namespace dd

extern "C" {

int dd_shuffle_indices(int64_t m, uint64_t seed, uint64_t epoch, int32_t* out, void* stream) {
    using namespace dd::shuffle;
    if (!size_ok(m) || !out) return hipErrorInvalidValue;
    if (m == 0) return 0;
    hipLaunchKernelGGL(indices_kernel, dim3((unsigned)dd::tiles_of(m)), dim3(dd::kBlock), 0,
                       static_cast<hipStream_t>(stream), out, key_of(m, seed, epoch));
    return dd::finish();
}

int dd_shuffle_rows(const DDShuffleIO* io, int64_t m, uint64_t seed, uint64_t epoch, void* stream) {
    using namespace dd::shuffle;
    if (!io || !size_ok(m)) return hipErrorInvalidValue;
    if ((io->states != nullptr) != (io->states_out != nullptr) ||
        (io->actions != nullptr) != (io->actions_out != nullptr) ||
        (io->old_log_probs != nullptr) != (io->old_log_probs_out != nullptr) ||
        (io->advantages != nullptr) != (io->advantages_out != nullptr) ||
        (io->returns != nullptr) != (io->returns_out != nullptr))
        return hipErrorInvalidValue;
    if (io->actions && io->action_format != DD_ACT_BITMASK && io->action_format != DD_ACT_F32X3)
        return hipErrorInvalidValue;
    const int act = io->actions ? (int)dd::action_bytes(io->action_format) : 0;
    const uint64_t rows = (uint64_t)m;
    const Range src[5] = {{(uintptr_t)io->states, rows * 4 * DD_OBS_DIM}, {(uintptr_t)io->actions, rows * act},
                          {(uintptr_t)io->old_log_probs, rows * 4}, {(uintptr_t)io->advantages, rows * 4},
                          {(uintptr_t)io->returns, rows * 4}};
    const Range dst[6] = {{(uintptr_t)io->states_out, rows * 4 * DD_OBS_DIM}, {(uintptr_t)io->actions_out, rows * act},
                          {(uintptr_t)io->old_log_probs_out, rows * 4}, {(uintptr_t)io->advantages_out, rows * 4},
                          {(uintptr_t)io->returns_out, rows * 4}, {(uintptr_t)io->indices, rows * 4}};
    bool any = false;
    for (const Range& d : dst) {
        if (!d.first) continue;
        any = true;
        for (const Range& s : src)
            if (s.first && overlap(d, s)) return hipErrorInvalidValue;  // a block would read rows another has rewritten
    }
    if (m == 0 || !any) return 0;
    const Key key = key_of(m, seed, epoch);
    dd::with_value<1, 12, 0>(act, [&](auto bytes) {
        hipLaunchKernelGGL(rows_kernel<decltype(bytes)::value>, dim3((unsigned)dd::tiles_of(m)), dim3(dd::kBlock), 0,
                           static_cast<hipStream_t>(stream), *io, key);
    });
    return dd::finish();
}

}  // extern "C"
