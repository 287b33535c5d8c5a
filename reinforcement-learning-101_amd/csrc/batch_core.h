// batch_core.h — what the two training-batch units share (train_batch.hip:
// each lane's first episode; train_batch_episodes.hip: every episode of an
// auto-reset rollout): the gather tile's geometry, the fixed-shape block sum
// and block scan (no atomics: the same bits on every run), and the 16-byte
// phase of an observation row.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dronestep.h"
#include "lane_io.h"

namespace dd {

constexpr int kGatherLanes = 64;                       // lanes of one gather tile: one frame's rows are 3,840 contiguous bytes
constexpr int kObsRow = kGatherLanes * DD_OBS_DIM;     // floats of one frame of a tile
constexpr int kObsRowPad = kObsRow + 4;                // + room for the source's 16-byte phase
constexpr int kStatBlocks = 512;                       // partial sums of the statistics: fixed, so the tree is
constexpr int kScanBlock = 1024;

// Sum over the block in a fixed tree (same bits on every run); every thread
// gets the result.  sh: kBlock elements, free again on return.
template <typename V>
__device__ __forceinline__ V block_sum(V v, V* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int half = kBlock / 2; half > 0; half >>= 1) {
        if (threadIdx.x < (unsigned)half) sh[threadIdx.x] += sh[threadIdx.x + half];
        __syncthreads();
    }
    const V total = sh[0];
    __syncthreads();
    return total;
}

// Hillis-Steele inclusive scan of one value per thread over a block of kThreads;
// sh: kThreads elements, free again on return.
template <int kThreads>
__device__ __forceinline__ int64_t block_scan_inclusive(int64_t v, int64_t* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < kThreads; off <<= 1) {
        const int64_t add = threadIdx.x >= (unsigned)off ? sh[threadIdx.x - off] : 0;
        __syncthreads();
        sh[threadIdx.x] += add;
        __syncthreads();
    }
    const int64_t r = sh[threadIdx.x];
    __syncthreads();
    return r;
}

// The 16-byte phase (0..3 floats) of element first_elem of obs.
__device__ __forceinline__ int obs_phase(const float* obs, int64_t first_elem) {
    return (int)((((uintptr_t)obs >> 2) + (uint64_t)first_elem) & 3);
}

}  // namespace dd
