// batch_core.h — what the training-batch units share (train_batch.hip: each
// lane's first episode; train_batch_episodes.hip: every episode of an
// auto-reset rollout; ppo_loss.hip and mlp_backward.hip for the block sums):
// the fixed-shape block sum, block scan and partial-sum total (no atomics: the
// same bits on every run), the scans of the plan kernels, the gather tile, and
// the argument checks the two units' entry points have in common.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dronestep.h"
#include "lane_io.h"
#include "launch.h"

namespace dd {

constexpr int kGatherLanes = 64;                       // lanes of one gather tile: one frame's rows are 3,840 contiguous bytes
constexpr int kObsRow = kGatherLanes * DD_OBS_DIM;     // floats of one frame of a tile
constexpr int kObsRowPad = kObsRow + 4;                // + room for the source's 16-byte phase
constexpr int kSide = kGatherLanes + 1;                // padded [frame][lane] side tiles
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

// block_sum's tree over kBlock values held by ONE wave, four per lane (lane l:
// the values of threads l, l + 64, l + 128 and l + 192 of the block it stands
// for): the same additions in the same grouping, so the same bits, without a
// barrier or LDS.  Lane 0 gets the result.
__device__ __forceinline__ double wave_block_sum(const double (&x)[4]) {
    static_assert(kBlock == 256, "four values per lane");
    double s = (x[0] + x[2]) + (x[1] + x[3]);  // half = 128, then 64
#pragma unroll
    for (int half = 32; half > 0; half >>= 1) s += __shfl_down(s, half, 64);
    return s;
}

// The batch's total from the kStatBlocks partials of a kStatBlocks-block
// launch, the same tree in every block.  sh as block_sum's.
template <typename V>
__device__ __forceinline__ V stat_total(const V* __restrict__ part, V* sh) {
    static_assert(kStatBlocks == 2 * kBlock, "one pair of partials per thread");
    V v = part[threadIdx.x];
    v += part[threadIdx.x + kBlock];
    return block_sum<V>(v, sh);
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

// One block of kScanBlock: exclusive scan of tile_sum[tiles] in place, a
// running carry from one kScanBlock stretch to the next; every thread gets the
// total.  sh: kScanBlock elements, free again on return.
__device__ __forceinline__ int64_t scan_tile_sums(int64_t* tile_sum, int64_t tiles, int64_t* sh) {
    __shared__ int64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < tiles; base += kScanBlock) {
        const int64_t j = base + threadIdx.x;
        const int64_t v = j < tiles ? tile_sum[j] : 0;
        const int64_t incl = block_scan_inclusive<kScanBlock>(v, sh);
        if (j < tiles) tile_sum[j] = carry + incl - v;
        __syncthreads();
        if (threadIdx.x == kScanBlock - 1) carry += incl;
        __syncthreads();
    }
    const int64_t total = carry;
    __syncthreads();
    return total;
}

// One block of kBlock per 256-lane tile: offset[i] = its tile's offset + the
// exclusive scan of the tile's counts (count may be offset itself).  sh: kBlock
// elements, free again on return.
template <typename C>
__device__ __forceinline__ void scan_lane_offsets(const C* count, const int64_t* __restrict__ tile_off, int64_t n,
                                                  int64_t* offset, int64_t* sh) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t v = i < n ? (int64_t)count[i] : 0;
    const int64_t incl = block_scan_inclusive<kBlock>(v, sh);
    if (i < n) offset[i] = tile_off[blockIdx.x] + incl - v;
}

// The 16-byte phase (0..3 floats) of element first_elem of obs.
__device__ __forceinline__ int obs_phase(const float* obs, int64_t first_elem) {
    return (int)((((uintptr_t)obs >> 2) + (uint64_t)first_elem) & 3);
}

// ---------------------------------------------------------------------------
// The gather tile.  A block owns kGatherLanes lanes x F frames of the [T][N]
// rollout; some of the tile's (frame, lane) cells are rows of the batch, and a
// lane's rows of one tile are consecutive rows of the flat outputs.
//   in   In obs[T][N][15] a frame of the tile is 64 x 60 contiguous bytes: read
//        16 bytes per thread where the source allows, in the source's 16-byte
//        phase (ph_s[f]) so that the LDS stores are aligned too, 4 bytes per
//        thread before the first and after the last 16-byte boundary.  A load
//        is made when a lane it touches has a row in that frame (a 16-byte
//        load can straddle two lanes: either).  The action byte and log-prob
//        of every row go to the padded [frame][lane] side tiles.
//   out  In states[M][15] a lane's rows are rows x 60 contiguous bytes, written
//        by a group of kGroup threads as 16-byte stores on the destination's
//        own 16-byte grid, with 4-byte stores at the two ragged ends.  Every
//        row's log-prob, and its action bitmask as [3] floats.
// Cells that are no row are neither read nor written, in any buffer.
//
// Which cells are rows is the kernel's row map, an object with
//   int row(f, l)      frame f of lane l: its row within the lane's run of
//                      this tile, or -1 when it is none
//   int count(l)       the rows of lane l in this tile
//   int64_t first(l)   and the first one's row in the flat outputs
//   int frame(l, r)    the frame of the tile that holds row r of lane l
// answered from the kernel's own shared arrays (any thread asks about any
// lane) for f < nf.  row() takes every l < kGatherLanes and is -1 for a lane
// past the rollout's edge; the others take l < lanes.
// ---------------------------------------------------------------------------
template <int F>
struct GatherTile {
    static constexpr int kGroup = F <= 8 ? 32 : 64;  // threads that write one lane's rows: (F * 15 + 3) / 4 + 1 float4 at most
    static_assert((F * DD_OBS_DIM + 3 + 3) / 4 <= kGroup, "a lane's rows of one tile fit one group's stores");
    float* tile;          // [F][kObsRowPad], 16-byte aligned
    float* lp_s;          // [F][kSide]
    uint8_t* act_s;       // [F][kSide]
    const int32_t* ph_s;  // [F]: each frame's 16-byte phase in obs
    int64_t i0, n;        // the tile's first lane; lanes of the rollout
    int32_t t0;           // the tile's first frame
    int lanes, nf;        // lanes and frames of the tile inside the rollout (nf: that some lane may need)

    template <typename Rows>
    __device__ __forceinline__ void obs_in(const Rows& rows, const float* __restrict__ obs) const {
        const int tid = (int)threadIdx.x;
        const int cnt = lanes * DD_OBS_DIM;
        for (int f = 0; f < nf; ++f) {
            const float* src = obs + ((int64_t)(t0 + f) * n + i0) * DD_OBS_DIM;
            const int a = ph_s[f];
            float* dst = tile + f * kObsRowPad + a;
            const int head = min((4 - a) & 3, cnt);
            const int nv = (cnt - head) >> 2;
            const int tail0 = head + (nv << 2);
            if (tid < nv) {
                const int e0 = head + (tid << 2);
                if (rows.row(f, e0 / DD_OBS_DIM) >= 0 || rows.row(f, (e0 + 3) / DD_OBS_DIM) >= 0)
                    *reinterpret_cast<f32x4*>(dst + e0) = *reinterpret_cast<const f32x4*>(src + e0);
            } else if (tid < nv + head) {  // the elements before the first 16-byte boundary
                const int e = tid - nv;
                if (rows.row(f, e / DD_OBS_DIM) >= 0) dst[e] = src[e];
            } else if (tid < nv + head + (cnt - tail0)) {  // and after the last
                const int e = tail0 + (tid - nv - head);
                if (rows.row(f, e / DD_OBS_DIM) >= 0) dst[e] = src[e];
            }
        }
    }

    template <typename Rows>
    __device__ __forceinline__ void side_in(const Rows& rows, const uint8_t* __restrict__ actions,
                                            const float* __restrict__ log_prob) const {
        for (int idx = (int)threadIdx.x; idx < nf * kGatherLanes; idx += kBlock) {
            const int f = idx / kGatherLanes, l = idx % kGatherLanes;
            if (rows.row(f, l) >= 0) {
                const int64_t o = (int64_t)(t0 + f) * n + i0 + l;
                if (actions) act_s[f * kSide + l] = actions[o];
                if (log_prob) lp_s[f * kSide + l] = log_prob[o];
            }
        }
    }

    template <typename Rows>
    __device__ __forceinline__ void states_out(const Rows& rows, float* __restrict__ states) const {
        const int k = (int)threadIdx.x % kGroup;
        for (int l = (int)threadIdx.x / kGroup; l < lanes; l += kBlock / kGroup) {
            const int nrows = rows.count(l);
            if (nrows <= 0) continue;
            const int cnt = nrows * DD_OBS_DIM;
            const int64_t s = rows.first(l) * DD_OBS_DIM;  // first element of the lane's rows in states
            const int a = (int)((((uintptr_t)states >> 2) + (uint64_t)s) & 3);
            const int j0 = (k << 2) - a;  // this thread's four elements: j0 .. j0 + 3 of the lane's cnt
            if (j0 >= cnt) continue;
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = min(max(j0 + q, 0), cnt - 1);
                // c from r, not j % 15: the compiler divided a second time otherwise (profiles/r14/README.md)
                const int r = j / DD_OBS_DIM, c = j - r * DD_OBS_DIM, f = rows.frame(l, r);
                v[q] = tile[f * kObsRowPad + ph_s[f] + l * DD_OBS_DIM + c];
            }
            float* dst = states + s + j0;
            if (j0 >= 0 && j0 + 4 <= cnt) {
                const f32x4 v4 = {v[0], v[1], v[2], v[3]};  // dst is on states' 16-byte grid
                __builtin_nontemporal_store(v4, reinterpret_cast<f32x4*>(dst));
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (j0 + q >= 0 && j0 + q < cnt) dst[q] = v[q];
            }
        }
    }

    // act_out, lp_out: null when their input is
    template <typename Rows>
    __device__ __forceinline__ void side_out(const Rows& rows, float* __restrict__ act_out,
                                             float* __restrict__ lp_out) const {
        for (int idx = (int)threadIdx.x; idx < kGatherLanes * F; idx += kBlock) {
            const int l = idx / F, f = idx % F;
            const int r = rows.row(f, l);
            if (f < nf && r >= 0) {
                const int64_t row = rows.first(l) + r;
                if (lp_out) lp_out[row] = lp_s[f * kSide + l];
                if (act_out) {  // (main, left, right) as Bernoulli.sample() lays them out
                    const uint32_t bits = act_s[f * kSide + l];
                    act_out[row * 3 + 0] = (float)(bits & 1u);
                    act_out[row * 3 + 1] = (float)((bits >> 1) & 1u);
                    act_out[row * 3 + 2] = (float)((bits >> 2) & 1u);
                }
            }
        }
    }

    // The whole tile, for a block whose row map and ph_s are written and
    // synchronised.  A null input is skipped, and its output with it.
    template <typename Rows>
    __device__ __forceinline__ void gather(const Rows& rows, const float* __restrict__ obs,
                                           const uint8_t* __restrict__ actions, const float* __restrict__ log_prob,
                                           float* __restrict__ states, float* __restrict__ act_out,
                                           float* __restrict__ lp_out) const {
        if (obs) obs_in(rows, obs);
        if (actions || log_prob) side_in(rows, actions, log_prob);
        __syncthreads();
        if (obs) states_out(rows, states);
        if (actions || log_prob) side_out(rows, actions ? act_out : nullptr, log_prob ? lp_out : nullptr);
    }
};

// ---------------------------------------------------------------------------
// Host side: the checks dd_batch_* and dd_episodes_* make alike.
// ---------------------------------------------------------------------------
inline bool shape_ok(int64_t T, int64_t n) { return T >= 0 && n >= 0 && T <= INT32_MAX && n <= INT32_MAX; }

// A gather's launch from its DDBatchGatherIO: every input paired with its
// output, the tile width (0: 8), nothing to gather (0 with blocks == 0), the
// unit's own inputs (inputs_ok), the grid.
struct GatherLaunch {
    int frames;
    int64_t lane_tiles, blocks;
};
inline int gather_launch(const DDBatchGatherIO* io, int64_t T, int64_t n, bool inputs_ok, GatherLaunch* out) {
    *out = {0, 0, 0};
    if ((io->obs != nullptr) != (io->states != nullptr) || (io->actions != nullptr) != (io->actions_out != nullptr) ||
        (io->log_prob != nullptr) != (io->old_log_probs != nullptr))
        return hipErrorInvalidValue;
    const int frames = io->tile_frames == 0 ? 8 : io->tile_frames;
    if (frames != 8 && frames != 16) return hipErrorInvalidValue;
    if (T == 0 || n == 0 || (!io->obs && !io->actions && !io->log_prob)) return 0;
    if (!inputs_ok) return hipErrorInvalidValue;
    const int64_t lane_tiles = (n + kGatherLanes - 1) / kGatherLanes;
    const int64_t blocks = lane_tiles * ((T + frames - 1) / frames);
    if (blocks > INT32_MAX) return hipErrorInvalidValue;
    *out = {frames, lane_tiles, blocks};
    return 0;
}

// A DDBatchAdvIO's mode, precision and the pointers its mode needs (reward
// apart: whether it is needed depends on the unit's empty cases).
inline int adv_io_check(const DDBatchAdvIO* io) {
    if (io->mode != DD_BATCH_GAE && io->mode != DD_BATCH_RETURNS) return hipErrorInvalidValue;
    if (io->precision != DD_F32 && io->precision != DD_F64) return hipErrorInvalidValue;
    if (io->mode == DD_BATCH_GAE ? (!io->values || !io->advantages) : !io->returns) return hipErrorInvalidValue;
    return 0;
}

// fn(R{}, mode, g, gl): the reward's storage type, the mode as an
// integral_constant, gamma and gamma * lambda rounded to float32 as gae() does.
template <typename Fn>
void with_adv_kernel(const DDBatchAdvIO* io, Fn fn) {
    const float g = (float)io->gamma;
    const float gl = (float)(io->gamma * io->lambda);
    with_storage(io->precision, [&](auto tag) {
        with_value<DD_BATCH_GAE, DD_BATCH_RETURNS>(io->mode, [&](auto mode) { fn(tag, mode, g, gl); });
    });
}

}  // namespace dd
