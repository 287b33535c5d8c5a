// train_batch_episodes.hip — the training batch of EVERY episode of a [T][N]
// rollout (train_batch.hip keeps each lane's first one): what a fixed-length
// rollout of an auto-reset env, continued across PPO iterations, feeds the
// notebooks' loss functions.  The rule is `done`'s alone (dronestep.h):
// frame t of a lane is dropped when the frame before it was done (the
// re-spawn frame of an auto-reset env; every later frame of a sticky one), an
// episode is a maximal run of kept frames, closed by a done ("ended") or cut by
// the end of the rollout ("open").  Dropped frames sit only after a done, so
// an episode's frames are consecutive: [ep_start, ep_start + ep_length).
//   count       per lane: episodes and rows; exclusive scans over the lanes
//               (fixed shape, no atomics), E and M          dd_episodes_count
//   fill        the per-episode records                     dd_episodes_fill
//   gather      states / actions / log-probs of the kept frames, a lane's
//               rows contiguous in frame order              dd_episodes_gather
//   advantages  compute_gae (gae_core.h) or compute_returns per episode, and
//               sum(rewards) per episode                    dd_episodes_advantages
// The normalisation is train_batch.hip's dd_batch_normalize on the M rows.
// Rows and elements are indexed in 64 bits throughout.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "batch_core.h"
#include "dronestep.h"
#include "gae_core.h"
#include "lane_io.h"
#include "launch.h"

namespace dd {

// One lane's episodes in time order: on(start, length, ended) for each.  Eight
// frames' loads are in flight; across the lanes of a wave they are coalesced.
template <typename OnEpisode>
__device__ __forceinline__ void walk_episodes(const uint8_t* __restrict__ done,
                                              const uint8_t* __restrict__ done_before, int32_t T, int64_t n,
                                              int64_t i, bool drop_open, OnEpisode on) {
    constexpr int kG = 8;
    bool prev = done_before && done_before[i] != 0;
    int32_t run = 0;  // kept frames of the episode that is running
    for (int32_t t0 = 0; t0 < T; t0 += kG) {
        uint8_t d[kG];
#pragma unroll
        for (int j = 0; j < kG; ++j) d[j] = t0 + j < T ? done[(int64_t)(t0 + j) * n + i] : (uint8_t)0;
#pragma unroll
        for (int j = 0; j < kG; ++j) {
            if (t0 + j < T) {
                const bool dn = d[j] != 0;
                if (!prev) {
                    ++run;
                    if (dn) {
                        on(t0 + j - run + 1, run, true);
                        run = 0;
                    }
                }
                prev = dn;
            }
        }
    }
    if (run > 0 && !drop_open) on(T - run, run, false);
}

// ---------------------------------------------------------------------------
// Count.  One thread per lane; the lane's counts go to lane_episode[i] and
// lane_row[i] (replaced by the offsets below), the block's sums to the two
// halves of the workspace.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void episodes_count_kernel(const uint8_t* __restrict__ done,
                                                                const uint8_t* __restrict__ done_before, int32_t T,
                                                                int64_t n, int32_t drop_open,
                                                                int64_t* __restrict__ lane_episode,
                                                                int64_t* __restrict__ lane_row,
                                                                int64_t* __restrict__ tile_episode,
                                                                int64_t* __restrict__ tile_row) {
    __shared__ int64_t part[kBlock];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int64_t episodes = 0, rows = 0;
    if (i < n) {
        walk_episodes(done, done_before, T, n, i, drop_open != 0, [&](int32_t, int32_t len, bool) {
            ++episodes;
            rows += len;
        });
        lane_episode[i] = episodes;
        lane_row[i] = rows;
    }
    const int64_t se = block_sum<int64_t>(episodes, part);
    const int64_t sr = block_sum<int64_t>(rows, part);
    if (threadIdx.x == 0) {
        tile_episode[blockIdx.x] = se;
        tile_row[blockIdx.x] = sr;
    }
}

// One block: exclusive scan of the tile sums of both quantities in place; the
// totals go to lane_episode[n], lane_row[n] and totals {E, M}.
__global__ __launch_bounds__(kScanBlock) void episodes_tile_scan_kernel(int64_t* tile_episode, int64_t* tile_row,
                                                                        int64_t tiles, int64_t* total_episode,
                                                                        int64_t* total_row, int64_t* totals) {
    __shared__ int64_t part[kScanBlock];
    const int64_t e = scan_tile_sums(tile_episode, tiles, part);
    const int64_t m = scan_tile_sums(tile_row, tiles, part);
    if (threadIdx.x == 0) {
        *total_episode = totals[0] = e;
        *total_row = totals[1] = m;
    }
}

// lane_x[i] = its tile's offset + the exclusive scan of the tile's counts.
__global__ __launch_bounds__(kBlock) void episodes_offset_kernel(const int64_t* __restrict__ tile_episode,
                                                                 const int64_t* __restrict__ tile_row, int64_t n,
                                                                 int64_t* lane_episode, int64_t* lane_row) {
    __shared__ int64_t part[kBlock];
    scan_lane_offsets(lane_episode, tile_episode, n, lane_episode, part);
    scan_lane_offsets(lane_row, tile_row, n, lane_row, part);
}

// ---------------------------------------------------------------------------
// Fill.  The same walk, writing each episode's record at lane_episode[i] + k.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void episodes_fill_kernel(const uint8_t* __restrict__ done,
                                                               const uint8_t* __restrict__ done_before, int32_t T,
                                                               int64_t n, int32_t drop_open,
                                                               const int64_t* __restrict__ lane_episode,
                                                               const int64_t* __restrict__ lane_row,
                                                               int32_t* __restrict__ ep_lane,
                                                               int32_t* __restrict__ ep_start,
                                                               int32_t* __restrict__ ep_length,
                                                               uint8_t* __restrict__ ep_ended,
                                                               int64_t* __restrict__ ep_offset) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    int64_t e = lane_episode[i];
    const int64_t e_end = lane_episode[i + 1];
    int64_t row = lane_row[i];
    walk_episodes(done, done_before, T, n, i, drop_open != 0, [&](int32_t start, int32_t len, bool ended) {
        if (e < e_end) {  // a layout counted with other flags: stay inside the lane's records
            ep_lane[e] = (int32_t)i;
            ep_start[e] = start;
            ep_length[e] = len;
            ep_ended[e] = ended ? 1 : 0;
            ep_offset[e] = row;
        }
        ++e;
        row += len;
    });
    if (i == n - 1) ep_offset[e_end] = lane_row[n];
}

// ---------------------------------------------------------------------------
// Gather.  batch_core.h's gather tile; a lane's rows are its kept frames that
// the layout counted, in frame order from lane_row[lane].  A lane's
// kept-frame rank at the tile's first frame is recomputed from done: t0 less
// the dropped frames before t0, and frame t is dropped exactly when
// done[t - 1] (done_before for t = 0) is set, so the count is a plain sum of
// non-zero bytes, split over four threads per lane.  Inside the tile one
// thread per lane ranks the F frames; a kept frame whose rank is not below the
// lane's row count belongs to a dropped open episode (the lane's last) and is
// no row.  A tile with no row returns after that.
// ---------------------------------------------------------------------------
template <int F>
struct EpisodeRows {
    const int8_t* rowidx_s;  // [F][kSide]: the frame's row within the lane's run of this tile, or -1
    const uint8_t* rowf_s;   // [kGatherLanes][F]: the inverse
    const int64_t* row0_s;   // [kGatherLanes]: the lane's first row of this tile
    const int32_t* rows_s;   // [kGatherLanes]: and how many
    __device__ __forceinline__ int row(int f, int l) const { return rowidx_s[f * kSide + l]; }
    __device__ __forceinline__ int count(int l) const { return rows_s[l]; }
    __device__ __forceinline__ int64_t first(int l) const { return row0_s[l]; }
    __device__ __forceinline__ int frame(int l, int r) const { return rowf_s[l * F + r]; }
};

template <int F>
__global__ __launch_bounds__(kBlock) void episodes_gather_kernel(const int64_t* __restrict__ lane_row,
                                                                 const uint8_t* __restrict__ done,
                                                                 const uint8_t* __restrict__ done_before,
                                                                 const float* __restrict__ obs,
                                                                 const uint8_t* __restrict__ actions,
                                                                 const float* __restrict__ log_prob,
                                                                 float* __restrict__ states,
                                                                 float* __restrict__ act_out,
                                                                 float* __restrict__ lp_out, int32_t T, int64_t n,
                                                                 int64_t lane_tiles) {
    static_assert(kBlock == 4 * kGatherLanes, "four threads per lane count the dropped frames");
    __shared__ __attribute__((aligned(16))) float tile[F * kObsRowPad];
    __shared__ float lp_s[F * kSide];
    __shared__ uint8_t act_s[F * kSide];
    __shared__ int8_t rowidx_s[F * kSide];
    __shared__ uint8_t rowf_s[kGatherLanes * F];
    __shared__ int64_t row0_s[kGatherLanes];
    __shared__ int32_t rows_s[kGatherLanes];
    __shared__ int32_t part_s[kBlock];
    __shared__ int32_t ph_s[F];
    __shared__ int32_t max_rows;

    const int tid = (int)threadIdx.x;
    const int64_t i0 = ((int64_t)blockIdx.x % lane_tiles) * kGatherLanes;
    const int32_t t0 = (int32_t)(((int64_t)blockIdx.x / lane_tiles) * F);
    const int lanes = (int)(n - i0 < kGatherLanes ? n - i0 : kGatherLanes);
    {
        const int l = tid % kGatherLanes, q = tid / kGatherLanes;
        int32_t c = 0;
        if (l < lanes)
            for (int32_t t = q; t < t0 - 1; t += 4) c += done[(int64_t)t * n + i0 + l] != 0 ? 1 : 0;
        part_s[tid] = c;
        if (tid < F) ph_s[tid] = obs ? obs_phase(obs, ((int64_t)(t0 + tid) * n + i0) * DD_OBS_DIM) : 0;
    }
    __syncthreads();
    if (tid < kGatherLanes) {
        int32_t k = 0;
        int64_t row0 = 0;
        if (tid < lanes) {
            const int64_t i = i0 + tid;
            const int64_t base = lane_row[i];
            const int64_t cnt = lane_row[i + 1] - base;
            const bool before = done_before && done_before[i] != 0;
            bool prev = t0 == 0 ? before : done[(int64_t)(t0 - 1) * n + i] != 0;
            const int32_t dropped = part_s[tid] + part_s[tid + kGatherLanes] + part_s[tid + 2 * kGatherLanes] +
                                    part_s[tid + 3 * kGatherLanes] + (t0 > 0 && before ? 1 : 0);
            const int32_t rank0 = t0 - dropped;
            row0 = base + rank0;
#pragma unroll
            for (int f = 0; f < F; ++f) {
                int8_t idx = -1;
                if (t0 + f < T) {
                    if (!prev && rank0 + k < cnt) {
                        idx = (int8_t)k;
                        rowf_s[tid * F + k] = (uint8_t)f;
                        ++k;
                    }
                    prev = done[(int64_t)(t0 + f) * n + i] != 0;
                }
                rowidx_s[f * kSide + tid] = idx;
            }
        } else {
#pragma unroll
            for (int f = 0; f < F; ++f) rowidx_s[f * kSide + tid] = -1;
        }
        rows_s[tid] = k;
        row0_s[tid] = row0;
        int32_t m = k;
        for (int o = kWave / 2; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
        if (tid == 0) max_rows = m;
    }
    __syncthreads();
    if (max_rows <= 0) return;  // no row in this tile
    GatherTile<F>{tile, lp_s, act_s, ph_s, i0, n, t0, lanes, min(F, T - t0)}.gather(
        EpisodeRows<F>{rowidx_s, rowf_s, row0_s, rows_s}, obs, actions, log_prob, states, act_out, lp_out);
}

// ---------------------------------------------------------------------------
// Advantages.  One thread per lane, all lanes at the same frame, so the
// reward is read from the rectangle coalesced over the lanes; only values,
// advantages and returns are flat.  Forward: sum(rewards) per episode in
// double.  Backward: per episode batch_adv_kernel's recursion (kMode
// DD_BATCH_GAE: gae_core.h on the reward rounded to float32, dones all false
// but the last frame of an ended episode, bootstrap[lane] after an open one;
// DD_BATCH_RETURNS: G = r + gamma * G in double, rounded to float32 once).
// ---------------------------------------------------------------------------
template <typename R, int kMode>
__global__ __launch_bounds__(kBlock) void episodes_adv_kernel(const int64_t* __restrict__ lane_episode,
                                                              const int32_t* __restrict__ ep_start,
                                                              const int32_t* __restrict__ ep_length,
                                                              const uint8_t* __restrict__ ep_ended,
                                                              const int64_t* __restrict__ ep_offset,
                                                              const R* __restrict__ reward,
                                                              const float* __restrict__ values,
                                                              const float* __restrict__ bootstrap,
                                                              float* __restrict__ adv, float* __restrict__ ret,
                                                              double* __restrict__ ep_ret, int32_t T, int64_t n,
                                                              float g, float gl, double gamma) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int64_t e0 = lane_episode[i], e1 = lane_episode[i + 1];
    if (e0 >= e1) return;
    if (ep_ret) {
        int64_t e = e0;
        int32_t s = ep_start[e], last = s + ep_length[e] - 1;
        double sum = 0.0;
        for (int32_t t = 0; t < T && e < e1; ++t) {
            if (t < s) continue;
            sum += (double)reward[(int64_t)t * n + i];
            if (t == last) {
                ep_ret[e] = sum;
                sum = 0.0;
                if (++e < e1) {
                    s = ep_start[e];
                    last = s + ep_length[e] - 1;
                }
            }
        }
    }
    int64_t e = e1 - 1;
    int32_t s = ep_start[e], last = s + ep_length[e] - 1;
    int64_t off = 0;  // row of frame t = off + t
    float v_next = 0.0f, mask = 1.0f, gae = 0.0f;
    double G = 0.0;
    for (int32_t t = T - 1; t >= 0 && e >= e0; --t) {
        if (t > last) continue;
        if (t == last) {
            off = ep_offset[e] - s;
            if constexpr (kMode == DD_BATCH_GAE) {
                const bool ended = ep_ended[e] != 0;
                v_next = !ended && bootstrap ? bootstrap[i] : 0.0f;
                mask = ended ? 0.0f : 1.0f;
                gae = 0.0f;
            } else {
                G = 0.0;
            }
        }
        const int64_t o = off + t;
        if constexpr (kMode == DD_BATCH_GAE) {
            const float v = values[o];
            const float a = gae_frame((float)reward[(int64_t)t * n + i], v, v_next, mask, g, gl, gae);
            adv[o] = a;
            if (ret) ret[o] = a + v;
            v_next = v;
            mask = 1.0f;
        } else {
            G = (double)reward[(int64_t)t * n + i] + gamma * G;
            ret[o] = (float)G;
        }
        if (t == s && --e >= e0) {
            s = ep_start[e];
            last = s + ep_length[e] - 1;
        }
    }
}

inline bool lanes_ok(const DDEpisodeLayout* lay) { return lay && lay->lane_episode && lay->lane_row; }
inline bool episodes_ok(const DDEpisodeLayout* lay) {
    return lanes_ok(lay) && lay->ep_lane && lay->ep_start && lay->ep_length && lay->ep_ended && lay->ep_offset;
}

}  // namespace dd

extern "C" {

int64_t dd_episodes_workspace(int64_t n) {
    const int64_t tiles = n <= 0 ? 1 : dd::tiles_of(n);
    return 16 * tiles;  // one int64 per 256-lane tile for the episodes, one for the rows
}

int dd_episodes_count(const uint8_t* done, const uint8_t* done_before, int64_t T, int64_t n, int32_t flags,
                      const DDEpisodeLayout* layout, int64_t* totals, void* workspace, void* stream) {
    if (!dd::shape_ok(T, n) || (flags & ~DD_EPISODES_DROP_OPEN) || !dd::lanes_ok(layout) || !totals || !workspace ||
        (T > 0 && n > 0 && !done))
        return hipErrorInvalidValue;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (T == 0 || n == 0) {  // no frame: no episode, no row
        hipError_t err = hipMemsetAsync(layout->lane_episode, 0, (size_t)(n + 1) * sizeof(int64_t), s);
        if (err == hipSuccess) err = hipMemsetAsync(layout->lane_row, 0, (size_t)(n + 1) * sizeof(int64_t), s);
        if (err == hipSuccess) err = hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), s);
        return (int)err;
    }
    const int64_t tiles = dd::tiles_of(n);
    int64_t* tile_episode = static_cast<int64_t*>(workspace);
    int64_t* tile_row = tile_episode + tiles;
    hipLaunchKernelGGL(dd::episodes_count_kernel, dim3((unsigned)tiles), dim3(dd::kBlock), 0, s, done, done_before,
                       (int32_t)T, n, flags & DD_EPISODES_DROP_OPEN, layout->lane_episode, layout->lane_row,
                       tile_episode, tile_row);
    hipLaunchKernelGGL(dd::episodes_tile_scan_kernel, dim3(1), dim3(dd::kScanBlock), 0, s, tile_episode, tile_row,
                       tiles, layout->lane_episode + n, layout->lane_row + n, totals);
    hipLaunchKernelGGL(dd::episodes_offset_kernel, dim3((unsigned)tiles), dim3(dd::kBlock), 0, s,
                       (const int64_t*)tile_episode, (const int64_t*)tile_row, n, layout->lane_episode,
                       layout->lane_row);
    return dd::finish();
}

int dd_episodes_fill(const uint8_t* done, const uint8_t* done_before, int64_t T, int64_t n, int32_t flags,
                     const DDEpisodeLayout* layout, void* stream) {
    if (!dd::shape_ok(T, n) || (flags & ~DD_EPISODES_DROP_OPEN) || !dd::lanes_ok(layout) || !layout->ep_offset)
        return hipErrorInvalidValue;
    if (T == 0 || n == 0) return 0;  // ep_offset[0] = M = 0 is the caller's (there is no lane to write it)
    if (!done || !dd::episodes_ok(layout)) return hipErrorInvalidValue;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(dd::episodes_fill_kernel, dim3((unsigned)dd::tiles_of(n)), dim3(dd::kBlock), 0, s, done,
                       done_before, (int32_t)T, n, flags & DD_EPISODES_DROP_OPEN,
                       (const int64_t*)layout->lane_episode, (const int64_t*)layout->lane_row, layout->ep_lane,
                       layout->ep_start, layout->ep_length, layout->ep_ended, layout->ep_offset);
    return dd::finish();
}

int dd_episodes_gather(const DDEpisodeLayout* layout, const uint8_t* done, const uint8_t* done_before,
                       const DDBatchGatherIO* io, int64_t T, int64_t n, void* stream) {
    if (!dd::shape_ok(T, n) || !dd::lanes_ok(layout) || !io) return hipErrorInvalidValue;
    dd::GatherLaunch g;
    if (const int err = dd::gather_launch(io, T, n, done != nullptr, &g); err || g.blocks == 0) return err;
    hipStream_t s = static_cast<hipStream_t>(stream);
    dd::with_value<16, 8>(g.frames, [&](auto f) {
        hipLaunchKernelGGL(dd::episodes_gather_kernel<decltype(f)::value>, dim3((unsigned)g.blocks), dim3(dd::kBlock),
                           0, s, (const int64_t*)layout->lane_row, done, done_before, io->obs, io->actions,
                           io->log_prob, io->states, io->actions_out, io->old_log_probs, (int32_t)T, n, g.lane_tiles);
    });
    return dd::finish();
}

int dd_episodes_advantages(const DDEpisodeLayout* layout, const DDBatchAdvIO* io, int64_t T, int64_t n,
                           void* stream) {
    if (!dd::shape_ok(T, n) || !dd::episodes_ok(layout) || !io) return hipErrorInvalidValue;
    if (const int err = dd::adv_io_check(io)) return err;
    if (T == 0 || n == 0) return 0;
    if (!io->reward) return hipErrorInvalidValue;
    hipStream_t s = static_cast<hipStream_t>(stream);
    dd::with_adv_kernel(io, [&](auto tag, auto mode, float g, float gl) {
        using R = decltype(tag);
        hipLaunchKernelGGL((dd::episodes_adv_kernel<R, decltype(mode)::value>), dim3((unsigned)dd::tiles_of(n)),
                           dim3(dd::kBlock), 0, s, (const int64_t*)layout->lane_episode,
                           (const int32_t*)layout->ep_start, (const int32_t*)layout->ep_length,
                           (const uint8_t*)layout->ep_ended, (const int64_t*)layout->ep_offset,
                           static_cast<const R*>(io->reward), io->values, io->bootstrap, io->advantages, io->returns,
                           io->episode_return, (int32_t)T, n, g, gl, io->gamma);
    });
    return dd::finish();
}

}  // extern "C"
