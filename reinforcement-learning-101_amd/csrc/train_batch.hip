// train_batch.hip — from a finished [T][N] rollout to the flat, episode-major
// training batch the notebooks' loss functions take (Actor_Critic_PPO.ipynb's
// training cell, "PHASE 2"; Policy_Gradients.ipynb's training cell):
//   plan        each lane's first-episode length, its row offset (exclusive
//               scan) and whether the episode ended          dd_batch_plan
//   gather      states [M][15], actions [M][3] float, old log-probs [M], each
//               lane's frames contiguous (the notebook's torch.cat over
//               episodes)                                    dd_batch_gather
//   advantages  compute_gae per episode (gae_core.h) or compute_returns, and
//               sum(rewards) per episode                     dd_batch_advantages
//   normalise   (a - mean) / (std + 1e-8) over the whole batch, statistics in
//               double by a reduction tree of fixed shape    dd_batch_normalize
// Rows and elements are indexed in 64 bits throughout: M * 15 floats passes
// 2^31 bytes at 262,144 lanes x 137 frames.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "batch_core.h"
#include "dronestep.h"
#include "gae_core.h"
#include "lane_io.h"
#include "launch.h"

namespace dd {

// ---------------------------------------------------------------------------
// Plan.  length: one thread per lane reads its column of done[T][N] forward,
// eight frames' loads in flight, and stops at the first group that holds a
// done; the block's row count goes to tile_sum.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void batch_length_kernel(const uint8_t* __restrict__ done, int32_t T, int64_t n,
                                                              int32_t* __restrict__ length,
                                                              uint8_t* __restrict__ ended,
                                                              int64_t* __restrict__ tile_sum) {
    constexpr int kG = 8;
    __shared__ int64_t part[kBlock];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int32_t len = 0;
    if (i < n) {
        len = T;
        bool e = false;
        for (int32_t t0 = 0; t0 < T && !e; t0 += kG) {
            uint8_t d[kG];
#pragma unroll
            for (int j = 0; j < kG; ++j) d[j] = t0 + j < T ? done[(int64_t)(t0 + j) * n + i] : (uint8_t)0;
#pragma unroll
            for (int j = 0; j < kG; ++j) {
                if (!e && d[j]) {
                    len = t0 + j + 1;
                    e = true;
                }
            }
        }
        length[i] = len;
        ended[i] = e ? 1 : 0;
    }
    const int64_t sum = block_sum<int64_t>(len, part);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = sum;
}

// One block: exclusive scan of the tile sums in place; the total (M) goes to
// offset[n].
__global__ __launch_bounds__(kScanBlock) void batch_tile_scan_kernel(int64_t* tile_sum, int64_t tiles,
                                                                     int64_t* total) {
    __shared__ int64_t part[kScanBlock];
    const int64_t m = scan_tile_sums(tile_sum, tiles, part);
    if (threadIdx.x == 0) *total = m;
}

// offset[i] = its tile's offset + the exclusive scan of the tile's lengths.
__global__ __launch_bounds__(kBlock) void batch_offset_kernel(const int32_t* __restrict__ length,
                                                              const int64_t* __restrict__ tile_off, int64_t n,
                                                              int64_t* __restrict__ offset) {
    __shared__ int64_t part[kBlock];
    scan_lane_offsets(length, tile_off, n, offset, part);
}

// ---------------------------------------------------------------------------
// Gather.  batch_core.h's gather tile; a lane's rows are the frames before its
// first episode's end, in place: frame t is row offset[lane] + t.  A tile with
// no live frame returns after reading its 64 lengths.
// ---------------------------------------------------------------------------
template <int F>
struct FirstEpisodeRows {
    const int32_t* len_s;  // [kGatherLanes]: the lanes' lengths, 0 past the rollout's edge
    const int64_t* off_s;  // [kGatherLanes]: and offsets
    int32_t t0;
    __device__ __forceinline__ int row(int f, int l) const { return len_s[l] > t0 + f ? f : -1; }
    __device__ __forceinline__ int count(int l) const { return min(F, len_s[l] - t0); }
    __device__ __forceinline__ int64_t first(int l) const { return off_s[l] + t0; }
    __device__ __forceinline__ int frame(int, int r) const { return r; }
};

template <int F>
__global__ __launch_bounds__(kBlock) void batch_gather_kernel(const int32_t* __restrict__ length,
                                                              const int64_t* __restrict__ offset,
                                                              const float* __restrict__ obs,
                                                              const uint8_t* __restrict__ actions,
                                                              const float* __restrict__ log_prob,
                                                              float* __restrict__ states, float* __restrict__ act_out,
                                                              float* __restrict__ lp_out, int32_t T, int64_t n,
                                                              int64_t lane_tiles) {
    __shared__ __attribute__((aligned(16))) float tile[F * kObsRowPad];
    __shared__ float lp_s[F * kSide];
    __shared__ uint8_t act_s[F * kSide];
    __shared__ int64_t off_s[kGatherLanes];
    __shared__ int32_t len_s[kGatherLanes];
    __shared__ int32_t ph_s[F];
    __shared__ int32_t max_len;

    const int tid = (int)threadIdx.x;
    const int64_t i0 = ((int64_t)blockIdx.x % lane_tiles) * kGatherLanes;
    const int32_t t0 = (int32_t)(((int64_t)blockIdx.x / lane_tiles) * F);
    const int lanes = (int)(n - i0 < kGatherLanes ? n - i0 : kGatherLanes);
    if (tid < kGatherLanes) {
        const int32_t l = tid < lanes ? length[i0 + tid] : 0;
        len_s[tid] = l;
        off_s[tid] = tid < lanes ? offset[i0 + tid] : 0;
        int32_t m = l;
        for (int o = kWave / 2; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
        if (tid == 0) max_len = m;
    } else if (tid < kGatherLanes + F && obs) {
        const int f = tid - kGatherLanes;
        ph_s[f] = obs_phase(obs, ((int64_t)(t0 + f) * n + i0) * DD_OBS_DIM);
    }
    __syncthreads();
    const int nf = min(F, min(max_len, T) - t0);  // frames of this tile that some lane needs
    if (nf <= 0) return;
    GatherTile<F>{tile, lp_s, act_s, ph_s, i0, n, t0, lanes, nf}.gather(
        FirstEpisodeRows<F>{len_s, off_s, t0}, obs, actions, log_prob, states, act_out, lp_out);
}

// ---------------------------------------------------------------------------
// Advantages.  One thread per lane: sum(rewards) forward in double, then the
// episode backwards.  kMode DD_BATCH_GAE: gae_core.h's recursion on the reward
// rounded to float32, dones all false but the last frame of an ended episode,
// bootstrap only where the episode did not end.  DD_BATCH_RETURNS:
// compute_returns on Python floats (G = r + gamma * G in double on the reward
// as stored), rounded to float32 once.
// ---------------------------------------------------------------------------
template <typename R, int kMode>
__global__ __launch_bounds__(kBlock) void batch_adv_kernel(const int32_t* __restrict__ length,
                                                           const int64_t* __restrict__ offset,
                                                           const uint8_t* __restrict__ ended,
                                                           const R* __restrict__ reward,
                                                           const float* __restrict__ values,
                                                           const float* __restrict__ bootstrap,
                                                           float* __restrict__ adv, float* __restrict__ ret,
                                                           double* __restrict__ ep_ret, int64_t n, float g, float gl,
                                                           double gamma) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t len = length[i];
    const int64_t off = offset[i];
    if (ep_ret) {
        double sum = 0.0;
#pragma unroll 8
        for (int32_t t = 0; t < len; ++t) sum += (double)reward[(int64_t)t * n + i];
        ep_ret[i] = sum;
    }
    if constexpr (kMode == DD_BATCH_GAE) {
        const bool e = ended[i] != 0;
        float v_next = !e && bootstrap ? bootstrap[i] : 0.0f;
        float mask = e ? 0.0f : 1.0f;
        float gae = 0.0f;
#pragma unroll 4
        for (int32_t t = len - 1; t >= 0; --t) {
            const int64_t o = off + t;
            const float v = values[o];
            const float a = gae_frame((float)reward[(int64_t)t * n + i], v, v_next, mask, g, gl, gae);
            adv[o] = a;
            if (ret) ret[o] = a + v;
            v_next = v;
            mask = 1.0f;
        }
    } else {
        double G = 0.0;
#pragma unroll 4
        for (int32_t t = len - 1; t >= 0; --t) {
            G = (double)reward[(int64_t)t * n + i] + gamma * G;
            ret[off + t] = (float)G;
        }
    }
}

// ---------------------------------------------------------------------------
// Normalise.  Three launches over x[m]: kStatBlocks partial sums; the mean
// (every block adds the partials in the same tree) and kStatBlocks partial
// sums of squared deviations; the standard deviation and the output.  No
// atomics: each element's place in the tree is fixed by m alone.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void stat_sum_kernel(const float* __restrict__ x, int64_t m,
                                                          double* __restrict__ part_sum) {
    __shared__ double sh[kBlock];
    double s = 0.0;
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < m; k += (int64_t)kStatBlocks * kBlock)
        s += (double)x[k];
    s = block_sum<double>(s, sh);
    if (threadIdx.x == 0) part_sum[blockIdx.x] = s;
}

__global__ __launch_bounds__(kBlock) void stat_dev_kernel(const float* __restrict__ x, int64_t m,
                                                          const double* __restrict__ part_sum,
                                                          double* __restrict__ part_ss, double* __restrict__ mean_out) {
    __shared__ double sh[kBlock];
    const double mean = stat_total(part_sum, sh) / (double)m;
    if (blockIdx.x == 0 && threadIdx.x == 0) *mean_out = mean;
    double s = 0.0;
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < m; k += (int64_t)kStatBlocks * kBlock) {
        const double d = (double)x[k] - mean;
        s += d * d;
    }
    s = block_sum<double>(s, sh);
    if (threadIdx.x == 0) part_ss[blockIdx.x] = s;
}

__global__ __launch_bounds__(kBlock) void stat_apply_kernel(const float* x, float* out, int64_t m,
                                                            const double* __restrict__ part_sum,
                                                            const double* __restrict__ part_ss,
                                                            double* __restrict__ std_out) {
    __shared__ double sh[kBlock];
    const double mean = stat_total(part_sum, sh) / (double)m;
    const double ss = stat_total(part_ss, sh);
    const double sd = m < 2 ? __builtin_nan("") : sqrt(ss / (double)(m - 1));  // torch.std's default: unbiased
    if (blockIdx.x == 0 && threadIdx.x == 0) *std_out = sd;
    if (!out) return;
    const double denom = sd + 1e-8;
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < m; k += (int64_t)gridDim.x * kBlock)
        out[k] = (float)(((double)x[k] - mean) / denom);
}

inline bool layout_ok(const DDBatchLayout* lay) { return lay && lay->length && lay->offset && lay->ended; }

}  // namespace dd

extern "C" {

int64_t dd_batch_workspace(int64_t n) {
    const int64_t tiles = n <= 0 ? 1 : dd::tiles_of(n);
    const int64_t stats = 2 * dd::kStatBlocks;
    return 8 * (tiles > stats ? tiles : stats);
}

int dd_batch_plan(const uint8_t* done, int64_t T, int64_t n, const DDBatchLayout* layout, void* workspace,
                  void* stream) {
    if (!dd::shape_ok(T, n) || !dd::layout_ok(layout) || !workspace || (T > 0 && n > 0 && !done))
        return hipErrorInvalidValue;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n == 0) return (int)hipMemsetAsync(layout->offset, 0, sizeof(int64_t), s);
    const int64_t tiles = dd::tiles_of(n);
    int64_t* tile_sum = static_cast<int64_t*>(workspace);
    hipLaunchKernelGGL(dd::batch_length_kernel, dim3((unsigned)tiles), dim3(dd::kBlock), 0, s, done, (int32_t)T, n,
                       layout->length, layout->ended, tile_sum);
    hipLaunchKernelGGL(dd::batch_tile_scan_kernel, dim3(1), dim3(dd::kScanBlock), 0, s, tile_sum, tiles,
                       layout->offset + n);
    hipLaunchKernelGGL(dd::batch_offset_kernel, dim3((unsigned)tiles), dim3(dd::kBlock), 0, s,
                       (const int32_t*)layout->length, (const int64_t*)tile_sum, n, layout->offset);
    return dd::finish();
}

int dd_batch_gather(const DDBatchLayout* layout, const DDBatchGatherIO* io, int64_t T, int64_t n, void* stream) {
    if (!dd::shape_ok(T, n) || !dd::layout_ok(layout) || !io) return hipErrorInvalidValue;
    dd::GatherLaunch g;
    if (const int err = dd::gather_launch(io, T, n, true, &g); err || g.blocks == 0) return err;
    hipStream_t s = static_cast<hipStream_t>(stream);
    dd::with_value<16, 8>(g.frames, [&](auto f) {
        hipLaunchKernelGGL(dd::batch_gather_kernel<decltype(f)::value>, dim3((unsigned)g.blocks), dim3(dd::kBlock), 0,
                           s, (const int32_t*)layout->length, (const int64_t*)layout->offset, io->obs, io->actions,
                           io->log_prob, io->states, io->actions_out, io->old_log_probs, (int32_t)T, n, g.lane_tiles);
    });
    return dd::finish();
}

int dd_batch_advantages(const DDBatchLayout* layout, const DDBatchAdvIO* io, int64_t T, int64_t n, void* stream) {
    if (!dd::shape_ok(T, n) || !dd::layout_ok(layout) || !io) return hipErrorInvalidValue;
    if (const int err = dd::adv_io_check(io)) return err;
    if (n == 0) return 0;
    if (T > 0 && !io->reward) return hipErrorInvalidValue;
    hipStream_t s = static_cast<hipStream_t>(stream);
    dd::with_adv_kernel(io, [&](auto tag, auto mode, float g, float gl) {
        using R = decltype(tag);
        hipLaunchKernelGGL((dd::batch_adv_kernel<R, decltype(mode)::value>), dim3((unsigned)dd::tiles_of(n)),
                           dim3(dd::kBlock), 0, s, (const int32_t*)layout->length, (const int64_t*)layout->offset,
                           (const uint8_t*)layout->ended, static_cast<const R*>(io->reward), io->values,
                           io->bootstrap, io->advantages, io->returns, io->episode_return, n, g, gl, io->gamma);
    });
    return dd::finish();
}

int dd_batch_normalize(const float* x, float* out, int64_t m, double* mean, double* std, void* workspace,
                       void* stream) {
    if (m < 0 || !mean || !std || !workspace || (m > 0 && !x)) return hipErrorInvalidValue;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* part_sum = static_cast<double*>(workspace);
    double* part_ss = part_sum + dd::kStatBlocks;
    const int64_t tiles = dd::tiles_of(m);
    const unsigned apply_blocks = (unsigned)(tiles < 1 ? 1 : tiles > 8192 ? 8192 : tiles);
    hipLaunchKernelGGL(dd::stat_sum_kernel, dim3(dd::kStatBlocks), dim3(dd::kBlock), 0, s, x, m, part_sum);
    hipLaunchKernelGGL(dd::stat_dev_kernel, dim3(dd::kStatBlocks), dim3(dd::kBlock), 0, s, x, m,
                       (const double*)part_sum, part_ss, mean);
    hipLaunchKernelGGL(dd::stat_apply_kernel, dim3(apply_blocks), dim3(dd::kBlock), 0, s, x, out, m,
                       (const double*)part_sum, (const double*)part_ss, std);
    return dd::finish();
}

}  // extern "C"
