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
    __shared__ int64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < tiles; base += kScanBlock) {
        const int64_t j = base + threadIdx.x;
        const int64_t v = j < tiles ? tile_sum[j] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < kScanBlock; off <<= 1) {  // Hillis-Steele inclusive scan
            const int64_t add = threadIdx.x >= (unsigned)off ? part[threadIdx.x - off] : 0;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        if (j < tiles) tile_sum[j] = carry + part[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == kScanBlock - 1) carry += part[kScanBlock - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

// offset[i] = its tile's offset + the exclusive scan of the tile's lengths.
__global__ __launch_bounds__(kBlock) void batch_offset_kernel(const int32_t* __restrict__ length,
                                                              const int64_t* __restrict__ tile_off, int64_t n,
                                                              int64_t* __restrict__ offset) {
    __shared__ int64_t part[kBlock];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t v = i < n ? length[i] : 0;
    part[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {
        const int64_t add = threadIdx.x >= (unsigned)off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    if (i < n) offset[i] = tile_off[blockIdx.x] + part[threadIdx.x] - v;
}

// ---------------------------------------------------------------------------
// Gather.  A block owns kGatherLanes lanes x F frames.  In obs[T][N][15] a
// frame of the tile is 64 x 60 contiguous bytes (read 16 bytes per thread
// where the source allows, in the source's 16-byte phase so that LDS stores
// are aligned too); in states[M][15] a lane's F rows are F x 60 contiguous
// bytes, written by a group of threads as 16-byte stores on the destination's
// own 16-byte grid, with 4-byte stores at the two ragged ends.  Frames and
// lanes past an episode's end are neither read nor written, and a tile with no
// live frame returns after reading its 64 lengths.
// ---------------------------------------------------------------------------
template <int F>
__global__ __launch_bounds__(kBlock) void batch_gather_kernel(const int32_t* __restrict__ length,
                                                              const int64_t* __restrict__ offset,
                                                              const float* __restrict__ obs,
                                                              const uint8_t* __restrict__ actions,
                                                              const float* __restrict__ log_prob,
                                                              float* __restrict__ states, float* __restrict__ act_out,
                                                              float* __restrict__ lp_out, int32_t T, int64_t n,
                                                              int64_t lane_tiles) {
    constexpr int kGroup = F <= 8 ? 32 : 64;  // threads that write one lane's F rows: (F * 15 + 3) / 4 + 1 float4 at most
    static_assert((F * DD_OBS_DIM + 3 + 3) / 4 <= kGroup, "a lane's rows of one tile fit one group's stores");
    constexpr int kSide = kGatherLanes + 1;   // padded [frame][lane] side tiles
    __shared__ __attribute__((aligned(16))) float tile[F * kObsRowPad];
    __shared__ float lp_s[F * kSide];
    __shared__ uint8_t act_s[F * kSide];
    __shared__ int64_t off_s[kGatherLanes];
    __shared__ int32_t len_s[kGatherLanes];
    __shared__ int32_t ph_s[F];  // each frame's 16-byte phase in obs
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

    if (obs) {
        const int cnt = lanes * DD_OBS_DIM;
        for (int f = 0; f < nf; ++f) {
            const int32_t t = t0 + f;
            const int64_t first = ((int64_t)t * n + i0) * DD_OBS_DIM;
            const float* src = obs + first;
            const int a = ph_s[f];
            float* dst = tile + f * kObsRowPad + a;
            const int head = min((4 - a) & 3, cnt);
            const int nv = (cnt - head) >> 2;
            const int tail0 = head + (nv << 2);
            if (tid < nv) {
                const int e0 = head + (tid << 2);
                if (len_s[e0 / DD_OBS_DIM] > t || len_s[(e0 + 3) / DD_OBS_DIM] > t)
                    *reinterpret_cast<f32x4*>(dst + e0) = *reinterpret_cast<const f32x4*>(src + e0);
            } else if (tid < nv + head) {  // the elements before the first 16-byte boundary
                const int e = tid - nv;
                if (len_s[e / DD_OBS_DIM] > t) dst[e] = src[e];
            } else if (tid < nv + head + (cnt - tail0)) {  // and after the last
                const int e = tail0 + (tid - nv - head);
                if (len_s[e / DD_OBS_DIM] > t) dst[e] = src[e];
            }
        }
    }
    if (actions || log_prob) {
        for (int idx = tid; idx < nf * kGatherLanes; idx += kBlock) {
            const int f = idx / kGatherLanes, l = idx % kGatherLanes;
            if (l < lanes && len_s[l] > t0 + f) {
                const int64_t o = (int64_t)(t0 + f) * n + i0 + l;
                if (actions) act_s[f * kSide + l] = actions[o];
                if (log_prob) lp_s[f * kSide + l] = log_prob[o];
            }
        }
    }
    __syncthreads();

    if (obs) {
        const int k = tid % kGroup;
        for (int l = tid / kGroup; l < lanes; l += kBlock / kGroup) {
            const int rows = min(F, len_s[l] - t0);
            if (rows <= 0) continue;
            const int cnt = rows * DD_OBS_DIM;
            const int64_t s = (off_s[l] + t0) * DD_OBS_DIM;  // first element of the lane's rows in states
            const int a = (int)((((uintptr_t)states >> 2) + (uint64_t)s) & 3);
            const int j0 = (k << 2) - a;  // this thread's four elements: j0 .. j0 + 3 of the lane's cnt
            if (j0 >= cnt) continue;
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = min(max(j0 + q, 0), cnt - 1);
                const int f = j / DD_OBS_DIM, c = j % DD_OBS_DIM;
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
    if (actions || log_prob) {
        for (int idx = tid; idx < kGatherLanes * F; idx += kBlock) {
            const int l = idx / F, f = idx % F;
            if (l < lanes && f < nf && len_s[l] > t0 + f) {
                const int64_t row = off_s[l] + t0 + f;
                if (log_prob) lp_out[row] = lp_s[f * kSide + l];
                if (actions) {  // (main, left, right) as Bernoulli.sample() lays them out
                    const uint32_t bits = act_s[f * kSide + l];
                    act_out[row * 3 + 0] = (float)(bits & 1u);
                    act_out[row * 3 + 1] = (float)((bits >> 1) & 1u);
                    act_out[row * 3 + 2] = (float)((bits >> 2) & 1u);
                }
            }
        }
    }
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
__device__ __forceinline__ double stat_total(const double* __restrict__ part, double* sh) {
    static_assert(kStatBlocks == 2 * kBlock, "one pair of partials per thread");
    return block_sum<double>(part[threadIdx.x] + part[threadIdx.x + kBlock], sh);
}

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
    if (T < 0 || n < 0 || T > INT32_MAX || n > INT32_MAX || !dd::layout_ok(layout) || !workspace ||
        (T > 0 && n > 0 && !done))
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
    if (T < 0 || n < 0 || T > INT32_MAX || n > INT32_MAX || !dd::layout_ok(layout) || !io) return hipErrorInvalidValue;
    if ((io->obs != nullptr) != (io->states != nullptr) || (io->actions != nullptr) != (io->actions_out != nullptr) ||
        (io->log_prob != nullptr) != (io->old_log_probs != nullptr))
        return hipErrorInvalidValue;
    const int frames = io->tile_frames == 0 ? 8 : io->tile_frames;
    if (frames != 8 && frames != 16) return hipErrorInvalidValue;
    if (T == 0 || n == 0 || (!io->obs && !io->actions && !io->log_prob)) return 0;
    const int64_t lane_tiles = (n + dd::kGatherLanes - 1) / dd::kGatherLanes;
    const int64_t blocks = lane_tiles * ((T + frames - 1) / frames);
    if (blocks > INT32_MAX) return hipErrorInvalidValue;
    hipStream_t s = static_cast<hipStream_t>(stream);
    dd::with_value<16, 8>(frames, [&](auto f) {
        hipLaunchKernelGGL(dd::batch_gather_kernel<decltype(f)::value>, dim3((unsigned)blocks), dim3(dd::kBlock), 0, s,
                           (const int32_t*)layout->length, (const int64_t*)layout->offset, io->obs, io->actions,
                           io->log_prob, io->states, io->actions_out, io->old_log_probs, (int32_t)T, n, lane_tiles);
    });
    return dd::finish();
}

int dd_batch_advantages(const DDBatchLayout* layout, const DDBatchAdvIO* io, int64_t T, int64_t n, void* stream) {
    if (T < 0 || n < 0 || T > INT32_MAX || n > INT32_MAX || !dd::layout_ok(layout) || !io) return hipErrorInvalidValue;
    if (io->mode != DD_BATCH_GAE && io->mode != DD_BATCH_RETURNS) return hipErrorInvalidValue;
    if (io->precision != DD_F32 && io->precision != DD_F64) return hipErrorInvalidValue;
    if (io->mode == DD_BATCH_GAE ? (!io->values || !io->advantages) : !io->returns) return hipErrorInvalidValue;
    if (n == 0) return 0;
    if (T > 0 && !io->reward) return hipErrorInvalidValue;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float g = (float)io->gamma;
    const float gl = (float)(io->gamma * io->lambda);
    dd::with_storage(io->precision, [&](auto tag) {
        using R = decltype(tag);
        dd::with_value<DD_BATCH_GAE, DD_BATCH_RETURNS>(io->mode, [&](auto mode) {
            hipLaunchKernelGGL((dd::batch_adv_kernel<R, decltype(mode)::value>), dim3((unsigned)dd::tiles_of(n)),
                               dim3(dd::kBlock), 0, s, (const int32_t*)layout->length, (const int64_t*)layout->offset,
                               (const uint8_t*)layout->ended, static_cast<const R*>(io->reward), io->values,
                               io->bootstrap, io->advantages, io->returns, io->episode_return, n, g, gl, io->gamma);
        });
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
