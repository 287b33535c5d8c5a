// env_ops.hip — the small kernels around the step: reset, the notebook
// reward's history reset, observation and info of the current state, GAE,
// ordered compaction, the sqrt self-test and the clock stamp, with their entry
// points and the C ABI's queries that launch nothing.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dronestep.h"
#include "frame.h"
#include "gae_core.h"
#include "lane_io.h"
#include "launch.h"
#include "philox.h"
#include "trig.h"

namespace dd {

// dd_selftest_sqrt kernel: trig::sqrt_unscaled against the compiler's sqrt()
// on doubles from 2^-767 up, drawn with a uniform exponent (Philox bits: 11
// exponent bits folded into [255, 2047), 52 random mantissa bits), plus the
// integers 0..2^20 (spawn distances) at the start of the range; counts the
// inputs whose results differ in any bit.
__global__ __launch_bounds__(kBlock) void sqrt_selftest_kernel(uint64_t seed, uint64_t first, int64_t len,
                                                               unsigned long long* mismatches) {
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t r[4];
    philox4x32_10((uint32_t)(first + 4 * t), (uint32_t)((first + 4 * t) >> 32), 0x5a17u, 0u, (uint32_t)seed,
                  (uint32_t)(seed >> 32), r);
    int bad = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint64_t idx = 4 * t + q;
        if ((int64_t)idx >= len) break;
        const uint64_t g = first + idx;
        double x;
        if (g <= (1u << 20)) {
            x = (double)g;
        } else {
            const uint32_t hi = r[q], lo = r[(q + 1) & 3] ^ r[(q + 2) & 3];
            const uint64_t exp = 256u + (hi >> 21) % 1791u;  // [256, 2047): 2^-767 .. below inf
            const uint64_t mant = ((uint64_t)(hi & 0xfffffu) << 32) | lo;
            x = __builtin_bit_cast(double, (exp << 52) | mant);
        }
        const double a = sqrt(x), b = trig::sqrt_unscaled(x);
        bad += __builtin_bit_cast(uint64_t, a) != __builtin_bit_cast(uint64_t, b);
    }
    const uint64_t m = __ballot(bad != 0);
    if (m) {
        int total = bad;
        for (int off = 32; off > 0; off >>= 1) total += __shfl_xor(total, off);
        if ((threadIdx.x & (kWave - 1)) == __ffsll((unsigned long long)m) - 1) atomicAdd(mismatches, (unsigned long long)total);
    }
}

// dd_stamp kernel: one lane stores the GPU's constant-rate wall clock
// (s_memrealtime) with a vector store.  Captured into a hipGraph beside the
// step kernels it marks where the graph reaches that point (bench.py).
__global__ __launch_bounds__(kWave) void stamp_kernel(unsigned long long* slot) {
    const unsigned long long t = (unsigned long long)wall_clock64();
    if (threadIdx.x == 0) *slot = t;
}

// dd_shaped_reset kernel: the notebook reward's history restarts from the
// current state (slot 0 = its distance, slot 1 = none).
template <typename T>
__global__ __launch_bounds__(kBlock) void shaped_reset_kernel(Consts k, Soa<T> a, const uint8_t* mask,
                                                              double* hist, int64_t stride, int32_t n) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= (uint32_t)n) return;
    if (mask && !at(mask, i)) return;
    Lane s;
    load_dynamics(a, i, s);
    measure(s);
    at(hist, i) = trig::div_exact(s.dist, k.c.world_width, k.inv_w);
    at(hist + stride, i) = __builtin_nan("");
}

// dd_reset kernel: masked re-spawn (+ optional reset observation).
template <typename T>
__global__ __launch_bounds__(kBlock) void reset_kernel(Consts k, Soa<T> a, const uint8_t* mask,
                                                       float* obs, int32_t n) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= (uint32_t)n) return;
    if (mask && !at(mask, i)) return;
    Lane s;
    s.episode = at(a.episode, i);
    spawn(k.c, k.c.max_fuel, a.env_id_base + i, s);
    store_spawn(a, i, s);
    if (obs) observe(k, s, obs + (size_t)i * DD_OBS_DIM);
}

// dd_write_obs kernel: observation of the current state, LDS-staged.
template <typename T>
__global__ __launch_bounds__(kBlock) void obs_kernel(Consts k, Soa<T> a, float* obs, int32_t n) {
    __shared__ __attribute__((aligned(16))) float tile[kBlock * DD_OBS_DIM];
    const uint32_t row0 = blockIdx.x * kBlock;
    const uint32_t i = row0 + threadIdx.x;
    if (i < (uint32_t)n) {
        Lane s;
        load_dynamics(a, i, s);
        s.status = at(a.status, i);
        measure(s);
        observe(k, s, tile + threadIdx.x * DD_OBS_DIM);
    }
    __syncthreads();
    const int rows = (int)min((uint32_t)kBlock, (uint32_t)n - row0);
    flush_obs_tile(tile, obs + (size_t)row0 * DD_OBS_DIM, rows);
}

// dd_get_info kernel: pixel distance and speed (game_engine.py:292-296).
template <typename T>
__global__ __launch_bounds__(kBlock) void info_kernel(Soa<T> a, T* distance, T* speed, int32_t n) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= (uint32_t)n) return;
    const double x = at(a.x, i), y = at(a.y, i), vx = at(a.vx, i), vy = at(a.vy, i);
    const double dx = (double)at(a.px, i) - x, dy = (double)at(a.py, i) - y;
    if (distance) at(distance, i) = (T)sqrt(dx * dx + dy * dy);
    if (speed) at(speed, i) = (T)sqrt(vx * vx + vy * vy);
}

// ---------------------------------------------------------------------------
// dd_gae: one lane per env walks its column of the [T][N] rollout backwards.
// The loads of a frame do not depend on the running gae, so the compiler
// keeps several frames' loads in flight (unroll 4).  The recursion itself is
// gae_core.h's gae_frame (float32, compute_gae's operation order), which the
// ragged scan of train_batch.hip shares.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void gae_kernel(const float* __restrict__ rewards,
                                                     const float* __restrict__ values,
                                                     const uint8_t* __restrict__ dones, float* __restrict__ adv,
                                                     float* __restrict__ ret, int32_t T, int64_t n, float g,
                                                     float gl) {
    // Frames are processed in groups of kG: the group's loads are all issued
    // before its (serial) arithmetic, so kG loads per array are in flight.
    constexpr int kG = 8;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float gae = 0.0f;
    float v_next = values[(int64_t)T * n + i];
    int32_t t = T - 1;
    for (; t >= kG - 1; t -= kG) {
        float r[kG], v[kG], d[kG];
#pragma unroll
        for (int j = 0; j < kG; ++j) {
            const int64_t o = (int64_t)(t - j) * n + i;
            r[j] = rewards[o];
            v[j] = values[o];
            d[j] = (float)dones[o];
        }
#pragma unroll
        for (int j = 0; j < kG; ++j) {
            const int64_t o = (int64_t)(t - j) * n + i;
            gae_frame(r[j], v[j], v_next, 1.0f - d[j], g, gl, gae);
            __builtin_nontemporal_store(gae, adv + o);
            if (ret) __builtin_nontemporal_store(gae + v[j], ret + o);
            v_next = v[j];
        }
    }
    for (; t >= 0; --t) {
        const int64_t o = (int64_t)t * n + i;
        const float v = values[o];
        gae_frame(rewards[o], v, v_next, 1.0f - (float)dones[o], g, gl, gae);
        __builtin_nontemporal_store(gae, adv + o);
        if (ret) __builtin_nontemporal_store(gae + v, ret + o);
        v_next = v;
    }
}

// ---------------------------------------------------------------------------
// Ordered compaction (dd_compact): count per tile -> exclusive scan of tile
// counts -> scatter in lane order.  Ballots give each wave its count and each
// lane its rank; LDS combines the block's four waves.
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool want_flag(const uint8_t* flags, int32_t want, int64_t i, int64_t n) {
    return i < n && ((flags[i] != 0) == (want != 0));
}

__global__ __launch_bounds__(kBlock) void compact_count_kernel(const uint8_t* flags, int32_t want,
                                                               int32_t* tile_counts, int64_t n) {
    __shared__ int wave_cnt[kBlock / kWave];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t m = __ballot(want_flag(flags, want, i, n));
    if ((threadIdx.x & (kWave - 1)) == 0) wave_cnt[threadIdx.x / kWave] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum = 0;
        for (int w = 0; w < kBlock / kWave; ++w) sum += wave_cnt[w];
        tile_counts[blockIdx.x] = sum;
    }
}

// Single-block exclusive scan over `m` tile counts; total goes to *count.
__global__ __launch_bounds__(1024) void compact_scan_kernel(int32_t* tile_counts, int64_t m, int32_t* count) {
    __shared__ int32_t part[1024];
    __shared__ int32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < m; base += 1024) {
        const int64_t j = base + threadIdx.x;
        const int32_t v = j < m ? tile_counts[j] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {  // Hillis-Steele inclusive scan
            const int32_t add = threadIdx.x >= (unsigned)off ? part[threadIdx.x - off] : 0;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        if (j < m) tile_counts[j] = carry + part[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry += part[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = carry;
}

__global__ __launch_bounds__(kBlock) void compact_scatter_kernel(const uint8_t* flags, int32_t want,
                                                                 const int32_t* tile_offsets,
                                                                 int32_t* idx_out, int64_t n) {
    __shared__ int wave_off[kBlock / kWave];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool keep = want_flag(flags, want, i, n);
    const uint64_t m = __ballot(keep);
    const int w = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) wave_off[w] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = tile_offsets[blockIdx.x];
        for (int k = 0; k < kBlock / kWave; ++k) { const int c = wave_off[k]; wave_off[k] = run; run += c; }
    }
    __syncthreads();
    if (keep) {
        const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
        idx_out[wave_off[w] + rank] = (int32_t)i;
    }
}

// The state kernels' launches: fn(T{}, grid, block, first, len) per chunk of
// lanes, T the state's storage width.
template <typename F>
void launch_chunks(int32_t precision, int64_t n, F fn) {
    with_storage(precision, [&](auto tag) {
        for_each_chunk(n, [&](int64_t first, int64_t len) {
            fn(tag, dim3((unsigned)tiles_of(len)), dim3(kBlock), first, (int32_t)len);
        });
    });
}

}  // namespace dd

extern "C" {

void dd_config_default(DDConfig* c) {
    if (c) *c = dd::reference_config();
}

int dd_reset(const DDConfig* cfg, const DDState* st, const uint8_t* mask, float* obs, int64_t n, void* stream) {
    if (!cfg || !st || n < 0 || n > INT32_MAX) return hipErrorInvalidValue;
    if (n == 0) return 0;
    if (!dd::state_ok(st)) return hipErrorInvalidValue;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dd::Consts k = dd::make_consts(*cfg);
    dd::launch_chunks(st->precision, n, [&](auto tag, dim3 g, dim3 b, int64_t first, int32_t len) {
        using T = decltype(tag);
        hipLaunchKernelGGL(dd::reset_kernel<T>, g, b, 0, s, k, dd::soa_of<T>(*st, first),
                           mask ? mask + first : nullptr, obs ? obs + first * DD_OBS_DIM : nullptr, len);
    });
    return dd::finish();
}

int dd_shaped_reset(const DDConfig* cfg, const DDState* st, const uint8_t* mask, double* hist, int64_t n,
                    void* stream) {
    if (!cfg || !st || n < 0 || n > INT32_MAX) return hipErrorInvalidValue;
    if (n == 0) return 0;
    if (!hist || !dd::state_ok(st)) return hipErrorInvalidValue;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dd::Consts k = dd::make_consts(*cfg);
    dd::launch_chunks(st->precision, n, [&](auto tag, dim3 g, dim3 b, int64_t first, int32_t len) {
        using T = decltype(tag);
        hipLaunchKernelGGL(dd::shaped_reset_kernel<T>, g, b, 0, s, k, dd::soa_of<T>(*st, first),
                           mask ? mask + first : nullptr, hist + first, n, len);
    });
    return dd::finish();
}

int dd_write_obs(const DDConfig* cfg, const DDState* st, float* obs, int64_t n, void* stream) {
    if (!cfg || !st || n < 0 || n > INT32_MAX) return hipErrorInvalidValue;
    if (n == 0) return 0;
    if (!obs || !dd::state_ok(st)) return hipErrorInvalidValue;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dd::Consts k = dd::make_consts(*cfg);
    dd::launch_chunks(st->precision, n, [&](auto tag, dim3 g, dim3 b, int64_t first, int32_t len) {
        using T = decltype(tag);
        hipLaunchKernelGGL(dd::obs_kernel<T>, g, b, 0, s, k, dd::soa_of<T>(*st, first), obs + first * DD_OBS_DIM, len);
    });
    return dd::finish();
}

int dd_get_info(const DDConfig* cfg, const DDState* st, void* distance, void* speed, int64_t n, void* stream) {
    if (!cfg || !st || n < 0 || n > INT32_MAX) return hipErrorInvalidValue;
    if (n == 0 || (!distance && !speed)) return 0;
    if (!dd::state_ok(st)) return hipErrorInvalidValue;
    hipStream_t s = static_cast<hipStream_t>(stream);
    dd::launch_chunks(st->precision, n, [&](auto tag, dim3 g, dim3 b, int64_t first, int32_t len) {
        using T = decltype(tag);
        hipLaunchKernelGGL(dd::info_kernel<T>, g, b, 0, s, dd::soa_of<T>(*st, first),
                           distance ? (T*)distance + first : nullptr, speed ? (T*)speed + first : nullptr, len);
    });
    return dd::finish();
}

int dd_gae(const float* rewards, const float* values, const uint8_t* dones, float* advantages, float* returns,
           int64_t T, int64_t n, double gamma, double lambda, void* stream) {
    if (T < 0 || n < 0 || T > INT32_MAX) return hipErrorInvalidValue;
    if (T == 0 || n == 0) return 0;
    if (!rewards || !values || !dones || !advantages) return hipErrorInvalidValue;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float g = (float)gamma;
    const float gl = (float)(gamma * lambda);
    hipLaunchKernelGGL(dd::gae_kernel, dim3((unsigned)dd::tiles_of(n)), dim3(dd::kBlock), 0, s, rewards, values,
                       dones, advantages, returns, (int32_t)T, n, g, gl);
    return dd::finish();
}

int dd_selftest_sqrt(uint64_t seed, int64_t n, unsigned long long* mismatches, void* stream) {
    if (n < 0 || n > ((int64_t)1 << 40) || !mismatches) return hipErrorInvalidValue;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t per = (int64_t)dd::kBlock * 4096;  // lanes per launch; 4 draws per lane
    for (int64_t first = 0; first < n; first += per * 4) {
        const int64_t len = n - first < per * 4 ? n - first : per * 4;
        const unsigned blocks = (unsigned)dd::tiles_of((len + 3) / 4);
        hipLaunchKernelGGL(dd::sqrt_selftest_kernel, dim3(blocks), dim3(dd::kBlock), 0, s, seed,
                           (uint64_t)first, len, mismatches);
    }
    return dd::finish();
}

int dd_stamp(unsigned long long* slot, void* stream) {
    if (!slot) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dd::stamp_kernel, dim3(1), dim3(dd::kWave), 0, static_cast<hipStream_t>(stream), slot);
    return dd::finish();
}

int dd_wall_clock_khz(int* khz) {
    if (!khz) return hipErrorInvalidValue;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(khz, hipDeviceAttributeWallClockRate, dev);
    return (int)e;
}

int64_t dd_compact_workspace(int64_t n) { return n <= 0 ? 1 : dd::tiles_of(n); }

int dd_compact(const uint8_t* flags, int32_t want, int32_t* idx_out, int32_t* count, int32_t* workspace,
               int64_t n, void* stream) {
    if (n < 0 || n > INT32_MAX || !count || (n > 0 && (!flags || !idx_out || !workspace)))
        return hipErrorInvalidValue;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n == 0) return (int)hipMemsetAsync(count, 0, sizeof(int32_t), s);
    const int64_t m = dd::tiles_of(n);
    hipLaunchKernelGGL(dd::compact_count_kernel, dim3((unsigned)m), dim3(dd::kBlock), 0, s, flags, want,
                       workspace, n);
    hipLaunchKernelGGL(dd::compact_scan_kernel, dim3(1), dim3(1024), 0, s, workspace, m, count);
    hipLaunchKernelGGL(dd::compact_scatter_kernel, dim3((unsigned)m), dim3(dd::kBlock), 0, s, flags, want,
                       (const int32_t*)workspace, idx_out, n);
    return dd::finish();
}

const char* dd_error_string(int code) { return hipGetErrorString((hipError_t)code); }

int dd_abi_version(void) { return DD_ABI_VERSION; }

}  // extern "C"
