// lane_io.h — device-side SoA access shared by the step, rollout and
// environment kernels (step.hip, rollout.hip, env_ops.hip), the fused policy
// loops (policy_rollout.hip, policy_eval.hip) and the fused trainers
// (ac_fused.hip, reinforce_fused.hip): block and chunk sizes, the typed view
// of a DDState, lane loads and stores (by 32-bit offset for the step and
// rollout kernels, load_lane / store_lane and the reward history's pair for
// the loops that hold a lane in registers), the observation tile flushes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dronestep.h"
#include "frame.h"

namespace dd {

constexpr int kBlock = 256;  // 4 waves; one obs tile = 256 rows
constexpr int kWave = 64;
// Lanes per launch: keeps every byte offset (lane x 8 B) below 2^31.
constexpr int64_t kChunk = int64_t(1) << 28;
typedef float f32x4 __attribute__((ext_vector_type(4)));

// element i of a lane array (i < kChunk)
template <typename E>
__device__ __forceinline__ E& at(E* base, uint32_t i) {
    using B = typename std::conditional<std::is_const<E>::value, const char, char>::type;
    return *reinterpret_cast<E*>(reinterpret_cast<B*>(base) + (uint32_t)(i * (uint32_t)sizeof(E)));
}

// A wave-uniform pointer the compiler cannot prove uniform (it comes from
// threadIdx-derived arithmetic, or is hoisted into a VGPR), moved to SGPRs so
// loads and stores use the SGPR-base + 32-bit lane offset form and its
// arithmetic stays on the scalar unit.
template <typename P>
__device__ __forceinline__ P* uniform_ptr(P* q) {
    const uint64_t v = reinterpret_cast<uint64_t>(q);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return reinterpret_cast<P*>(((uint64_t)hi << 32) | lo);
}

// The SoA of one batch (DDState) with typed pointers, offset to lane `first`.
template <typename T>
struct Soa {
    T *x, *y, *vx, *vy, *angle, *omega, *fuel, *px, *py, *total;
    uint8_t* status;
    int32_t *steps, *episode;
    int64_t env_id_base;
};

template <typename T>
Soa<T> soa_of(const DDState& st, int64_t first) {
    Soa<T> s;
    s.x = (T*)st.x + first; s.y = (T*)st.y + first; s.vx = (T*)st.vx + first; s.vy = (T*)st.vy + first;
    s.angle = (T*)st.angle + first; s.omega = (T*)st.omega + first; s.fuel = (T*)st.fuel + first;
    s.px = (T*)st.px + first; s.py = (T*)st.py + first; s.total = (T*)st.total_reward + first;
    s.status = st.status + first; s.steps = st.steps + first; s.episode = st.episode + first;
    s.env_id_base = st.env_id_base + first;
    return s;
}

inline bool state_ok(const DDState* st) {
    return st && st->x && st->y && st->vx && st->vy && st->angle && st->omega && st->fuel && st->px &&
           st->py && st->total_reward && st->status && st->steps && st->episode &&
           (st->precision == DD_F32 || st->precision == DD_F64);
}

// ---------------------------------------------------------------------------
// SoA access: wave-uniform base pointers (SGPRs) + one 32-bit byte offset per
// lane, so every load/store is `global_load_dword v, v_off, s[base]`.
// ---------------------------------------------------------------------------

// Store cache policies (gfx950), measured per stream: the
// SoA state is stored plainly (write-back into the XCD's L2; the next step
// reads it there), the output streams this kernel never re-reads (reward,
// done, observation rows) with the non-temporal hint (+2-6 % at 262,144 and
// 16.8M lanes).  Write-through (sc1) state stores made the next step's loads
// miss L2 (0.5 -> 1.35 us), non-temporal state stores / loads were slower.
template <typename E>
__device__ __forceinline__ void store_nt(E* base, uint32_t i, E v) {
    __builtin_nontemporal_store(v, &at(base, i));
}

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Output streams this kernel never re-reads (reward, done) are stored
// non-temporally, like the obs tile.
template <typename E>
__device__ __forceinline__ void put_out(E* base, uint32_t i, E v) {
    asm volatile("" : "+v"(i));  // keep the offset 32-bit and local: SGPR-base store
    store_nt(base, i, v);
}

template <typename T>
__device__ __forceinline__ void load_dynamics(const Soa<T>& a, uint32_t i, Lane& s) {
    s.x = at(a.x, i); s.y = at(a.y, i); s.vx = at(a.vx, i); s.vy = at(a.vy, i);
    s.angle = at(a.angle, i); s.omega = at(a.omega, i); s.fuel = at(a.fuel, i);
    s.px = at(a.px, i); s.py = at(a.py, i);
}

template <typename E>
__device__ __forceinline__ void put_state(E* base, uint32_t i, E v) {
    at(base, i) = v;
}

template <typename T>
__device__ __forceinline__ void store_dynamics(const Soa<T>& a, uint32_t i, const Lane& s) {
    put_state(a.x, i, (T)s.x); put_state(a.y, i, (T)s.y); put_state(a.vx, i, (T)s.vx);
    put_state(a.vy, i, (T)s.vy); put_state(a.angle, i, (T)s.angle); put_state(a.omega, i, (T)s.omega);
    put_state(a.fuel, i, (T)s.fuel);
}

template <typename T, bool kTotal = true>
__device__ __forceinline__ void store_spawn(const Soa<T>& a, uint32_t i, const Lane& s) {
    store_dynamics(a, i, s);
    at(a.px, i) = (T)s.px; at(a.py, i) = (T)s.py;
    if constexpr (kTotal) at(a.total, i) = (T)s.total;
    at(a.status, i) = (uint8_t)s.status;
    at(a.steps, i) = s.steps;
    at(a.episode, i) = s.episode;
}

// A whole lane between the SoA and a Lane by its 64-bit index, for the loops
// that hold a lane in registers across frames (policy_rollout.hip,
// policy_eval.hip, ac_fused.hip, reinforce_fused.hip); the step and rollout
// kernels keep the 32-bit offset forms above.  kEpisode = false is for a loop
// that never re-spawns: the episode counter is neither read (0) nor written.
template <bool kEpisode = true, typename T>
__device__ __forceinline__ void load_lane(const Soa<T>& a, int64_t d, Lane& s) {
    s.x = a.x[d]; s.y = a.y[d]; s.vx = a.vx[d]; s.vy = a.vy[d]; s.angle = a.angle[d]; s.omega = a.omega[d];
    s.fuel = a.fuel[d]; s.px = a.px[d]; s.py = a.py[d]; s.total = a.total[d];
    s.status = a.status[d]; s.steps = a.steps[d];
    s.episode = kEpisode ? a.episode[d] : 0;
}

template <bool kEpisode = true, typename T>
__device__ __forceinline__ void store_lane(const Soa<T>& a, int64_t d, const Lane& s) {
    a.x[d] = (T)s.x; a.y[d] = (T)s.y; a.vx[d] = (T)s.vx; a.vy[d] = (T)s.vy; a.angle[d] = (T)s.angle;
    a.omega[d] = (T)s.omega; a.fuel[d] = (T)s.fuel; a.px[d] = (T)s.px; a.py[d] = (T)s.py;
    a.total[d] = (T)s.total; a.status[d] = (uint8_t)s.status; a.steps[d] = s.steps;
    if constexpr (kEpisode) a.episode[d] = s.episode;
}

// Lane d's pair of the notebook reward's two-frame distance history, hist [2][n]
// (policy_rollout.hip, reinforce_fused.hip; ac_fused.hip moves the pair by hand).
__device__ __forceinline__ void load_hist(const double* hist, int64_t n, int64_t d, double& h0, double& h1) {
    h0 = hist[d];
    h1 = hist[n + d];
}

__device__ __forceinline__ void store_hist(double* hist, int64_t n, int64_t d, double h0, double h1) {
    hist[d] = h0;
    hist[n + d] = h1;
}

// Writes a block's [rows, 15] observation tile from LDS to global memory as
// 16-byte stores (non-temporal: the rows are the step's output stream, read
// by the consumer, not by this kernel again).  dst = first row of the tile.
template <int NB = kBlock>
__device__ __forceinline__ void flush_obs_tile(const float* tile, float* dst, int rows) {
    const int nf = rows * DD_OBS_DIM;
    // tiles start at multiples of 256 rows (15360 B): dst is 16-B aligned iff obs is
    if ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
        const int nv = nf >> 2;
        const f32x4* src4 = reinterpret_cast<const f32x4*>(tile);
        f32x4* dst4 = reinterpret_cast<f32x4*>(dst);
        for (int k = threadIdx.x; k < nv; k += NB) __builtin_nontemporal_store(src4[k], &dst4[k]);
        for (int k = (nv << 2) + threadIdx.x; k < nf; k += NB) dst[k] = tile[k];
    } else {
        for (int k = threadIdx.x; k < nf; k += NB) dst[k] = tile[k];
    }
}

// The same for one wave's slice of the tile (rows <= 64, starting at the
// wave's first row): only this wave wrote and reads the slice, so a
// wave-level sync stands in for the block barrier and each wave's rows leave
// as soon as its own lanes are done.  dst + 64-row slices of 3840 B keep
// the 16-byte alignment of the tile.
__device__ __forceinline__ void flush_obs_wave(const float* wtile, float* dst, int rows) {
    __syncwarp();
    const int lane = threadIdx.x & (kWave - 1);
    const int nf = rows * DD_OBS_DIM;
    if ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
        const int nv = nf >> 2;
        const f32x4* src4 = reinterpret_cast<const f32x4*>(wtile);
        f32x4* dst4 = reinterpret_cast<f32x4*>(uniform_ptr(dst));
        for (int k = lane; k < nv; k += kWave) store_nt(dst4, (uint32_t)k, src4[k]);
        for (int k = (nv << 2) + lane; k < nf; k += kWave) dst[k] = wtile[k];
    } else {
        for (int k = lane; k < nf; k += kWave) dst[k] = wtile[k];
    }
    __syncwarp();  // the slice may be rewritten next (rollout frames)
}

// flush_obs_wave for a wave whose 64 rows all exist and whose dst is 16-byte
// aligned (the step kernel's usual case; the caller tests both, wave-uniform).
// The trip count is a constant, so the loop unrolls: the four LDS reads are
// issued together and the four stores follow, where the general loop's
// run-time bound made each store wait for its own read in turn, at the very
// end of the wave's life.
__device__ __forceinline__ void flush_obs_wave_full(const float* wtile, float* dst) {
    __syncwarp();
    const int lane = threadIdx.x & (kWave - 1);
    constexpr int nv = kWave * DD_OBS_DIM / 4;
    static_assert(kWave * DD_OBS_DIM % 4 == 0, "a full wave's rows are whole 16-byte vectors");
    const f32x4* src4 = reinterpret_cast<const f32x4*>(wtile);
    f32x4* dst4 = reinterpret_cast<f32x4*>(uniform_ptr(dst));
    // (all four reads into registers of their own before the first store
    // measured slower than leaving the order to the compiler: -1.0 % against
    // this loop's -3.1 %, profiles/r13/)
#pragma unroll
    for (int k = lane; k < nv; k += kWave) store_nt(dst4, (uint32_t)k, src4[k]);
    __syncwarp();
}

template <int AFMT>
__device__ __forceinline__ uint32_t load_action(const void* actions, uint32_t i) {
    if constexpr (AFMT == DD_ACT_BITMASK) {
        return at(static_cast<const uint8_t*>(actions), i);
    } else if constexpr (AFMT == DD_ACT_F32X3) {
        const float* a = &at(static_cast<const float*>(actions), 3 * i);
        return (a[0] != 0.0f ? 1u : 0u) | (a[1] != 0.0f ? 2u : 0u) | (a[2] != 0.0f ? 4u : 0u);
    } else {
        const uint8_t* a = &at(static_cast<const uint8_t*>(actions), 3 * i);
        return (a[0] ? 1u : 0u) | (a[1] ? 2u : 0u) | (a[2] ? 4u : 0u);
    }
}

}  // namespace dd
