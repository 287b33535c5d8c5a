// step_tile.h — one dd_step tile: a lane's loads, its frame (or sticky done /
// auto reset), its stores and the observation flush.  Shared by the generic
// kernels (step.hip: 72 instantiations over storage, action format, physics,
// reward shape and ping-pong) and the headline shape's kernel (step_fast.hip),
// so there is one copy of the lane's work.  Also the host's choice between the
// two families (step_variant_of).
//
// kFast hard-wires the switches that are launch-uniform and never change over
// a run of the headline shape: auto_reset and both spawn switches on, obs
// present and 16-byte aligned, no done_idx, n a multiple of kStepBlock (no
// `i < n` test, every wave's flush the unrolled one).  With kFast = false each
// of them is read from the call as before.  kEpisode (kFast only): every lane
// loads `episode` with the rest of its state, so a re-spawn needs no second
// memory round trip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dronestep.h"
#include "frame.h"
#include "lane_io.h"
#include "launch.h"
#include "trig.h"

namespace dd {

// ---------------------------------------------------------------------------
// dd_step kernel: one 256-lane tile per block, one chunk of lanes per launch.
// ---------------------------------------------------------------------------
struct StepArgs {
    Consts k;              // runtime constants (switches, spawn; physics when !kRef)
    const void* actions;   // chunk-relative
    void* reward;
    uint8_t* done;
    float* obs;
    int32_t* done_idx;
    int32_t* done_count;
    int32_t n;             // lanes in this chunk
    int32_t idx_base;      // chunk start, for done_idx entries
    double* shaped_hist;   // slot 0 of this chunk; slot 1 at + hist_stride
    int64_t hist_stride;
    void* shaped_reward;
    uint8_t* shaped_done;
    int32_t max_steps;
};

// 256 lanes per block: 128 / 512 / 1024 measured +0 / +4 / +14 % at 262,144
// drones; no occupancy floor (forcing 8 waves per SIMD spilled).
constexpr int kStepBlock = 256;

// A lane's inputs as loaded (storage width), before widening to double.
// (episode: loaded only by the kernels that ask for it, load_raw's kEpisode)
template <typename T>
struct Raw {
    T x, y, vx, vy, angle, omega, fuel, px, py, total;
    uint32_t status, act;
    int32_t steps, episode;
};

template <typename T, int AFMT, bool kEpisode = false>
__device__ __forceinline__ void load_raw(const Soa<T>& a, const void* actions, uint32_t i, Raw<T>& r) {
    // The action is loaded first and pinned below: only the live branch reads
    // it, and left to itself the compiler sank its load into that branch,
    // i.e. behind the wait for the status byte: a second memory round trip.
    r.act = load_action<AFMT>(actions, i);
    r.x = at(a.x, i); r.y = at(a.y, i); r.vx = at(a.vx, i); r.vy = at(a.vy, i);
    r.angle = at(a.angle, i); r.omega = at(a.omega, i); r.fuel = at(a.fuel, i);
    r.px = at(a.px, i); r.py = at(a.py, i); r.total = at(a.total, i);
    r.status = at(a.status, i);
    r.steps = at(a.steps, i);
    if constexpr (kEpisode) r.episode = at(a.episode, i);
    asm volatile("" ::"v"(r.act));  // every load is issued; this waits for the oldest only
}

// Everything after the loads for one lane: the frame (or sticky done / auto
// reset), the state and output stores, the observation row into `orow`
// (LDS).  Returns whether the lane's episode ended in this call.  The fast
// frame may report the lane risky (frame.h): then, in a wave-uniform rare
// branch, the lane's frame is redone at once from its loaded inputs with
// kExact (glibc's sin, cos and pow), and the rest of the lane's work is
// shared.  (Until round 6 a second finish_lane pass over the risky lanes
// redid everything after the loads: the same results, but that copy of the
// observation, reward and store code cost config 3 1-2 % in time and ~110
// instruction-wait cycles per wave, profiles/r06/lab/step_inline_exact.jsonl.)
// kShape: the notebooks' reward fused (frame.h, kShapePpo / kShapeReinforce).
// kPP (ping-pong, DDStepIO.state_out): the nine per-frame fields (x y vx vy
// angle omega fuel total steps) go to `o`; px, py, status and episode always
// go to `a`.  In place (the usual case) the kernel has no `o` at all.
template <typename T, bool kRef, int kShape, bool kPP, bool kFast = false, bool kEpisode = false>
__device__ __forceinline__ bool finish_lane(const StepArgs& p, const Soa<T>& a, const Soa<T>& o, uint32_t i,
                                            const Raw<T>& r, float* orow) {
    static_assert(!kFast || (kRef && kShape == kShapeNone && !kPP), "the headline shape: kRef, engine reward, in place");
    static_assert(!kEpisode || kFast, "only the headline kernel loads episode with the state");
    const DDConfig& sw = p.k.c;
    const Consts& k = kRef ? kRefConsts : p.k;
    Lane s;
    s.x = r.x; s.y = r.y; s.vx = r.vx; s.vy = r.vy; s.angle = r.angle; s.omega = r.omega;
    s.fuel = r.fuel; s.px = r.px; s.py = r.py; s.total = r.total;
    s.status = r.status;
    s.steps = r.steps;
    bool ended = false;
    bool respawned = false;
    double reward;
    double shaped = 0.0;
    bool shaped_done = false;
    if (s.status & DD_ST_DONE) {
        reward = 0.0;
        if (kFast || sw.auto_reset) {  // next-step reset: fresh episode, reward 0, done 0
            if constexpr (kEpisode) s.episode = r.episode;
            else s.episode = at(a.episode, i);
            spawn<kFast>(sw, k.c.max_fuel, a.env_id_base + i, s);
            respawned = true;
            if constexpr (kShape == kShapePpo) {  // the notebook's history restarts: prev_state None
                at(p.shaped_hist, i) = trig::div_exact(s.dist, k.c.world_width, k.inv_w);
                at(p.shaped_hist + p.hist_stride, i) = __builtin_nan("");
            }
        } else {  // sticky done (game_engine.py:107-111): nothing changes
            measure(s);
            shaped_done = true;
        }
    } else {
        bool rk = false;
        reward = frame<kRef, false>(k, sw, r.act, s, &rk);
        if (__builtin_expect(__ballot(rk) != 0, 0)) {
            if (rk) {  // the frame again from the loaded state, the reference's functions (frame.h)
                s.x = r.x; s.y = r.y; s.vx = r.vx; s.vy = r.vy; s.angle = r.angle; s.omega = r.omega;
                s.fuel = r.fuel; s.px = r.px; s.py = r.py; s.total = r.total; s.status = r.status;
                s.steps = r.steps;
                reward = frame<kRef, false, true>(k, sw, r.act, s, nullptr);
            }
        }
        if constexpr (kShape != kShapeNone) {
            double v[13];
            observe_values<false, true>(k, s, v);  // the notebook reward's doubles: exact quotients
            if constexpr (kShape == kShapePpo) {
                double* slot = p.shaped_hist + (s.steps & 1) * p.hist_stride;  // two frames back
                shaped = notebook_reward(v, s.status, at(slot, i));
                at(slot, i) = v[9];
            } else {
                shaped = reinforce_reward(v, s.status);
            }
            shaped_done = (s.status & DD_ST_DONE) != 0;
            if (p.max_steps > 0 && s.steps >= p.max_steps) {  // the collection loops' timeout
                shaped = (s.status & DD_ST_LANDED) ? shaped : shaped - 500;
                shaped_done = true;
                s.status |= DD_ST_DONE;  // the episode ends here (TimeLimit)
            }
            if (kFast || p.obs) observe(k, s, orow);  // rows as every other path writes them
        }
        ended = (s.status & DD_ST_DONE) != 0;
    }
    // State stores after the branches merge, so each is one SGPR-base +
    // lane-offset store (stores inside the branches got 64-bit per-lane
    // addresses, 22 VGPRs live across the frame).  A sticky-done lane
    // writes nothing; status and px only change on the terminal frame, a
    // respawn or a moving platform; py and episode only on a respawn.
    // (with separate out arrays a sticky lane copies its fields across)
    const bool sticky = !kFast && (r.status & DD_ST_DONE) && !respawned && !kPP;
    if (!sticky) {
        uint32_t j = i;
        asm volatile("" : "+v"(j));  // an offset defined in this block: isel folds it into saddr stores
        store_dynamics(o, j, s);
        put_state(o.steps, j, s.steps);
        put_state(o.total, j, (T)s.total);
        const bool moving = !kRef && sw.platform_moving;
        if (moving || respawned) put_state(a.px, j, (T)s.px);
        if (moving || ended || respawned) put_state(a.status, j, (uint8_t)s.status);
        if (respawned) { put_state(a.py, j, (T)s.py); put_state(a.episode, j, s.episode); }
    }
    put_out(static_cast<T*>(p.reward), i, (T)reward);
    put_out(p.done, i, (uint8_t)((s.status & DD_ST_DONE) ? 1 : 0));
    if constexpr (kShape != kShapeNone) {
        put_out(static_cast<T*>(p.shaped_reward), i, (T)shaped);
        put_out(p.shaped_done, i, (uint8_t)(shaped_done ? 1 : 0));
        if ((kFast || p.obs) && ((r.status & DD_ST_DONE) != 0)) observe(k, s, orow);  // the live path wrote its row
    } else {
        if (kFast || p.obs) observe(k, s, orow);
    }
    return ended;
}

// One step tile: one drone per lane, kStepBlock lanes.  `o` is `a` unless kPP.
template <typename T, int AFMT, bool kRef, int kShape, bool kPP, bool kFast = false, bool kEpisode = false>
__device__ __forceinline__ void step_tile(const StepArgs& p, const Soa<T>& a, const Soa<T>& o) {
    __shared__ __attribute__((aligned(16))) float tile[kStepBlock * DD_OBS_DIM];
    const uint32_t row0 = blockIdx.x * kStepBlock;
    const uint32_t i = row0 + threadIdx.x;
    // The load bases are wanted in SGPRs before the lane test: left to
    // itself the compiler sank their kernarg loads into the `i < n` branch,
    // one scalar-load latency later than the state loads could start.
    asm volatile("" ::"s"(a.x), "s"(a.y), "s"(a.vx), "s"(a.vy), "s"(a.angle), "s"(a.omega), "s"(a.fuel),
                 "s"(a.px), "s"(a.py), "s"(a.total), "s"(a.status), "s"(a.steps), "s"(p.actions));
    Raw<T> r;
    // (kFast: whole tiles only, every lane exists)
    if (kFast || i < (uint32_t)p.n) load_raw<T, AFMT, kEpisode>(a, p.actions, i, r);
    const bool ended = (kFast || i < (uint32_t)p.n) &&
                       finish_lane<T, kRef, kShape, kPP, kFast, kEpisode>(p, a, o, i, r, tile + threadIdx.x * DD_OBS_DIM);
    if (!kFast && p.done_idx) {  // wave-ballot compaction of the lanes that just ended
        const uint64_t m = __ballot(ended);
        if (m) {
            const int lane = threadIdx.x & (kWave - 1);
            const int leader = __ffsll((unsigned long long)m) - 1;
            const int before = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                         __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
            int b = 0;
            if (lane == leader) b = atomicAdd(p.done_count, __popcll(m));
            b = __shfl(b, leader);
            if (ended) p.done_idx[b + before] = p.idx_base + (int32_t)i;
        }
    }
    if (kFast || p.obs) {  // each wave's 64 rows leave as 16-byte stores
        const uint32_t wrow0 = row0 + (threadIdx.x & ~(kWave - 1));
        const float* wtile = tile + (threadIdx.x & ~(kWave - 1)) * DD_OBS_DIM;
        float* dst = p.obs + (size_t)wrow0 * DD_OBS_DIM;
        // every wave but a ragged batch's last has all 64 rows: the unrolled flush (lane_io.h)
        if (kFast || (wrow0 + kWave <= (uint32_t)p.n && (reinterpret_cast<uintptr_t>(p.obs) & 15u) == 0)) {
            flush_obs_wave_full(wtile, dst);
        } else {
            const int rows = (int)min((int64_t)kWave, max((int64_t)0, (int64_t)p.n - wrow0));
            flush_obs_wave(wtile, dst, rows);
        }
    }
}

// ---------------------------------------------------------------------------
// Host side: which kernel family a chunk takes.
// ---------------------------------------------------------------------------
enum { kStepGeneric = 0, kStepFast = 1 };  // dd_step_variant's values (dronestep.h DD_STEP_*)

// Most lanes a chunk may have and still take the headline kernel.  Its
// `episode` load (4 B per lane more than the generic kernel reads) gained
// 1.1 % (f32) and 3.1 % (f64) on top of the switches at 262,144 lanes and lost
// 3 % at 524,288, more beyond (profiles/r17/lab/): larger
// batches keep the generic kernel and its traffic.
constexpr int64_t kStepFastMaxLanes = int64_t(1) << 18;

// The family of the chunk [first, first + len) of a dd_step call: the
// headline kernel only for the shape it hard-wires (above), anything else the
// generic matrix.
inline int step_variant_of(const DDConfig& c, const DDStepIO& io, int shape, bool ref, int64_t first, int64_t len) {
    if (!ref || shape != kShapeNone || io.action_format != DD_ACT_BITMASK) return kStepGeneric;
    if (io.state_out || io.done_idx || io.shaped_hist || io.shaped_reward || io.shaped_done) return kStepGeneric;
    if (!c.auto_reset || !c.randomize_drone || !c.randomize_platform) return kStepGeneric;
    if (!io.obs || (reinterpret_cast<uintptr_t>(io.obs + first * DD_OBS_DIM) & 15u) != 0) return kStepGeneric;
    if (len <= 0 || len % kStepBlock != 0 || len > kStepFastMaxLanes) return kStepGeneric;
    return kStepFast;
}

// The headline kernel's launch (step_fast.hip); p and a as launch_step's.
template <typename T>
void launch_step_fast(const StepArgs& p, const Soa<T>& a, hipStream_t s);

}  // namespace dd
