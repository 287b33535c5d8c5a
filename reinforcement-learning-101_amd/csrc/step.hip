// step.hip — dd_step: one frame for every drone, its kernels (in place and
// ping-pong) and its entry point.  The frame itself is frame.h's, shared with
// the rollout kernels (rollout.hip: the design notes on the frame's shape) and
// the fused policy rollout; the lane loads and stores are lane_io.h's.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared
// (-ffp-contract=off keeps every a*b+c as the reference's two roundings.)

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
template <typename T>
struct Raw {
    T x, y, vx, vy, angle, omega, fuel, px, py, total;
    uint32_t status, act;
    int32_t steps;
};

template <typename T, int AFMT>
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
template <typename T, bool kRef, int kShape, bool kPP>
__device__ __forceinline__ bool finish_lane(const StepArgs& p, const Soa<T>& a, const Soa<T>& o, uint32_t i,
                                            const Raw<T>& r, float* orow) {
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
        if (sw.auto_reset) {  // next-step reset: fresh episode, reward 0, done 0
            s.episode = at(a.episode, i);
            spawn(sw, k.c.max_fuel, a.env_id_base + i, s);
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
            if (p.obs) observe(k, s, orow);  // rows as every other path writes them
        }
        ended = (s.status & DD_ST_DONE) != 0;
    }
    // State stores after the branches merge, so each is one SGPR-base +
    // lane-offset store (stores inside the branches got 64-bit per-lane
    // addresses, 22 VGPRs live across the frame).  A sticky-done lane
    // writes nothing; status and px only change on the terminal frame, a
    // respawn or a moving platform; py and episode only on a respawn.
    // (with separate out arrays a sticky lane copies its fields across)
    const bool sticky = (r.status & DD_ST_DONE) && !respawned && !kPP;
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
        if (p.obs && ((r.status & DD_ST_DONE) != 0)) observe(k, s, orow);  // the live path wrote its row
    } else {
        if (p.obs) observe(k, s, orow);
    }
    return ended;
}

// One step tile: one drone per lane, kStepBlock lanes.  `o` is `a` unless kPP.
template <typename T, int AFMT, bool kRef, int kShape, bool kPP>
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
    if (i < (uint32_t)p.n) load_raw<T, AFMT>(a, p.actions, i, r);
    const bool ended = i < (uint32_t)p.n &&
                       finish_lane<T, kRef, kShape, kPP>(p, a, o, i, r, tile + threadIdx.x * DD_OBS_DIM);
    if (p.done_idx) {  // wave-ballot compaction of the lanes that just ended
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
    if (p.obs) {  // each wave's 64 rows leave as 16-byte stores
        const uint32_t wrow0 = row0 + (threadIdx.x & ~(kWave - 1));
        const float* wtile = tile + (threadIdx.x & ~(kWave - 1)) * DD_OBS_DIM;
        float* dst = p.obs + (size_t)wrow0 * DD_OBS_DIM;
        // every wave but a ragged batch's last has all 64 rows: the unrolled flush (lane_io.h)
        if (wrow0 + kWave <= (uint32_t)p.n && (reinterpret_cast<uintptr_t>(p.obs) & 15u) == 0) {
            flush_obs_wave_full(wtile, dst);
        } else {
            const int rows = (int)min((int64_t)kWave, max((int64_t)0, (int64_t)p.n - wrow0));
            flush_obs_wave(wtile, dst, rows);
        }
    }
}

// dd_step kernel, in place (the usual case: one set of state bases).
template <typename T, int AFMT, bool kRef, int kShape>
__global__ __launch_bounds__(kStepBlock) void step_kernel(StepArgs p, Soa<T> a) {
    step_tile<T, AFMT, kRef, kShape, false>(p, a, a);
}

// dd_step kernel with ping-pong state (DDStepIO.state_out): its own
// instantiation, so the in-place kernel carries none of its plumbing (the
// shared kernel's `if (!ping_pong) o = a` had cost config 3 ~0.1 us).
template <typename T, int AFMT, bool kRef, int kShape>
__global__ __launch_bounds__(kStepBlock) void step_pp_kernel(StepArgs p, Soa<T> a, Soa<T> o) {
    step_tile<T, AFMT, kRef, kShape, true>(p, a, o);
}

#ifdef DD_ISA_PROBE
// tools/lab/isa_probe.sh: one kernel instantiation alone (device assembly in
// seconds instead of the whole library's minutes), for reading its ISA.
#define DD_PROBE_KERNEL_(k) template __global__ void k;
DD_PROBE_KERNEL_(DD_ISA_PROBE)
}  // namespace dd
#else
// ---------------------------------------------------------------------------
// Host side: argument checks, chunking and launches.
// ---------------------------------------------------------------------------
template <typename T, int AFMT, bool kRef, int kShape>
void launch_step(const StepArgs& p, const Soa<T>& a, const Soa<T>* o, hipStream_t s) {
    const unsigned blocks = (unsigned)((p.n + kStepBlock - 1) / kStepBlock);
    if (o)
        hipLaunchKernelGGL((step_pp_kernel<T, AFMT, kRef, kShape>), dim3(blocks), dim3(kStepBlock), 0, s, p, a, *o);
    else
        hipLaunchKernelGGL((step_kernel<T, AFMT, kRef, kShape>), dim3(blocks), dim3(kStepBlock), 0, s, p, a);
}

template <typename T>
void step_chunks(StepArgs p, const DDState& st, const DDStepIO& io, int64_t n, hipStream_t s) {
    const bool ref = uses_reference_physics(p.k.c);
    const int shape = shape_of(io.shaped_mode, io.shaped_hist, io.shaped_reward);
    const int64_t act_w = action_bytes(io.action_format);
    for_each_chunk(n, [&](int64_t first, int64_t len) {
        p.actions = static_cast<const char*>(io.actions) + first * act_w;
        p.reward = static_cast<T*>(io.reward) + first;
        p.done = io.done + first;
        p.obs = io.obs ? io.obs + first * DD_OBS_DIM : nullptr;
        p.n = (int32_t)len;
        p.idx_base = (int32_t)first;
        p.shaped_hist = shape == kShapePpo ? io.shaped_hist + first : nullptr;
        p.hist_stride = n;
        p.shaped_reward = shape != kShapeNone ? static_cast<void*>(static_cast<T*>(io.shaped_reward) + first) : nullptr;
        p.shaped_done = shape != kShapeNone ? io.shaped_done + first : nullptr;
        p.max_steps = io.max_steps;
        const Soa<T> a = soa_of<T>(st, first);
        Soa<T> o;
        if (io.state_out) o = soa_of<T>(*io.state_out, first);
        with_bool(ref, [&](auto r) {
            with_value<kShapeNone, kShapePpo, kShapeReinforce>(shape, [&](auto sh) {
                with_value<DD_ACT_BITMASK, DD_ACT_F32X3, DD_ACT_U8X3>(io.action_format, [&](auto fmt) {
                    launch_step<T, decltype(fmt)::value, decltype(r)::value, decltype(sh)::value>(
                        p, a, io.state_out ? &o : nullptr, s);
                });
            });
        });
    });
}

}  // namespace dd

extern "C" {

int dd_step(const DDConfig* cfg, const DDState* st, const DDStepIO* io, int64_t n, void* stream) {
    if (!cfg || !io || !st || n < 0 || n > INT32_MAX) return hipErrorInvalidValue;
    if (io->action_format < DD_ACT_BITMASK || io->action_format > DD_ACT_U8X3) return hipErrorInvalidValue;
    if (st->precision != DD_F32 && st->precision != DD_F64) return hipErrorInvalidValue;
    if (io->done_idx && !io->done_count) return hipErrorInvalidValue;
    if (io->shaped_mode == DD_SHAPED_REINFORCE) {  // no history: shaped_hist is not read
        if (!io->shaped_reward || !io->shaped_done) return hipErrorInvalidValue;
    } else if (io->shaped_mode == DD_SHAPED_PPO) {
        const int ptrs = (io->shaped_hist != nullptr) + (io->shaped_reward != nullptr) + (io->shaped_done != nullptr);
        if (ptrs != 0 && ptrs != 3) return hipErrorInvalidValue;
    } else {
        return hipErrorInvalidValue;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (io->done_count) {
        const hipError_t e = hipMemsetAsync(io->done_count, 0, sizeof(int32_t), s);
        if (e != hipSuccess) return (int)e;
    }
    if (n == 0) return 0;  // empty batch: pointers may be null
    if (!dd::state_ok(st) || !io->actions || !io->reward || !io->done) return hipErrorInvalidValue;
    if (const DDState* so = io->state_out) {  // ping-pong: the shared fields, distinct per-frame arrays
        if (!dd::state_ok(so) || so->precision != st->precision || so->env_id_base != st->env_id_base ||
            so->px != st->px || so->py != st->py || so->status != st->status || so->episode != st->episode)
            return hipErrorInvalidValue;
        const void* in[9] = {st->x, st->y, st->vx, st->vy, st->angle, st->omega, st->fuel, st->total_reward,
                             st->steps};
        const void* out[9] = {so->x, so->y, so->vx, so->vy, so->angle, so->omega, so->fuel, so->total_reward,
                              so->steps};
        for (int q = 0; q < 9; ++q)
            if (in[q] == out[q]) return hipErrorInvalidValue;
    }
    dd::StepArgs p{};
    p.k = dd::make_consts(*cfg);
    p.done_idx = io->done_idx;
    p.done_count = io->done_count;
    dd::with_storage(st->precision, [&](auto tag) { dd::step_chunks<decltype(tag)>(p, *st, *io, n, s); });
    return dd::finish();
}

int64_t dd_step_bytes_per_env(int32_t precision, int32_t action_format, int32_t with_obs) {
    const int64_t f = precision == DD_F64 ? 8 : 4;
    const int64_t act = dd::action_bytes(action_format);
    // reads: x y vx vy angle omega fuel px py total (10 f) + status 1 + steps 4 + action
    const int64_t rd = 10 * f + 1 + 4 + act;
    // writes: x y vx vy angle omega fuel total reward (9 f) + steps 4 + done 1
    // (status is rewritten only on the frame an episode ends)
    const int64_t wr = 9 * f + 4 + 1;
    return rd + wr + (with_obs ? DD_OBS_DIM * 4 : 0);
}

}  // extern "C"
#endif  // DD_ISA_PROBE
