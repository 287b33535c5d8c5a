// step.hip — dd_step: one frame for every drone, its generic kernels (in
// place and ping-pong) and its entry point.  The tile (a lane's loads, frame,
// stores and observation flush) is step_tile.h's, shared with the headline
// shape's kernel (step_fast.hip), which step_chunks picks per chunk.  The
// frame itself is frame.h's, shared with the rollout kernels (rollout.hip:
// the design notes on the frame's shape) and the fused policy rollout; the
// lane loads and stores are lane_io.h's.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared
// (-ffp-contract=off keeps every a*b+c as the reference's two roundings.)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dronestep.h"
#include "frame.h"
#include "lane_io.h"
#include "launch.h"
#include "step_tile.h"
#include "trig.h"

namespace dd {

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
        if (step_variant_of(p.k.c, io, shape, ref, first, len) == kStepFast) {
            launch_step_fast<T>(p, a, s);
            return;
        }
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

int32_t dd_step_variant(const DDConfig* cfg, const DDState* st, const DDStepIO* io, int64_t n) {
    if (!cfg || !st || !io || n < 0 || n > INT32_MAX) return -1;
    const int64_t len = n < dd::kChunk ? n : dd::kChunk;
    return dd::step_variant_of(*cfg, *io, dd::shape_of(io->shaped_mode, io->shaped_hist, io->shaped_reward),
                               dd::uses_reference_physics(*cfg), 0, len);
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
