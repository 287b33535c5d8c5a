// step_fast.hip — dd_step's kernel for the headline shape (bench.py's config 3:
// reference physics, engine reward, bitmask actions, in place, auto-reset with
// both random spawns, the [N, 15] row every frame, whole 256-lane tiles, no
// done_idx).  The lane's work is step_tile.h's, shared with the generic
// kernels of step.hip; here every launch-uniform switch of that shape is a
// compile-time constant, so the kernel neither loads nor tests them, and every
// lane loads `episode` with its state (kFastLoadsEpisode).  step.hip's
// step_chunks picks it per chunk (step_tile.h, step_variant_of); spawn ranges
// and the seed still come from the call.
//
// Its own translation unit: step.hip's device code is the 72-kernel matrix and
// nothing else.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dronestep.h"
#include "step_tile.h"

namespace dd {

// `episode` loaded by every lane with the rest of the state: the re-spawn (in
// ~35 % of config 3's waves) then starts its Philox block without a second
// memory round trip.  4 B per lane more read than the generic kernel, which
// pays up to 262,144 lanes only: step_variant_of keeps larger batches off
// this kernel (step_tile.h, kStepFastMaxLanes).
constexpr bool kFastLoadsEpisode = true;

template <typename T>
__global__ __launch_bounds__(kStepBlock) void step_fast_kernel(StepArgs p, Soa<T> a) {
    step_tile<T, DD_ACT_BITMASK, true, kShapeNone, false, true, kFastLoadsEpisode>(p, a, a);
}

template <typename T>
void launch_step_fast(const StepArgs& p, const Soa<T>& a, hipStream_t s) {
    const unsigned blocks = (unsigned)(p.n / kStepBlock);  // whole tiles (step_variant_of)
    hipLaunchKernelGGL((step_fast_kernel<T>), dim3(blocks), dim3(kStepBlock), 0, s, p, a);
}

template void launch_step_fast<float>(const StepArgs&, const Soa<float>&, hipStream_t);
template void launch_step_fast<double>(const StepArgs&, const Soa<double>&, hipStream_t);

}  // namespace dd
