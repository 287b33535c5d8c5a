// mlp_backward.hip — the parameter gradients of the notebooks' policy / value
// network (DroneGamerBoi / DroneTeacherBoi, Actor_Critic_PPO.ipynb:376-424)
// from the gradient at its output: what loss.backward() leaves in every
// parameter's .grad when autograd starts from grad_out at the last Linear's
// output (for the actor the pre-Sigmoid logits, so there is no Sigmoid here;
// dd_ppo_losses' grad_logits / grad_values are exactly that), and the notebook's
// clip_grad_norm_ on them.  Float32 on v_mfma_f32_32x32x2_f32, reading the plain
// float32 parameters (DDMlpParams), whatever the forward's compute.
//
// The mathematics, per layer L of  Linear LayerNorm ReLU  (a = the layer's
// input, N = its width; the last Linear(64, K) has no LayerNorm and no ReLU):
//   forward    h = W a + b
//              xh = (h - mean h) rstd,  rstd = 1 / sqrt(var_biased(h) + eps)
//              y = gamma xh + beta
//              a' = max(y, 0)
//   backward   dy = da' [y > 0]                  (strict, as torch's ReLU)
//              dgamma = sum_rows dy xh           dbeta = sum_rows dy
//              g = dy gamma
//              dh = rstd (g - mean(g) - xh mean(g xh))
//              dW = sum_rows dh (x) a            db = sum_rows dh
//              da = W^T dh
//   last layer dW9 = sum_rows dz (x) a3,  db9 = sum_rows dz,  da3 = W9^T dz.
//
// Decomposition.  kGradBlocks blocks of 4 waves; a block
// takes the 128-row tiles b, b + kGradBlocks, ... (by m alone), each wave 32
// rows of the tile.
//   * Data path, per wave, in registers: the forward is recomputed (no
//     activation is ever stored for all m rows) in the forward kernel's own
//     orientation, out^T[hidden][row] = W . in^T: the accumulator holds the row
//     on lane & 31 and 16 hidden units per tile in its registers, which is the
//     next MFMA's B operand as it stands once the weights' k order is permuted
//     to match (hid()).  da = W^T dh is the same product with the layer's
//     dimensions swapped: dh, in that same layout, is the B operand, W^T the A
//     operand.  LayerNorm and its backward reduce over registers and the other
//     lane half.  xh of the three layers (160 registers) stays live from the
//     forward to the backward; the activations are recomputed from it.
//   * The A operands stream from L2: the five weight images (W0, W3, W6 for
//     the forward, W6^T, W3^T for da), 200 KB in MFMA fragment order, are
//     written into the workspace by a pack kernel at the start of every call
//     and read as 16-byte fragments, one k-step group ahead of its MFMAs.  LDS
//     cannot hold them next to the transposition buffers below.
//   * dW = dh . a^T contracts over rows, which sit on the lanes: both operands
//     go through LDS as [row][hidden] images (odd strides: the b32 writes of a
//     32-lane half hit 32 banks), and are read back with the hidden index on
//     the lane, the row as k.  One layer at a time, two images of 128 x 129
//     floats (132 KB), then the same space again for dy and xh, whose column
//     sums are dbeta and dgamma.  The 28 dW tiles of the network are spread
//     over the four waves, 7 accumulator tiles each, which live in registers
//     across all of the block's row tiles.  The vector gradients are column
//     sums over the images by VALU (a thread per column and row quarter / half).
//   * Determinism: every block writes one partial gradient set; dd_mlp_backward's
//     finish kernel adds the kGradBlocks partials of each element in block
//     order in double and rounds once; the squared norm is summed in double over
//     a fixed tree.  No atomics.  Rows past m load zeros for grad_out, and
//     every contribution of such a row is an exact zero.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "batch_core.h"
#include "dronestep.h"
#include "launch.h"
#include "mlp_backward_core.h"

namespace dd {
namespace mlpbwd {

__global__ __launch_bounds__(256) void pack_kernel(DDMlpParams p, float* __restrict__ packed) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= kPackedB) return;
    packed[idx] = packed_value(p, idx);
}

template <int K>
__global__ __launch_bounds__(kThreadsB) void backward_kernel(DDMlpParams p, const float* __restrict__ states,
                                                            const float* __restrict__ grad_out, int64_t m,
                                                            const float* __restrict__ packed,
                                                            float* __restrict__ part) {
    extern __shared__ float lds[];
    backward_block<K>(p, states, grad_out, m, packed, part + (int64_t)blockIdx.x * kPartStride, blockIdx.x,
                      kGradBlocks, lds);
}

// Where element e of the flat gradient vector goes.
__device__ __forceinline__ float* slot_of(const DDMlpGrads& g, int e, int k) {
    float* const ptr[14] = {g.w0, g.b0, g.ln1_w, g.ln1_b, g.w3, g.b3, g.ln4_w, g.ln4_b,
                            g.w6, g.b6, g.ln7_w, g.ln7_b, g.w9, g.b9};
    const int start[15] = {oW0, oB0, oG1, oE1, oW3, oB3, oG4, oE4, oW6, oB6, oG7, oE7, oW9, oW9 + 64 * k, params_of(k)};
    int s = 0;
#pragma unroll
    for (int i = 1; i < 14; ++i) s += e >= start[i] ? 1 : 0;
    float* base = ptr[0];
#pragma unroll
    for (int i = 1; i < 14; ++i) base = s == i ? ptr[i] : base;
    int first = 0;
#pragma unroll
    for (int i = 1; i < 14; ++i) first = s == i ? start[i] : first;
    return base + (e - first);
}

// Each element: the kGradBlocks partials in block order, in double, rounded
// once; the block's share of the squared norm of the rounded gradients.
__global__ __launch_bounds__(kBlock) void sum_kernel(const float* __restrict__ part, DDMlpGrads g, int k,
                                                     double* __restrict__ norm_part) {
    __shared__ double sh[kBlock];
    const int e = blockIdx.x * kBlock + threadIdx.x;
    double sq = 0.0;
    if (e < params_of(k)) {
        double s = 0.0;
        for (int b = 0; b < kGradBlocks; ++b) s += (double)part[(int64_t)b * kPartStride + e];
        const float f = (float)s;
        *slot_of(g, e, k) = f;
        sq = (double)f * (double)f;
    }
    sq = block_sum<double>(sq, sh);
    if (threadIdx.x == 0) norm_part[blockIdx.x] = sq;
}

// The norm from the sum kernel's partials (every block the same tree), and
// clip_grad_norm_'s scaling.
__global__ __launch_bounds__(kBlock) void clip_kernel(const double* __restrict__ norm_part, DDMlpGrads g, int k,
                                                      double max_norm, bool clip, double* __restrict__ grad_norm) {
    __shared__ double sh[kBlock];
    const double total = block_sum<double>(threadIdx.x < kFinishBlocks ? norm_part[threadIdx.x] : 0.0, sh);
    const double norm = sqrt(total);
    if (blockIdx.x == 0 && threadIdx.x == 0 && grad_norm) *grad_norm = norm;
    if (!clip) return;
    const double coef = clip_coef(max_norm, norm);
    if (coef == 1.0) return;
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e < params_of(k)) {
        float* q = slot_of(g, e, k);
        *q = (float)((double)*q * coef);
    }
}

}  // namespace mlpbwd
}  // namespace dd

extern "C" {

int64_t dd_mlp_backward_workspace(void) { return dd::mlpbwd::kWorkspaceBytes; }

int dd_mlp_backward(const DDMlpParams* params, const DDMlpBackwardIO* io, int64_t m, void* workspace, void* stream) {
    using namespace dd::mlpbwd;
    if (!params || !io || m < 0) return hipErrorInvalidValue;
    if (params->out_dim != 1 && params->out_dim != 3) return hipErrorInvalidValue;
    const float* const src[14] = {params->w0, params->b0, params->ln1_w, params->ln1_b, params->w3, params->b3,
                                  params->ln4_w, params->ln4_b, params->w6, params->b6, params->ln7_w, params->ln7_b,
                                  params->w9, params->b9};
    float* const dst[14] = {io->grads.w0, io->grads.b0, io->grads.ln1_w, io->grads.ln1_b, io->grads.w3, io->grads.b3,
                            io->grads.ln4_w, io->grads.ln4_b, io->grads.w6, io->grads.b6, io->grads.ln7_w,
                            io->grads.ln7_b, io->grads.w9, io->grads.b9};
    for (int i = 0; i < 14; ++i)
        if (!src[i] || !dst[i]) return hipErrorInvalidValue;
    if (m > 0 && (!io->states || !io->grad_out || !workspace)) return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) return hipErrorInvalidValue;  // 16-byte weight fragments
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int k = params->out_dim;
    if (m == 0) {  // no rows: zeros and a zero norm
        const int count[14] = {128 * 15, 128, 128, 128, 128 * 128, 128, 128, 128, 64 * 128, 64, 64, 64, 64 * k, k};
        for (int i = 0; i < 14; ++i) {
            const hipError_t e = hipMemsetAsync(dst[i], 0, count[i] * sizeof(float), s);
            if (e != hipSuccess) return (int)e;
        }
        if (io->grad_norm) return (int)hipMemsetAsync(io->grad_norm, 0, sizeof(double), s);
        return 0;
    }
    double* norm_part = static_cast<double*>(workspace);
    float* packed = reinterpret_cast<float*>(static_cast<char*>(workspace) + kNormBytes);
    float* part = packed + kPackedB;
    const bool clip = io->max_norm > 0.0 && __builtin_isfinite(io->max_norm);
    hipLaunchKernelGGL(pack_kernel, dim3((kPackedB + 255) / 256), dim3(256), 0, s, *params, packed);
    return dd::with_value<1, 3>(k, [&](auto kk) {
        constexpr int K = decltype(kk)::value;
        // the LDS images exceed the 64 KB default; the attribute is per device, so it is set on every launch
        const hipError_t e = hipFuncSetAttribute((const void*)backward_kernel<K>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsB);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(backward_kernel<K>, dim3(kGradBlocks), dim3(kThreadsB), kLdsB, s, *params, io->states,
                           io->grad_out, m, (const float*)packed, part);
        hipLaunchKernelGGL(sum_kernel, dim3(kFinishBlocks), dim3(dd::kBlock), 0, s, (const float*)part, io->grads, K,
                           norm_part);
        hipLaunchKernelGGL(clip_kernel, dim3(kFinishBlocks), dim3(dd::kBlock), 0, s, (const double*)norm_part,
                           io->grads, K, io->max_norm, clip, io->grad_norm);
        return dd::finish();
    });
}

}  // extern "C"
