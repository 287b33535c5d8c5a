// mlp_backward_core.h — dd_mlp_backward's device code (mlp_backward.hip has
// the mathematics and the decomposition): the flat gradient layout, the packed
// weight images, and one block's whole pass over its row tiles.  Shared with
// the fused PPO update (ppo_fused.hip), which runs the same body on its one
// tile, so both produce the same bits.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "batch_core.h"
#include "dronestep.h"
#include "launch.h"
#include "mlp_core.h"

namespace dd {
namespace mlpbwd {

using mlp::add_other_half;
using mlp::f32x16;
using mlp::f32x4;
using mlp::hid;

constexpr int kGradBlocks = 256;  // fixed: the partial sums' grouping does not depend on the device
constexpr int kWavesB = 4;
constexpr int kThreadsB = kWavesB * 64;
constexpr int kTileRows = kWavesB * 32;
static_assert(kThreadsB == kBlock, "block_sum's width");

// The flat gradient vector: the fourteen tensors in DDMlpParams' order.
constexpr int oW0 = 0, oB0 = oW0 + 128 * 15, oG1 = oB0 + 128, oE1 = oG1 + 128;
constexpr int oW3 = oE1 + 128, oB3 = oW3 + 128 * 128, oG4 = oB3 + 128, oE4 = oG4 + 128;
constexpr int oW6 = oE4 + 128, oB6 = oW6 + 64 * 128, oG7 = oB6 + 64, oE7 = oG7 + 64;
constexpr int oW9 = oE7 + 64;
__host__ __device__ constexpr int params_of(int k) { return oW9 + 65 * k; }
constexpr int kPartStride = (params_of(3) + 15) / 16 * 16;
constexpr int kFinishBlocks = (params_of(3) + kBlock - 1) / kBlock;
static_assert(kFinishBlocks <= kBlock, "one thread per norm partial");

// Workspace: the finish kernels' norm partials (doubles), the packed weight
// images, the blocks' partial gradient sets.
constexpr int pA1 = 0;                   // W0   [4 tiles][8 k-steps]   k = 2q + h (column 15 zero)
constexpr int pA2 = pA1 + 4 * 8 * 64;    // W3   [4][64]                k = hid(q >> 4, q & 15, h)
constexpr int pA3 = pA2 + 4 * 64 * 64;   // W6   [2][64]
constexpr int pA3T = pA3 + 2 * 64 * 64;  // W6^T [4][32]
constexpr int pA2T = pA3T + 4 * 32 * 64; // W3^T [4][64]
constexpr int kPackedB = pA2T + 4 * 64 * 64;
constexpr int64_t kNormBytes = 256 * sizeof(double);
constexpr int64_t kWorkspaceBytes =
    kNormBytes + (int64_t)(kPackedB + (int64_t)kGradBlocks * kPartStride) * (int64_t)sizeof(float);

// LDS: two [128][129] images, the vectors, the tile's grad_out rows.
constexpr int kStrideW = 129, kStrideN = 65, kStrideX = 17;
constexpr int lA = 0, lB = lA + kTileRows * kStrideW, lVec = lB + kTileRows * kStrideW;
constexpr int vB0 = 0, vG1 = 128, vE1 = 256, vB3 = 384, vG4 = 512, vE4 = 640, vB6 = 768, vG7 = 832, vE7 = 896;
constexpr int vW9 = 960, vEnd = vW9 + 3 * 64;
constexpr int lDz = lVec + vEnd, lEnd = lDz + kTileRows * 4;
constexpr size_t kLdsB = (size_t)lEnd * sizeof(float);
static_assert(kLdsB <= 160 * 1024, "LDS of one CU");
static_assert(15 * kThreadsB <= lVec, "the final combine reuses the images");

// Element idx of the packed images.
__device__ __forceinline__ float packed_value(const DDMlpParams& p, int idx) {
    int base, steps;
    const float* w;
    bool transposed = false;
    if (idx < pA2) { base = pA1; steps = 8; w = p.w0; }
    else if (idx < pA3) { base = pA2; steps = 64; w = p.w3; }
    else if (idx < pA3T) { base = pA3; steps = 64; w = p.w6; }
    else if (idx < pA2T) { base = pA3T; steps = 32; w = p.w6; transposed = true; }
    else { base = pA2T; steps = 64; w = p.w3; transposed = true; }
    const int e = idx - base, j = e & 3, lane = (e >> 2) & 63, rest = e >> 8;
    const int g = rest % (steps / 4), t = rest / (steps / 4), q = 4 * g + j, h = lane >> 5;
    const int i = 32 * t + (lane & 31);
    float v;
    if (base == pA1) {
        const int k = 2 * q + h;
        v = k < 15 ? w[i * 15 + k] : 0.0f;
    } else {
        const int k = hid(q >> 4, q & 15, h);
        v = transposed ? w[k * 128 + i] : w[i * 128 + k];
    }
    return v;
}

// acc (NT tiles of 32 outputs x 32 rows) += A . B over STEPS k-steps of 2: the A
// fragments from the packed image (global memory, one group of 4 k-steps
// ahead), bval(q) the lane's B operand of k-step q.
template <int NT, int STEPS, typename BVal>
__device__ __forceinline__ void mfma_stream(const float* image, int lane, BVal bval, f32x16 (&acc)[NT]) {
    const f32x4* a4 = reinterpret_cast<const f32x4*>(image);  // no __restrict__: the fused update rewrites the image
    constexpr int kGroups = STEPS / 4;
    f32x4 next[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) next[t] = a4[(t * kGroups) * 64 + lane];
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
        f32x4 a[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) a[t] = next[t];
        if (g + 1 < kGroups) {
#pragma unroll
            for (int t = 0; t < NT; ++t) next[t] = a4[(t * kGroups + g + 1) * 64 + lane];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float b = bval(4 * g + j);
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t][j], b, acc[t], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// LayerNorm's statistics over the column's 32 NT hidden units: xh and rstd.
template <int NT>
__device__ __forceinline__ void ln_forward(const f32x16 (&acc)[NT], float eps, float (&xh)[NT][16], float& rstd) {
    constexpr float kN = 32.0f * NT;
    float s = 0.0f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) s += acc[t][r];
    const float mean = add_other_half(s) / kN;
    float q = 0.0f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float d = acc[t][r] - mean;
            xh[t][r] = d;
            q = __builtin_fmaf(d, d, q);
        }
    rstd = 1.0f / sqrtf(add_other_half(q) / kN + eps);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) xh[t][r] *= rstd;
}

// a' = max(gamma xh + beta, 0) of hidden unit hid(t, r, h); gb = the layer's
// gamma (LDS), beta follows it.
template <int N>
__device__ __forceinline__ float act_of(float xh, const float* gb, int unit) {
    return fmaxf(__builtin_fmaf(xh, gb[unit], gb[N + unit]), 0.0f);
}

// dh from da' (in dy: masked here by y > 0), LayerNorm's backward; dy keeps the
// masked gradient.
template <int NT>
__device__ __forceinline__ void ln_backward(float (&dy)[NT][16], const float (&xh)[NT][16], float rstd,
                                            const float* gb, int h, float (&dh)[NT][16]) {
    constexpr int N = 32 * NT;
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int unit = hid(t, r, h);
            const bool on = __builtin_fmaf(xh[t][r], gb[unit], gb[N + unit]) > 0.0f;
            dy[t][r] = on ? dy[t][r] : 0.0f;
            const float g = dy[t][r] * gb[unit];
            dh[t][r] = g;
            s1 += g;
            s2 = __builtin_fmaf(g, xh[t][r], s2);
        }
    const float m1 = add_other_half(s1) / (float)N, m2 = add_other_half(s2) / (float)N;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) dh[t][r] = rstd * ((dh[t][r] - m1) - xh[t][r] * m2);
}

// The lane's 16 NT values of its row into a [row][hidden] LDS image.
template <int NT, typename F>
__device__ __forceinline__ void stage(float* image, int stride, int row, int h, F value) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) image[row * stride + hid(t, r, h)] = value(t, r);
}

// clip_grad_norm_'s factor, torch.clamp(max_norm / (norm + 1e-6), max=1.0): a NaN stays.
__device__ __forceinline__ double clip_coef(double max_norm, double norm) {
    const double coef = max_norm / (norm + 1e-6);
    return coef > 1.0 ? 1.0 : coef;
}

// One block's pass: the row tiles first_tile, first_tile + tile_step, ... of the
// m rows, and the block's partial gradient set in the flat layout at out.  lds:
// kLdsB bytes.  Row r's observation is states[r], or with a row map (not
// InPlace) states[where.cell(r)]: reinforce_fused.hip reads a batch's rows in
// place in its frame-major record; grad_out is indexed by r either way.
struct InPlace {};
template <int K, typename Where = InPlace>
__device__ __forceinline__ void backward_block(const DDMlpParams& p, const float* states, const float* grad_out,
                                               int64_t m, const float* packed, float* out, int64_t first_tile,
                                               int64_t tile_step, float* lds, Where where = {}) {
    float* bufA = lds + lA;
    float* bufB = lds + lB;
    float* vec = lds + lVec;
    float* bufZ = lds + lDz;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, c = lane & 31;
    const int trow = wave * 32 + c;  // the lane's row of the block tile
    const float eps = p.ln_eps;

    for (int i = tid; i < 128; i += kThreadsB) {
        vec[vB0 + i] = p.b0[i]; vec[vG1 + i] = p.ln1_w[i]; vec[vE1 + i] = p.ln1_b[i];
        vec[vB3 + i] = p.b3[i]; vec[vG4 + i] = p.ln4_w[i]; vec[vE4 + i] = p.ln4_b[i];
    }
    for (int i = tid; i < 64; i += kThreadsB) {
        vec[vB6 + i] = p.b6[i]; vec[vG7 + i] = p.ln7_w[i]; vec[vE7 + i] = p.ln7_b[i];
    }
    for (int i = tid; i < 3 * 64; i += kThreadsB) vec[vW9 + i] = i < K * 64 ? p.w9[i] : 0.0f;
    __syncthreads();

    // the wave's 7 dW tiles and the thread's column sums, over all of the block's row tiles
    f32x16 accW3[4], accW6[2], accW0[1];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int t = 0; t < 4; ++t) accW3[t][r] = 0.0f;
        accW6[0][r] = accW6[1][r] = accW0[0][r] = 0.0f;
    }
    float sB6 = 0.0f, sG7 = 0.0f, sE7 = 0.0f, sB3 = 0.0f, sG4 = 0.0f, sE4 = 0.0f, sB0 = 0.0f, sG1 = 0.0f, sE1 = 0.0f;
    float sW9[3] = {0.0f, 0.0f, 0.0f}, sB9[3] = {0.0f, 0.0f, 0.0f};
    const int q3 = tid >> 6, j3 = tid & 63;    // 64 columns: a thread per column and row quarter
    const int q2 = tid >> 7, j2 = tid & 127;   // 128 columns: per column and row half
    const int ti6 = wave & 1, tj6 = 2 * (wave >> 1);

    for (int64_t tile = first_tile; tile * kTileRows < m; tile += tile_step) {
        const int64_t row = tile * kTileRows + trow;
        const bool live = row < m;
        float x[8], dz[K];
        if constexpr (std::is_same<Where, InPlace>::value) {
#pragma unroll
            for (int q = 0; q < 8; ++q) x[q] = live && 2 * q + h < 15 ? states[row * 15 + 2 * q + h] : 0.0f;
        } else {
            const int64_t cell = live ? where.cell(row) : 0;
#pragma unroll
            for (int q = 0; q < 8; ++q) x[q] = live && 2 * q + h < 15 ? states[cell * 15 + 2 * q + h] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) dz[k] = live ? grad_out[row * K + k] : 0.0f;

        // ---- forward, keeping xh and rstd of the three LayerNorms --------------
        float xh1[4][16], xh2[4][16], xh3[2][16], rs1, rs2, rs3;
        {
            f32x16 acc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = vec[vB0 + hid(t, r, h)];
            mfma_stream<4, 8>(packed + pA1, lane, [&](int q) { return x[q]; }, acc);
            ln_forward<4>(acc, eps, xh1, rs1);
            float a[4][16];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    a[t][r] = act_of<128>(xh1[t][r], vec + vG1, hid(t, r, h));
                    acc[t][r] = vec[vB3 + hid(t, r, h)];
                }
            mfma_stream<4, 64>(packed + pA2, lane, [&](int q) { return a[q >> 4][q & 15]; }, acc);
            ln_forward<4>(acc, eps, xh2, rs2);
            f32x16 acc2[2];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) a[t][r] = act_of<128>(xh2[t][r], vec + vG4, hid(t, r, h));
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc2[t][r] = vec[vB6 + hid(t, r, h)];
            mfma_stream<2, 64>(packed + pA3, lane, [&](int q) { return a[q >> 4][q & 15]; }, acc2);
            ln_forward<2>(acc2, eps, xh3, rs3);
        }

        // ---- layer 3 and the last Linear ----------------------------------------
        float dy3[2][16], dh3[2][16];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float s = 0.0f;
#pragma unroll
                for (int k = 0; k < K; ++k) s = __builtin_fmaf(vec[vW9 + k * 64 + hid(t, r, h)], dz[k], s);
                dy3[t][r] = s;  // da3 = W9^T dz
            }
        ln_backward<2>(dy3, xh3, rs3, vec + vG7, h, dh3);
        stage<2>(bufA, kStrideN, trow, h, [&](int t, int r) { return dh3[t][r]; });
        stage<4>(bufB, kStrideW, trow, h, [&](int t, int r) { return act_of<128>(xh2[t][r], vec + vG4, hid(t, r, h)); });
        __syncthreads();
#pragma unroll 4
        for (int ks = 0; ks < kTileRows / 2; ++ks) {  // dW6 = dh3 . a2^T
            const int k = 2 * ks + h;
            const float a = bufA[k * kStrideN + 32 * ti6 + c];
            const float b0 = bufB[k * kStrideW + 32 * tj6 + c], b1 = bufB[k * kStrideW + 32 * tj6 + 32 + c];
            accW6[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, accW6[0], 0, 0, 0);
            accW6[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, accW6[1], 0, 0, 0);
        }
        for (int rr = 0; rr < 32; ++rr) sB6 += bufA[(q3 * 32 + rr) * kStrideN + j3];
        __syncthreads();
        stage<2>(bufA, kStrideN, trow, h, [&](int t, int r) { return dy3[t][r]; });
        stage<2>(bufB, kStrideN, trow, h, [&](int t, int r) { return xh3[t][r]; });
        if (h == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) bufZ[trow * 4 + k] = dz[k];
        }
        __syncthreads();
        {
            const float g7 = vec[vG7 + j3], e7 = vec[vE7 + j3];
            for (int rr = 0; rr < 32; ++rr) {
                const int k = q3 * 32 + rr;
                const float d = bufA[k * kStrideN + j3], xv = bufB[k * kStrideN + j3];
                sE7 += d;
                sG7 = __builtin_fmaf(d, xv, sG7);
                const float a3 = fmaxf(__builtin_fmaf(xv, g7, e7), 0.0f);
#pragma unroll
                for (int kk = 0; kk < K; ++kk) {
                    const float z = bufZ[k * 4 + kk];
                    sW9[kk] = __builtin_fmaf(z, a3, sW9[kk]);
                    sB9[kk] += z;
                }
            }
        }
        __syncthreads();

        // ---- layer 2 ------------------------------------------------------------
        float dy2[4][16], dh2[4][16];
        {
            f32x16 acc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
            mfma_stream<4, 32>(packed + pA3T, lane, [&](int q) { return dh3[q >> 4][q & 15]; }, acc);  // da2 = W6^T dh3
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) dy2[t][r] = acc[t][r];
        }
        ln_backward<4>(dy2, xh2, rs2, vec + vG4, h, dh2);
        stage<4>(bufA, kStrideW, trow, h, [&](int t, int r) { return dh2[t][r]; });
        stage<4>(bufB, kStrideW, trow, h, [&](int t, int r) { return act_of<128>(xh1[t][r], vec + vG1, hid(t, r, h)); });
        __syncthreads();
#pragma unroll 2
        for (int ks = 0; ks < kTileRows / 2; ++ks) {  // dW3 = dh2 . a1^T: out tile `wave`, the four in tiles
            const int k = 2 * ks + h;
            const float a = bufA[k * kStrideW + 32 * wave + c];
            float b[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) b[t] = bufB[k * kStrideW + 32 * t + c];
#pragma unroll
            for (int t = 0; t < 4; ++t) accW3[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[t], accW3[t], 0, 0, 0);
        }
        for (int rr = 0; rr < 64; ++rr) sB3 += bufA[(q2 * 64 + rr) * kStrideW + j2];
        __syncthreads();
        stage<4>(bufA, kStrideW, trow, h, [&](int t, int r) { return dy2[t][r]; });
        stage<4>(bufB, kStrideW, trow, h, [&](int t, int r) { return xh2[t][r]; });
        __syncthreads();
        for (int rr = 0; rr < 64; ++rr) {
            const int k = q2 * 64 + rr;
            const float d = bufA[k * kStrideW + j2];
            sE4 += d;
            sG4 = __builtin_fmaf(d, bufB[k * kStrideW + j2], sG4);
        }
        __syncthreads();

        // ---- layer 1 ------------------------------------------------------------
        float dy1[4][16], dh1[4][16];
        {
            f32x16 acc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
            mfma_stream<4, 64>(packed + pA2T, lane, [&](int q) { return dh2[q >> 4][q & 15]; }, acc);  // da1 = W3^T dh2
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) dy1[t][r] = acc[t][r];
        }
        ln_backward<4>(dy1, xh1, rs1, vec + vG1, h, dh1);
        stage<4>(bufA, kStrideW, trow, h, [&](int t, int r) { return dh1[t][r]; });
#pragma unroll
        for (int q = 0; q < 8; ++q) bufB[trow * kStrideX + 2 * q + h] = x[q];  // column 15: the zero loaded above
        __syncthreads();
#pragma unroll 4
        for (int ks = 0; ks < kTileRows / 2; ++ks) {  // dW0 = dh1 . x^T: out tile `wave`, 15 of the tile's 32 columns
            const int k = 2 * ks + h;
            const float a = bufA[k * kStrideW + 32 * wave + c];
            const float b = c < 16 ? bufB[k * kStrideX + c] : 0.0f;
            accW0[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, accW0[0], 0, 0, 0);
        }
        for (int rr = 0; rr < 64; ++rr) sB0 += bufA[(q2 * 64 + rr) * kStrideW + j2];
        __syncthreads();
        stage<4>(bufA, kStrideW, trow, h, [&](int t, int r) { return dy1[t][r]; });
        stage<4>(bufB, kStrideW, trow, h, [&](int t, int r) { return xh1[t][r]; });
        __syncthreads();
        for (int rr = 0; rr < 64; ++rr) {
            const int k = q2 * 64 + rr;
            const float d = bufA[k * kStrideW + j2];
            sE1 += d;
            sG1 = __builtin_fmaf(d, bufB[k * kStrideW + j2], sG1);
        }
        __syncthreads();
    }

    // ---- the block's partial gradient set ------------------------------------------
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = hid(0, r, h);  // the accumulator register's row of its tile
#pragma unroll
        for (int t = 0; t < 4; ++t) out[oW3 + (32 * wave + i) * 128 + 32 * t + c] = accW3[t][r];
        out[oW6 + (32 * ti6 + i) * 128 + 32 * tj6 + c] = accW6[0][r];
        out[oW6 + (32 * ti6 + i) * 128 + 32 * tj6 + 32 + c] = accW6[1][r];
        if (c < 15) out[oW0 + (32 * wave + i) * 15 + c] = accW0[0][r];
    }
    // the row quarters' / halves' column sums, added in a fixed order
    float* sh = lds;
    const float mine[15] = {sB6, sG7, sE7, sW9[0], sW9[1], sW9[2], sB9[0], sB9[1], sB9[2], sB3, sG4, sE4, sB0, sG1, sE1};
#pragma unroll
    for (int v = 0; v < 15; ++v) sh[v * kThreadsB + tid] = mine[v];
    __syncthreads();
    auto quarters = [&](int v, int j) {
        return ((sh[v * kThreadsB + j] + sh[v * kThreadsB + 64 + j]) + sh[v * kThreadsB + 128 + j]) +
               sh[v * kThreadsB + 192 + j];
    };
    auto halves = [&](int v, int j) { return sh[v * kThreadsB + j] + sh[v * kThreadsB + 128 + j]; };
    if (tid < 64) {
        out[oB6 + tid] = quarters(0, tid);
        out[oG7 + tid] = quarters(1, tid);
        out[oE7 + tid] = quarters(2, tid);
#pragma unroll
        for (int k = 0; k < K; ++k) out[oW9 + k * 64 + tid] = quarters(3 + k, tid);
        if (tid < K) out[oW9 + K * 64 + tid] = quarters(6 + tid, 0);
    }
    if (tid < 128) {
        out[oB3 + tid] = halves(9, tid);
        out[oG4 + tid] = halves(10, tid);
        out[oE4 + tid] = halves(11, tid);
        out[oB0 + tid] = halves(12, tid);
        out[oG1 + tid] = halves(13, tid);
        out[oE1 + tid] = halves(14, tid);
    }
}

}  // namespace mlpbwd
}  // namespace dd
