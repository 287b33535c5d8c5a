// shuffle_core.h — the keyed permutation of a training batch's rows
// (include/dronestep.h has the definition): its parameters and perm(j), for
// the units that move rows through it (shuffle.hip) or read rows through it in
// place (ppo_fused_population.hip).
//
// perm(j) is stateless: an 8-round balanced Feistel network over the smallest
// even-width domain that holds [0, m), its round function one Philox4x32-10
// block keyed by (seed, epoch), and cycle walking back into [0, m).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "philox.h"

namespace dd {
namespace shuffle {

constexpr int kRounds = 8;  // 4 are measurably not uniform, 6 and 8 are clean (tests/test_shuffle_cpu.py)

struct Key {
    uint32_t m;       // rows
    uint32_t h;       // bits of each Feistel half
    uint32_t mask;    // 2^h - 1
    uint32_t k0, k1;  // seed
    uint32_t e0, e1;  // epoch_lo, epoch_hi ^ 0xC3C3C3C3
};

__device__ __forceinline__ uint32_t perm(uint32_t j, const Key& k) {
    uint32_t x = j;
    do {
        uint32_t left = x >> k.h, right = x & k.mask;
#pragma unroll
        for (uint32_t r = 0; r < (uint32_t)kRounds; ++r) {
            uint32_t o[4];
            philox4x32_10(right, r, k.e0, k.e1, k.k0, k.k1, o);
            const uint32_t next = left ^ (o[0] & k.mask);
            left = right;
            right = next;
        }
        x = (left << k.h) | right;
    } while (x >= k.m);  // the cipher is a bijection of [0, 2^(2h)): the walk re-enters [0, m)
    return x;
}

// m in [1, 2^31): the permutation's parameters
__host__ __device__ inline Key key_of(int64_t m, uint64_t seed, uint64_t epoch) {
    const int b = m > 1 ? 64 - __builtin_clzll((unsigned long long)(m - 1)) : 0;
    const int h = b > 1 ? (b + 1) / 2 : 1;
    return {(uint32_t)m, (uint32_t)h, (uint32_t)((1u << h) - 1u), (uint32_t)seed, (uint32_t)(seed >> 32),
            (uint32_t)epoch, (uint32_t)(epoch >> 32) ^ 0xC3C3C3C3u};
}

}  // namespace shuffle
}  // namespace dd
