// collect_core.h — what the fused trainers that collect before they update
// share: dd_reinforce_train (reinforce_fused.hip has the design, the early
// stop's proof and the contract) and dd_ppo_train (ppo_train_fused.hip), so
// both leave the bits of the same rollout.
//
//   collect_episodes  phase 1 of both: one member's workgroup plays its L <= 128
//                     lanes on a sticky env, the actor's image in LDS, into the
//                     member's frame-major record; each lane's first episode is
//                     counted on the way.  kLogProb also records the log-prob
//                     of every drawn action (the float dd_policy_rollout
//                     returns), which PPO's ratio needs.
//   Cells             row r of the batch is cell map[r] of the record.
//   rows_total        a total over the batch's rows in the tree of a
//                     kStatBlocks-block launch.
//
// LDS as ppo_fused_core.h lays it out, with the lanes' current observation rows
// behind the forward image.
#pragma once

#include "frame.h"
#include "lane_io.h"
#include "ppo_fused_core.h"

namespace dd {
namespace collect {

using fused::kNormAt;
using fused::kRedAt;
using fused::kRowFloats;
using fused::kRowsAt;
using fused::kTileRows;
using fused::load_image;
using fused::load_row;

// The lanes' current observation rows, behind the forward image.
constexpr int kTileAt = mlp::kPacked;  // in floats
static_assert((size_t)(kTileAt + kTileRows * DD_OBS_DIM) * sizeof(float) <= mlpbwd::kLdsB,
              "the tile fits beside the image");
// rows_total's partials and its block_sum scratch share the reductions' scratch.
static_assert((size_t)(kStatBlocks + kBlock) * sizeof(double) <= kNormAt - kRedAt, "the partials fit");
// the lanes' lengths sit in the per-row buffer
static_assert(kTileRows * sizeof(int32_t) <= kRedAt - kRowsAt, "the lengths fit");

// The env side of a collecting launch: the same for every member.
struct Env {
    Consts k;  // runtime constants (switches, spawn; physics when !kRef)
    float* obs;
    double* shaped_hist;  // [2][n] (PPO's reward) or null
    uint64_t seed;
    int64_t step;
    int64_t n;
    int32_t lanes, frames, max_steps, shape;
};

// Thread k's lane k of the member after collecting: its first episode, and its status word.
struct Episode {
    int32_t len;
    bool ended;
    double ep_return;  // sum(rewards), forward, in double
    uint32_t status;
};

// Row r of the batch is cell map[r] of the record.
struct Cells {
    const int32_t* map;
    __device__ __forceinline__ int64_t cell(int64_t row) const { return map[row]; }
};

// The total over m rows of value(k) as a kStatBlocks-block launch forms it
// (stat_sum_kernel, stat_dev_kernel, pg_rows_kernel, ppo_rows_kernel's sums):
// stat block sb, thread t adds its rows sb kBlock + t + j kStatBlocks kBlock in
// order from 0.0, the block's 256 sums go through block_sum's tree
// (wave_block_sum: the same additions), the partials through stat_total.  A
// block with no row has the partial +0.  part: kStatBlocks doubles, sh: kBlock
// doubles (LDS).  Every thread gets the total; ends with a barrier.
template <typename F>
__device__ __forceinline__ double rows_total(int64_t m, F value, double* part, double* sh) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t full = (m + kBlock - 1) / kBlock;
    const int nb = (int)(full < kStatBlocks ? full : kStatBlocks);
    for (int sb = nb + tid; sb < kStatBlocks; sb += kBlock) part[sb] = 0.0;
    for (int sb = wave; sb < nb; sb += kBlock / 64) {
        double x[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            double s = 0.0;
            for (int64_t k = (int64_t)sb * kBlock + 64 * q + lane; k < m; k += (int64_t)kStatBlocks * kBlock)
                s += value(k);
            x[q] = s;
        }
        const double t = wave_block_sum(x);
        if (lane == 0) part[sb] = t;
    }
    __syncthreads();
    return stat_total<double>(part, sh);
}

// Phase 1 for member g (reinforce_fused.hip, "Collect" and "Early stop").  All
// threads call it.  On return the state arrays, shaped_hist and obs of the
// member's lanes are stored, the actor's image is still in LDS and the record
// holds every played frame: rec_obs [frames][L][15], rec_bits and rec_reward
// (and rec_lp when kLogProb) [frames][L].  The caller's next barrier orders the
// per-row buffer's last reads before its reuse.
template <bool kRef, bool kLogProb>
__device__ __forceinline__ Episode collect_episodes(const Env& a, const Soa<float>& soa, int g, const float* packed,
                                                    float* lds, float* rec_obs, uint32_t* rec_bits,
                                                    float* rec_reward, float* rec_lp) {
    float* rowbuf = reinterpret_cast<float*>(reinterpret_cast<char*>(lds) + kRowsAt);
    float* tile = lds + kTileAt;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, c = lane & 31;
    const int L = a.lanes, T = a.frames;
    const int64_t d0 = (int64_t)g * L;
    float* obs = a.obs + d0 * DD_OBS_DIM;
    const bool mine = tid < L;  // thread k has the member's lane k
    const int64_t d = d0 + (mine ? tid : 0);
    const DDConfig& sw = a.k.c;
    const Consts& k = kRef ? kRefConsts : a.k;
    const bool shaped = a.shape != kShapeNone;
    const bool ppo = a.shape == kShapePpo;

    Lane s;
    load_lane(soa, d, s);
    s.speed = 0.0; s.dist = 0.0;
    double h0 = 0.0, h1 = 0.0;  // the notebook reward's two-frame distance history
    if (ppo) load_hist(a.shaped_hist, a.n, d, h0, h1);
    load_image(packed, lds);
    for (int idx = tid; idx < L * DD_OBS_DIM; idx += kBlock) tile[idx] = obs[idx];
    __syncthreads();  // the image and the tile are written

    int32_t len = T;  // the lane's first episode
    bool ended = false;
    double ep_return = 0.0;
    for (int f = 0; f < T; ++f) {
        float* frame_obs = rec_obs + (int64_t)f * L * DD_OBS_DIM;
        for (int idx = tid; idx < L * DD_OBS_DIM; idx += kBlock) frame_obs[idx] = tile[idx];
        if (wave * mlp::kCols < L) {
            const int r = wave * mlp::kCols + c;
            const bool live = r < L;
            float x[8], z[3];
            load_row(tile + (live ? r : 0) * DD_OBS_DIM, live, h, x);
            mlp::mlp_body<3, false>(lds, lane, x, z);
            if (live && h == 0) {
                float prob[3], lp_drawn;
                uint32_t bits;
                mlp::actor_probs(z, prob);
                mlp::actor_sample(prob, (uint64_t)(soa.env_id_base + d0 + r), (uint64_t)(a.step + f), a.seed, bits,
                                  lp_drawn);
                rowbuf[r * kRowFloats] = __uint_as_float(bits);
                if constexpr (kLogProb) rec_lp[(int64_t)f * L + r] = lp_drawn;
            }
        }
        __syncthreads();  // the lanes' actions are written; the tile is read

        bool was_done = true;
        if (mine) {
            const uint32_t act = __float_as_uint(rowbuf[tid * kRowFloats]);
            was_done = (s.status & DD_ST_DONE) != 0;
            double reward;
            if (was_done) {  // sticky done (game_engine.py:107-111)
                measure(s);
                reward = 0.0;
            } else {
                reward = frame_checked<kRef, true>(k, sw, act, s);
            }
            float reward_f;
            bool done_f;
            if (shaped) {  // frame.h's shaped tail on a sticky env: never re-spawned
                double v[13];
                observe_values<false, true>(k, s, v);  // the notebook reward's doubles: exact quotients
                double sr;
                done_f = shaped_tail(v, s, ppo, was_done, false, a.max_steps, h0, h1, sr);
                reward_f = (float)sr;
            } else {
                reward_f = (float)reward;
                done_f = (s.status & DD_ST_DONE) != 0;
            }
            observe(k, s, tile + tid * DD_OBS_DIM);  // from the unrounded frame, like dd_step's obs
            quantize<float, kRef>(s);
            rec_bits[(int64_t)f * L + tid] = act;
            rec_reward[(int64_t)f * L + tid] = reward_f;
            if (!ended) {
                ep_return += (double)reward_f;
                if (done_f) {
                    len = f + 1;
                    ended = true;
                }
            }
        }
        if (__syncthreads_and(was_done ? 1 : 0)) break;  // the tile is written; see "Early stop"
    }
    if (mine) {
        store_lane(soa, d, s);
        if (ppo) store_hist(a.shaped_hist, a.n, d, h0, h1);
    }
    for (int idx = tid; idx < L * DD_OBS_DIM; idx += kBlock) obs[idx] = tile[idx];
    return {len, ended, ep_return, (uint32_t)s.status};
}

// A collecting launch's shape: what dd_reinforce_train refuses of it.
inline bool shape_ok(int32_t members, int64_t lanes, int32_t max_steps) {
    return members >= 1 && lanes >= 1 && lanes <= DD_PPO_FUSED_ROWS && max_steps >= 1 &&
           lanes * (int64_t)max_steps <= DD_REINFORCE_MAX_CELLS;
}

}  // namespace collect
}  // namespace dd
