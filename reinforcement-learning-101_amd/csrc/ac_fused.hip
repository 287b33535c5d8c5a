// ac_fused.hip — dd_actor_critic_train: Actor_Critic_Basic.ipynb's training
// loop, `frames` passes of its `while not all(games_done)` body, for every
// learner of a population in one launch.
//
// The one-step actor-critic learner updates both networks after every frame,
// and the next frame's actions come from the actor that was just updated: no
// frame can be collected ahead.  The loop of launches (MlpNet.act, dd_step,
// actor_critic_update: about 25 per frame) is replaced by one persistent
// workgroup of 256 threads per member, which runs the notebook's order inside a
// frame on the member's L <= 128 lanes (one backward row tile):
//
//   1. state = the lanes' observation rows, copied to the block's stage;
//      the actor's image into LDS, its forward on state (mlp_core.h mlp_body,
//      a wave per 32 rows) and the Bernoulli draw (actor_sample); the action,
//      its log-probability (actor_evaluate: the float dd_mlp_evaluate_actions
//      gives, which is actor_sample's own) and the probabilities stay in LDS;
//   2. the frame, thread k the member's lane k: the lane's state from the env's
//      arrays, frame.h's frame as step_tile.h's finish_lane runs it (re-spawn, sticky
//      done, the notebook reward with its history and timeout: frame.h's
//      shaped_tail for the PPO shape, written out in the kernel, see there), the
//      state (lane_io.h load_lane / store_lane), the outputs and the new
//      observation row stored as dd_step leaves them;
//   3. the critic's image into LDS, its forward on state and on the new rows;
//   4. the TD rows and totals (pg_core.h), the head gradient;
//   5. the critic's backward, norm, clip, AdamW and re-pack (ppo_fused_core.h);
//   6. the score loss on those TD errors with step 1's probabilities;
//   7. the actor's backward, norm, clip, AdamW and re-pack.
//
// The two networks run one after the other: on two workgroups the actor's
// would wait for the critic's TD errors every frame.  No workgroup waits on
// another (no flag, no spin, no grid barrier), so nothing assumes co-residency:
// the grid is `members` blocks, and those past the card's CUs (one block per CU,
// the LDS) start when a CU is free, as ppo_fused_population.hip's do.
//
// Totals: with at most 128 rows only block 0 of td_rows_kernel and
// pg_rows_kernel holds rows, so fused::stat_sum forms each total as the launch
// kernels do: block 0's block_sum, then the second one over (it, nothing, ...).
//
// Memory the block rewrites and reads again (parameters, moments, gradients,
// images, head gradients, the stage, the env's arrays and obs): ppo_fused_core.h's
// rule: ordered by __syncthreads(), never behind a const __restrict__ pointer,
// stored with ordinary vector stores.  The env state lives in the env's arrays
// between frames; no lane holds it in registers across a backward.  The member
// table is uploaded into the head of the workspace and only ever read.
#include <vector>

#include "frame.h"
#include "lane_io.h"
#include "pg_core.h"
#include "ppo_fused_core.h"

namespace dd {
namespace acf {

using fused::kNetWorkspace;
using fused::kRedAt;
using fused::kRowFloats;
using fused::kRowsAt;
using fused::kTileRows;
using fused::load_image;
using fused::Net;
using mlp::f32x4;

// A row's slots in the per-row LDS buffer (kRowFloats floats a row).
enum { rLogProb = 0, rBits = 1, rProb = 2, rValue = 5, rNextValue = 6 };
static_assert(rNextValue < kRowFloats, "a row's slots");

// The new observation rows' tile, behind the forward image: free whenever the image is.
constexpr int kTileAt = mlp::kPacked;  // in floats
static_assert((size_t)(kTileAt + kTileRows * DD_OBS_DIM) * sizeof(float) <= mlpbwd::kLdsB,
              "the tile fits beside the image");

// One member's workspace: both networks' backward images and head gradients, the state stage.
constexpr int64_t kStageBytes = (int64_t)kTileRows * DD_OBS_DIM * (int64_t)sizeof(float);
constexpr int64_t kMemberWorkspace = 2 * kNetWorkspace + kStageBytes;
static_assert(kMemberWorkspace % 16 == 0, "every member's images are 16-byte aligned");

struct alignas(16) Member {
    Net net[2];  // actor, critic
    double gamma, value_reg, max_norm;
    int32_t clip, _pad;
};
static_assert(sizeof(Member) % 16 == 0, "the members' workspaces follow the table");

inline int64_t table_bytes(int64_t members) { return members * (int64_t)sizeof(Member); }

struct Args {
    Consts k;  // runtime constants (switches, spawn; physics when !kRef)
    float* obs;
    float* reward;
    uint8_t* done;
    double* shaped_hist;  // [2][n] (notebook reward) or null
    float* shaped_reward;
    uint8_t* shaped_done;
    const uint8_t* active0;
    uint8_t* done_last;
    float* record_reward;
    uint8_t* record_done;
    double* logs;
    uint64_t seed;
    int64_t step;
    int64_t n;
    int32_t lanes, members, frames, max_steps;
};

// One optimizer step of a network from its head gradient: ppo_fused_core.h's phases.
template <int K>
__device__ __forceinline__ double update(const Net& n, const Member& mb, const float* states, int rows,
                                         fused::Running& run, float* lds) {
    const DDMlpParams p = adamw::params_view(n.params, K, n.ln_eps);
    const double norm = fused::backward_norm<K>(n, p, states, rows, lds);
    fused::clip_adamw<K>(n, mb.clip != 0, mb.max_norm, norm, run);
    fused::repack(n, p, lds);
    return norm;
}

// Layer 1's B operand of row d of `rows_at` [rows][15] for this lane half (zero past column 14 and row `rows`).
// The kernel keeps this index form: with ppo_fused_core.h's row-pointer load_row it spilled one to two more
// SGPRs than before (profiles/fused_share/), and its instructions stay as they were this way.
__device__ __forceinline__ void load_row(const float* rows_at, int d, bool live, int h, float (&x)[8]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int col = 2 * q + h;
        x[q] = live && col < DD_OBS_DIM ? rows_at[d * DD_OBS_DIM + col] : 0.0f;
    }
}

template <bool kRef>
__global__ __launch_bounds__(kBlock) void train_kernel(const Member* __restrict__ table, char* workspace, Args a,
                                                       Soa<float> soa) {
    extern __shared__ f32x4 lds4[];
    float* lds = reinterpret_cast<float*>(lds4);
    float* rowbuf = reinterpret_cast<float*>(reinterpret_cast<char*>(lds) + kRowsAt);
    float* tile = lds + kTileAt;
    char* red = reinterpret_cast<char*>(lds) + kRedAt;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, c = lane & 31;
    const int g = blockIdx.x;
    const Member mb = table[g];
    const Net& actor = mb.net[0];
    const Net& critic = mb.net[1];
    const int rows = a.lanes;
    const int64_t d0 = (int64_t)g * rows;
    float* stage = reinterpret_cast<float*>(workspace + (int64_t)g * kMemberWorkspace + 2 * kNetWorkspace);
    float* obs = a.obs + d0 * DD_OBS_DIM;
    const bool mine = tid < rows;       // thread k has the member's lane k, and the batch's row k
    const int64_t d = d0 + (mine ? tid : 0);
    const DDConfig& sw = a.k.c;
    const Consts& k = kRef ? kRefConsts : a.k;
    const bool shaped = a.shaped_hist != nullptr;
    const double gamma = mb.gamma;
    fused::Running run_actor = fused::running_of(actor), run_critic = fused::running_of(critic);
    bool done_prev = mine && a.active0 && a.active0[d] == 0;

    for (int f = 0; f < a.frames; ++f) {
        double* entry = a.logs + (int64_t)f * a.members + g;
        const int64_t log_row = (int64_t)a.frames * a.members;

        // ---- 1. state; the actor on it and the draw ----------------------------------
        for (int idx = tid; idx < rows * DD_OBS_DIM; idx += kBlock) stage[idx] = obs[idx];
        load_image(actor.packed, lds);
        __syncthreads();  // the stage and the image are written
        if (wave * mlp::kCols < rows) {
            const int r = wave * mlp::kCols + c;
            const bool live = r < rows;
            float x[8], z[3];
            load_row(stage, r, live, h, x);
            mlp::mlp_body<3, false>(lds, lane, x, z);
            if (live && h == 0) {
                float prob[3], lp, lp_drawn, ent;
                uint32_t bits;
                mlp::actor_probs(z, prob);
                mlp::actor_sample(prob, (uint64_t)(soa.env_id_base + d0 + r), (uint64_t)(a.step + f), a.seed, bits,
                                  lp_drawn);
                mlp::actor_evaluate(prob, bits, lp, ent);
                float* out = rowbuf + r * kRowFloats;
                out[rLogProb] = lp;
                out[rBits] = __uint_as_float(bits);
#pragma unroll
                for (int j = 0; j < 3; ++j) out[rProb + j] = prob[j];
            }
        }
        __syncthreads();  // the rows' actions are written; the image is free

        // ---- 2. the frame (dd_step's, a lane per thread) ------------------------------
        float reward_f = 0.0f;  // the returned reward and done of this thread's lane
        bool done_f = false;
        if (mine) {
            const uint32_t act = __float_as_uint(rowbuf[tid * kRowFloats + rBits]);
            const int64_t env = soa.env_id_base + d;
            Lane s;
            load_lane(soa, d, s);
            double h0 = 0.0, h1 = 0.0;  // the notebook reward's two-frame distance history
            if (shaped) { h0 = a.shaped_hist[d]; h1 = a.shaped_hist[a.n + d]; }
            const bool was_done = (s.status & DD_ST_DONE) != 0;
            double reward;
            if (was_done) {
                reward = 0.0;
                if (sw.auto_reset) spawn(sw, k.c.max_fuel, env, s);  // next-step reset: a fresh episode
                else measure(s);                                     // sticky done (game_engine.py:107-111)
            } else {
                reward = frame_checked<kRef, false>(k, sw, act, s);  // dd_step's frame, with its exact redo
            }
            // dd_step's notebook path.  The tail below is frame.h's shaped_tail (ppo, this kernel's re-spawn
            // case) written out, and the history's pair is loaded and stored by hand: with shaped_tail the kernel
            // spilled two more SGPRs than before, with load_hist / store_hist its instructions changed
            // (profiles/fused_share/).  A fix to shaped_tail belongs here too; tests/test_gpu_shaped_tail.py
            // holds the two to the same bits.
            if (shaped) {
                double v[13];
                observe_values<false, true>(k, s, v);  // the notebook reward's doubles: exact quotients
                double sr = 0.0;
                bool sd;
                if (sw.auto_reset && was_done) {  // re-spawned: prev_state None
                    h0 = v[9];
                    h1 = __builtin_nan("");
                    sd = false;
                } else if (was_done) {
                    sd = true;
                } else {
                    const bool odd = (s.steps & 1) != 0;
                    sr = notebook_reward(v, s.status, odd ? h1 : h0);
                    h1 = odd ? v[9] : h1;
                    h0 = odd ? h0 : v[9];
                    sd = (s.status & DD_ST_DONE) != 0;
                    if (a.max_steps > 0 && s.steps >= a.max_steps) {  // the collection loop's timeout
                        sr = (s.status & DD_ST_LANDED) ? sr : sr - 500;
                        sd = true;
                        s.status |= DD_ST_DONE;
                    }
                }
                reward_f = (float)sr;
                done_f = sd;
                a.shaped_reward[d] = reward_f;
                a.shaped_done[d] = (uint8_t)(sd ? 1 : 0);
                a.shaped_hist[d] = h0;
                a.shaped_hist[a.n + d] = h1;
            } else {
                reward_f = (float)reward;
                done_f = (s.status & DD_ST_DONE) != 0;
            }
            a.reward[d] = (float)reward;
            a.done[d] = (uint8_t)((s.status & DD_ST_DONE) ? 1 : 0);
            if (a.record_reward) {
                a.record_reward[(int64_t)f * a.n + d] = reward_f;
                a.record_done[(int64_t)f * a.n + d] = (uint8_t)(done_f ? 1 : 0);
            }
            observe(k, s, tile + tid * DD_OBS_DIM);  // from the unrounded frame, like dd_step's obs
            store_lane(soa, d, s);
        }
        __syncthreads();  // the new rows are in the tile

        // ---- 3. the critic on state and on the new rows -------------------------------
        for (int idx = tid; idx < rows * DD_OBS_DIM; idx += kBlock) obs[idx] = tile[idx];
        load_image(critic.packed, lds);
        __syncthreads();
        if (wave * mlp::kCols < rows) {
            const int r = wave * mlp::kCols + c;
            const bool live = r < rows;
            float x[8], z[1];
            load_row(stage, r, live, h, x);
            mlp::mlp_body<1, false>(lds, lane, x, z);
            if (live && h == 0) rowbuf[r * kRowFloats + rValue] = z[0];
            load_row(tile, r, live, h, x);
            mlp::mlp_body<1, false>(lds, lane, x, z);
            if (live && h == 0) rowbuf[r * kRowFloats + rNextValue] = z[0];
        }
        __syncthreads();  // the values are written; the image and the tile are free

        // ---- 4. the TD rows, totals and the critic's head gradient ----------------------
        const bool active = mine && !done_prev;
        float td_error = 0.0f;
        {
            pg::TdPart acc = {0.0, 0.0, 0.0};
            double delta = 0.0, v = 0.0;
            if (active) {
                double target;
                v = (double)rowbuf[tid * kRowFloats + rValue];
                pg::td_row_of(v, (double)rowbuf[tid * kRowFloats + rNextValue], (double)reward_f, done_f ? 1.0 : 0.0,
                              gamma, &target, &delta);
                acc += pg::td_part_of(delta, v);
                td_error = (float)delta;
            }
            const pg::TdPart t = fused::stat_sum<pg::TdPart>(acc, {0.0, 0.0, 0.0}, reinterpret_cast<pg::TdPart*>(red));
            if (mine) critic.head[tid] = active ? pg::td_grad_value_of(delta, v, mb.value_reg, t.cnt) : 0.0f;
            if (tid == 0) {
                const double mse = pg::td_mse_of(t), reg = pg::td_reg_of(t, mb.value_reg);
                entry[DD_AC_CRITIC_LOSS * log_row] = mse + reg;
                entry[DD_AC_MSE * log_row] = mse;
                entry[DD_AC_VALUE_REG * log_row] = reg;
                entry[DD_AC_COUNT * log_row] = t.cnt;
            }
        }

        // ---- 5. the critic's step ----------------------------------------------------------
        const double norm_critic = update<1>(critic, mb, stage, rows, run_critic, lds);
        if (tid == 0) entry[DD_AC_CRITIC_GRAD_NORM * log_row] = norm_critic;

        // ---- 6. the score loss on the TD errors, the actor's head gradient -----------------
        {
            pg::PgPart acc = {0.0, 0.0};
            const float* out = rowbuf + tid * kRowFloats;
            if (active) acc += pg::pg_row(out[rLogProb], td_error);
            const pg::PgPart t = fused::stat_sum<pg::PgPart>(acc, {0.0, 0.0}, reinterpret_cast<pg::PgPart*>(red));
            if (mine) {
                float gl[3] = {0.0f, 0.0f, 0.0f};
                if (active) {
                    const double gw = pg::pg_grad_of(td_error, t.cnt);
                    const uint32_t bits = __float_as_uint(out[rBits]);
#pragma unroll
                    for (int j = 0; j < 3; ++j) gl[j] = pg::pg_grad_logit_of(gw, (bits >> j) & 1u, out[rProb + j]);
                }
#pragma unroll
                for (int j = 0; j < 3; ++j) actor.head[tid * 3 + j] = gl[j];
            }
            if (tid == 0) entry[DD_AC_ACTOR_LOSS * log_row] = pg::pg_loss_of(t);
        }

        // ---- 7. the actor's step ------------------------------------------------------------
        const double norm_actor = update<3>(actor, mb, stage, rows, run_actor, lds);
        if (tid == 0) entry[DD_AC_ACTOR_GRAD_NORM * log_row] = norm_actor;
        done_prev = done_f;
    }
    if (mine) a.done_last[d] = (uint8_t)(done_prev ? 1 : 0);
}

}  // namespace acf
}  // namespace dd

extern "C" {

int64_t dd_actor_critic_train_workspace(int32_t members) {
    using namespace dd::acf;
    if (members < 1) return 0;
    return table_bytes(members) + (int64_t)members * kMemberWorkspace;
}

int dd_actor_critic_train(const DDConfig* cfg, const DDState* st, const DDActorCriticIO* io, int64_t n,
                          void* workspace, void* stream) {
    using namespace dd::acf;
    if (!cfg || !io || !workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u)) return hipErrorInvalidValue;
    if (!dd::state_ok(st) || st->precision != DD_F32) return hipErrorInvalidValue;
    if (!io->table || io->members < 1 || io->frames < 1) return hipErrorInvalidValue;
    if (io->lanes_per_member < 1 || io->lanes_per_member > DD_PPO_FUSED_ROWS) return hipErrorInvalidValue;
    if (n != (int64_t)io->members * io->lanes_per_member) return hipErrorInvalidValue;
    if (!io->obs || !io->reward || !io->done || !io->done_last || !io->logs) return hipErrorInvalidValue;
    if (io->shaped_mode != DD_SHAPED_PPO) return hipErrorInvalidValue;
    const int shaped = (io->shaped_hist != nullptr) + (io->shaped_reward != nullptr) + (io->shaped_done != nullptr);
    if (shaped != 0 && shaped != 3) return hipErrorInvalidValue;
    if ((io->record_reward != nullptr) != (io->record_done != nullptr)) return hipErrorInvalidValue;
    const int32_t members = io->members;
    char* blocks = static_cast<char*>(workspace) + table_bytes(members);
    std::vector<Member> table((size_t)members);
    std::vector<dd::fused::Owned> owned;  // every buffer its own owner: no two may overlap
    owned.reserve((size_t)members * 12);
    int32_t owner = 0;
    for (int32_t p = 0; p < members; ++p) {
        const DDActorCriticMember& m = io->table[p];
        if (!dd::fused::net_ok(m.actor) || !dd::fused::net_ok(m.critic)) return hipErrorInvalidValue;
        if (!__builtin_isfinite(m.gamma) || !__builtin_isfinite(m.value_reg)) return hipErrorInvalidValue;
        if (m.max_grad_norm != m.max_grad_norm) return hipErrorInvalidValue;
        char* ws = blocks + (int64_t)p * kMemberWorkspace;
        Member& t = table[p];
        t.net[0] = dd::fused::net_of(m.actor, ws);
        t.net[1] = dd::fused::net_of(m.critic, ws + kNetWorkspace);
        t.gamma = (double)(float)m.gamma;
        t.value_reg = m.value_reg;
        t.max_norm = m.max_grad_norm;
        t.clip = dd::fused::clip_of(m.max_grad_norm) ? 1 : 0;
        t._pad = 0;
        dd::fused::owned_apart(m.actor, 3, owner, owned);
        dd::fused::owned_apart(m.critic, 1, owner, owned);
    }
    if (dd::fused::shared_between_owners(owned)) return hipErrorInvalidValue;

    Args a{};
    a.k = dd::make_consts(*cfg);
    a.obs = io->obs;
    a.reward = static_cast<float*>(io->reward);
    a.done = io->done;
    a.shaped_hist = io->shaped_hist;
    a.shaped_reward = static_cast<float*>(io->shaped_reward);
    a.shaped_done = io->shaped_done;
    a.active0 = io->active0;
    a.done_last = io->done_last;
    a.record_reward = static_cast<float*>(io->record_reward);
    a.record_done = io->record_done;
    a.logs = io->logs;
    a.seed = io->seed;
    a.step = io->step;
    a.n = n;
    a.lanes = (int32_t)io->lanes_per_member;
    a.members = members;
    a.frames = io->frames;
    a.max_steps = io->max_steps;
    const dd::Soa<float> soa = dd::soa_of<float>(*st, 0);
    const bool ref = dd::uses_reference_physics(*cfg);

    hipStream_t s = static_cast<hipStream_t>(stream);
    return dd::with_bool(ref, [&](auto r) {
        const hipError_t e = dd::fused::launch_with_table(train_kernel<decltype(r)::value>, table, workspace,
                                                          (unsigned)members, s, blocks, a, soa);
        return e != hipSuccess ? (int)e : dd::finish();
    });
}

}  // extern "C"
