// reinforce_fused.hip — dd_reinforce_train: one iteration of
// Policy_Gradients.ipynb's training loop (collect_episodes, compute_returns,
// the baseline and normalisation, the score loss, backward, clip, AdamW) for
// every learner of a population in one launch.
//
// The loop of launches it replaces, per member (collect_reinforce +
// reinforce_update: dd_policy_rollout, dd_batch_plan / gather / advantages /
// normalize, dd_mlp_evaluate_actions, dd_pg_losses, dd_mlp_pack,
// dd_mlp_backward, dd_adamw_step, dd_mlp_pack: about fifteen), becomes one
// workgroup of 256 threads per member on the member's L <= 128 lanes; no
// workgroup waits on another (no flag, no spin, no grid barrier), so the grid
// is `members` blocks and those past the card's CUs start when a CU is free.
//
//   1. Collect (collect_core.h's collect_episodes, shared with dd_ppo_train).
//      The actor's image is loaded into LDS once (the parameters do
//      not change while collecting).  Per frame: the lanes' observation rows
//      (an LDS tile) go to the member's frame-major record, the forward
//      (mlp_core.h mlp_body, a wave per 32 rows) and the Bernoulli draw
//      (actor_sample, keys (seed; env id, step + f)), then the frame, thread k
//      the member's lane k with its state in registers (lane_io.h load_lane /
//      store_lane), exactly policy_rollout.hip's frame for a sticky env:
//      frame.h's frame, the reward stream (engine, or frame.h's shaped_tail:
//      PPO's calc_reward with its history, REINFORCE's, the timeout), quantize.
//      Action bits and the returned reward go to the record.
//      Early stop.  The frame loop ends after the first frame in which every
//      lane of the member was done BEFORE the frame.  Such a frame maps a done
//      lane's stored (quantized) state to itself: frame.h's sticky path is
//      measure(s) (speed and dist from x, y, px, py, none of which it changes),
//      reward 0, no step count, no status change, the reward history untouched
//      (`was_done` writes neither h0 nor h1), and quantize is idempotent; the
//      observation row is a function of that state alone.  (The frame that
//      ENDS an episode is different: its row comes from the unrounded state,
//      which is why one frame on the done state is played first when frames
//      remain.)  So every further frame would store the same arrays and the
//      same obs, and rows past a lane's first episode are no rows of the batch.
//   2. Batch.  Per lane the first episode's length, ended flag and sum(rewards)
//      (forward, in double) are counted while collecting; offsets are the
//      exclusive scan of the lengths.  compute_returns backwards in double,
//      rounded once (batch_adv_kernel's DD_BATCH_RETURNS line).  Mean, unbiased
//      std and (x - mean) / (std + 1e-8) as dd_batch_normalize: rows_total
//      below forms each of the kStatBlocks partials with block_sum's tree
//      (wave_block_sum, a wave per stat block) and adds them with stat_total.
//      Rows are never compacted: row r of the batch is cell rowmap[r] = t L + k
//      of the record (an index per row, written once), and the observation
//      rows, action bits and rewards are read in place through it.
//   3. Update.  The batch's own actions scored tile by tile on the image still
//      in LDS (actor_probs, actor_evaluate: dd_mlp_evaluate_actions' floats);
//      dd_pg_losses' totals (rows_total again) and gradient rows; then
//      dd_mlp_backward for M rows: block b of kGradBlocks takes tiles b, b +
//      256, ..., the workgroup runs backward_block for b = 0, 1, ... in order
//      into one partial set and adds it, in double, into the accumulators
//      (sum_kernel's loop, s = 0.0 first), rounding once at the end.
//      Blocks with no tile are skipped: such a block's accumulators and column
//      sums are never touched after their 0.0f initialisation, and its fixed
//      order sums add +0 to +0, so every element of its partial is +0; and the
//      running double sum is never -0 (it starts at +0, and x + y is -0 only
//      when both are), so adding +0 leaves its bits.  The norm tree, the clip,
//      AdamW and the re-pack are ppo_fused_core.h's.
//
// Memory the block rewrites and reads again: ppo_fused_core.h's rule (ordered
// by __syncthreads(), never behind a const __restrict__ pointer, ordinary
// vector stores).  The member table is uploaded into the head of the workspace
// and only ever read.
#include <vector>

#include "collect_core.h"
#include "pg_core.h"

namespace dd {
namespace rf {

using collect::Cells;
using collect::rows_total;
using collect::shape_ok;
using fused::kNormAt;
using fused::kRedAt;
using fused::kRowsAt;
using fused::kTileRows;
using fused::load_row;
using fused::Net;
using mlp::f32x4;
using mlpbwd::kFinishBlocks;
using mlpbwd::kGradBlocks;
using mlpbwd::kPackedB;
using mlpbwd::kPartStride;

constexpr int kCount = adamw::params_of(3);

// One member's workspace, in bytes from its start: the backward's weight
// images, one partial gradient set, the double accumulators; then per cell of
// the [frames][lanes] record (rounded up to 4 cells) the observation row, the
// action bits, the reward; and per row of the batch its cell, return,
// advantage, log-prob, probabilities and gradient at the logits.
constexpr int64_t kCellBytes = (DD_OBS_DIM + 1 + 1 + 1 + 1 + 1 + 1 + 3 + 3) * (int64_t)sizeof(float);
constexpr int64_t kFixedBytes =
    ((int64_t)(kPackedB + kPartStride) * (int64_t)sizeof(float) + (int64_t)kCount * (int64_t)sizeof(double) + 15) / 16 * 16;
static_assert(kCellBytes == DD_REINFORCE_CELL_BYTES, "the header's figure");

struct Layout {
    int64_t image, part, acc, obs, bits, reward, rowmap, ret, adv, lp, prob, head, total;
};
__host__ __device__ inline Layout layout_of(int64_t cells) {
    const int64_t c4 = (cells + 3) / 4 * 4 * (int64_t)sizeof(float);  // bytes of one 4-byte column
    Layout l;
    l.image = 0;
    l.part = l.image + (int64_t)kPackedB * (int64_t)sizeof(float);
    l.acc = l.part + (int64_t)kPartStride * (int64_t)sizeof(float);
    l.obs = kFixedBytes;
    l.bits = l.obs + DD_OBS_DIM * c4;
    l.reward = l.bits + c4;
    l.rowmap = l.reward + c4;
    l.ret = l.rowmap + c4;
    l.adv = l.ret + c4;
    l.lp = l.adv + c4;
    l.prob = l.lp + c4;
    l.head = l.prob + 3 * c4;
    l.total = l.head + 3 * c4;
    return l;
}
static_assert(((int64_t)(kPackedB + kPartStride) * (int64_t)sizeof(float)) % 8 == 0, "the accumulators are doubles");

struct alignas(16) Member {
    Net net;
    double gamma, max_norm;
    int32_t clip, _pad;
};
static_assert(sizeof(Member) % 16 == 0, "the members' workspaces follow the table");

inline int64_t table_bytes(int64_t members) { return members * (int64_t)sizeof(Member); }

struct Args {
    collect::Env env;
    int32_t* lengths;
    uint8_t* ended;
    double* episode_return;
    float* record_reward;
    uint8_t* record_done;
    float* record_returns;
    float* record_advantages;
    double* logs;
    int64_t member_bytes;
    int32_t members, normalize;
};

template <bool kRef>
__global__ __launch_bounds__(kBlock) void train_kernel(const Member* __restrict__ table, char* workspace, Args a,
                                                       Soa<float> soa) {
    extern __shared__ f32x4 lds4[];
    float* lds = reinterpret_cast<float*>(lds4);
    float* rowbuf = reinterpret_cast<float*>(reinterpret_cast<char*>(lds) + kRowsAt);
    double* part = reinterpret_cast<double*>(reinterpret_cast<char*>(lds) + kRedAt);
    double* redd = part + kStatBlocks;
    double* normp = reinterpret_cast<double*>(reinterpret_cast<char*>(lds) + kNormAt);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, c = lane & 31;
    const int g = blockIdx.x;
    const Member mb = table[g];
    const Net& actor = mb.net;
    const int L = a.env.lanes, T = a.env.frames;
    const int64_t n = a.env.n;
    const int64_t d0 = (int64_t)g * L;
    const Layout lay = layout_of((int64_t)L * T);
    char* ws = workspace + (int64_t)g * a.member_bytes;
    float* image = reinterpret_cast<float*>(ws + lay.image);
    float* gpart = reinterpret_cast<float*>(ws + lay.part);
    double* acc = reinterpret_cast<double*>(ws + lay.acc);
    float* rec_obs = reinterpret_cast<float*>(ws + lay.obs);
    uint32_t* rec_bits = reinterpret_cast<uint32_t*>(ws + lay.bits);
    float* rec_reward = reinterpret_cast<float*>(ws + lay.reward);
    int32_t* rowmap = reinterpret_cast<int32_t*>(ws + lay.rowmap);
    float* ret = reinterpret_cast<float*>(ws + lay.ret);
    float* adv = reinterpret_cast<float*>(ws + lay.adv);
    float* lpv = reinterpret_cast<float*>(ws + lay.lp);
    float* probv = reinterpret_cast<float*>(ws + lay.prob);
    float* head = reinterpret_cast<float*>(ws + lay.head);
    const bool mine = tid < L;  // thread k has the member's lane k
    const int64_t d = d0 + (mine ? tid : 0);
    fused::Running run = fused::running_of(actor);

    // ---- 1. collect (collect_core.h) ------------------------------------------------------
    const collect::Episode ep =
        collect::collect_episodes<kRef, false>(a.env, soa, g, actor.packed, lds, rec_obs, rec_bits, rec_reward, nullptr);
    const int32_t len = ep.len;
    const bool ended = ep.ended;
    const double ep_return = ep.ep_return;

    // ---- 2. batch -----------------------------------------------------------------------
    int32_t* len_s = reinterpret_cast<int32_t*>(rowbuf);
    __syncthreads();  // the actions in the per-row buffer are read
    if (mine) len_s[tid] = len;
    __syncthreads();
    int32_t off = 0, m32 = 0;  // the lane's first row; the batch's rows
    for (int i = 0; i < L; ++i) {
        const int32_t v = len_s[i];
        off += i < tid ? v : 0;
        m32 += v;
    }
    const int64_t M = m32;
    if (mine) {
        a.lengths[d] = len;
        a.ended[d] = (uint8_t)(ended ? 1 : 0);
        a.episode_return[d] = ep_return;
        double G = 0.0;
        for (int32_t t = len - 1; t >= 0; --t) {
            G = (double)rec_reward[(int64_t)t * L + tid] + mb.gamma * G;
            ret[off + t] = (float)G;
            rowmap[off + t] = t * L + tid;
        }
        if (a.record_reward) {
            for (int32_t t = 0; t < T; ++t) {
                a.record_reward[(int64_t)t * n + d] = t < len ? rec_reward[(int64_t)t * L + tid] : 0.0f;
                a.record_done[(int64_t)t * n + d] = (uint8_t)(ended && t == len - 1 ? 1 : 0);
            }
        }
    }
    __syncthreads();  // the returns and the row map are written

    const double md = (double)M;
    const double mean = rows_total(M, [&](int64_t r) { return (double)ret[r]; }, part, redd) / md;
    const double ss = rows_total(M, [&](int64_t r) {
        const double dv = (double)ret[r] - mean;
        return dv * dv;
    }, part, redd);
    const double sd = M < 2 ? __builtin_nan("") : sqrt(ss / (double)(M - 1));  // torch.std's default: unbiased
    {
        const double denom = sd + 1e-8;
        for (int64_t r = tid; r < M; r += kBlock)
            adv[r] = a.normalize ? (float)(((double)ret[r] - mean) / denom) : ret[r];
    }
    __syncthreads();  // the advantages are written
    if (mine && a.record_returns) {
        for (int32_t t = 0; t < T; ++t) {
            a.record_returns[(int64_t)t * n + d] = t < len ? ret[off + t] : 0.0f;
            a.record_advantages[(int64_t)t * n + d] = t < len ? adv[off + t] : 0.0f;
        }
    }

    // ---- 3. update: the batch's actions scored on the image still in LDS ----------------
    for (int64_t first = 0; first < M; first += kTileRows) {
        if (first + wave * mlp::kCols < M) {
            const int64_t r = first + wave * mlp::kCols + c;
            const bool live = r < M;
            const int64_t cell = live ? rowmap[r] : 0;
            float x[8], z[3];
            load_row(rec_obs + cell * DD_OBS_DIM, live, h, x);
            mlp::mlp_body<3, false>(lds, lane, x, z);
            if (live && h == 0) {
                float prob[3], lp, ent;
                mlp::actor_probs(z, prob);
                mlp::actor_evaluate(prob, rec_bits[cell], lp, ent);
                lpv[r] = lp;
#pragma unroll
                for (int j = 0; j < 3; ++j) probv[r * 3 + j] = prob[j];
            }
        }
    }
    __syncthreads();  // the rows' outputs are written; the image is free

    pg::PgPart t;
    t.s = rows_total(M, [&](int64_t r) { return pg::pg_row(lpv[r], adv[r]).s; }, part, redd);
    t.cnt = rows_total(M, [&](int64_t r) { return pg::pg_row(lpv[r], adv[r]).cnt; }, part, redd);
    for (int64_t r = tid; r < M; r += kBlock) {
        const double gw = pg::pg_grad_of(adv[r], t.cnt);
        const uint32_t bits = rec_bits[rowmap[r]];
#pragma unroll
        for (int j = 0; j < 3; ++j) head[r * 3 + j] = pg::pg_grad_logit_of(gw, (bits >> j) & 1u, probv[r * 3 + j]);
    }

    // dd_mlp_backward for M rows: the blocks' partial sets in block order
    const DDMlpParams p = adamw::params_view(actor.params, 3, actor.ln_eps);
    for (int idx = tid; idx < kPackedB; idx += kBlock) image[idx] = mlpbwd::packed_value(p, idx);
    __syncthreads();  // the images and the head gradient are written
    const int64_t tiles = (M + kTileRows - 1) / kTileRows;
    const int blocks = (int)(tiles < kGradBlocks ? tiles : kGradBlocks);  // the blocks that have a tile
    for (int b = 0; b < blocks; ++b) {
        mlpbwd::backward_block<3>(p, rec_obs, head, M, image, gpart, b, kGradBlocks, lds, Cells{rowmap});
        __syncthreads();  // the partial set is written
        for (int e = tid; e < kCount; e += kBlock) acc[e] = (b == 0 ? 0.0 : acc[e]) + (double)gpart[e];
        __syncthreads();  // and read; LDS is free again
    }
    for (int b = wave; b < kFinishBlocks; b += kBlock / 64) {
        double sq[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = b * kBlock + 64 * j + lane;
            sq[j] = 0.0;
            if (e < kCount) {
                const float f = (float)acc[e];  // the one rounding
                actor.grads[e] = f;
                sq[j] = (double)f * (double)f;
            }
        }
        const double sum = wave_block_sum(sq);
        if (lane == 0) normp[b] = sum;
    }
    __syncthreads();
    const double norm = sqrt(block_sum<double>(tid < kFinishBlocks ? normp[tid] : 0.0, redd));

    fused::clip_adamw<3>(actor, mb.clip != 0, mb.max_norm, norm, run);
    fused::repack(actor, p, lds);
    if (tid == 0) {
        double* entry = a.logs + g;
        entry[(int64_t)DD_RF_LOSS * a.members] = pg::pg_loss_of(t);
        entry[(int64_t)DD_RF_GRAD_NORM * a.members] = norm;
        entry[(int64_t)DD_RF_BASELINE * a.members] = mean;
        entry[(int64_t)DD_RF_STD * a.members] = sd;
        entry[(int64_t)DD_RF_ROWS * a.members] = md;
    }
}

}  // namespace rf
}  // namespace dd

extern "C" {

int64_t dd_reinforce_train_workspace(int32_t members, int64_t lanes, int32_t max_steps) {
    using namespace dd::rf;
    if (!shape_ok(members, lanes, max_steps)) return 0;
    return table_bytes(members) + (int64_t)members * layout_of(lanes * (int64_t)max_steps).total;
}

int dd_reinforce_train(const DDConfig* cfg, const DDState* st, const DDReinforceIO* io, int64_t n, void* workspace,
                       void* stream) {
    using namespace dd::rf;
    if (!cfg || !io || !workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u)) return hipErrorInvalidValue;
    if (!dd::state_ok(st) || st->precision != DD_F32) return hipErrorInvalidValue;
    if (!io->table || !shape_ok(io->members, io->lanes_per_member, io->max_steps)) return hipErrorInvalidValue;
    if (n != (int64_t)io->members * io->lanes_per_member) return hipErrorInvalidValue;
    if (cfg->auto_reset) return hipErrorInvalidValue;  // one episode per lane
    if (!io->obs || !io->lengths || !io->ended || !io->episode_return || !io->logs) return hipErrorInvalidValue;
    const int shape = dd::loop_shape(io->shaped_mode, io->shaped_hist, nullptr, nullptr);
    if (shape < 0) return hipErrorInvalidValue;
    if ((io->record_reward != nullptr) != (io->record_done != nullptr)) return hipErrorInvalidValue;
    if ((io->record_returns != nullptr) != (io->record_advantages != nullptr)) return hipErrorInvalidValue;
    const int32_t members = io->members;
    const int64_t member_bytes = layout_of(io->lanes_per_member * (int64_t)io->max_steps).total;
    char* blocks = static_cast<char*>(workspace) + table_bytes(members);
    std::vector<Member> table((size_t)members);
    std::vector<dd::fused::Owned> owned;  // every buffer its own owner: no two may overlap
    owned.reserve((size_t)members * 6);
    int32_t owner = 0;
    for (int32_t q = 0; q < members; ++q) {
        const DDReinforceMember& m = io->table[q];
        if (!dd::fused::net_ok(m.actor)) return hipErrorInvalidValue;
        if (!__builtin_isfinite(m.gamma) || m.max_grad_norm != m.max_grad_norm) return hipErrorInvalidValue;
        Member& t = table[q];
        t.net = dd::fused::net_of(m.actor, blocks + (int64_t)q * member_bytes);
        t.gamma = m.gamma;
        t.max_norm = m.max_grad_norm;
        t.clip = dd::fused::clip_of(m.max_grad_norm) ? 1 : 0;
        t._pad = 0;
        dd::fused::owned_apart(m.actor, 3, owner, owned);
    }
    if (dd::fused::shared_between_owners(owned)) return hipErrorInvalidValue;

    Args a{};
    a.env.k = dd::make_consts(*cfg);
    a.env.obs = io->obs;
    a.env.shaped_hist = shape == dd::kShapePpo ? io->shaped_hist : nullptr;
    a.env.seed = io->seed;
    a.env.step = io->step;
    a.env.n = n;
    a.env.lanes = (int32_t)io->lanes_per_member;
    a.env.frames = io->max_steps;
    a.env.max_steps = shape == dd::kShapeNone ? 0 : io->env_max_steps;
    a.env.shape = shape;
    a.lengths = io->lengths;
    a.ended = io->ended;
    a.episode_return = io->episode_return;
    a.record_reward = static_cast<float*>(io->record_reward);
    a.record_done = io->record_done;
    a.record_returns = io->record_returns;
    a.record_advantages = io->record_advantages;
    a.logs = io->logs;
    a.member_bytes = member_bytes;
    a.members = members;
    a.normalize = io->normalize ? 1 : 0;
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
