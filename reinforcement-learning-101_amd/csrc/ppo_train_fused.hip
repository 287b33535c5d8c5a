// ppo_train_fused.hip — dd_ppo_train: one iteration of Actor_Critic_PPO.ipynb's
// training cell (collect_episodes_ppo, the critic's values and the bootstrap,
// compute_gae, returns = advantages + values, the batch normalisation, and
// num_epochs of losses, backward, clip_grad_norm_ and the two AdamW steps) for
// every learner of a population in one launch.
//
// The loop of launches it replaces, per member (collect_ppo + ppo_update: the
// rollout, plan / gather / critic forward / advantages / normalize, then the
// update's steps), becomes one workgroup of 256 threads per member on the
// member's L <= 128 lanes, which runs both networks; no workgroup waits on
// another (no flag, no spin, no grid barrier), so the grid is `members` blocks
// and those past the card's CUs start when a CU is free.  Every loop bound is a
// host integer or a count fixed before the loop starts.
//
//   1. Collect.  collect_core.h's collect_episodes (dd_reinforce_train's phase
//      1), which also records the log-prob of every drawn action.
//   2. Batch.  Lengths, ended flags, sum(rewards) and the row map as
//      reinforce_fused.hip (row r of the batch is cell rowmap[r] = t L + k of the
//      record; rows are never compacted).  The critic's image replaces the
//      actor's in LDS (the lanes' final observation rows sit behind it): its
//      value on those rows is the bootstrap, its value on every row of the batch,
//      tile by tile, dd_mlp_forward's floats.  Thread k then runs gae_core.h's
//      recursion backwards over lane k as batch_adv_kernel does (bootstrap 0 and
//      mask 0 at the last frame of an ended episode), returns = advantage +
//      value; mean, unbiased std and (x - mean) / (std + 1e-8) as
//      dd_batch_normalize, through rows_total.
//   3. Update.  The two networks' steps never read each other's parameters, so
//      the workgroup walks all of the actor's steps, then all of the critic's.
//      Steps of at most one row tile (minibatch_size = B, or a full batch of M
//      <= 128 rows: what ppo_update runs fused) are ppo_fused_core.h's learn<K>
//      on rows staged through the keyed permutation composed with the row map.
//      A full batch of more rows is the loop of launches' step: the forward on
//      every row, dd_ppo_losses' totals (rows_total: the five sums field by
//      field, which is Part's tree; min and max, which no grouping changes) and
//      gradient rows, then dd_mlp_backward for M rows exactly as
//      reinforce_fused.hip runs it (block order, double accumulators rounded
//      once), the norm, the clip, AdamW and the re-pack.
//
// Memory the block rewrites and reads again: ppo_fused_core.h's rule (ordered
// by __syncthreads(), never behind a const __restrict__ pointer, ordinary
// vector stores).  The member table is uploaded into the head of the workspace
// and only ever read.
#include <vector>

#include "collect_core.h"
#include "gae_core.h"
#include "shuffle_core.h"

namespace dd {
namespace pt {

using collect::Cells;
using collect::kTileAt;
using collect::rows_total;
using fused::kNetWorkspace;
using fused::kNormAt;
using fused::kRedAt;
using fused::kRowFloats;
using fused::kRowsAt;
using fused::kTileRows;
using fused::load_image;
using fused::load_row;
using fused::Net;
using mlp::f32x4;
using mlpbwd::kFinishBlocks;
using mlpbwd::kGradBlocks;
using mlpbwd::kPackedB;
using mlpbwd::kPartStride;

// A staged minibatch (learn<K>'s rows): states [128][15], then a column each of
// action bits, old log-probs, advantages and returns.
constexpr int kStageStates = 0;
constexpr int kStageBits = kStageStates + kTileRows * DD_OBS_DIM;
constexpr int kStageOld = kStageBits + kTileRows;
constexpr int kStageAdv = kStageOld + kTileRows;
constexpr int kStageRet = kStageAdv + kTileRows;
constexpr int kStageWords = kStageRet + kTileRows;

// One member's workspace, in bytes from its start.  Fixed: each network's
// backward images and one-tile head gradient (learn<K>'s), one partial gradient
// set, the double accumulators, the stage.  Then per cell of the [frames][lanes]
// record (rounded up to 4 cells): the observation row, the action bits, the
// reward, the drawn action's log-prob; and per row of the batch its cell, value,
// return, raw and normalised advantage, the step's forward outputs (log-prob,
// entropy, three probabilities; or the value) and its head gradient.
constexpr int kOutFloats = 5;
constexpr int64_t kCellBytes = (DD_OBS_DIM + 1 + 1 + 1 + 1 + 1 + 1 + 1 + 1 + kOutFloats + 3) * (int64_t)sizeof(float);
constexpr int64_t kFixedBytes =
    (2 * kNetWorkspace + (int64_t)(kPartStride + kStageWords) * (int64_t)sizeof(float) +
     (int64_t)adamw::params_of(3) * (int64_t)sizeof(double) + 15) / 16 * 16;
static_assert(kCellBytes == DD_PPO_TRAIN_CELL_BYTES, "the header's figure");
static_assert((2 * kNetWorkspace + (int64_t)(kPartStride + kStageWords) * (int64_t)sizeof(float)) % 8 == 0,
              "the accumulators are doubles");

struct Layout {
    int64_t net0, net1, part, stage, acc, obs, bits, reward, old, rowmap, val, ret, raw, adv, out, head, total;
};
__host__ __device__ inline Layout layout_of(int64_t cells) {
    const int64_t c4 = (cells + 3) / 4 * 4 * (int64_t)sizeof(float);  // bytes of one 4-byte column
    Layout l;
    l.net0 = 0;
    l.net1 = kNetWorkspace;
    l.part = 2 * kNetWorkspace;
    l.stage = l.part + (int64_t)kPartStride * (int64_t)sizeof(float);
    l.acc = l.stage + (int64_t)kStageWords * (int64_t)sizeof(float);
    l.obs = kFixedBytes;
    l.bits = l.obs + DD_OBS_DIM * c4;
    l.reward = l.bits + c4;
    l.old = l.reward + c4;
    l.rowmap = l.old + c4;
    l.val = l.rowmap + c4;
    l.ret = l.val + c4;
    l.raw = l.ret + c4;
    l.adv = l.raw + c4;
    l.out = l.adv + c4;
    l.head = l.out + kOutFloats * c4;
    l.total = l.head + 3 * c4;
    return l;
}

struct alignas(16) Member {
    Net net[2];  // actor, critic
    double entropy_coef, value_coef, max_norm;
    uint64_t seed;
    float g, gl;   // gamma and gamma * lambda as gae() rounds them
    float lo, hi;  // the clip range, as float32
    int32_t clip, _pad[3];
};
static_assert(sizeof(Member) % 16 == 0, "the members' workspaces follow the table");

inline int64_t table_bytes(int64_t members) { return members * (int64_t)sizeof(Member); }

struct Args {
    collect::Env env;
    int32_t* lengths;
    uint8_t* ended;
    double* episode_return;
    uint8_t* landed;
    float* record_reward;
    uint8_t* record_done;
    float* record_values;
    float* record_returns;
    float* record_advantages;
    double* logs;
    double* batch_logs;
    uint64_t shuffle_epoch;
    int64_t member_bytes;
    int32_t members, normalize, num_epochs, minibatch, drop_last, log_steps;
};

// The member's batch where the kernel left it: per cell (the record) and per row.
struct Batch {
    const int32_t* rowmap;
    const float* rec_obs;
    const uint32_t* rec_bits;
    const float* rec_old;
    const float* adv;
    const float* ret;
};

// learn<K>'s rows: minibatch i of epoch e is rows perm(i size + k; m, seed, epoch
// + e) of the batch (i size + k without shuffle), read through the row map into
// the stage, as ppo_fused_population.hip stages them from a flat batch.
struct TrainRows {
    const fused::Args& a;
    const Batch& b;
    const uint64_t seed, epoch;
    const bool shuffle;
    uint32_t* stage;  // workspace: kStageWords words
    uint32_t* from;   // LDS: the minibatch's cells, kTileRows words

    struct At {
        uint32_t* stage;
        __device__ __forceinline__ const float* states() const {
            return reinterpret_cast<const float*>(stage + kStageStates);
        }
        __device__ __forceinline__ uint32_t bits(int d) const { return stage[kStageBits + d]; }
        __device__ __forceinline__ float old_log_prob(int d) const { return __uint_as_float(stage[kStageOld + d]); }
        __device__ __forceinline__ float advantage(int d) const { return __uint_as_float(stage[kStageAdv + d]); }
        __device__ __forceinline__ float ret(int d) const { return __uint_as_float(stage[kStageRet + d]); }
    };

    template <bool kActor>
    __device__ __forceinline__ At begin(int epoch_index, int i, int rows) const {
        const int tid = threadIdx.x;
        if (tid < rows) {  // rows <= kTileRows
            const uint32_t j = (uint32_t)(i * a.size + tid);  // < m
            const uint32_t s =
                shuffle ? shuffle::perm(j, shuffle::key_of(a.m, seed, epoch + (uint64_t)epoch_index)) : j;  // < m
            const int32_t cell = b.rowmap[s];
            from[tid] = (uint32_t)cell;
            if constexpr (kActor) {
                stage[kStageBits + tid] = b.rec_bits[cell];
                stage[kStageOld + tid] = __float_as_uint(b.rec_old[cell]);
                stage[kStageAdv + tid] = __float_as_uint(b.adv[s]);
            } else {
                stage[kStageRet + tid] = __float_as_uint(b.ret[s]);
            }
        }
        __syncthreads();
        const uint32_t* src = reinterpret_cast<const uint32_t*>(b.rec_obs);
        for (int idx = tid; idx < rows * DD_OBS_DIM; idx += kBlock) {
            const int r = idx / DD_OBS_DIM, c = idx - r * DD_OBS_DIM;
            stage[kStageStates + idx] = src[(uint64_t)from[r] * DD_OBS_DIM + (uint32_t)c];
        }
        __syncthreads();  // the stage is written; `from` is free again
        return {stage};
    }
};
static_assert(kTileRows * sizeof(uint32_t) <= kBlock * sizeof(ppo::Part), "the cells fit the reductions' scratch");

// The launch's logs: [DD_PPO_FUSED_LOGS][num_epochs][log_steps][members], a.logs at the member's column.
struct StridedLogs {
    int64_t log_steps, members;
    __device__ __forceinline__ double* entry(const fused::Args& a, int epoch, int i) const {
        return a.logs + ((int64_t)epoch * log_steps + i) * members;
    }
    __device__ __forceinline__ int64_t row(const fused::Args& a) const {
        return (int64_t)a.num_epochs * log_steps * members;
    }
};

// The smallest and the largest of value(r) over m rows with Part's node: a NaN is carried on.
template <typename F>
__device__ __forceinline__ void rows_min_max(int64_t m, F value, float* sh, float& lo_out, float& hi_out) {
    const int tid = threadIdx.x;
    ppo::Part acc = ppo::no_rows();
    for (int64_t r = tid; r < m; r += kBlock) {
        const float v = value(r);
        ppo::Part row = {0.0, 0.0, 0.0, 0.0, 0.0, v, v};
        acc += row;
    }
    sh[2 * tid] = acc.rmin;
    sh[2 * tid + 1] = acc.rmax;
    __syncthreads();
    for (int half = kBlock / 2; half > 0; half >>= 1) {
        if (tid < half) {
            ppo::Part mine = {0.0, 0.0, 0.0, 0.0, 0.0, sh[2 * tid], sh[2 * tid + 1]};
            const ppo::Part other = {0.0, 0.0, 0.0, 0.0, 0.0, sh[2 * (tid + half)], sh[2 * (tid + half) + 1]};
            mine += other;
            sh[2 * tid] = mine.rmin;
            sh[2 * tid + 1] = mine.rmax;
        }
        __syncthreads();
    }
    lo_out = sh[0];
    hi_out = sh[1];
    __syncthreads();
}

// num_epochs full-batch steps of one network over M > kTileRows rows: per epoch
// what ppo_losses, MlpNet.backward and AdamW.step launch.  entry: the member's
// column of the logs; log_row: one log row's stride (log_steps is 1 here).
template <int K>
__device__ __forceinline__ void learn_full(const Member& mb, const Net& n, const Batch& b, int64_t M, int num_epochs,
                                           float* out, float* head, float* gpart, double* acc, double* logs,
                                           int64_t members, float* lds) {
    constexpr bool kActor = K == 3;
    constexpr int kCount = adamw::params_of(K);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, c = lane & 31;
    double* part = reinterpret_cast<double*>(reinterpret_cast<char*>(lds) + kRedAt);
    double* redd = part + kStatBlocks;
    double* normp = reinterpret_cast<double*>(reinterpret_cast<char*>(lds) + kNormAt);
    const DDMlpParams p = adamw::params_view(n.params, K, n.ln_eps);
    fused::Running run = fused::running_of(n);
    const double md = (double)M;
    const int64_t log_row = (int64_t)num_epochs * members;

    for (int epoch = 0; epoch < num_epochs; ++epoch) {
        double* entry = logs + (int64_t)epoch * members;
        // ---- forward on every row: the packed image into LDS, a wave per 32 rows ----
        load_image(n.packed, lds);
        __syncthreads();
        for (int64_t first = 0; first < M; first += kTileRows) {
            if (first + wave * mlp::kCols < M) {
                const int64_t r = first + wave * mlp::kCols + c;
                const bool live = r < M;
                const int64_t cell = live ? b.rowmap[r] : 0;
                float x[8], z[K];
                load_row(b.rec_obs + cell * DD_OBS_DIM, live, h, x);
                mlp::mlp_body<K, false>(lds, lane, x, z);
                if (live && h == 0) {
                    if constexpr (kActor) {
                        float prob[3], lp, ent;
                        mlp::actor_probs(z, prob);
                        mlp::actor_evaluate(prob, b.rec_bits[cell], lp, ent);
                        out[r * kOutFloats + 0] = lp;
                        out[r * kOutFloats + 1] = ent;
#pragma unroll
                        for (int j = 0; j < 3; ++j) out[r * kOutFloats + 2 + j] = prob[j];
                    } else {
                        out[r] = z[0];
                    }
                }
            }
        }
        __syncthreads();  // the rows' outputs are written; the image is free

        // ---- dd_ppo_losses: the totals and the gradient rows ---------------------
        if constexpr (kActor) {
            const auto row_of = [&](int64_t r) {
                return ppo::surrogate_of(out[r * kOutFloats], b.rec_old[b.rowmap[r]], b.adv[r], mb.lo, mb.hi);
            };
            ppo::Part t = ppo::no_rows();
            t.surr = rows_total(M, [&](int64_t r) { return row_of(r).smaller(); }, part, redd);
            t.ent = rows_total(M, [&](int64_t r) { return (double)out[r * kOutFloats + 1]; }, part, redd);
            t.r = rows_total(M, [&](int64_t r) { return row_of(r).r; }, part, redd);
            t.clipped = rows_total(M, [&](int64_t r) { return row_of(r).outside ? 1.0 : 0.0; }, part, redd);
            rows_min_max(M, [&](int64_t r) { return row_of(r).rf; }, reinterpret_cast<float*>(redd), t.rmin, t.rmax);
            const double mean = t.r / md;
            const double ss = rows_total(M, [&](int64_t r) {
                const double d = (double)row_of(r).rf - mean;
                return d * d;
            }, part, redd);
            for (int64_t r = tid; r < M; r += kBlock) {
                const double g = row_of(r).grad(md);
                const uint32_t bits = b.rec_bits[b.rowmap[r]];
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    head[r * 3 + j] =
                        ppo::grad_logit_of(g, (bits >> j) & 1u, out[r * kOutFloats + 2 + j], mb.entropy_coef, md);
            }
            if (tid == 0) {
                entry[DD_PPO_POLICY_LOSS * log_row] = ppo::policy_loss_of(t, md);
                entry[DD_PPO_ENTROPY * log_row] = ppo::entropy_of(t, md);
                entry[DD_PPO_RATIO_MEAN * log_row] = mean;
                entry[DD_PPO_RATIO_MIN * log_row] = (double)t.rmin;
                entry[DD_PPO_RATIO_MAX * log_row] = (double)t.rmax;
                entry[DD_PPO_RATIO_STD * log_row] = ppo::ratio_std_of(ss, M);
                entry[DD_PPO_CLIPPED_FRAC * log_row] = t.clipped / md;
            }
        } else {
            const double sq = rows_total(M, [&](int64_t r) {
                const double dv = (double)out[r] - (double)b.ret[r];
                return dv * dv;
            }, part, redd);
            for (int64_t r = tid; r < M; r += kBlock)
                head[r] = ppo::grad_value_of(mb.value_coef, (double)out[r] - (double)b.ret[r], md);
            if (tid == 0) entry[DD_PPO_VALUE_LOSS * log_row] = ppo::value_loss_of(sq, md);
        }

        // ---- dd_mlp_backward for M rows: the blocks' partial sets in block order ---
        for (int idx = tid; idx < kPackedB; idx += kBlock) n.image[idx] = mlpbwd::packed_value(p, idx);
        __syncthreads();  // the images and the head gradient are written
        const int64_t tiles = (M + kTileRows - 1) / kTileRows;
        const int blocks = (int)(tiles < kGradBlocks ? tiles : kGradBlocks);  // the blocks that have a tile
        for (int blk = 0; blk < blocks; ++blk) {
            mlpbwd::backward_block<K>(p, b.rec_obs, head, M, n.image, gpart, blk, kGradBlocks, lds, Cells{b.rowmap});
            __syncthreads();  // the partial set is written
            for (int e = tid; e < kCount; e += kBlock) acc[e] = (blk == 0 ? 0.0 : acc[e]) + (double)gpart[e];
            __syncthreads();  // and read; LDS is free again
        }
        for (int blk = wave; blk < kFinishBlocks; blk += kBlock / 64) {
            double sq[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = blk * kBlock + 64 * j + lane;
                sq[j] = 0.0;
                if (e < kCount) {
                    const float f = (float)acc[e];  // the one rounding
                    n.grads[e] = f;
                    sq[j] = (double)f * (double)f;
                }
            }
            const double sum = wave_block_sum(sq);
            if (lane == 0) normp[blk] = sum;
        }
        __syncthreads();
        const double norm = sqrt(block_sum<double>(tid < kFinishBlocks ? normp[tid] : 0.0, redd));
        if (tid == 0) entry[(kActor ? DD_PPO_POLICY_GRAD_NORM : DD_PPO_CRITIC_GRAD_NORM) * log_row] = norm;

        fused::clip_adamw<K>(n, mb.clip != 0, mb.max_norm, norm, run);
        fused::repack(n, p, lds);
    }
}

template <bool kRef>
__global__ __launch_bounds__(kBlock) void train_kernel(const Member* __restrict__ table, char* workspace, Args a,
                                                       Soa<float> soa) {
    extern __shared__ f32x4 lds4[];
    float* lds = reinterpret_cast<float*>(lds4);
    float* rowbuf = reinterpret_cast<float*>(reinterpret_cast<char*>(lds) + kRowsAt);
    float* tile = lds + kTileAt;
    double* part = reinterpret_cast<double*>(reinterpret_cast<char*>(lds) + kRedAt);
    double* redd = part + kStatBlocks;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, c = lane & 31;
    const int g = blockIdx.x;
    const Member mb = table[g];
    const int L = a.env.lanes, T = a.env.frames;
    const int64_t n = a.env.n;
    const int64_t d0 = (int64_t)g * L;
    const Layout lay = layout_of((int64_t)L * T);
    char* ws = workspace + (int64_t)g * a.member_bytes;
    float* gpart = reinterpret_cast<float*>(ws + lay.part);
    uint32_t* stage = reinterpret_cast<uint32_t*>(ws + lay.stage);
    double* acc = reinterpret_cast<double*>(ws + lay.acc);
    float* rec_obs = reinterpret_cast<float*>(ws + lay.obs);
    uint32_t* rec_bits = reinterpret_cast<uint32_t*>(ws + lay.bits);
    float* rec_reward = reinterpret_cast<float*>(ws + lay.reward);
    float* rec_old = reinterpret_cast<float*>(ws + lay.old);
    int32_t* rowmap = reinterpret_cast<int32_t*>(ws + lay.rowmap);
    float* val = reinterpret_cast<float*>(ws + lay.val);
    float* ret = reinterpret_cast<float*>(ws + lay.ret);
    float* raw = reinterpret_cast<float*>(ws + lay.raw);
    float* adv = reinterpret_cast<float*>(ws + lay.adv);
    float* out = reinterpret_cast<float*>(ws + lay.out);
    float* head = reinterpret_cast<float*>(ws + lay.head);
    const bool mine = tid < L;  // thread k has the member's lane k
    const int64_t d = d0 + (mine ? tid : 0);

    // ---- 1. collect (collect_core.h) ------------------------------------------------------
    const collect::Episode ep = collect::collect_episodes<kRef, true>(a.env, soa, g, mb.net[0].packed, lds, rec_obs,
                                                                      rec_bits, rec_reward, rec_old);
    const int32_t len = ep.len;

    // ---- 2. batch -----------------------------------------------------------------------
    int32_t* len_s = reinterpret_cast<int32_t*>(rowbuf);
    float* boot_s = rowbuf + kTileRows;  // the lanes' bootstrap values, behind their lengths
    static_assert(2 * kTileRows <= kTileRows * kRowFloats, "lengths and bootstrap values fit the per-row buffer");
    __syncthreads();  // the actions in the per-row buffer are read; so is the actor's image
    if (mine) len_s[tid] = len;
    load_image(mb.net[1].packed, lds);  // the critic's; the lanes' final rows stay behind it
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
        a.ended[d] = (uint8_t)(ep.ended ? 1 : 0);
        a.episode_return[d] = ep.ep_return;
        a.landed[d] = (uint8_t)((ep.status & DD_ST_LANDED) ? 1 : 0);
        for (int32_t t = 0; t < len; ++t) rowmap[off + t] = t * L + tid;
        if (a.record_reward) {
            for (int32_t t = 0; t < T; ++t) {
                a.record_reward[(int64_t)t * n + d] = t < len ? rec_reward[(int64_t)t * L + tid] : 0.0f;
                a.record_done[(int64_t)t * n + d] = (uint8_t)(ep.ended && t == len - 1 ? 1 : 0);
            }
        }
    }
    if (wave * mlp::kCols < L) {  // the bootstrap: the critic on the lanes' final observation
        const int r = wave * mlp::kCols + c;
        const bool live = r < L;
        float x[8], z[1];
        load_row(tile + (live ? r : 0) * DD_OBS_DIM, live, h, x);
        mlp::mlp_body<1, false>(lds, lane, x, z);
        if (live && h == 0) boot_s[r] = z[0];
    }
    __syncthreads();  // the row map and the bootstrap values are written
    for (int64_t first = 0; first < M; first += kTileRows) {
        if (first + wave * mlp::kCols < M) {
            const int64_t r = first + wave * mlp::kCols + c;
            const bool live = r < M;
            const int64_t cell = live ? rowmap[r] : 0;
            float x[8], z[1];
            load_row(rec_obs + cell * DD_OBS_DIM, live, h, x);
            mlp::mlp_body<1, false>(lds, lane, x, z);
            if (live && h == 0) val[r] = z[0];
        }
    }
    __syncthreads();  // the values are written; the image is free
    if (mine) {  // batch_adv_kernel's DD_BATCH_GAE branch
        float v_next = ep.ended ? 0.0f : boot_s[tid];
        float mask = ep.ended ? 0.0f : 1.0f;
        float gae = 0.0f;
        for (int32_t t = len - 1; t >= 0; --t) {
            const int64_t o = off + t;
            const float v = val[o];
            const float x = gae_frame(rec_reward[(int64_t)t * L + tid], v, v_next, mask, mb.g, mb.gl, gae);
            raw[o] = x;
            ret[o] = x + v;
            v_next = v;
            mask = 1.0f;
        }
    }
    __syncthreads();  // the raw advantages and the returns are written

    const double md = (double)M;
    const double mean = rows_total(M, [&](int64_t r) { return (double)raw[r]; }, part, redd) / md;
    const double ss = rows_total(M, [&](int64_t r) {
        const double dv = (double)raw[r] - mean;
        return dv * dv;
    }, part, redd);
    const double sd = M < 2 ? __builtin_nan("") : sqrt(ss / (double)(M - 1));  // torch.std's default: unbiased
    {
        const double denom = sd + 1e-8;
        for (int64_t r = tid; r < M; r += kBlock)
            adv[r] = a.normalize ? (float)(((double)raw[r] - mean) / denom) : raw[r];
    }
    __syncthreads();  // the advantages are written
    if (mine && a.record_values) {
        for (int32_t t = 0; t < T; ++t) {
            a.record_values[(int64_t)t * n + d] = t < len ? val[off + t] : 0.0f;
            a.record_returns[(int64_t)t * n + d] = t < len ? ret[off + t] : 0.0f;
            a.record_advantages[(int64_t)t * n + d] = t < len ? adv[off + t] : 0.0f;
        }
    }
    if (tid == 0) {
        double* entry = a.batch_logs + g;
        entry[(int64_t)DD_PT_ROWS * a.members] = md;
        entry[(int64_t)DD_PT_ADV_MEAN * a.members] = mean;
        entry[(int64_t)DD_PT_ADV_STD * a.members] = sd;
    }

    // ---- 3. update ------------------------------------------------------------------------
    const Batch batch = {rowmap, rec_obs, rec_bits, rec_old, adv, ret};
    double* logs = a.logs + g;
    const int64_t count = (int64_t)a.num_epochs * a.log_steps;  // a log row's entries of this member
    int steps = 1;
    if (a.minibatch == 0 && M > kTileRows) {
        learn_full<3>(mb, mb.net[0], batch, M, a.num_epochs, out, head, gpart, acc, logs, a.members, lds);
        learn_full<1>(mb, mb.net[1], batch, M, a.num_epochs, out, head, gpart, acc, logs, a.members, lds);
    } else {
        fused::Args la = {};
        la.num_epochs = a.num_epochs;
        la.m = m32;
        if (a.minibatch == 0) {
            la.size = m32;
        } else {
            la.size = min(a.minibatch, m32);  // as the single call is given it
            steps = a.drop_last ? (m32 < a.minibatch ? 0 : m32 / la.size) : (m32 + la.size - 1) / la.size;
        }
        la.steps = steps;
        la.lo = mb.lo;
        la.hi = mb.hi;
        la.entropy_coef = mb.entropy_coef;
        la.value_coef = mb.value_coef;
        la.max_norm = mb.max_norm;
        la.clip = mb.clip != 0;
        la.logs = logs;
        if (steps < a.log_steps) {  // the steps this member does not take log NaN
            for (int64_t j = tid; j < DD_PPO_FUSED_LOGS * count; j += kBlock) {
                const int64_t i = j % a.log_steps;
                if (i >= steps) logs[j * a.members] = __builtin_nan("");
            }
        }
        uint32_t* from = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(lds) + kRedAt);
        const TrainRows src = {la, batch, mb.seed, a.shuffle_epoch, a.minibatch != 0, stage, from};
        const StridedLogs at_logs = {a.log_steps, a.members};
        fused::learn<3>(la, mb.net[0], src, lds, at_logs);
        fused::learn<1>(la, mb.net[1], src, lds, at_logs);
    }
    // total_loss of every step taken (the steps' logs were written before learn's last barrier)
    for (int64_t j = tid; j < count; j += kBlock) {
        if (j % a.log_steps >= steps) continue;
        double* entry = logs + j * a.members;
        const int64_t log_row = count * a.members;
        entry[DD_PPO_TOTAL_LOSS * log_row] =
            ppo::total_loss_of(entry[DD_PPO_POLICY_LOSS * log_row], entry[DD_PPO_VALUE_LOSS * log_row],
                               entry[DD_PPO_ENTROPY * log_row], mb.entropy_coef, mb.value_coef);
    }
}

inline bool shape_ok(int32_t members, int64_t lanes, int32_t max_steps) {
    return collect::shape_ok(members, lanes, max_steps);
}

// The log's steps per epoch: the most any member can take.
inline int64_t log_steps_of(int64_t lanes, int32_t max_steps, int32_t minibatch) {
    return minibatch == 0 ? 1 : (lanes * (int64_t)max_steps + minibatch - 1) / minibatch;
}

}  // namespace pt
}  // namespace dd

extern "C" {

int64_t dd_ppo_train_workspace(int32_t members, int64_t lanes, int32_t max_steps) {
    using namespace dd::pt;
    if (!shape_ok(members, lanes, max_steps)) return 0;
    return table_bytes(members) + (int64_t)members * layout_of(lanes * (int64_t)max_steps).total;
}

int dd_ppo_train(const DDConfig* cfg, const DDState* st, const DDPpoTrainIO* io, int64_t n, void* workspace,
                 void* stream) {
    using namespace dd::pt;
    if (!cfg || !io || !workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u)) return hipErrorInvalidValue;
    if (!dd::state_ok(st) || st->precision != DD_F32) return hipErrorInvalidValue;
    if (!io->table || !shape_ok(io->members, io->lanes_per_member, io->max_steps)) return hipErrorInvalidValue;
    if (n != (int64_t)io->members * io->lanes_per_member) return hipErrorInvalidValue;
    if (cfg->auto_reset) return hipErrorInvalidValue;  // one episode per lane
    if (!io->obs || !io->lengths || !io->ended || !io->episode_return || !io->landed || !io->logs || !io->batch_logs)
        return hipErrorInvalidValue;
    if (io->num_epochs < 1 || io->minibatch_size < 0 || io->minibatch_size > DD_PPO_FUSED_ROWS)
        return hipErrorInvalidValue;
    const int shape = dd::loop_shape(io->shaped_mode, io->shaped_hist, nullptr, nullptr);
    if (shape < 0) return hipErrorInvalidValue;
    if ((io->record_reward != nullptr) != (io->record_done != nullptr)) return hipErrorInvalidValue;
    if ((io->record_values != nullptr) != (io->record_returns != nullptr) ||
        (io->record_values != nullptr) != (io->record_advantages != nullptr))
        return hipErrorInvalidValue;
    const int32_t members = io->members;
    const int64_t member_bytes = layout_of(io->lanes_per_member * (int64_t)io->max_steps).total;
    const Layout lay = layout_of(io->lanes_per_member * (int64_t)io->max_steps);
    char* blocks = static_cast<char*>(workspace) + table_bytes(members);
    std::vector<Member> table((size_t)members);
    std::vector<dd::fused::Owned> owned;  // every buffer its own owner: no two may overlap
    owned.reserve((size_t)members * 12);
    int32_t owner = 0;
    for (int32_t q = 0; q < members; ++q) {
        const DDPpoTrainMember& m = io->table[q];
        if (!dd::fused::net_ok(m.actor) || !dd::fused::net_ok(m.critic)) return hipErrorInvalidValue;
        if (!__builtin_isfinite(m.gamma) || !__builtin_isfinite(m.lambda)) return hipErrorInvalidValue;
        if (!(m.clip_epsilon >= 0.0) || !__builtin_isfinite(m.clip_epsilon)) return hipErrorInvalidValue;
        if (!__builtin_isfinite(m.entropy_coef) || !__builtin_isfinite(m.value_coef)) return hipErrorInvalidValue;
        if (m.max_grad_norm != m.max_grad_norm) return hipErrorInvalidValue;
        Member& t = table[q];
        char* ws = blocks + (int64_t)q * member_bytes;
        t.net[0] = dd::fused::net_of(m.actor, ws + lay.net0);
        t.net[1] = dd::fused::net_of(m.critic, ws + lay.net1);
        t.entropy_coef = m.entropy_coef;
        t.value_coef = m.value_coef;
        t.max_norm = m.max_grad_norm;
        t.seed = m.shuffle_seed;
        t.g = (float)m.gamma;  // as with_adv_kernel rounds them
        t.gl = (float)(m.gamma * m.lambda);
        t.lo = (float)(1.0 - m.clip_epsilon);
        t.hi = (float)(1.0 + m.clip_epsilon);
        t.clip = dd::fused::clip_of(m.max_grad_norm) ? 1 : 0;
        t._pad[0] = t._pad[1] = t._pad[2] = 0;
        dd::fused::owned_apart(m.actor, 3, owner, owned);
        dd::fused::owned_apart(m.critic, 1, owner, owned);
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
    a.landed = io->landed;
    a.record_reward = static_cast<float*>(io->record_reward);
    a.record_done = io->record_done;
    a.record_values = io->record_values;
    a.record_returns = io->record_returns;
    a.record_advantages = io->record_advantages;
    a.logs = io->logs;
    a.batch_logs = io->batch_logs;
    a.shuffle_epoch = io->shuffle_epoch;
    a.member_bytes = member_bytes;
    a.members = members;
    a.normalize = io->normalize ? 1 : 0;
    a.num_epochs = io->num_epochs;
    a.minibatch = io->minibatch_size;
    a.drop_last = io->drop_last ? 1 : 0;
    a.log_steps = (int32_t)log_steps_of(io->lanes_per_member, io->max_steps, io->minibatch_size);
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
