/*
 * dronestep.h — C-ABI of the MI355X-native vectorised delivery-drone step.
 *
 * This is the drop-in boundary for the reference's per-frame hot path
 * (vedant-jumle/reinforcement-learning-101, delivery_drone/game/):
 *
 *   DroneGame.step     game_engine.py:95-138   -> dd_step
 *   DroneGame.reset    game_engine.py:59-93    -> dd_reset
 *   DroneGame.get_state game_engine.py:140-177 -> dd_write_obs
 *   DroneGame._get_info game_engine.py:281-298 -> dd_get_info
 *   DroneGame.render    game_engine.py:300-337 -> dd_render ('rgb_array' frames)
 *   config.py:17-68 module constants           -> DDConfig (dd_config_default)
 *
 * and for the notebooks' side of the loop:
 *
 *   calc_reward + max_steps  Actor_Critic_PPO.ipynb:164-263, :886-888 -> dd_step (shaped_*)
 *   calc_reward + max_steps  Policy_Gradients.ipynb:162-238, :590-593 (REINFORCE)
 *                                                       -> dd_step (shaped_mode)
 *   the collection loop       Actor_Critic_PPO.ipynb:797-917          -> dd_rollout
 *   DroneGamerBoi / DroneTeacherBoi + Bernoulli.sample / log_prob
 *                             Actor_Critic_PPO.ipynb:376-424, :851-859 -> dd_mlp_forward
 *   compute_gae               Actor_Critic_PPO.ipynb:733-787          -> dd_gae
 *   collect_episodes_ppo with the actor in the loop
 *                             Actor_Critic_PPO.ipynb:797-917          -> dd_policy_rollout
 *   evaluate_policy* (temperature / greedy action selection, one episode per
 *   game, {total_reward, steps, landed, crashed, final_fuel})
 *                             Actor_Critic_PPO.ipynb:1469-1532 (evaluate_policy),
 *                             :997-1101 (evaluate_policy_simple; called at T = 0.3, :1388),
 *                             Actor_Critic_Basic.ipynb:925-988, :638-742,
 *                             Policy_Gradients.ipynb:879-940, :633-738, :1061-1266
 *                             (evaluate_policy_live), Policy_Gradients_inference.ipynb:
 *                             295-356, Actor_Critic_inference.ipynb:229-295, :444-500
 *                                          -> dd_mlp_forward_sampled (one frame's action)
 *                                             dd_policy_rollout_sampled (the episode loop)
 *   evaluate_policy's `rewards` (the calc_reward dicts) as plot_accumulated_rewards /
 *   evaluate_policy_simple accumulate them per component
 *                             Actor_Critic_PPO.ipynb:1469-1532, :1543-1609, :997-1101
 *                                          -> dd_policy_evaluate_parts
 *   run_inference_loop's table for several checkpoints (one policy per group of lanes)
 *                             Actor_Critic_inference.ipynb:229-295   -> dd_policy_rollout_population
 *
 * One call processes a batch of N independent drones stored as a
 * struct-of-arrays (SoA) in device memory.  The reference has no FFI of its
 * own (it is 100 % Python and its only cross-process surface is the JSON
 * socket protocol of game/socket_server.py:126-263); these entry points are
 * what a ctypes / cffi binding of that path binds.
 *
 * Conventions
 *  - The caller owns every buffer.  Nothing here allocates, frees or keeps a
 *    pointer past the call.  All work is enqueued on `stream` (a hipStream_t
 *    passed as void*; NULL = the legacy default stream) and is asynchronous.
 *  - Return value: 0 on success, otherwise a hipError_t code
 *    (1 = hipErrorInvalidValue for argument errors).  No exceptions cross the
 *    ABI.  dd_error_string() turns a code into text.
 *  - Floating-point fields are either all float (DD_F32) or all double
 *    (DD_F64); the arithmetic is always IEEE double, matching the reference's
 *    Python floats, and results are rounded once on store.
 */
#ifndef DRONESTEP_H
#define DRONESTEP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DD_ABI_VERSION 13 /* 13: DDSampling, DDEpisodeStats, dd_mlp_forward_sampled, dd_policy_rollout_sampled (additions only: the
                              spawn stream and every existing entry point are ABI 12's; DDRewardParts and
                              dd_policy_evaluate_parts, then dd_policy_rollout_population, were added to 13 the same way); 12: spawns drawn from Philox4x32-7; 11: shaped_mode (REINFORCE reward), DDRolloutIO.kernel, dd_rollout_kernel,
                              dd_device_errors; 10: DDStepIO.state_out (ping-pong state) */

/* Storage precision of the SoA floating-point fields. */
enum { DD_F32 = 0, DD_F64 = 1 };

/* Action encodings accepted by dd_step (DDStepIO.action_format).
 * The reference takes a dict {main_thrust, left_thrust, right_thrust} and
 * casts each with bool() (game_engine.py:114-118). */
enum {
    DD_ACT_BITMASK = 0, /* uint8[N], bit0 = main, bit1 = left, bit2 = right  */
    DD_ACT_F32X3 = 1,   /* float[N][3] (main, left, right), nonzero = on;     */
                        /* the notebooks' Bernoulli(probs).sample() layout     */
    DD_ACT_U8X3 = 2,    /* uint8/bool[N][3] (main, left, right), nonzero = on */
    DD_ACT_PHILOX = 3   /* dd_rollout only: no action buffer; step s's
                           bitmask is nibble s & 31 of Philox4x32-10(key =
                           action_seed, ctr = {env, s >> 5}) & 7 — a uniform
                           random policy, one block per 32 steps            */
};

/* Status byte bits (DDState.status). */
enum {
    DD_ST_DONE = 1u << 0,    /* DroneGame.done                    */
    DD_ST_LANDED = 1u << 1,  /* Drone.landed                      */
    DD_ST_CRASHED = 1u << 2, /* Drone.crashed                     */
    DD_ST_PLAT_LEFT = 1u << 3 /* Platform.direction == -1 (moving) */
};

/* The notebooks' shaped reward (DDStepIO / DDRolloutIO / DDPolicyRolloutIO
 * shaped_mode), each with its collection loop's max_steps timeout (done, -500
 * unless landed):
 *   DD_SHAPED_PPO        calc_reward(state, prev_state) of Actor_Critic_PPO.ipynb:
 *                        164-263 (also Actor_Critic_Basic), prev_state two frames
 *                        back as collect_episodes_ppo passes it; needs shaped_hist.
 *   DD_SHAPED_REINFORCE  calc_reward(state) of Policy_Gradients.ipynb:162-238
 *                        (distance-scaled time penalty, terminal 500 + fuel * 100
 *                        or -200 / -300), timeout :590-593; no history. */
enum { DD_SHAPED_PPO = 0, DD_SHAPED_REINFORCE = 1 };

/* Width of one observation row: state_to_array order of
 * Actor_Critic_PPO.ipynb:346-366 (x, y, vx, vy, angle, omega, fuel, px, py,
 * distance, dx, dy, speed, landed, crashed), each normalised exactly as
 * DroneGame.get_state (game_engine.py:151-175). */
#define DD_OBS_DIM 15

/* World constants.  dd_config_default() fills the values of config.py. */
typedef struct DDConfig {
    /* physics — config.py:18-29, drone.py:44-103 */
    double gravity;           /* GRAVITY 0.3                  */
    double drag;              /* DRAG 0.99                    */
    double angular_drag;      /* ANGULAR_DRAG 0.95            */
    double main_thrust_power; /* MAIN_THRUST_POWER 0.6        */
    double side_thrust_power; /* SIDE_THRUST_POWER 0.3        */
    double fuel_main;         /* FUEL_CONSUMPTION_MAIN 2.0    */
    double fuel_side;         /* FUEL_CONSUMPTION_SIDE 1.0    */
    double max_fuel;          /* MAX_FUEL 1000.0              */
    double drone_half_height; /* DRONE_HEIGHT / 2 = 10.0 (get_bottom_center) */
    double dt;                /* update(dt=1.0)               */
    /* platform — config.py:32-36, platform.py:11-62 */
    double platform_half_width;  /* PLATFORM_WIDTH / 2 = 50.0  */
    double platform_half_height; /* PLATFORM_HEIGHT / 2 = 10.0 */
    double platform_speed;       /* PLATFORM_SPEED 1.0         */
    double platform_min_x;       /* width // 2 = 50            */
    double platform_max_x;       /* WINDOW_WIDTH - width // 2 = 750 */
    /* landing — config.py:39-40 */
    double max_landing_velocity; /* 3.0  */
    double max_landing_angle;    /* 20.0 */
    /* bounds — config.py:3-4, 45; game_engine.py:254 */
    double world_width;  /* 800 */
    double world_height; /* 600 */
    double oob_margin;   /* 50  */
    double ground_level; /* WINDOW_HEIGHT - 50 = 550 */
    /* wind — config.py:48-49, game_engine.py:121-123 */
    double wind_x, wind_y;
    /* rewards — config.py:54-58, game_engine.py:185-214 */
    double reward_step;          /* -0.1   */
    double reward_landing;       /* 100.0  */
    double reward_crash;         /* -100.0 */
    double reward_out_of_fuel;   /* -50.0  */
    double reward_out_of_bounds; /* -50.0  */
    double shaping_offset;       /* 500  in (500 - dist) / 5000 */
    double shaping_scale;        /* 5000 */
    /* observation scales — game_engine.py:155-171 */
    double vel_scale;   /* 10.0  */
    double angle_scale; /* 180.0 */
    /* spawn — config.py:61-68, game_engine.py:66-85 (integer ranges) */
    int32_t drone_start_x, drone_start_y;         /* fixed spawn 400, 100 */
    int32_t drone_x_min, drone_x_max;             /* inclusive 100..700   */
    int32_t drone_y_min, drone_y_max;             /* inclusive 50..250    */
    int32_t platform_start_x, platform_start_y;   /* fixed 400, 500       */
    int32_t platform_x_lo, platform_x_hi;         /* half-open [100, 700) */
    int32_t platform_y_lo, platform_y_hi;         /* half-open [100, 550) */
    /* switches */
    int32_t wind_enabled;       /* WIND_ENABLED False      */
    int32_t platform_moving;    /* PLATFORM_MOVING False   */
    int32_t randomize_drone;    /* DroneGame(randomize_drone=False)   */
    int32_t randomize_platform; /* DroneGame(randomize_platform=True) */
    int32_t auto_reset;         /* 0: sticky done (game_engine.py:107-111);
                                   1: a lane that is done when dd_step starts is
                                   re-spawned and returns its reset observation
                                   with reward 0 and done 0 (next-step reset). */
    int32_t _pad;
    uint64_t seed; /* key of the spawn draws: Philox4x32-7 of (env id, episode) (ABI 12; 10 rounds before) */
} DDConfig;

/* The SoA.  Every pointer addresses N elements in device memory.  The ten
 * floating-point arrays are float* (DD_F32) or double* (DD_F64). */
typedef struct DDState {
    void *x, *y, *vx, *vy, *angle, *omega, *fuel; /* Drone: drone.py:19-33      */
    void *px, *py;                                /* Platform.x / .y            */
    void *total_reward;                           /* DroneGame.total_reward     */
    uint8_t *status;                              /* DD_ST_* bits               */
    int32_t *steps;                               /* DroneGame.steps            */
    int32_t *episode;                             /* DroneGame.episode          */
    int64_t env_id_base; /* global id of element 0 (sharding-invariant RNG)    */
    int32_t precision;   /* DD_F32 or DD_F64                                   */
    int32_t _pad;
} DDState;

/* Per-call inputs and outputs of dd_step. */
typedef struct DDStepIO {
    const void *actions;  /* see action_format (required)                      */
    int32_t action_format;
    int32_t _pad;
    void *reward;         /* float or double [N] by precision (required)        */
    uint8_t *done;        /* uint8 [N], 1 = done after this call (required)     */
    float *obs;           /* float [N][15] (nullable)                           */
    int32_t *done_idx;    /* lanes whose episode ended in this call, in any
                             order (nullable; wave-ballot compaction)            */
    int32_t *done_count;  /* number of entries written to done_idx (zeroed by
                             dd_step; required iff done_idx != NULL)             */
    /* The notebooks' shaped reward, fused (all three pointers set, or none):
     * calc_reward(state, prev_state) of Actor_Critic_PPO.ipynb:164-263 on the
     * frame's double-precision observation, with prev_state the state two
     * frames back as collect_episodes_ppo passes it (:797-917), plus its
     * max_steps truncation (:886-888: steps >= max_steps ends the episode,
     * -500 unless landed; the lane's done bit is set so it stops / re-spawns). */
    double *shaped_hist;  /* [2][N] per-lane distance history, slot = steps & 1;
                             NaN = no previous state (dd_shaped_reset fills it) */
    void *shaped_reward;  /* float or double [N] by precision                   */
    uint8_t *shaped_done; /* uint8 [N]: done or truncated                        */
    int32_t max_steps;    /* <= 0: no truncation                                 */
    int32_t shaped_mode;  /* DD_SHAPED_PPO (the three pointers above, or none) or
                             DD_SHAPED_REINFORCE (shaped_reward and shaped_done
                             required, shaped_hist not read)                     */
    /* Ping-pong state (nullable = in place): the step reads the nine fields
     * that change every frame (x y vx vy angle omega fuel total_reward steps)
     * from `st` and writes them to *state_out's arrays, which must not alias
     * st's; px, py, status and episode change only on a terminal frame or a
     * re-spawn and stay in place (state_out's pointers for them must equal
     * st's, and so must precision and env_id_base).  Separate in / out arrays
     * spare the kernel the in-place update's end-of-launch write-back of lines
     * it also read.  A sticky-done lane copies its fields. */
    const struct DDState *state_out;
} DDStepIO;

/* Inputs and outputs of dd_rollout: `frames` consecutive frames, frame-major.
 * Buffers are [frames][N] (actions in action_format, reward, done) and
 * [frames][N][15] (obs).  The rollout equals `frames` dd_step calls with
 * actions[k], bit for bit; the state stays in registers between frames. */
typedef struct DDRolloutIO {
    const void *actions;  /* [frames][N] per action_format; NULL for DD_ACT_PHILOX */
    int32_t action_format;
    int32_t frames;
    void *reward;         /* float or double [frames][N] (required)             */
    uint8_t *done;        /* uint8 [frames][N] (required)                       */
    float *obs;           /* float [frames][N][15] (nullable)                   */
    uint64_t action_seed; /* DD_ACT_PHILOX key                                  */
    int64_t action_step;  /* DD_ACT_PHILOX counter of frame 0 (frame k: +k)     */
    /* Notebook reward mode (as DDStepIO's shaped_*): with shaped_mode
     * DD_SHAPED_PPO and shaped_hist set, or DD_SHAPED_REINFORCE, reward / done
     * receive the notebook's calc_reward and done with the max_steps timeout,
     * and the PPO [2][N] history is read at launch and written back at its end.
     * DD_SHAPED_PPO with shaped_hist NULL = the engine reward.              */
    double *shaped_hist;  /* double [2][N] (nullable)                           */
    void *engine_reward;  /* shaped mode: the engine's reward [frames][N] (nullable) */
    uint8_t *engine_done; /* and done; both or neither                          */
    int32_t max_steps;    /* shaped mode: episode cap, <= 0 = none              */
    int32_t shaped_mode;  /* DD_SHAPED_*                                        */
    int32_t kernel;       /* DD_ROLLOUT_AUTO / _SINGLE / _SPLIT_NO_WAIT          */
    int32_t _pad;
} DDRolloutIO;

/* DDRolloutIO.kernel.  AUTO: the split kernel (frame waves + writer waves,
 * DESIGN.md §4) where it applies (reference world, engine reward, obs rows,
 * one block per CU or fewer), the single-role kernel elsewhere.  SINGLE: never
 * the split kernel.  SPLIT_NO_WAIT (diagnostic): as AUTO with the split
 * kernel's hand-over waits capped at zero polls, which reports DD_ERR_HANDOVER
 * through dd_device_errors — the check that a broken hand-over is not silent. */
enum { DD_ROLLOUT_AUTO = 0, DD_ROLLOUT_SINGLE = 1, DD_ROLLOUT_SPLIT_NO_WAIT = 2 };
/* dd_rollout_kernel(): the kernel a dd_rollout call launches (its first chunk). */
enum { DD_ROLLOUT_FLUSHED = 16, DD_ROLLOUT_HELD = 17, DD_ROLLOUT_SPLIT = 18 };

/* Fills *cfg with config.py's values (randomize_platform = 1, others 0). */
void dd_config_default(DDConfig *cfg);

/* One frame for every lane: DroneGame.step (game_engine.py:95-138). */
int dd_step(const DDConfig *cfg, const DDState *st, const DDStepIO *io,
            int64_t n, void *stream);

/* dd_step_variant(): the kernel family a dd_step call takes. */
enum { DD_STEP_GENERIC = 0, DD_STEP_FAST = 1 };

/* Which kernel family dd_step takes for these arguments (its first chunk):
 * DD_STEP_FAST, the kernel with the headline shape's switches compiled in,
 * when the call has reference physics, the engine reward, bitmask actions,
 * auto_reset, randomize_drone and randomize_platform on, a 16-byte aligned
 * obs, no done_idx, no state_out, no shaped pointers, and n is a multiple of
 * 256 and at most 262,144 (beyond it the kernel's extra `episode` load
 * costs more than it saves);
 * DD_STEP_GENERIC for every other call (n = 0 included); -1 for a null
 * argument or an n dd_step refuses.  Both families compute the same bits.
 * Host only: no GPU work, the pointers are not dereferenced. */
int32_t dd_step_variant(const DDConfig *cfg, const DDState *st, const DDStepIO *io,
                        int64_t n);

/* `frames` consecutive frames in one launch (open-loop action sequences,
 * random-policy collection, PPO-shaped rollouts with known actions): the
 * same frame as dd_step, game_engine.py:95-138, applied frames times. */
int dd_rollout(const DDConfig *cfg, const DDState *st, const DDRolloutIO *io,
               int64_t n, void *stream);

/* Which kernel dd_rollout takes for these arguments (DD_ROLLOUT_FLUSHED /
 * _HELD / _SPLIT), -1 for invalid ones.  No GPU work. */
int dd_rollout_kernel(const DDConfig *cfg, const DDState *st, const DDRolloutIO *io,
                      int64_t n);

/* Sticky error bits the kernels set on the device (DD_ERR_*), read after a
 * hipDeviceSynchronize (work on every stream, non-blocking ones included, has
 * finished) and cleared if `clear`. */
enum { DD_ERR_HANDOVER = 1 }; /* a split-rollout hand-over wait ran out: rows of
                                 that launch are not to be trusted */
int dd_device_errors(uint32_t *bits, int32_t clear);

/* Re-spawn lanes (DroneGame.reset, game_engine.py:59-93).  mask: uint8 [N],
 * nonzero = reset that lane; NULL = all lanes.  obs (nullable) receives the
 * reset observation of the reset lanes; other rows are left untouched. */
int dd_reset(const DDConfig *cfg, const DDState *st, const uint8_t *mask,
             float *obs, int64_t n, void *stream);

/* (Re)start the shaped-reward history of the masked lanes (NULL = all) from
 * their current state: slot 0 = this state's distance, slot 1 = none.  Call
 * after dd_reset; auto-reset inside dd_step restarts it by itself. */
int dd_shaped_reset(const DDConfig *cfg, const DDState *st, const uint8_t *mask,
                    double *shaped_hist, int64_t n, void *stream);

/* Observation rows from the current state (DroneGame.get_state). */
int dd_write_obs(const DDConfig *cfg, const DDState *st, float *obs,
                 int64_t n, void *stream);

/* Pixel-unit distance to the platform and speed (DroneGame._get_info,
 * game_engine.py:292-296); float or double [N] by precision. */
int dd_get_info(const DDConfig *cfg, const DDState *st, void *distance,
                void *speed, int64_t n, void *stream);

/* Ordered compaction: idx_out receives, in ascending order, every i with
 * (flags[i] != 0) == (want != 0); *count its length.  Builds the notebooks'
 * active-game list (Actor_Critic_PPO.ipynb:840-850) on device.
 * workspace: int32 [dd_compact_workspace(n)] scratch. */
int64_t dd_compact_workspace(int64_t n);
int dd_compact(const uint8_t *flags, int32_t want, int32_t *idx_out,
               int32_t *count, int32_t *workspace, int64_t n, void *stream);

/* Generalised advantage estimation over a [T][N] rollout (compute_gae of
 * Actor_Critic_PPO.ipynb:733-787, per lane; a done at t cuts the recursion):
 *   delta = r[t] + gamma * v[t+1] * (1 - d[t]) - v[t]
 *   gae   = delta + gamma * lambda * (1 - d[t]) * gae
 * in float32 with the notebook's operation order (torch float32 tensors,
 * Python-float gamma / lambda).  values is [T+1][N] (row T = bootstrap).
 * returns (nullable) = advantages + values[t], as the notebook forms them. */
int dd_gae(const float *rewards, const float *values, const uint8_t *dones,
           float *advantages, float *returns, int64_t T, int64_t n,
           double gamma, double lambda, void *stream);

/* ---- Policy and value networks ------------------
 * The notebooks' DroneGamerBoi (actor) and DroneTeacherBoi (critic),
 * Actor_Critic_PPO.ipynb:376-424:
 *   Linear(15,128) LayerNorm(128) ReLU  Linear(128,128) LayerNorm(128) ReLU
 *   Linear(128,64) LayerNorm(64) ReLU   Linear(64,K)  [+ Sigmoid, actor]
 * with K = 3 (main, left, right) for the actor and K = 1 for the critic, in
 * float32.  The parameters are the state_dict tensors (torch layout: weight
 * [out][in] row-major, device pointers), repacked once by dd_mlp_pack into
 * the kernel's MFMA operand order. */
typedef struct DDMlpParams {
    const float *w0, *b0, *ln1_w, *ln1_b; /* network.0 (Linear), network.1 (LayerNorm) */
    const float *w3, *b3, *ln4_w, *ln4_b; /* network.3, network.4 */
    const float *w6, *b6, *ln7_w, *ln7_b; /* network.6, network.7 */
    const float *w9, *b9;                 /* network.9: [K][64], [K] */
    int32_t out_dim;                      /* K: 3 (actor) or 1 (critic) */
    float ln_eps;                         /* nn.LayerNorm eps (1e-5) */
} DDMlpParams;

/* One forward pass over N observation rows.  The actor (K = 3) writes the
 * Sigmoid probabilities, and optionally samples actions as
 * Bernoulli(probs).sample() (Actor_Critic_PPO.ipynb:857-858: bit j set iff
 * u_j < p_j, u_j uniform in [0,1) from Philox4x32-10 keyed by
 * (seed; env_id_base + i, step, 0x5A5A5A5A)) packed as the dd_step bitmask,
 * with Bernoulli.log_prob(actions).sum(-1) (:859).  The critic (K = 1)
 * writes the value. */
typedef struct DDMlpIO {
    const float *obs;    /* [N][15] f32, dd_step / dd_write_obs rows */
    float *out;          /* nullable: [N][3] probabilities (actor) or [N] values (critic) */
    uint8_t *actions;    /* actor, nullable: uint8 [N] sampled bitmask */
    float *log_prob;     /* actor, nullable: [N] summed log-probability of `actions` */
    uint64_t seed;
    int64_t step;
    int64_t env_id_base;
} DDMlpIO;

/* Arithmetic of the three hidden GEMMs.  DD_MLP_F32: the f32 MFMA, the
 * notebook's float32 model as is.  DD_MLP_F16X3 (opt-in, ~2.7x faster:
 * 65,536 rows 33 -> 12-13 us on MI355X): each operand split into two f16
 * halves, a = hi + lo, three f16 MFMAs per product with f32 accumulation
 * (~21-22 bits per product, about the f32 path's end-to-end error).  Its
 * operands must fit the f16 halves at the packing's powers of two: hidden
 * weights |w| < 2047, observations |obs| < 1023, each LayerNorm's output
 * below 128 (max|weight| sqrt(rows) + max|bias| < 128); beyond, results are
 * wrong or NaN (MlpNet checks the parameters before packing).  LayerNorm,
 * the last layer and sampling are f32 either way. */
enum { DD_MLP_F32 = 0, DD_MLP_F16X3 = 1 };

/* Floats of a packed parameter buffer (same for K = 1 and 3, either compute).
 * The buffer ends in a layout tag: the compute and K it was packed for.  A
 * consumer launched with another compute or K (or, for dd_policy_rollout, a
 * critic's buffer) does not misread it: its probabilities, log-probabilities
 * and values come out NaN. */
int64_t dd_mlp_packed_floats(void);
/* Repack state_dict tensors into `packed` (device, dd_mlp_packed_floats()
 * floats, 16-byte aligned: every consumer reads it in 16-byte fragments;
 * a misaligned pointer is hipErrorInvalidValue) for `compute` (DD_MLP_*). */
int dd_mlp_pack(const DDMlpParams *params, int32_t compute, float *packed, void *stream);
/* Forward pass; out_dim and compute must match the packed parameters. */
int dd_mlp_forward(const float *packed, int32_t compute, int32_t out_dim,
                   const DDMlpIO *io, int64_t n, void *stream);

/* ---- Action selection of the notebooks' evaluate_policy* cells (ABI 13) -----
 * Every evaluate_policy, evaluate_policy_simple and evaluate_policy_live picks
 * its action as
 *   temperature == 0:  action = probs > 0.5
 *   else:              q = p^(1/T) / (p^(1/T) + (1-p)^(1/T));  action = Bernoulli(q).sample()
 * DD_SAMPLE_BERNOULLI  the collection loop's Bernoulli(probs).sample(), as
 *                      dd_mlp_forward / dd_policy_rollout draw it (T = 1).
 * DD_SAMPLE_TEMPERED   T > 0 and finite: q_k = Sigmoid(z_k / T) on the last
 *                      layer's outputs z before the Sigmoid, which is the
 *                      formula above (p / (1 - p) = e^z) without its float32
 *                      loss of 1 - p.  The same Philox4x32-10 draw and keying:
 *                      bit k iff u_k < q_k.  log_prob is
 *                      Bernoulli(q).log_prob(a).sum(), the distribution drawn
 *                      from.
 * DD_SAMPLE_GREEDY     bit k iff p_k > 0.5 on the kernel's own float32 p (what
 *                      `out` receives); nothing is drawn.  log_prob is that
 *                      action's log-probability under p. */
enum { DD_SAMPLE_BERNOULLI = 0, DD_SAMPLE_TEMPERED = 1, DD_SAMPLE_GREEDY = 2 };
typedef struct DDSampling {
    int32_t mode;       /* DD_SAMPLE_*                                          */
    float temperature;  /* DD_SAMPLE_TEMPERED only                              */
    float *probs_used;  /* nullable; forward: [N][3]; rollout: [frames][N][3]:
                           the probabilities the draw was compared with (p, q,
                           or p for DD_SAMPLE_GREEDY)                           */
} DDSampling;

/* dd_mlp_forward with the action selected by *sampling (actor only).
 * sampling == NULL is dd_mlp_forward exactly.  hipErrorInvalidValue, before
 * any launch: an unknown mode, DD_SAMPLE_TEMPERED with a temperature that is
 * not finite or <= 0, a non-NULL sampling with out_dim == 1. */
int dd_mlp_forward_sampled(const float *packed, int32_t compute, int32_t out_dim,
                           const DDMlpIO *io, const DDSampling *sampling, int64_t n,
                           void *stream);

/* ---- Scoring given actions (compute_ppo_losses' first lines) ---------------
 * compute_ppo_losses (Actor_Critic_PPO.ipynb, the cell after
 * collect_episodes_ppo) re-evaluates the actor on the batch's states and
 * scores the actions that were taken:
 *   dist = Bernoulli(probs=policy(states))
 *   new_log_probs = dist.log_prob(actions).sum(dim=1);  dist.entropy()
 * dd_mlp_evaluate_actions is dd_mlp_forward's actor (K = 3, either compute)
 * with the action an input instead of a draw.  actions: DD_ACT_BITMASK, uint8
 * [n], bits 0-2 as dd_step reads them; or DD_ACT_F32X3, float [n][3] (main,
 * left, right), where a float is "on" by dd_step's rule for that format:
 * nonzero = on (a != 0.0f, so -0.0 is off and NaN is on).
 * log_prob: dd_mlp_forward's own arithmetic (each factor p or 1 - p on the
 * probability clamped to [FLT_EPSILON, 1 - FLT_EPSILON], one logf of the
 * three factors' product), so for the actions dd_mlp_forward drew on the same
 * rows it is bit-equal to the log_prob that call wrote.  entropy: the row's
 * sum over its three factors of -(pc log pc + (1 - pc) log(1 - pc)) on the
 * same clamped pc, Bernoulli(probs=p).entropy().  A buffer packed for the
 * other compute or for K = 1 gives NaN probabilities, log_prob and entropy.
 * hipErrorInvalidValue, before any HIP call: a null io, n < 0, an unknown
 * format or compute; and with n > 0 a null or misaligned packed pointer, null
 * obs or null actions.  n == 0 is success. */
typedef struct DDMlpEvalIO {
    const float *obs;      /* [n][15] f32                                        */
    const void *actions;   /* by action_format (required)                        */
    int32_t action_format; /* DD_ACT_BITMASK or DD_ACT_F32X3                     */
    int32_t _pad;
    float *probs;          /* nullable: [n][3] Sigmoid probabilities             */
    float *log_prob;       /* nullable: [n] summed log-probability of `actions`  */
    float *entropy;        /* nullable: [n] the three factors' entropies, summed */
    int64_t n;
} DDMlpEvalIO;

int dd_mlp_evaluate_actions(const float *packed, int32_t compute, const DDMlpEvalIO *io,
                            void *stream);

/* ---- The collection loop with the actor in it --
 * collect_episodes_ppo (Actor_Critic_PPO.ipynb:797-917) for N drones and
 * `frames` frames in one launch: per frame, the actor on the current
 * observation (dd_mlp_forward's network and sampling, :851-859), then the
 * drone frame (dd_step) with the sampled action.  Frame k writes
 *   obs[k]      the policy input (the observation before the frame; frame 0's
 *               is obs0, later ones are the previous frame's dd_step obs)
 *   actions[k], log_prob[k]   as dd_mlp_forward with step = step + k
 *   reward[k], done[k]        as dd_step (reward_mode as DDRolloutIO)
 * and obs_final receives the observation after the last frame.  Equal, bit
 * for bit, to `frames` x (dd_mlp_forward(obs) ; dd_step(actions)) with the
 * state's env ids as the sampling ids.  The actor's packed parameters
 * (dd_mlp_pack, out_dim 3) are read into LDS once per launch. */
typedef struct DDPolicyRolloutIO {
    const float *obs0;    /* [N][15] observation before frame 0 (required)      */
    float *obs_final;     /* [N][15] observation after the last frame (nullable;
                             may be obs0)                                        */
    float *obs;           /* [frames][N][15] policy inputs (nullable)           */
    uint8_t *actions;     /* [frames][N] sampled bitmask (nullable)             */
    float *log_prob;      /* [frames][N] summed log-probability (nullable)      */
    void *reward;         /* float or double [frames][N] by precision (required) */
    uint8_t *done;        /* uint8 [frames][N] (required)                       */
    uint64_t seed;        /* Bernoulli draws: Philox4x32-10 key                 */
    int64_t step;         /* sampling step of frame 0 (frame k: step + k)       */
    int32_t frames;
    int32_t max_steps;    /* notebook mode: episode cap, <= 0 = none            */
    double *shaped_hist;  /* notebook reward mode, as DDRolloutIO (nullable)    */
    void *engine_reward;  /* notebook mode: the engine's reward / done          */
    uint8_t *engine_done; /* [frames][N] (both or neither, nullable)            */
    int32_t shaped_mode;  /* DD_SHAPED_* as DDRolloutIO                         */
    int32_t _pad;
} DDPolicyRolloutIO;

int dd_policy_rollout(const DDConfig *cfg, const DDState *st, const float *packed,
                      int32_t compute, const DDPolicyRolloutIO *io, int64_t n,
                      void *stream);

/* Per-lane episode statistics of a policy rollout: the notebooks'
 * evaluate_policy result {total_reward, steps, landed, crashed, final_fuel}
 * for every lane.  All four pointers set (or all NULL = no statistics).  They
 * are in/out accumulators that carry across launches, so a long evaluation
 * may be chunked; the caller zeroes them before an episode.  A lane adds to
 * them only while ep_status[i] & DD_ST_DONE is clear at the start of the
 * frame, so its first episode is counted once, whatever the env does after it
 * (sticky done or re-spawn).  The flag that ends the episode is the one
 * done[k] carries: the notebook's done in the notebook reward modes. */
typedef struct DDEpisodeStats {
    double *ep_return;  /* [N] sum of the stored reward values (as written to
                           `reward`, i.e. rounded to the storage precision),
                           added in double, in frame order                      */
    int32_t *ep_steps;  /* [N] frames played                                    */
    uint8_t *ep_status; /* [N] DD_ST_* of the frame that ended the episode
                           (DD_ST_DONE set), else 0                             */
    void *ep_fuel;      /* [N] float / double by precision: fuel after the last
                           frame played                                         */
} DDEpisodeStats;

/* dd_policy_rollout with the action selected by *sampling (probs_used:
 * [frames][N][3]) and per-lane episode statistics.  sampling == NULL and
 * stats == NULL are dd_policy_rollout exactly.  With statistics, io's reward,
 * done, actions and log_prob may all be NULL: an evaluation then writes no
 * [frames][N] buffer at all.  The notebooks' evaluation stops at max_steps
 * without the collection loops' timeout penalty: pass io->max_steps = 0 and
 * max_steps frames.  hipErrorInvalidValue, before any launch: an unknown
 * mode, DD_SAMPLE_TEMPERED with a temperature that is not finite or <= 0, a
 * DDEpisodeStats with some but not all pointers set. */
int dd_policy_rollout_sampled(const DDConfig *cfg, const DDState *st, const float *packed,
                              int32_t compute, const DDPolicyRolloutIO *io,
                              const DDSampling *sampling, const DDEpisodeStats *stats,
                              int64_t n, void *stream);

/* ---- A population of actors in one launch -----------------------------------
 * dd_policy_rollout_sampled with the lanes [0, n) split into `members`
 * contiguous groups of lanes_per_member = L lanes, group g driven by the packed
 * image packed_table[g] (dd_mlp_pack, out_dim 3, all of `compute`): checkpoint
 * tournaments and sweeps fill the card with one launch where P launches of L
 * lanes each leave most of it idle.  Equal, bit for bit, to `members` calls of
 * dd_policy_rollout_sampled on the sub-batches [g L, (g+1) L), each with
 * env_id_base + g L and packed_table[g], writing the matching lane columns of
 * the same [frames][n] buffers, shaped_hist [2][n] and DDEpisodeStats [n]
 * (Philox is keyed by env id, so a lane's draws do not depend on its group's
 * neighbours).  members == 1 is dd_policy_rollout_sampled exactly.
 * packed_table is DEVICE memory, [members] pointers to device images, each
 * 16-byte aligned, and is read by the kernel: the call copies no weight and
 * no pointer, so a member re-packed in place (same address) is seen by the next
 * launch on the stream, and the table must stay valid until the launch is done.
 * A block of 256 lanes belongs to one group (the grid is members *
 * ceil(L / 256) blocks); an image of the wrong layout gives NaN by its tag, as
 * in dd_mlp_forward.
 * hipErrorInvalidValue, before any launch: every argument error of
 * dd_policy_rollout_sampled; a NULL or not 8-byte-aligned packed_table;
 * members < 1; lanes_per_member < 1; members * lanes_per_member != n for
 * n > 0.  n == 0 and frames == 0 behave as in dd_policy_rollout_sampled. */
int dd_policy_rollout_population(const DDConfig *cfg, const DDState *st,
                                 const float *const *packed_table, int32_t members,
                                 int64_t lanes_per_member, int32_t compute,
                                 const DDPolicyRolloutIO *io, const DDSampling *sampling,
                                 const DDEpisodeStats *stats, int64_t n, void *stream);

/* ---- evaluate_policy with the reward's components ---------------------------
 * calc_reward returns a dict; the notebooks' evaluate_policy keeps the list of
 * them (`rewards`) and plot_accumulated_rewards / evaluate_policy_simple draw
 * the running sum of every key.  dd_policy_evaluate_parts is the evaluation
 * loop of dd_policy_rollout_sampled (sticky done, DDSampling, DDEpisodeStats)
 * keeping the frame's DD_REWARD_PARTS = 8 values, in the notebooks' key order:
 *   slot  Actor_Critic_PPO / _Basic (DD_SHAPED_PPO)   Policy_Gradients (DD_SHAPED_REINFORCE)
 *   0     time_penalty                                time_penalty
 *   1     distance                                    distance
 *   2     hovering                                    velocity_alignment
 *   3     angle                                       angle
 *   4     speed                                       speed
 *   5     vertical_position                           vertical_position
 *   6     terminal                                    terminal
 *   7     total                                       total
 * total is summed in the notebook's order from the same doubles as the slots.
 * The PPO notebook's quirk is kept: its time_penalty entry is
 * -inverse_quadratic(dist, decay=100, scaler=1), but its total adds the literal
 * -0.5 instead, so there slot 0 is reported and is NOT a term of slot 7
 * (slot 7 = -0.5 + slots 1..6).  REINFORCE's slot 7 = slots 0..6, and equals
 * the reward dd_step / dd_policy_rollout_sampled store, bit for bit.
 * Rounding: a frame's eight values are the doubles rounded to the state's
 * storage width (float / double by precision), as the stored reward is; the
 * sums are double, added in frame order under DDEpisodeStats' rule (while
 * ep_status[i] & DD_ST_DONE is clear at the start of the frame, the frame that
 * ends the episode included).  Frames after a lane's episode has ended add
 * nothing, and per_frame holds zeros for them.
 * prev_state (PPO shape): the notebooks' evaluation passes the state the actor
 * saw, ONE frame back; prev_dist[i] is that state's distance_to_platform as a
 * double (of the unrounded frame).  The caller sets it before frame 0 to the
 * reset state's value (dd_shaped_reset's slot 0; never NaN: prev_state is
 * present from frame 0 on) and the call carries it forward, so the results do
 * not depend on how the frames are split into launches.  The collection
 * loop's two-frame history io->shaped_hist only selects the PPO shape, as in
 * dd_policy_rollout_sampled: it is neither read nor written. */
#define DD_REWARD_PARTS 8
typedef struct DDRewardParts {
    double *sum;       /* [8][N] in/out: per-episode sums, slot-major (required) */
    double *prev_dist; /* [N] in/out; required for the PPO shape, unused otherwise */
    void *per_frame;   /* [frames][8][N] float / double by precision, or NULL    */
} DDRewardParts;

/* io->obs0, obs_final, obs, actions, log_prob, reward, done, seed, step and
 * frames as dd_policy_rollout_sampled (all per-frame buffers nullable);
 * reward[k] is slot 7 of frame k.  io->max_steps is not read: the notebooks'
 * evaluation stops after its frames without the collection loops' timeout
 * penalty.  hipErrorInvalidValue, before any launch: every argument error of
 * dd_policy_rollout_sampled (sampling mode, temperature, compute, packed
 * alignment, n < 0, frames < 0); a NULL parts or parts->sum; the PPO shape with
 * a NULL prev_dist; the engine's reward (DD_SHAPED_PPO with a NULL shaped_hist:
 * it has no notebook components); io->engine_reward / engine_done set (not
 * written here); cfg->auto_reset (one episode per lane); stats NULL or with
 * fewer than its four pointers.  n == 0 is success; so is frames == 0, which
 * writes obs_final if set and leaves every accumulator as it was. */
int dd_policy_evaluate_parts(const DDConfig *cfg, const DDState *st, const float *packed,
                             int32_t compute, const DDPolicyRolloutIO *io,
                             const DDSampling *sampling, const DDEpisodeStats *stats,
                             const DDRewardParts *parts, int64_t n, void *stream);

/* ---- Rendering -------------------------------------
 * DroneGame.render() in 'rgb_array' mode (game_engine.py:300-337): the scene
 * of platform.py:76-102, drone.py:155-218, _render_hud (game_engine.py:339-384)
 * and, for a lane that is done, _render_game_over (:386-412), as
 * surfarray.array3d(screen).transpose(1, 0, 2) gives it: uint8 [H][W][3] with
 * W x H = world_width x world_height (800 x 600; width a multiple of 4).
 * pygame's primitives are restated (render.hip's header), not pixel-verified:
 * pygame is absent here, and the text uses DejaVu Sans Bold for pygame's
 * bundled font. */
enum { DD_RENDER_HUD = 1, DD_RENDER_GAME_OVER = 2, DD_RENDER_LABELS = 4 /* dd_render_grid only */ };

/* Renders `count` frames into rgb: uint8 [count][H][W][3].  The SoA holds n
 * lanes.  lanes: int32 [count] device indices into it, or NULL for lanes
 * 0..count-1 (count <= n); a frame whose index is outside [0, n) is left
 * all zero.  actions (nullable): the uint8 [n] bitmask of the last step, which
 * _render_thrust draws as flames (drone.py:189-218, where fuel > 0); NULL
 * draws none, and so does a lane whose steps is 0 (Drone.reset clears the
 * thrusters).  flags: DD_RENDER_*. */
int dd_render(const DDConfig *cfg, const DDState *st, const uint8_t *actions,
              const int32_t *lanes, int64_t count, int64_t n, uint8_t *rgb,
              int32_t flags, void *stream);

/* The composite of socket_server.py --render-all (:155-225): the same `count`
 * frames as tiles of one surface, rgb: uint8 [rows * H][cols * W][3].  Slot
 * k < count is the tile at row k / cols, column k % cols, and holds exactly
 * dd_render's frame k for the same arguments; the frame is stored straight
 * into the mosaic (no intermediate, no second pass).  With DD_RENDER_LABELS,
 * "Game {lane}" (the reference's game id; pygame.font.Font(None, 36), yellow)
 * is blended over each tile with its top left at (10, 10) of the tile, after
 * the HUD and the game-over overlay.  Unlike pygame, which clips to the whole
 * surface, the label is clipped to its own tile (visible only where a tile is
 * narrower than its label and the next tile is empty).  Every byte of rgb is
 * written: tiles count <= k < rows * cols are all zero, and so is, without a
 * label, a slot whose lane is outside [0, n).  Checks what dd_render checks,
 * and cols >= 1, rows >= 1, count <= rows * cols <= 65535; count == 0 blacks
 * out the whole grid.  dd_render ignores DD_RENDER_LABELS. */
int dd_render_grid(const DDConfig *cfg, const DDState *st, const uint8_t *actions,
                   const int32_t *lanes, int64_t count, int64_t n,
                   int32_t cols, int32_t rows, uint8_t *rgb, int32_t flags, void *stream);

/* Algorithmic HBM bytes of one dd_step lane (the roofline byte model,
 * DESIGN.md §4): precision, action format, obs on/off. */
int64_t dd_step_bytes_per_env(int32_t precision, int32_t action_format,
                              int32_t with_obs);

const char *dd_error_string(int code);
int dd_abi_version(void);
/* "abi=<n>;step_isa=<sha256/16>;policy_rollout_isa=<sha256/16>": the ABI version
 * and hashes of the device ISA this library was built with (tools/build_info.py);
 * bench.py reports PMC traffic only for the build it was measured on. */
const char *dd_build_info(void);

/* Self-check of the frame's square root (not a reference interface): the
 * kernels take sqrt through an unscaled form of the compiler's sequence
 * (trig.h sqrt_unscaled) for operands >= 2^-767.  Evaluates both on n
 * doubles (the integers 0..2^20, then Philox-drawn values with exponents
 * spread over the whole range) and adds the number whose results differ in
 * any bit to *mismatches (device memory). */
int dd_selftest_sqrt(uint64_t seed, int64_t n, unsigned long long *mismatches, void *stream);

/* Measurement helpers for bench.py (not reference interfaces).  dd_stamp
 * launches a one-lane kernel on `stream` that writes the GPU's constant-rate
 * wall clock to *slot (device memory) when it runs; captured into a hipGraph
 * between step launches it stamps that point of the graph.  dd_wall_clock_khz
 * gives the clock's rate (hipDeviceAttributeWallClockRate, current device). */
int dd_stamp(unsigned long long *slot, void *stream);
int dd_wall_clock_khz(int *khz);

/* Device memory for an env's arrays (not a reference interface;
 * VecDroneEnv(memory=...) carves its SoA fields and per-step outputs from
 * one range).  DD_MEM_DEFAULT: hipMalloc.  DD_MEM_CONTIGUOUS:
 * hipExtMallocWithFlags(hipDeviceMallocContiguous), one physically
 * contiguous range: an HBM-resident batch (16.8M drones) steps at the same
 * speed from every such allocation (within ~1 %) where hipMalloc'd ones vary
 * ~10 % with the driver's placement, but a cache-resident
 * batch (262,144 drones) steps ~35 % slower from it (profiles/r06/lab/).
 * dd_device_free(NULL) is a no-op. */
#define DD_MEM_DEFAULT 0
#define DD_MEM_CONTIGUOUS 1
int dd_device_alloc(void **ptr, uint64_t bytes, int32_t flags);
int dd_device_free(void *ptr);

/* ---- Training batches from rollout buffers ------------------------------
 * The stretch between a finished rollout and the tensors the notebooks' loss
 * functions take: Actor_Critic_PPO.ipynb's training cell ("PHASE 2": per
 * episode stack the states, run the critic, compute_gae, returns = advantages
 * + values; then torch.cat over the episodes and normalise the advantages),
 * and Policy_Gradients.ipynb's (per episode compute_returns; then the
 * baseline and the same normalisation).  The input is one rollout as the
 * policy rollout returns it: done uint8 [T][N], reward [T][N], and optionally
 * obs float [T][N][15], actions uint8 bitmasks [T][N], log_prob float [T][N].
 * Only each lane's FIRST episode counts, and the layout is decided by `done`
 * alone (the same on a sticky-done and an auto-reset env).
 *
 * DDBatchLayout (caller-owned, device): length int32 [N], (first t with
 * done[t][i] != 0) + 1 or T if there is none; ended uint8 [N], which of the
 * two; offset int64 [N + 1], the exclusive prefix sum of length, offset[N] =
 * M the batch size.  Row offset[i] + t of every flat buffer is lane i's frame
 * t: episode-major, the order of the notebook's torch.cat.  All index
 * arithmetic is 64-bit.
 *
 * The plan writes a DDBatchLayout (deterministic scan; the host reads M =
 * offset[N] to size the flat buffers); the other stages read it.  workspace:
 * the workspace function's count of bytes, 8-byte aligned, shared by the plan
 * and the normalisation (calls on one stream may reuse it). */
typedef struct DDBatchLayout {
    int32_t *length;
    int64_t *offset;
    uint8_t *ended;
} DDBatchLayout;

int64_t dd_batch_workspace(int64_t n);
int dd_batch_plan(const uint8_t *done, int64_t T, int64_t n, const DDBatchLayout *layout,
                  void *workspace, void *stream);

/* Gather (the notebook's torch.stack per episode + torch.cat): states [M][15]
 * from obs, actions_out float [M][3] = 1.0 / 0.0 in (main, left, right) order
 * (the Bernoulli.sample() layout compute_ppo_losses consumes) from the
 * bitmasks, old_log_probs [M] from log_prob.  Each input is optional together
 * with its output (one without the other: hipErrorInvalidValue).  No row >=
 * M is written.  tile_frames: the frames of one LDS tile (64 lanes x
 * tile_frames frames per block), 8 or 16, 0 = the default (8). */
typedef struct DDBatchGatherIO {
    const float *obs;
    const uint8_t *actions;
    const float *log_prob;
    float *states;
    float *actions_out;
    float *old_log_probs;
    int32_t tile_frames;
    int32_t _pad;
} DDBatchGatherIO;

int dd_batch_gather(const DDBatchLayout *layout, const DDBatchGatherIO *io, int64_t T, int64_t n,
                    void *stream);

/* Advantages over the flat layout, one episode per lane.  Both modes write
 * episode_return double [N] (nullable): the lane's rewards summed in frame
 * order in double, the notebooks' sum(rewards).
 * DD_BATCH_GAE (Actor_Critic_PPO.ipynb:733-787 as its training cell calls it):
 *   values float [M] (the critic on the gathered states), bootstrap float [N]
 *   (nullable = 0): the value of the state after frame T-1, used only by
 *   lanes with ended == 0.  dones is all false but the last frame of an ended
 *   episode; rewards are rounded to float32 first; the recursion is the
 *   rectangular GAE's, bit for bit.  advantages float [M], returns (nullable)
 *   = advantages + values.
 * DD_BATCH_RETURNS (compute_returns, Policy_Gradients.ipynb): G = r + gamma *
 *   G backwards in double on the reward as stored, rounded to float32 once
 *   (torch.tensor(batch_returns, dtype=float32)) into returns float [M].
 * precision: the reward's storage, DD_F32 or DD_F64. */
#define DD_BATCH_GAE 0
#define DD_BATCH_RETURNS 1
typedef struct DDBatchAdvIO {
    const void *reward;
    int32_t precision;
    int32_t mode;
    const float *values;
    const float *bootstrap;
    float *advantages;
    float *returns;
    double *episode_return;
    double gamma;
    double lambda;
} DDBatchAdvIO;

int dd_batch_advantages(const DDBatchLayout *layout, const DDBatchAdvIO *io, int64_t T, int64_t n,
                        void *stream);

/* Batch statistics and normalisation of x float [m] (the advantages, or
 * REINFORCE's returns): *mean and *std (device doubles; std unbiased, as
 * torch.std's default) accumulated in double by a reduction tree of fixed
 * shape (no atomics: the same bits on every run), and out (nullable; may be
 * x) = (x - mean) / (std + 1e-8) evaluated in double and rounded to float32
 * once: the notebooks' `(a - a.mean()) / (a.std() + 1e-8)`, and for REINFORCE
 * equally its baseline subtraction followed by that line (mean = the
 * baseline).  m < 2: std and out are NaN, as torch's. */
int dd_batch_normalize(const float *x, float *out, int64_t m, double *mean, double *std,
                       void *workspace, void *stream);

/* ---- Training batches of every episode of a rollout ----------------------
 * The stages above keep each lane's first episode, as collect_episodes_ppo
 * plays one episode per game.  These keep every episode of the same [T][N]
 * buffers: a fixed-length rollout of an auto_reset env, continued from one
 * PPO iteration to the next (the notebook's "rollout_steps ... steps to
 * collect before update"), then uses every frame but the one re-spawn frame
 * per episode.  The rule is done's alone:
 *   - frame t of lane i is DROPPED when the frame before it was done:
 *     done[t-1][i] != 0, or for t = 0 done_before[i] != 0 (done_before uint8
 *     [N]: the env's done flags before the rollout; null = all zero).  On an
 *     auto-reset env that is exactly the re-spawn frame (DDConfig.auto_reset:
 *     terminal observation in, action ignored, reward 0, not done); on a
 *     sticky-done env every frame after the first done, so there the batch
 *     is the first-episode batch above.
 *   - an EPISODE is a maximal run of kept frames of one lane: frames
 *     [ep_start, ep_start + ep_length), consecutive because a dropped frame
 *     only follows a done.  It is ended (ep_ended = 1) when its last frame is
 *     done, else open: cut by the end of the rollout, the lane's last, at most
 *     one per lane.  With done_before[i] == 0 a lane's first episode continues
 *     what the lane was doing before the rollout; it is an ordinary episode.
 *   - order: lanes ascending, a lane's episodes in time order, so a lane's
 *     rows are its kept frames in frame order:
 *     row(i, t) = lane_row[i] + (kept frames of lane i before t).
 * DD_EPISODES_DROP_OPEN (count and fill) leaves open episodes out of the
 * batch, frames and records: a discounted return cut by the rollout's end is
 * no return (REINFORCE).  An episode that began before the rollout and ends
 * in it stays: its G_t depend on later rewards only.
 *
 * DDEpisodeLayout (caller-owned, device): lane_episode / lane_row, the
 * exclusive prefix sums over lanes of the episode and row counts, [N] = E and
 * M; per episode its lane, first frame, length, ended flag and first row
 * (ep_offset[E] = M).
 *
 * dd_episodes_count writes lane_episode and lane_row (one thread per lane
 * walks its T flags; deterministic fixed-shape scan, no atomics) and E, M
 * also to totals (device, 16 bytes), which the host reads once to size the
 * rest.  workspace: dd_episodes_workspace(n) bytes, 8-byte aligned.  T == 0 or
 * n == 0: all zero.  dd_episodes_fill writes the five per-episode arrays
 * (same flags as the count).  dd_episodes_gather is dd_batch_gather for this
 * layout (same DDBatchGatherIO, same LDS tiles; it reads lane_row only, and
 * recomputes a lane's kept-frame rank at a tile's first frame from done, so it
 * needs done and done_before again; frames of a dropped open episode are
 * those whose rank is not below the lane's row count).  No row >= M and
 * nothing for a dropped frame is written.  dd_episodes_advantages is
 * dd_batch_advantages per episode (same DDBatchAdvIO and arithmetic):
 * episode_return double [E], bootstrap float [N] used after an open episode's
 * last frame (bootstrap[ep_lane]; null = 0; 0 after an ended one).  The
 * normalisation is dd_batch_normalize on the M rows.  Errors as above: a null
 * required pointer, negative T or n, an unknown flag, mode or precision, an
 * input without its output: hipErrorInvalidValue before any launch. */
typedef struct DDEpisodeLayout {
    int64_t *lane_episode;   /* [N+1], [N] = E */
    int64_t *lane_row;       /* [N+1], [N] = M */
    int32_t *ep_lane;        /* [E]   (the ep_ fields may be null for dd_episodes_count and _gather) */
    int32_t *ep_start;       /* [E]   */
    int32_t *ep_length;      /* [E]   */
    uint8_t *ep_ended;       /* [E]   */
    int64_t *ep_offset;      /* [E+1] */
} DDEpisodeLayout;
#define DD_EPISODES_DROP_OPEN 1

int64_t dd_episodes_workspace(int64_t n);
int dd_episodes_count(const uint8_t *done, const uint8_t *done_before, int64_t T, int64_t n, int32_t flags,
                      const DDEpisodeLayout *layout, int64_t *totals, void *workspace, void *stream);
int dd_episodes_fill(const uint8_t *done, const uint8_t *done_before, int64_t T, int64_t n, int32_t flags,
                     const DDEpisodeLayout *layout, void *stream);
int dd_episodes_gather(const DDEpisodeLayout *layout, const uint8_t *done, const uint8_t *done_before,
                       const DDBatchGatherIO *io, int64_t T, int64_t n, void *stream);
int dd_episodes_advantages(const DDEpisodeLayout *layout, const DDBatchAdvIO *io, int64_t T, int64_t n,
                           void *stream);

/* ---- PPO losses and head gradients (compute_ppo_losses, the rest) ---------
 * From the per-row outputs of dd_mlp_evaluate_actions (log_prob, entropy,
 * probs) and of dd_mlp_forward on the critic (values), with the batch's
 * old_log_prob, advantages and returns, all float [m]:
 *   r           = exp(log_prob - old_log_prob)      the difference in float32,
 *                 exp in double, rounded to float32 once
 *   policy_loss = -mean(min(r A, clip(r, 1 - eps, 1 + eps) A))
 *   value_loss  = mean((v - R)^2)
 *   entropy     = sum(row entropy) / (3 m)          dist.entropy().mean()
 *   total_loss  = policy_loss + value_coef value_loss - entropy_coef entropy
 *   ratio_mean, ratio_min, ratio_max, ratio_std (unbiased: NaN at m == 1, as
 *   torch.std), clipped_frac = share of rows with r < 1 - eps or r > 1 + eps
 * into result[DD_PPO_*] (device doubles).  The clip bounds are float32(1 -
 * eps) and float32(1 + eps), as torch compares a float32 tensor with a Python
 * number; products and sums are in double (a product of two floats is exact
 * there), the sums over a reduction tree of fixed shape (no atomics: the same
 * bits on every run and every device), the std by a second pass over the
 * deviations from the mean.  Optional per-row outputs: ratio [m], and the
 * gradient of total_loss at the two networks' outputs, what torch autograd
 * leaves there:
 *   grad_values[i]    = value_coef 2 (v_i - R_i) / m
 *   grad_logits[i][k] = g_i (a_ik - p_ik)
 *                       + entropy_coef / (3 m) logit(p_ik) p_ik (1 - p_ik)
 *   g_i = -A_i r_i / m  where r_i A_i < clip(r_i) A_i or 1 - eps <= r_i <= 1 + eps,
 *         else 0;  a factor whose p lies outside [FLT_EPSILON, 1 - FLT_EPSILON]
 *         contributes 0 (clamp_probs passes no gradient there)
 * at the actor's pre-Sigmoid outputs and the critic's value (the derivation
 * is csrc/ppo_loss.hip's header).  grad_logits needs probs and actions
 * (action_format as DDMlpEvalIO); without it both may be NULL.  workspace:
 * dd_ppo_loss_workspace() bytes, 8-byte aligned.  hipErrorInvalidValue, before
 * any HIP call: a null io, m <= 0 (a mean over no rows has no value), a null
 * required pointer, a clip_epsilon that is negative or not finite, an unknown
 * action_format.  All indices are 64-bit. */
enum {
    DD_PPO_TOTAL_LOSS = 0,
    DD_PPO_POLICY_LOSS = 1,
    DD_PPO_VALUE_LOSS = 2,
    DD_PPO_ENTROPY = 3,
    DD_PPO_RATIO_MEAN = 4,
    DD_PPO_RATIO_MIN = 5,
    DD_PPO_RATIO_MAX = 6,
    DD_PPO_RATIO_STD = 7,
    DD_PPO_CLIPPED_FRAC = 8,
    DD_PPO_RESULTS = 9
};
typedef struct DDPpoLossIO {
    const float *log_prob;     /* [m]                                            */
    const float *entropy;      /* [m] row sums over the three factors            */
    const float *probs;        /* [m][3]; required with grad_logits              */
    const float *values;       /* [m]                                            */
    const float *old_log_prob; /* [m]                                            */
    const float *advantages;   /* [m]                                            */
    const float *returns;      /* [m]                                            */
    const void *actions;       /* by action_format; required with grad_logits    */
    int32_t action_format;     /* DD_ACT_BITMASK or DD_ACT_F32X3                 */
    int32_t _pad;
    double clip_epsilon;
    double entropy_coef;
    double value_coef;
    double *result;            /* [DD_PPO_RESULTS]                               */
    float *ratio;              /* nullable [m]                                   */
    float *grad_logits;        /* nullable [m][3]                                */
    float *grad_values;        /* nullable [m]                                   */
} DDPpoLossIO;

int64_t dd_ppo_loss_workspace(void);
int dd_ppo_losses(const DDPpoLossIO *io, int64_t m, void *workspace, void *stream);

/* ---- The networks' backward pass (additions to ABI 13) ----------------------
 * The parameter gradients of DroneGamerBoi / DroneTeacherBoi from the gradient
 * at the last Linear's output: for the actor the pre-Sigmoid logits, for the
 * critic the value, i.e. dd_ppo_losses' grad_logits / grad_values.  What
 * loss.backward() leaves in every parameter's .grad, then the notebook's
 * clip_grad_norm_ (per network, with max_grad_norm).  Per layer (a = its input):
 *   dy = da' [y > 0]          dgamma = sum_rows dy xh     dbeta = sum_rows dy
 *   g = dy gamma              dh = rstd (g - mean(g) - xh mean(g xh))
 *   dW = sum_rows dh (x) a    db = sum_rows dh            da = W^T dh
 * (csrc/mlp_backward.hip's header).  Float32 on the f32 MFMA from the plain
 * float32 parameters, whatever compute the forward was packed for; the
 * forward is recomputed tile by tile, so the workspace does not grow with m.
 * A fixed number of blocks each writes one partial gradient set; each element
 * is then the partials' sum in a fixed order in double, rounded once, and the
 * norm a fixed tree in double: the same bits on every run and every device.
 * grads: the fourteen tensors in DDMlpParams' order and torch's shapes
 * (w0 [128][15], ... w9 [K][64], b9 [K]).  grad_norm (nullable): the L2 norm
 * over all fourteen, before clipping.  max_norm finite and > 0: every gradient
 * is scaled by min(1, max_norm / (norm + 1e-6)); <= 0, +inf or NaN: no clipping.
 * workspace: dd_mlp_backward_workspace() bytes, 16-byte aligned.
 * hipErrorInvalidValue, before any HIP call: a null params, io, parameter or
 * gradient pointer, m < 0, out_dim not 1 or 3, and with m > 0 a null states,
 * grad_out or workspace (or a misaligned one).  m == 0 writes zeros and a zero
 * norm.  All row indices are 64-bit. */
typedef struct DDMlpGrads {
    float *w0, *b0, *ln1_w, *ln1_b;
    float *w3, *b3, *ln4_w, *ln4_b;
    float *w6, *b6, *ln7_w, *ln7_b;
    float *w9, *b9;
} DDMlpGrads;

typedef struct DDMlpBackwardIO {
    const float *states;   /* [m][15]                                    */
    const float *grad_out; /* [m][K]                                     */
    DDMlpGrads grads;
    double *grad_norm;     /* nullable                                   */
    double max_norm;
} DDMlpBackwardIO;

int64_t dd_mlp_backward_workspace(void);
int dd_mlp_backward(const DDMlpParams *params, const DDMlpBackwardIO *io, int64_t m, void *workspace,
                    void *stream);

/* ---- AdamW on one network's parameters (additions to ABI 13) ----------------
 * One step of torch.optim.AdamW (decoupled weight decay, amsgrad=False,
 * maximize=False), the training cell's policy_optimizer.step() /
 * critic_optimizer.step():
 *   p' = p (1 - lr wd);  m' = beta1 m + (1 - beta1) g;  v' = beta2 v + (1 - beta2) g g
 *   p'' = p' - (lr / (1 - beta1^t)) (m' / (sqrt(v') / sqrt(1 - beta2^t) + eps))
 * params, grads, exp_avg, exp_avg_sq: flat float32 buffers of 27,456 + 65 K
 * elements, the fourteen tensors in DDMlpParams' order and torch's shapes (the
 * layout of dd_mlp_backward's gradients when they share one buffer).  Every
 * element is evaluated in double from the four float32 inputs, in exactly the
 * order written above (1 - lr wd, 1 - beta1, 1 - beta2 are formed once on the
 * host; no contraction), and p'', m', v' are each rounded to float32 once;
 * float32 denormals are kept.  The step count lives on the device:
 * DDAdamWState holds step, the running products beta1^t and beta2^t (one
 * multiplication per step, not pow) and a status word; the kernel advances
 * them, the host never passes t, so a captured launch can be replayed.
 *
 * compute == DD_MLP_F16X3: the candidate parameters must be ones the f16x3
 * forward can hold: every element of w0, w3, w6 finite and below 65504 / 32 in
 * magnitude, and for each LayerNorm max|gamma| sqrt(rows) (1 + 2^-8) +
 * max|beta| < 128 (in double; a NaN fails).  If they are not, nothing is
 * committed (params, exp_avg, exp_avg_sq, step and the products keep their
 * bits, packed is rebuilt from the unchanged parameters) and
 * DD_ADAMW_REFUSED is or-ed into status, where it stays.  DD_MLP_F32: no check.
 * One launch of one 1,024-thread block: the candidates stay in registers
 * across the verdict's block maximum.  No atomics; the same bits on every run.
 * packed (nullable): dd_mlp_pack of the updated parameters into it afterwards,
 * on the same stream (ln_eps as DDMlpParams').
 *
 * dd_adamw_init zeroes exp_avg, exp_avg_sq (nullable together, count
 * elements), step and status and sets the products to 1, on the stream.
 * hipErrorInvalidValue, before any launch: a null io, hyper, state or buffer,
 * out_dim not 1 or 3, an unknown compute, a hyper-parameter that is not
 * finite or is negative, a beta outside [0, 1), a packed that is not 16-byte
 * aligned or comes with ln_eps <= 0, a negative count. */
typedef struct DDAdamWHyper {
    double lr;
    double beta1;
    double beta2;
    double eps;
    double weight_decay;
} DDAdamWHyper;

#define DD_ADAMW_REFUSED 1
typedef struct DDAdamWState {
    int64_t step;     /* t: steps committed                         */
    double beta1_t;   /* beta1^t, 1 at t = 0                        */
    double beta2_t;   /* beta2^t                                    */
    int32_t status;   /* DD_ADAMW_* bits, sticky                    */
    int32_t _pad;
} DDAdamWState;

typedef struct DDAdamWIO {
    float *params;         /* [27456 + 65 K]                            */
    const float *grads;    /* same length                               */
    float *exp_avg;        /* same length                               */
    float *exp_avg_sq;     /* same length                               */
    DDAdamWState *state;   /* device, dd_adamw_state_bytes(), 8-aligned */
    float *packed;         /* nullable: the network's dd_mlp_pack image */
    int32_t out_dim;       /* K: 3 actor, 1 critic                      */
    int32_t compute;       /* DD_MLP_F32 or DD_MLP_F16X3                */
    float ln_eps;          /* for the repack                            */
    int32_t _pad;
} DDAdamWIO;

int64_t dd_adamw_state_bytes(void);
int dd_adamw_init(float *exp_avg, float *exp_avg_sq, int64_t count, DDAdamWState *state, void *stream);
int dd_adamw_step(const DDAdamWHyper *hyper, const DDAdamWIO *io, void *stream);

/* ---- The REINFORCE and one-step actor-critic losses (additions to ABI 13) ----
 * The elementwise loss stages of Policy_Gradients.ipynb's and
 * Actor_Critic_Basic.ipynb's training cells, from per-row network outputs, with
 * the gradient of each loss at its network's output (csrc/pg_loss.hip's header
 * has the notebooks' lines and the derivation).  Products and sums are in
 * double on the float32 inputs, the sums over a reduction tree of fixed shape
 * (no atomics: the same bits on every run and every device); every per-row
 * output is rounded to float32 once.
 *
 * active (nullable, uint8 [m]; NULL = every row): a row with active == 0 is
 * out of every mean, its inputs are not read, its gradient rows are exactly 0
 * and its td_targets / td_errors are 0.  cnt = the number of active rows,
 * counted on the device.  cnt == 0: the scalars are NaN (torch's mean over no
 * element), DD_*_COUNT is 0 and every gradient row is 0.
 *
 * dd_pg_losses, the score-function loss of both notebooks, from
 * dd_mlp_evaluate_actions' log_prob [m] and probs [m][3], the given actions and
 * weights [m] (REINFORCE: the normalised advantages; actor-critic: td_errors):
 *   result[DD_PG_LOSS]  = -sum_active(log_prob_i w_i) / cnt
 *   result[DD_PG_COUNT] = cnt
 *   grad_logits[i][k]   = -(w_i / cnt) (a_ik - p_ik)   at the actor's pre-Sigmoid
 *       outputs; a factor whose p lies outside [FLT_EPSILON, 1 - FLT_EPSILON]
 *       gets 0 (clamp_probs passes no gradient there), a NaN p stays NaN
 * grad_logits needs probs and actions (action_format as DDMlpEvalIO); without
 * it both may be NULL.
 *
 * dd_td_losses, the actor-critic notebook's critic stage, from dd_mlp_forward
 * of the critic on the states (values) and the next states (next_values), with
 * rewards and dones (1.0 = the episode ended), all float [m]:
 *   td_targets[i] = r_i + (gamma v'_i) (1 - d_i)       gamma rounded to float32, as
 *                   torch multiplies a float32 tensor by a Python number
 *   td_errors[i]  = delta_i = target_i - v_i           from the unrounded target;
 *                   these float32 values are dd_pg_losses' weights
 *   result[DD_TD_MSE]         = sum_active(delta_i^2) / cnt
 *   result[DD_TD_VALUE_REG]   = value_reg (sum_active(v_i^2) / cnt)
 *   result[DD_TD_CRITIC_LOSS] = their sum
 *   result[DD_TD_COUNT]       = cnt
 *   grad_values[i] = (-2 delta_i + 2 value_reg v_i) / cnt   at the critic's value
 *       (next_values carries no gradient, as under the notebook's no_grad)
 *
 * workspace: dd_pg_loss_workspace() / dd_td_loss_workspace() bytes, 8-byte
 * aligned.  hipErrorInvalidValue, before any HIP call: a null io, m <= 0, a null
 * or misaligned workspace, a null required pointer, an unknown action_format,
 * grad_logits without probs or actions, a gamma or value_reg that is not
 * finite.  All indices are 64-bit. */
enum { DD_PG_LOSS = 0, DD_PG_COUNT = 1, DD_PG_RESULTS = 2 };
typedef struct DDPgLossIO {
    const float *log_prob;   /* [m]                                            */
    const float *probs;      /* [m][3]; required with grad_logits              */
    const void *actions;     /* by action_format; required with grad_logits    */
    int32_t action_format;   /* DD_ACT_BITMASK or DD_ACT_F32X3                 */
    int32_t _pad;
    const float *weights;    /* [m]                                            */
    const uint8_t *active;   /* nullable [m]                                   */
    double *result;          /* [DD_PG_RESULTS]                                */
    float *grad_logits;      /* nullable [m][3]                                */
} DDPgLossIO;

int64_t dd_pg_loss_workspace(void);
int dd_pg_losses(const DDPgLossIO *io, int64_t m, void *workspace, void *stream);

enum { DD_TD_CRITIC_LOSS = 0, DD_TD_MSE = 1, DD_TD_VALUE_REG = 2, DD_TD_COUNT = 3, DD_TD_RESULTS = 4 };
typedef struct DDTdLossIO {
    const float *values;      /* [m]                                           */
    const float *next_values; /* [m]                                           */
    const float *rewards;     /* [m]                                           */
    const float *dones;       /* [m] 1.0 / 0.0                                 */
    const uint8_t *active;    /* nullable [m]                                  */
    double gamma;
    double value_reg;
    float *td_targets;        /* [m]                                           */
    float *td_errors;         /* [m]                                           */
    double *result;           /* [DD_TD_RESULTS]                               */
    float *grad_values;       /* nullable [m]                                  */
} DDTdLossIO;

int64_t dd_td_loss_workspace(void);
int dd_td_losses(const DDTdLossIO *io, int64_t m, void *workspace, void *stream);

/* ---- Shuffled minibatch epochs: a keyed permutation of rows (additions to ABI 13) ----
 * perm(j), j in [0, m), is a stateless bijection of [0, m) that depends on
 * (m, seed, epoch) alone: every thread computes it for its own j, so there is
 * no sort, no atomic, no workspace, and launch geometry or sharding cannot
 * change it.  The definition (tests/shuffle_ref.py restates it in NumPy):
 *   b = bit_length(m - 1) (0 for m == 1);  h = max(1, ceil(b / 2));  mask = 2^h - 1
 *   cipher(x), on the domain [0, 2^(2h)), m <= 2^(2h) < 4 m for m >= 2:
 *     (L, R) = (x >> h, x & mask); for r = 0 .. 7:
 *       F = philox4x32_10(counter = (R, r, epoch_lo, epoch_hi ^ 0xC3C3C3C3),
 *                         key = (seed_lo, seed_hi))[0] & mask
 *       (L, R) = (R, L ^ F)
 *     cipher(x) = (L << h) | R          a balanced Feistel network: a bijection
 *   perm(j): x = j; do x = cipher(x) while x >= m      cycle walking: j < m lies on
 *     a cycle of the cipher, which re-enters [0, m) at the latest at j itself
 * dd_shuffle_indices: out[j] = perm(j).
 * dd_shuffle_rows: dst[j] = src[perm(j)] for the columns of a training batch,
 * moved as bits (NaN payloads survive).  Every column is a (source,
 * destination) pair that is null together; indices (nullable) also receives
 * perm.  Sources and destinations need 4-byte alignment only (1 for uint8
 * actions).  It cannot run in place.
 * Both are asynchronous on the stream, allocate nothing and read nothing back;
 * a captured launch replays the permutation of the (seed, epoch) it was
 * captured with.
 * hipErrorInvalidValue, before any launch: m < 0 or m >= 2^31, a null io (or
 * out), a column with one of its two pointers null, actions with an
 * action_format other than DD_ACT_BITMASK or DD_ACT_F32X3, a destination
 * range that overlaps a source range.  m == 0 (or no column at all): 0, no
 * launch. */
typedef struct DDShuffleIO {
    const float *states;         /* [m][15]                                   */
    const void *actions;         /* uint8 [m] or float [m][3], action_format  */
    const float *old_log_probs;  /* [m]                                       */
    const float *advantages;     /* [m]                                       */
    const float *returns;        /* [m]                                       */
    int32_t action_format;       /* DD_ACT_BITMASK or DD_ACT_F32X3            */
    int32_t _pad;
    float *states_out;           /* each null exactly when its source is      */
    void *actions_out;
    float *old_log_probs_out;
    float *advantages_out;
    float *returns_out;
    int32_t *indices;            /* nullable [m]: perm                        */
} DDShuffleIO;

int dd_shuffle_indices(int64_t m, uint64_t seed, uint64_t epoch, int32_t *out, void *stream);
int dd_shuffle_rows(const DDShuffleIO *io, int64_t m, uint64_t seed, uint64_t epoch, void *stream);

/* ---- PPO's minibatch epochs in one launch (additions to ABI 13) --------------
 * The training cell's `for epoch: for minibatch:` loop for minibatches of at
 * most DD_PPO_FUSED_ROWS rows (dd_mlp_backward's row tile) and DD_MLP_F32
 * networks: for e in [0, num_epochs) and minibatch i of the epoch, in that
 * order, exactly what these calls do on rows [first, first + rows) with first =
 * e epoch_stride + i minibatch_size, rows = min(minibatch_size, m - i
 * minibatch_size):
 *   dd_mlp_evaluate_actions (actor) and dd_mlp_forward (critic) on the rows,
 *   dd_ppo_losses with both gradients,
 *   dd_mlp_backward of each network with max_norm = max_grad_norm,
 *   dd_adamw_step of each network with its packed image,
 * bit for bit: parameters, moments, state blocks, packed images and logs.  One
 * persistent kernel of two 256-thread workgroups, one per network (total_loss
 * separates: the actor's gradient needs the actor alone, the critic's the
 * critic), each walking the minibatches in order with its forward, loss sums,
 * backward tile, norm, clip, AdamW step and re-pack; then one small kernel that
 * forms total_loss from both.  The number of launches does not depend on m /
 * minibatch_size, and nothing is read back.
 *
 * The epochs' rows: epoch e reads rows [e epoch_stride, e epoch_stride + m) of
 * every column, so the caller lays out num_epochs shuffled copies of the batch
 * (dd_shuffle_rows with epoch + e, epoch_stride >= m), or passes epoch_stride =
 * 0 and every epoch reads the same rows.  The minibatches of an epoch are i =
 * 0 .. steps - 1 with steps = ceil(m / minibatch_size), or floor(m /
 * minibatch_size) when drop_last.
 * logs: [DD_PPO_FUSED_LOGS][num_epochs][steps] doubles: rows DD_PPO_TOTAL_LOSS
 * .. DD_PPO_CLIPPED_FRAC as dd_ppo_losses' result, then the actor's and the
 * critic's gradient norm before clipping.
 * grads: each network's flat gradient buffer, left holding the last
 * minibatch's clipped gradient.  max_grad_norm as DDMlpBackwardIO's max_norm.
 * workspace: dd_ppo_update_fused_workspace() bytes, 16-byte aligned.
 * hipErrorInvalidValue, before any launch: a null io, workspace, column, logs
 * or network buffer; a state that is not 8-byte or a packed or workspace that
 * is not 16-byte aligned; ln_eps <= 0; hyper-parameters dd_adamw_step refuses;
 * m < 1 or m >= 2^31; minibatch_size outside [1, DD_PPO_FUSED_ROWS]; num_epochs
 * < 1; no minibatch (drop_last with m < minibatch_size); epoch_stride negative,
 * or positive and below m; an unknown action_format; a clip_epsilon that is
 * negative or not finite; a coefficient that is not finite; a NaN
 * max_grad_norm. */
#define DD_PPO_FUSED_ROWS 128
enum { DD_PPO_POLICY_GRAD_NORM = 9, DD_PPO_CRITIC_GRAD_NORM = 10, DD_PPO_FUSED_LOGS = 11 };
typedef struct DDPpoFusedNet {
    float *params;         /* [27456 + 65 K], updated in place               */
    float *grads;          /* same length, scratch                           */
    float *exp_avg;        /* same length                                    */
    float *exp_avg_sq;     /* same length                                    */
    DDAdamWState *state;   /* the optimizer's device block                   */
    float *packed;         /* the network's DD_MLP_F32 dd_mlp_pack image     */
    DDAdamWHyper hyper;
    float ln_eps;
    int32_t _pad;
} DDPpoFusedNet;

typedef struct DDPpoFusedIO {
    DDPpoFusedNet actor;         /* K = 3                                     */
    DDPpoFusedNet critic;        /* K = 1                                     */
    const float *states;         /* [epochs' rows][15]                        */
    const void *actions;         /* uint8 [rows] or float [rows][3]           */
    const float *old_log_probs;  /* [rows]                                    */
    const float *advantages;     /* [rows]                                    */
    const float *returns;        /* [rows]                                    */
    int32_t action_format;       /* DD_ACT_BITMASK or DD_ACT_F32X3            */
    int32_t drop_last;           /* nonzero: no tail minibatch                */
    int64_t m;                   /* rows of one epoch                         */
    int64_t epoch_stride;        /* rows from one epoch's batch to the next   */
    int32_t num_epochs;
    int32_t minibatch_size;
    double clip_epsilon;
    double entropy_coef;
    double value_coef;
    double max_grad_norm;        /* <= 0 or inf: no clipping                  */
    double *logs;                /* [DD_PPO_FUSED_LOGS][num_epochs][steps]    */
} DDPpoFusedIO;

int64_t dd_ppo_update_fused_workspace(void);
int dd_ppo_update_fused(const DDPpoFusedIO *io, void *workspace, void *stream);

/* ---- A population of PPO learners in one fused launch (additions to ABI 13) ---
 * dd_ppo_update_fused for every member of a population (the learners of a
 * hyper-parameter sweep) at once.  For every member p the call leaves its
 * parameters, both moments, both state blocks, both packed images, both gradient
 * buffers and all DD_PPO_FUSED_LOGS log rows bit for bit as one
 * dd_ppo_update_fused call with that member's networks, coefficients and
 * num_epochs shuffled copies of its batch (dd_shuffle_rows with (shuffle_seed,
 * shuffle_epoch + e), epoch_stride = m; or epoch_stride = 0 without shuffle),
 * minibatch_size = min(minibatch_size, m) and the same drop_last leaves them.
 *
 * One persistent kernel of 2 * members 256-thread workgroups: block b is
 * network b & 1 (0 actor, 1 critic) of member b >> 1.  No workgroup waits on
 * another, so nothing needs them co-resident; past the card's CUs (one
 * workgroup per CU) the later ones start when a CU is free.  Then one small
 * kernel forms every member's total_loss.
 *
 * The batch is read in place: at minibatch i of epoch e a workgroup gathers its
 * rows, source row perm(i size + k; m, shuffle_seed, shuffle_epoch + e) (the
 * permutation above; i size + k when shuffle is 0), k in [0, rows), into a stage
 * of its own in the workspace and runs the step from there.  No shuffled copy
 * of a batch exists.  The columns need 4-byte alignment only (1 for uint8
 * actions).
 * num_epochs, minibatch_size and drop_last hold for every member; a member's
 * steps follow from its own m, and its logs are [DD_PPO_FUSED_LOGS][num_epochs]
 * [steps_p].
 * The members' descriptors are a host array: the call turns them into a table
 * it copies into the head of the workspace on the stream (hipMemcpyAsync from
 * pageable memory: the array may be freed when the call returns) before the
 * launch.  Nothing is read back.  Not for stream capture: a replay would copy
 * from host memory that is gone.
 * workspace: dd_ppo_update_population_workspace(members) bytes, 16-byte
 * aligned: the table, then per workgroup the backward's weight images, the head
 * gradient and the stage.  It grows linearly in members (0 for members < 1).
 * hipErrorInvalidValue, before any HIP call: a null io, table or workspace, a
 * workspace that is not 16-byte aligned; members < 1; num_epochs < 1;
 * minibatch_size outside [1, DD_PPO_FUSED_ROWS]; for any member, what
 * dd_ppo_update_fused refuses of a network, a column, logs, action_format, m,
 * clip_epsilon, the two coefficients or max_grad_norm; a member with no
 * minibatch (drop_last with m < minibatch_size); two members that share a
 * network buffer (params, grads, a moment, state or packed overlapping). */
typedef struct DDPpoPopulationMember {
    DDPpoFusedNet actor;         /* K = 3                                     */
    DDPpoFusedNet critic;        /* K = 1                                     */
    const float *states;         /* [m][15], the batch as built: unshuffled   */
    const void *actions;         /* uint8 [m] or float [m][3]                 */
    const float *old_log_probs;  /* [m]                                       */
    const float *advantages;     /* [m]                                       */
    const float *returns;        /* [m]                                       */
    int32_t action_format;       /* DD_ACT_BITMASK or DD_ACT_F32X3            */
    int32_t shuffle;             /* nonzero: rows through perm                */
    int64_t m;
    double clip_epsilon;
    double entropy_coef;
    double value_coef;
    double max_grad_norm;        /* <= 0 or inf: no clipping                  */
    uint64_t shuffle_seed;
    uint64_t shuffle_epoch;      /* epoch e of the call uses shuffle_epoch + e */
    double *logs;                /* [DD_PPO_FUSED_LOGS][num_epochs][steps_p]  */
} DDPpoPopulationMember;

typedef struct DDPpoPopulationIO {
    const DDPpoPopulationMember *table;  /* host memory, [members]            */
    int32_t members;
    int32_t num_epochs;
    int32_t minibatch_size;
    int32_t drop_last;           /* nonzero: no tail minibatch                */
} DDPpoPopulationIO;

int64_t dd_ppo_update_population_workspace(int32_t members);
int dd_ppo_update_population(const DDPpoPopulationIO *io, void *workspace, void *stream);

/* ---- One-step actor-critic learners trained online, one launch (additions to ABI 13)
 * Actor_Critic_Basic.ipynb's `while not all(games_done)` body for `frames`
 * frames and every member of a population, in one launch.  Member g drives
 * lanes [g L, (g + 1) L) of the batch `st` (L = lanes_per_member, 1 <= L <=
 * DD_PPO_FUSED_ROWS, members L == n).  For t in [0, frames), exactly what these
 * calls do on the member's lanes, bit for bit:
 *   state = the lanes' rows of obs (copied)
 *   dd_mlp_forward of the actor on state with (seed; env_id_base + lane, step + t)
 *   dd_step with those actions (engine reward, or the notebook reward with
 *     max_steps when shaped_hist / shaped_reward / shaped_done are set; obs,
 *     reward, done, shaped_* are dd_step's outputs of the same names)
 *   active = not done_prev (done_prev: the previous frame's returned done: the
 *     shaped one when shaped, else the engine's; before frame 0, not active0,
 *     all active when active0 is null)
 *   dd_mlp_forward of the critic on state and on the new obs, dd_td_losses with
 *     the returned reward and done, gamma, value_reg, the mask and grad_values,
 *   dd_mlp_backward (max_norm = max_grad_norm) and dd_adamw_step of the critic,
 *   dd_mlp_evaluate_actions of the actor (not yet stepped) on state, dd_pg_losses
 *     with weights = td_errors, the mask and grad_logits,
 *   dd_mlp_backward and dd_adamw_step of the actor.
 * One persistent kernel of `members` 256-thread workgroups, one per member,
 * which runs both networks one after the other; no workgroup waits on another,
 * so past the card's CUs (one workgroup per CU) the later ones start when a CU
 * is free.  DD_MLP_F32 networks and DD_F32 state storage only.
 * logs: [DD_AC_LOGS][frames][members] doubles.  A frame with no active row logs
 * NaN losses, count 0 and zero norms, and both zero-gradient steps are taken.
 * done_last [n]: the last frame's returned done (the next call's active0 is its
 * complement).  record_reward (float) / record_done [frames][n]: every frame's
 * returned reward and done, both or neither.
 * The members' descriptors are a host array, copied into the head of the
 * workspace on the stream as dd_ppo_update_population does; not for stream
 * capture.  Nothing is read back.
 * workspace: dd_actor_critic_train_workspace(members) bytes, 16-byte aligned;
 * linear in members (0 for members < 1).
 * hipErrorInvalidValue, before any HIP call: a null cfg, st, io, table, obs,
 * reward, done, done_last, logs or workspace; a workspace that is not 16-byte
 * aligned; a state dd_step refuses, or not DD_F32; members < 1; frames < 1;
 * lanes_per_member outside [1, DD_PPO_FUSED_ROWS]; members lanes_per_member !=
 * n; shaped_mode not DD_SHAPED_PPO, or some but not all of shaped_hist,
 * shaped_reward, shaped_done; one record buffer without the other; for any
 * member, what dd_ppo_update_fused refuses of a network or of max_grad_norm, a
 * gamma or value_reg that is not finite; network buffers that overlap (between
 * members, or the actor's with the critic's). */
enum { DD_AC_ACTOR_LOSS = 0, DD_AC_CRITIC_LOSS = 1, DD_AC_MSE = 2, DD_AC_VALUE_REG = 3, DD_AC_COUNT = 4,
       DD_AC_ACTOR_GRAD_NORM = 5, DD_AC_CRITIC_GRAD_NORM = 6, DD_AC_LOGS = 7 };
typedef struct DDActorCriticMember {
    DDPpoFusedNet actor;         /* K = 3                                     */
    DDPpoFusedNet critic;        /* K = 1                                     */
    double gamma;                /* rounded to float32, as dd_td_losses does  */
    double value_reg;
    double max_grad_norm;        /* <= 0 or inf: no clipping                  */
} DDActorCriticMember;

typedef struct DDActorCriticIO {
    const DDActorCriticMember *table;  /* host memory, [members]              */
    int32_t members;
    int32_t frames;
    int64_t lanes_per_member;
    float *obs;                  /* [n][15]: in, the current observation; out, the last frame's */
    void *reward;                /* float [n]: the engine's, as dd_step       */
    uint8_t *done;               /* [n]                                       */
    double *shaped_hist;         /* [2][n] or null (all three, or none)       */
    void *shaped_reward;         /* float [n]                                 */
    uint8_t *shaped_done;        /* [n]                                       */
    int32_t shaped_mode;         /* DD_SHAPED_PPO                             */
    int32_t max_steps;           /* the notebook's timeout; <= 0: none        */
    const uint8_t *active0;      /* nullable [n]: nonzero = trains at frame 0 */
    uint8_t *done_last;          /* [n]                                       */
    void *record_reward;         /* nullable float [frames][n]                */
    uint8_t *record_done;        /* nullable [frames][n]                      */
    uint64_t seed;
    int64_t step;
    double *logs;                /* [DD_AC_LOGS][frames][members]             */
} DDActorCriticIO;

int64_t dd_actor_critic_train_workspace(int32_t members);
int dd_actor_critic_train(const DDConfig *cfg, const DDState *st, const DDActorCriticIO *io, int64_t n,
                          void *workspace, void *stream);

/* ---- REINFORCE learners, one iteration in one launch (additions to ABI 13) ------
 * One iteration of Policy_Gradients.ipynb's training loop for every member of a
 * population.  Member g drives lanes [g L, (g + 1) L) of the batch `st` (L =
 * lanes_per_member, 1 <= L <= DD_PPO_FUSED_ROWS, members L == n), which the
 * caller has just reset (dd_reset), on a sticky env (cfg->auto_reset == 0: one
 * episode per lane).  Exactly what these calls do on the member's lanes, bit
 * for bit:
 *   dd_policy_rollout of the actor for max_steps frames with (seed; env_id_base +
 *     lane, step + t) and the reward stream of shaped_mode / shaped_hist (the
 *     engine's; PPO's calc_reward with shaped_hist; DD_SHAPED_REINFORCE's), the
 *     shaped ones with the timeout env_max_steps and its -500
 *   dd_batch_plan, dd_batch_gather, dd_batch_advantages (DD_BATCH_RETURNS, gamma
 *     as the double it is) and dd_batch_normalize over the member's M rows (each
 *     lane's first episode; lanes ascending, a lane's rows in frame order)
 *   dd_mlp_evaluate_actions, dd_pg_losses with weights = the normalised returns
 *     (the returns when normalize == 0) and grad_logits,
 *   dd_mlp_backward (max_norm = max_grad_norm) and dd_adamw_step of the actor.
 * One persistent kernel of `members` 256-thread workgroups, one per member; no
 * workgroup waits on another.  The batch's rows are read in place in a
 * frame-major record of the member's frames (no compacted copy).  The frame
 * loop stops after the first frame that every lane of the member entered done:
 * further frames would store the same state arrays and obs.
 * DD_MLP_F32 networks and DD_F32 state storage only.
 * obs [n][15]: in, the current observation; out, the last frame's.  The state
 * arrays and shaped_hist are left as the rollout leaves them.
 * logs: [DD_RF_LOGS][members] doubles: the loss, the gradient norm before
 * clipping, the mean and the unbiased std of the member's returns (NaN for M <
 * 2), and M.  lengths / ended / episode_return [n]: dd_batch_plan's and
 * dd_batch_advantages' per lane.  record_reward (float) / record_done
 * [max_steps][n], both or neither, and record_returns / record_advantages
 * [max_steps][n], both or neither: each lane's rows at their frames, zeros after
 * its episode.
 * The members' descriptors are a host array, copied into the head of the
 * workspace on the stream as dd_ppo_update_population does; not for stream
 * capture.  Nothing is read back.
 * workspace: dd_reinforce_train_workspace(members, lanes, max_steps) bytes,
 * 16-byte aligned: linear in members, and DD_REINFORCE_CELL_BYTES per cell of a
 * member's lanes x max_steps cells (rounded up to a multiple of 4) on top of a
 * fixed part per member; 0 for arguments the call refuses.
 * hipErrorInvalidValue, before any HIP call: a null cfg, st, io, table, obs,
 * lengths, ended, episode_return, logs or workspace; a workspace that is not
 * 16-byte aligned; a state dd_step refuses, or not DD_F32; members < 1;
 * lanes_per_member outside [1, DD_PPO_FUSED_ROWS]; max_steps < 1, or lanes x
 * max_steps above DD_REINFORCE_MAX_CELLS; members lanes_per_member != n;
 * cfg->auto_reset set; an unknown shaped_mode; one buffer of a record pair
 * without the other; for any member, what dd_ppo_update_fused refuses of a
 * network or of max_grad_norm, a gamma that is not finite; network buffers
 * that overlap between members. */
#define DD_REINFORCE_CELL_BYTES 108
#define DD_REINFORCE_MAX_CELLS (1 << 24)
enum { DD_RF_LOSS = 0, DD_RF_GRAD_NORM = 1, DD_RF_BASELINE = 2, DD_RF_STD = 3, DD_RF_ROWS = 4, DD_RF_LOGS = 5 };
typedef struct DDReinforceMember {
    DDPpoFusedNet actor;         /* K = 3                                     */
    double gamma;
    double max_grad_norm;        /* <= 0 or inf: no clipping                  */
} DDReinforceMember;

typedef struct DDReinforceIO {
    const DDReinforceMember *table;  /* host memory, [members]                */
    int32_t members;
    int32_t max_steps;           /* frames collected at most                  */
    int64_t lanes_per_member;
    float *obs;                  /* [n][15]                                   */
    double *shaped_hist;         /* [2][n]: PPO's reward; null otherwise      */
    int32_t shaped_mode;         /* DD_SHAPED_PPO or DD_SHAPED_REINFORCE      */
    int32_t env_max_steps;       /* the shaped rewards' timeout; <= 0: none   */
    int32_t normalize;           /* nonzero: weights = normalised returns     */
    int32_t _pad;
    uint64_t seed;
    int64_t step;
    int32_t *lengths;            /* [n]                                       */
    uint8_t *ended;              /* [n]                                       */
    double *episode_return;      /* [n]                                       */
    void *record_reward;         /* nullable float [max_steps][n]             */
    uint8_t *record_done;        /* nullable [max_steps][n]                   */
    float *record_returns;       /* nullable [max_steps][n]                   */
    float *record_advantages;    /* nullable [max_steps][n]                   */
    double *logs;                /* [DD_RF_LOGS][members]                     */
} DDReinforceIO;

int64_t dd_reinforce_train_workspace(int32_t members, int64_t lanes, int32_t max_steps);
int dd_reinforce_train(const DDConfig *cfg, const DDState *st, const DDReinforceIO *io, int64_t n, void *workspace,
                       void *stream);

/* ---- PPO learners, one iteration in one launch (additions to ABI 13) ------------
 * One iteration of Actor_Critic_PPO.ipynb's training cell for every member of a
 * population.  Member g drives lanes [g L, (g + 1) L) of the batch `st` (L =
 * lanes_per_member, 1 <= L <= DD_PPO_FUSED_ROWS, members L == n), which the
 * caller has just reset (dd_reset), on a sticky env (cfg->auto_reset == 0: one
 * episode per lane).  Exactly what these calls do on the member's lanes, bit
 * for bit:
 *   dd_policy_rollout of the actor for max_steps frames, as dd_reinforce_train
 *     runs it (the same reward streams, timeout and early stop), its log-probs
 *     kept as the batch's old log-probs
 *   dd_batch_plan, dd_batch_gather, dd_mlp_forward of the critic on the M rows
 *     (each lane's first episode; lanes ascending, a lane's rows in frame order)
 *     and on the lanes' final observation (the bootstrap of a lane whose episode
 *     did not end; 0 for one that did), dd_batch_advantages (DD_BATCH_GAE with
 *     gamma and lambda, returns = advantages + values) and dd_batch_normalize
 *   num_epochs epochs of PPO steps with the member's coefficients:
 *     minibatch_size = B in [1, DD_PPO_FUSED_ROWS]: dd_ppo_update_fused's steps
 *       on the rows perm(i min(B, M) + k; M, shuffle_seed, shuffle_epoch + e),
 *       the tail shorter than B a step of its own unless drop_last (a member
 *       with M < B and drop_last takes no step);
 *     minibatch_size = 0: one step per epoch on all M rows in batch order:
 *       dd_ppo_update_fused's for M <= DD_PPO_FUSED_ROWS; above that
 *       dd_mlp_evaluate_actions / dd_mlp_forward, dd_ppo_losses with both
 *       gradients, dd_mlp_backward (max_norm = max_grad_norm) and dd_adamw_step
 *       of the actor and of the critic.
 * One persistent kernel of `members` 256-thread workgroups, one per member,
 * which runs both networks; no workgroup waits on another.  The batch's rows are
 * read in place in a frame-major record of the member's frames.
 * DD_MLP_F32 networks and DD_F32 state storage only.
 * obs [n][15]: in, the current observation; out, the last frame's.  The state
 * arrays and shaped_hist are left as the rollout leaves them.
 * logs: [DD_PPO_FUSED_LOGS][num_epochs][steps][members] doubles, the rows of
 * dd_ppo_update_fused; steps is 1 for minibatch_size 0, else ceil(L max_steps /
 * minibatch_size), the most a member can take: the entries of the steps a member
 * does not take are NaN.  batch_logs: [DD_PT_BATCH_LOGS][members] doubles: M,
 * the mean and the unbiased std of the member's raw advantages (NaN for M < 2).
 * lengths / ended / episode_return [n]: dd_batch_plan's and
 * dd_batch_advantages' per lane; landed [n]: whether the lane's drone landed.
 * record_reward (float) / record_done [max_steps][n], both or neither, and
 * record_values / record_returns / record_advantages [max_steps][n], all or
 * none: each lane's rows at their frames, zeros after its episode.
 * The members' descriptors are a host array, copied into the head of the
 * workspace on the stream as dd_ppo_update_population does; not for stream
 * capture.  Nothing is read back.
 * workspace: dd_ppo_train_workspace(members, lanes, max_steps) bytes, 16-byte
 * aligned: linear in members, and DD_PPO_TRAIN_CELL_BYTES per cell of a member's
 * lanes x max_steps cells (rounded up to a multiple of 4) on top of a fixed part
 * per member; 0 for arguments the call refuses.
 * hipErrorInvalidValue, before any HIP call: everything dd_reinforce_train
 * refuses (with landed and batch_logs among the buffers that must be set, and
 * the three-buffer record all or none); num_epochs < 1; minibatch_size outside
 * {0} and [1, DD_PPO_FUSED_ROWS]; for any member, what dd_ppo_update_population
 * refuses of a network, clip_epsilon, the two coefficients or max_grad_norm, a
 * gamma or lambda that is not finite; network buffers that overlap (between
 * members, or the actor's with the critic's). */
#define DD_PPO_TRAIN_CELL_BYTES 124
enum { DD_PT_ROWS = 0, DD_PT_ADV_MEAN = 1, DD_PT_ADV_STD = 2, DD_PT_BATCH_LOGS = 3 };
typedef struct DDPpoTrainMember {
    DDPpoFusedNet actor;         /* K = 3                                     */
    DDPpoFusedNet critic;        /* K = 1                                     */
    double gamma;                /* rounded to float32, as dd_gae does        */
    double lambda;               /* gamma * lambda rounded to float32         */
    double clip_epsilon;
    double entropy_coef;
    double value_coef;
    double max_grad_norm;        /* <= 0 or inf: no clipping                  */
    uint64_t shuffle_seed;
} DDPpoTrainMember;

typedef struct DDPpoTrainIO {
    const DDPpoTrainMember *table;  /* host memory, [members]                 */
    int32_t members;
    int32_t max_steps;           /* frames collected at most                  */
    int64_t lanes_per_member;
    float *obs;                  /* [n][15]                                   */
    double *shaped_hist;         /* [2][n]: PPO's reward; null otherwise      */
    int32_t shaped_mode;         /* DD_SHAPED_PPO or DD_SHAPED_REINFORCE      */
    int32_t env_max_steps;       /* the shaped rewards' timeout; <= 0: none   */
    int32_t normalize;           /* nonzero: normalised advantages            */
    int32_t num_epochs;
    int32_t minibatch_size;      /* 0: the full batch                         */
    int32_t drop_last;           /* nonzero: no tail minibatch                */
    uint64_t shuffle_epoch;      /* epoch e of the call uses shuffle_epoch + e */
    uint64_t seed;
    int64_t step;
    int32_t *lengths;            /* [n]                                       */
    uint8_t *ended;              /* [n]                                       */
    double *episode_return;      /* [n]                                       */
    uint8_t *landed;             /* [n]                                       */
    void *record_reward;         /* nullable float [max_steps][n]             */
    uint8_t *record_done;        /* nullable [max_steps][n]                   */
    float *record_values;        /* nullable [max_steps][n]                   */
    float *record_returns;       /* nullable [max_steps][n]                   */
    float *record_advantages;    /* nullable [max_steps][n]                   */
    double *logs;                /* [DD_PPO_FUSED_LOGS][num_epochs][steps][members] */
    double *batch_logs;          /* [DD_PT_BATCH_LOGS][members]               */
} DDPpoTrainIO;

int64_t dd_ppo_train_workspace(int32_t members, int64_t lanes, int32_t max_steps);
int dd_ppo_train(const DDConfig *cfg, const DDState *st, const DDPpoTrainIO *io, int64_t n, void *workspace,
                 void *stream);

#ifdef __cplusplus
}
#endif

#endif /* DRONESTEP_H */
