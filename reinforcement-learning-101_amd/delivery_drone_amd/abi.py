"""ctypes mirror of ``include/dronestep.h`` and the loader of ``libdronestep.so``.

The shared library is the product: HIP kernels for gfx950 behind a plain C ABI.
There is no CPU fallback anywhere in this package — if the library is missing
or cannot be loaded, :func:`lib` raises.
"""
from __future__ import annotations

import ctypes
import os
import threading

import torch  # noqa: F401  -- must be loaded first so the library binds torch's HIP runtime

__all__ = [
    "DD_F32", "DD_F64", "DD_ACT_BITMASK", "DD_ACT_F32X3", "DD_ACT_U8X3", "DD_ACT_PHILOX",
    "DD_ST_DONE", "DD_ST_LANDED", "DD_ST_CRASHED", "DD_ST_PLAT_LEFT", "DD_OBS_DIM",
    "DD_RENDER_HUD", "DD_RENDER_GAME_OVER", "DD_RENDER_LABELS", "DD_MLP_F32", "DD_MLP_F16X3",
    "DD_SHAPED_PPO", "DD_SHAPED_REINFORCE", "DD_ROLLOUT_AUTO", "DD_ROLLOUT_SINGLE", "DD_ROLLOUT_SPLIT_NO_WAIT",
    "DD_ROLLOUT_FLUSHED", "DD_ROLLOUT_HELD", "DD_ROLLOUT_SPLIT", "DD_STEP_GENERIC", "DD_STEP_FAST", "DD_ERR_HANDOVER",
    "DD_SAMPLE_BERNOULLI", "DD_SAMPLE_TEMPERED", "DD_SAMPLE_GREEDY",
    "DDConfig", "DDState", "DDStepIO", "DDRolloutIO", "DDMlpParams", "DDMlpIO", "DDPolicyRolloutIO", "DDSampling",
    "DDEpisodeStats", "DD_BATCH_GAE", "DD_BATCH_RETURNS", "DDBatchLayout", "DDBatchGatherIO", "DDBatchAdvIO",
    "DD_EPISODES_DROP_OPEN", "DDEpisodeLayout", "DDMlpEvalIO", "DDPpoLossIO", "DDMlpGrads", "DDMlpBackwardIO",
    "DD_PPO_TOTAL_LOSS", "DD_PPO_POLICY_LOSS", "DD_PPO_VALUE_LOSS", "DD_PPO_ENTROPY", "DD_PPO_RATIO_MEAN",
    "DD_PPO_RATIO_MIN", "DD_PPO_RATIO_MAX", "DD_PPO_RATIO_STD", "DD_PPO_CLIPPED_FRAC", "DD_PPO_RESULTS",
    "DD_ADAMW_REFUSED", "DDAdamWHyper", "DDAdamWState", "DDAdamWIO",
    "DD_PG_LOSS", "DD_PG_COUNT", "DD_PG_RESULTS", "DDPgLossIO",
    "DD_TD_CRITIC_LOSS", "DD_TD_MSE", "DD_TD_VALUE_REG", "DD_TD_COUNT", "DD_TD_RESULTS", "DDTdLossIO",
    "DDShuffleIO", "DD_PPO_FUSED_ROWS", "DD_PPO_POLICY_GRAD_NORM", "DD_PPO_CRITIC_GRAD_NORM", "DD_PPO_FUSED_LOGS",
    "DDPpoFusedNet", "DDPpoFusedIO", "DDPpoPopulationMember", "DDPpoPopulationIO", "DDActorCriticMember",
    "DDActorCriticIO", "DD_AC_LOGS", "AC_LOG_NAMES", "DDReinforceMember", "DDReinforceIO", "DD_RF_LOGS",
    "RF_LOG_NAMES", "DD_REINFORCE_CELL_BYTES", "DD_REINFORCE_MAX_CELLS", "DDPpoTrainMember", "DDPpoTrainIO",
    "DD_PPO_TRAIN_CELL_BYTES", "DD_PT_BATCH_LOGS", "PT_BATCH_LOG_NAMES", "DD_REWARD_PARTS", "DDRewardParts", "REWARD_PART_NAMES",
    "sampling_mode", "lib", "load", "library_path", "check",
    "NativeLibraryError",
]

DD_ABI_VERSION = 13
DD_F32, DD_F64 = 0, 1
DD_ACT_BITMASK, DD_ACT_F32X3, DD_ACT_U8X3, DD_ACT_PHILOX = 0, 1, 2, 3
DD_ST_DONE, DD_ST_LANDED, DD_ST_CRASHED, DD_ST_PLAT_LEFT = 1, 2, 4, 8
DD_OBS_DIM = 15
DD_RENDER_HUD, DD_RENDER_GAME_OVER, DD_RENDER_LABELS = 1, 2, 4
DD_MLP_F32, DD_MLP_F16X3 = 0, 1
DD_SHAPED_PPO, DD_SHAPED_REINFORCE = 0, 1
DD_ROLLOUT_AUTO, DD_ROLLOUT_SINGLE, DD_ROLLOUT_SPLIT_NO_WAIT = 0, 1, 2
DD_ROLLOUT_FLUSHED, DD_ROLLOUT_HELD, DD_ROLLOUT_SPLIT = 16, 17, 18
DD_STEP_GENERIC, DD_STEP_FAST = 0, 1
DD_ERR_HANDOVER = 1
DD_MEM_DEFAULT, DD_MEM_CONTIGUOUS = 0, 1
DD_SAMPLE_BERNOULLI, DD_SAMPLE_TEMPERED, DD_SAMPLE_GREEDY = 0, 1, 2
DD_BATCH_GAE, DD_BATCH_RETURNS = 0, 1
DD_REWARD_PARTS = 8
#: calc_reward's keys in the notebooks' order, by ``reward_mode`` (the slots of ``DDRewardParts``)
REWARD_PART_NAMES = {
    "notebook": ("time_penalty", "distance", "hovering", "angle", "speed", "vertical_position", "terminal",
                 "total"),
    "reinforce": ("time_penalty", "distance", "velocity_alignment", "angle", "speed", "vertical_position",
                  "terminal", "total"),
}
DD_EPISODES_DROP_OPEN = 1
(DD_PPO_TOTAL_LOSS, DD_PPO_POLICY_LOSS, DD_PPO_VALUE_LOSS, DD_PPO_ENTROPY, DD_PPO_RATIO_MEAN, DD_PPO_RATIO_MIN,
 DD_PPO_RATIO_MAX, DD_PPO_RATIO_STD, DD_PPO_CLIPPED_FRAC, DD_PPO_RESULTS) = range(10)

DD_ADAMW_REFUSED = 1
DD_PPO_FUSED_ROWS = 128
DD_PPO_POLICY_GRAD_NORM, DD_PPO_CRITIC_GRAD_NORM, DD_PPO_FUSED_LOGS = 9, 10, 11
DD_PG_LOSS, DD_PG_COUNT, DD_PG_RESULTS = range(3)
#: the log rows of ``dd_actor_critic_train``, in the header's DD_AC_* order
AC_LOG_NAMES = ("actor_loss", "critic_loss", "mse", "value_reg", "count", "actor_grad_norm", "critic_grad_norm")
DD_AC_LOGS = len(AC_LOG_NAMES)
#: the log rows of ``dd_reinforce_train``, in the header's DD_RF_* order
RF_LOG_NAMES = ("loss", "grad_norm", "baseline", "std", "rows")
DD_RF_LOGS = len(RF_LOG_NAMES)
DD_REINFORCE_CELL_BYTES = 108
DD_REINFORCE_MAX_CELLS = 1 << 24
#: the rows of ``dd_ppo_train``'s batch logs, in the header's DD_PT_* order
PT_BATCH_LOG_NAMES = ("rows", "adv_mean", "adv_std")
DD_PT_BATCH_LOGS = len(PT_BATCH_LOG_NAMES)
DD_PPO_TRAIN_CELL_BYTES = 124
DD_TD_CRITIC_LOSS, DD_TD_MSE, DD_TD_VALUE_REG, DD_TD_COUNT, DD_TD_RESULTS = range(5)

_D = ctypes.c_double
_I = ctypes.c_int32


class DDConfig(ctypes.Structure):
    """``DDConfig`` (include/dronestep.h); field order is the ABI."""

    _fields_ = [
        ("gravity", _D), ("drag", _D), ("angular_drag", _D),
        ("main_thrust_power", _D), ("side_thrust_power", _D),
        ("fuel_main", _D), ("fuel_side", _D), ("max_fuel", _D),
        ("drone_half_height", _D), ("dt", _D),
        ("platform_half_width", _D), ("platform_half_height", _D),
        ("platform_speed", _D), ("platform_min_x", _D), ("platform_max_x", _D),
        ("max_landing_velocity", _D), ("max_landing_angle", _D),
        ("world_width", _D), ("world_height", _D), ("oob_margin", _D), ("ground_level", _D),
        ("wind_x", _D), ("wind_y", _D),
        ("reward_step", _D), ("reward_landing", _D), ("reward_crash", _D),
        ("reward_out_of_fuel", _D), ("reward_out_of_bounds", _D),
        ("shaping_offset", _D), ("shaping_scale", _D),
        ("vel_scale", _D), ("angle_scale", _D),
        ("drone_start_x", _I), ("drone_start_y", _I),
        ("drone_x_min", _I), ("drone_x_max", _I),
        ("drone_y_min", _I), ("drone_y_max", _I),
        ("platform_start_x", _I), ("platform_start_y", _I),
        ("platform_x_lo", _I), ("platform_x_hi", _I),
        ("platform_y_lo", _I), ("platform_y_hi", _I),
        ("wind_enabled", _I), ("platform_moving", _I),
        ("randomize_drone", _I), ("randomize_platform", _I),
        ("auto_reset", _I), ("_pad", _I),
        ("seed", ctypes.c_uint64),
    ]


class DDState(ctypes.Structure):
    _fields_ = [
        ("x", ctypes.c_void_p), ("y", ctypes.c_void_p), ("vx", ctypes.c_void_p),
        ("vy", ctypes.c_void_p), ("angle", ctypes.c_void_p), ("omega", ctypes.c_void_p),
        ("fuel", ctypes.c_void_p), ("px", ctypes.c_void_p), ("py", ctypes.c_void_p),
        ("total_reward", ctypes.c_void_p),
        ("status", ctypes.c_void_p), ("steps", ctypes.c_void_p), ("episode", ctypes.c_void_p),
        ("env_id_base", ctypes.c_int64), ("precision", _I), ("_pad", _I),
    ]


class DDStepIO(ctypes.Structure):
    _fields_ = [
        ("actions", ctypes.c_void_p), ("action_format", _I), ("_pad", _I),
        ("reward", ctypes.c_void_p), ("done", ctypes.c_void_p), ("obs", ctypes.c_void_p),
        ("done_idx", ctypes.c_void_p), ("done_count", ctypes.c_void_p),
        ("shaped_hist", ctypes.c_void_p), ("shaped_reward", ctypes.c_void_p), ("shaped_done", ctypes.c_void_p),
        ("max_steps", _I), ("shaped_mode", _I), ("state_out", ctypes.c_void_p),
    ]


class DDRolloutIO(ctypes.Structure):
    _fields_ = [
        ("actions", ctypes.c_void_p), ("action_format", _I), ("frames", _I),
        ("reward", ctypes.c_void_p), ("done", ctypes.c_void_p), ("obs", ctypes.c_void_p),
        ("action_seed", ctypes.c_uint64), ("action_step", ctypes.c_int64),
        ("shaped_hist", ctypes.c_void_p), ("engine_reward", ctypes.c_void_p), ("engine_done", ctypes.c_void_p),
        ("max_steps", _I), ("shaped_mode", _I), ("kernel", _I), ("_pad", _I),
    ]


class DDMlpParams(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in (
        "w0", "b0", "ln1_w", "ln1_b", "w3", "b3", "ln4_w", "ln4_b",
        "w6", "b6", "ln7_w", "ln7_b", "w9", "b9")] + [("out_dim", _I), ("ln_eps", ctypes.c_float)]


class DDMlpIO(ctypes.Structure):
    _fields_ = [
        ("obs", ctypes.c_void_p), ("out", ctypes.c_void_p), ("actions", ctypes.c_void_p),
        ("log_prob", ctypes.c_void_p), ("seed", ctypes.c_uint64), ("step", ctypes.c_int64),
        ("env_id_base", ctypes.c_int64),
    ]


class DDPolicyRolloutIO(ctypes.Structure):
    _fields_ = [
        ("obs0", ctypes.c_void_p), ("obs_final", ctypes.c_void_p), ("obs", ctypes.c_void_p),
        ("actions", ctypes.c_void_p), ("log_prob", ctypes.c_void_p),
        ("reward", ctypes.c_void_p), ("done", ctypes.c_void_p),
        ("seed", ctypes.c_uint64), ("step", ctypes.c_int64), ("frames", _I), ("max_steps", _I),
        ("shaped_hist", ctypes.c_void_p), ("engine_reward", ctypes.c_void_p), ("engine_done", ctypes.c_void_p),
        ("shaped_mode", _I), ("_pad", _I),
    ]


class DDSampling(ctypes.Structure):
    _fields_ = [("mode", _I), ("temperature", ctypes.c_float), ("probs_used", ctypes.c_void_p)]


class DDEpisodeStats(ctypes.Structure):
    _fields_ = [("ep_return", ctypes.c_void_p), ("ep_steps", ctypes.c_void_p), ("ep_status", ctypes.c_void_p),
                ("ep_fuel", ctypes.c_void_p)]


class DDRewardParts(ctypes.Structure):
    _fields_ = [("sum", ctypes.c_void_p), ("prev_dist", ctypes.c_void_p), ("per_frame", ctypes.c_void_p)]


class DDBatchLayout(ctypes.Structure):
    _fields_ = [("length", ctypes.c_void_p), ("offset", ctypes.c_void_p), ("ended", ctypes.c_void_p)]


class DDBatchGatherIO(ctypes.Structure):
    _fields_ = [("obs", ctypes.c_void_p), ("actions", ctypes.c_void_p), ("log_prob", ctypes.c_void_p),
                ("states", ctypes.c_void_p), ("actions_out", ctypes.c_void_p), ("old_log_probs", ctypes.c_void_p),
                ("tile_frames", _I), ("_pad", _I)]


class DDBatchAdvIO(ctypes.Structure):
    _fields_ = [("reward", ctypes.c_void_p), ("precision", _I), ("mode", _I), ("values", ctypes.c_void_p),
                ("bootstrap", ctypes.c_void_p), ("advantages", ctypes.c_void_p), ("returns", ctypes.c_void_p),
                ("episode_return", ctypes.c_void_p), ("gamma", _D), ("lambda_", _D)]


class DDEpisodeLayout(ctypes.Structure):
    _fields_ = [("lane_episode", ctypes.c_void_p), ("lane_row", ctypes.c_void_p), ("ep_lane", ctypes.c_void_p),
                ("ep_start", ctypes.c_void_p), ("ep_length", ctypes.c_void_p), ("ep_ended", ctypes.c_void_p),
                ("ep_offset", ctypes.c_void_p)]


class DDMlpEvalIO(ctypes.Structure):
    _fields_ = [("obs", ctypes.c_void_p), ("actions", ctypes.c_void_p), ("action_format", _I), ("_pad", _I),
                ("probs", ctypes.c_void_p), ("log_prob", ctypes.c_void_p), ("entropy", ctypes.c_void_p),
                ("n", ctypes.c_int64)]


class DDPpoLossIO(ctypes.Structure):
    _fields_ = [("log_prob", ctypes.c_void_p), ("entropy", ctypes.c_void_p), ("probs", ctypes.c_void_p),
                ("values", ctypes.c_void_p), ("old_log_prob", ctypes.c_void_p), ("advantages", ctypes.c_void_p),
                ("returns", ctypes.c_void_p), ("actions", ctypes.c_void_p), ("action_format", _I), ("_pad", _I),
                ("clip_epsilon", _D), ("entropy_coef", _D), ("value_coef", _D), ("result", ctypes.c_void_p),
                ("ratio", ctypes.c_void_p), ("grad_logits", ctypes.c_void_p), ("grad_values", ctypes.c_void_p)]


class DDMlpGrads(ctypes.Structure):
    """The fourteen gradients, in ``DDMlpParams``' order."""

    _fields_ = [(name, ctypes.c_void_p) for name in (
        "w0", "b0", "ln1_w", "ln1_b", "w3", "b3", "ln4_w", "ln4_b",
        "w6", "b6", "ln7_w", "ln7_b", "w9", "b9")]


class DDMlpBackwardIO(ctypes.Structure):
    _fields_ = [("states", ctypes.c_void_p), ("grad_out", ctypes.c_void_p), ("grads", DDMlpGrads),
                ("grad_norm", ctypes.c_void_p), ("max_norm", _D)]


class DDAdamWHyper(ctypes.Structure):
    _fields_ = [("lr", _D), ("beta1", _D), ("beta2", _D), ("eps", _D), ("weight_decay", _D)]


class DDAdamWState(ctypes.Structure):
    """The optimizer's device-side state block (``dd_adamw_state_bytes()``)."""

    _fields_ = [("step", ctypes.c_int64), ("beta1_t", _D), ("beta2_t", _D), ("status", _I), ("_pad", _I)]


class DDAdamWIO(ctypes.Structure):
    _fields_ = [("params", ctypes.c_void_p), ("grads", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p),
                ("exp_avg_sq", ctypes.c_void_p), ("state", ctypes.c_void_p), ("packed", ctypes.c_void_p),
                ("out_dim", _I), ("compute", _I), ("ln_eps", ctypes.c_float), ("_pad", _I)]


class DDPgLossIO(ctypes.Structure):
    _fields_ = [("log_prob", ctypes.c_void_p), ("probs", ctypes.c_void_p), ("actions", ctypes.c_void_p),
                ("action_format", _I), ("_pad", _I), ("weights", ctypes.c_void_p), ("active", ctypes.c_void_p),
                ("result", ctypes.c_void_p), ("grad_logits", ctypes.c_void_p)]


class DDTdLossIO(ctypes.Structure):
    _fields_ = [("values", ctypes.c_void_p), ("next_values", ctypes.c_void_p), ("rewards", ctypes.c_void_p),
                ("dones", ctypes.c_void_p), ("active", ctypes.c_void_p), ("gamma", _D), ("value_reg", _D),
                ("td_targets", ctypes.c_void_p), ("td_errors", ctypes.c_void_p), ("result", ctypes.c_void_p),
                ("grad_values", ctypes.c_void_p)]


class DDShuffleIO(ctypes.Structure):
    _fields_ = [("states", ctypes.c_void_p), ("actions", ctypes.c_void_p), ("old_log_probs", ctypes.c_void_p),
                ("advantages", ctypes.c_void_p), ("returns", ctypes.c_void_p), ("action_format", _I), ("_pad", _I),
                ("states_out", ctypes.c_void_p), ("actions_out", ctypes.c_void_p),
                ("old_log_probs_out", ctypes.c_void_p), ("advantages_out", ctypes.c_void_p),
                ("returns_out", ctypes.c_void_p), ("indices", ctypes.c_void_p)]


class DDPpoFusedNet(ctypes.Structure):
    """One network of ``dd_ppo_update_fused``: its flat buffers, state block,
    packed image and optimizer settings."""

    _fields_ = [("params", ctypes.c_void_p), ("grads", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p),
                ("exp_avg_sq", ctypes.c_void_p), ("state", ctypes.c_void_p), ("packed", ctypes.c_void_p),
                ("hyper", DDAdamWHyper), ("ln_eps", ctypes.c_float), ("_pad", _I)]


class DDPpoFusedIO(ctypes.Structure):
    _fields_ = [("actor", DDPpoFusedNet), ("critic", DDPpoFusedNet), ("states", ctypes.c_void_p),
                ("actions", ctypes.c_void_p), ("old_log_probs", ctypes.c_void_p), ("advantages", ctypes.c_void_p),
                ("returns", ctypes.c_void_p), ("action_format", _I), ("drop_last", _I), ("m", ctypes.c_int64),
                ("epoch_stride", ctypes.c_int64), ("num_epochs", _I), ("minibatch_size", _I), ("clip_epsilon", _D),
                ("entropy_coef", _D), ("value_coef", _D), ("max_grad_norm", _D), ("logs", ctypes.c_void_p)]


class DDPpoPopulationMember(ctypes.Structure):
    """One learner of ``dd_ppo_update_population``: its networks, its
    unshuffled batch, its coefficients, its shuffle key and its logs."""

    _fields_ = [("actor", DDPpoFusedNet), ("critic", DDPpoFusedNet), ("states", ctypes.c_void_p),
                ("actions", ctypes.c_void_p), ("old_log_probs", ctypes.c_void_p), ("advantages", ctypes.c_void_p),
                ("returns", ctypes.c_void_p), ("action_format", _I), ("shuffle", _I), ("m", ctypes.c_int64),
                ("clip_epsilon", _D), ("entropy_coef", _D), ("value_coef", _D), ("max_grad_norm", _D),
                ("shuffle_seed", ctypes.c_uint64), ("shuffle_epoch", ctypes.c_uint64), ("logs", ctypes.c_void_p)]


class DDPpoPopulationIO(ctypes.Structure):
    _fields_ = [("table", ctypes.POINTER(DDPpoPopulationMember)), ("members", _I), ("num_epochs", _I),
                ("minibatch_size", _I), ("drop_last", _I)]


class DDActorCriticMember(ctypes.Structure):
    """One learner of ``dd_actor_critic_train``: its networks and its coefficients."""

    _fields_ = [("actor", DDPpoFusedNet), ("critic", DDPpoFusedNet), ("gamma", _D), ("value_reg", _D),
                ("max_grad_norm", _D)]


class DDActorCriticIO(ctypes.Structure):
    _fields_ = [("table", ctypes.POINTER(DDActorCriticMember)), ("members", _I), ("frames", _I),
                ("lanes_per_member", ctypes.c_int64), ("obs", ctypes.c_void_p), ("reward", ctypes.c_void_p),
                ("done", ctypes.c_void_p), ("shaped_hist", ctypes.c_void_p), ("shaped_reward", ctypes.c_void_p),
                ("shaped_done", ctypes.c_void_p), ("shaped_mode", _I), ("max_steps", _I),
                ("active0", ctypes.c_void_p), ("done_last", ctypes.c_void_p), ("record_reward", ctypes.c_void_p),
                ("record_done", ctypes.c_void_p), ("seed", ctypes.c_uint64), ("step", ctypes.c_int64),
                ("logs", ctypes.c_void_p)]


class DDReinforceMember(ctypes.Structure):
    """One learner of ``dd_reinforce_train``: its actor and its coefficients."""

    _fields_ = [("actor", DDPpoFusedNet), ("gamma", _D), ("max_grad_norm", _D)]


class DDReinforceIO(ctypes.Structure):
    _fields_ = [("table", ctypes.POINTER(DDReinforceMember)), ("members", _I), ("max_steps", _I),
                ("lanes_per_member", ctypes.c_int64), ("obs", ctypes.c_void_p), ("shaped_hist", ctypes.c_void_p),
                ("shaped_mode", _I), ("env_max_steps", _I), ("normalize", _I), ("_pad", _I),
                ("seed", ctypes.c_uint64), ("step", ctypes.c_int64), ("lengths", ctypes.c_void_p),
                ("ended", ctypes.c_void_p), ("episode_return", ctypes.c_void_p), ("record_reward", ctypes.c_void_p),
                ("record_done", ctypes.c_void_p), ("record_returns", ctypes.c_void_p),
                ("record_advantages", ctypes.c_void_p), ("logs", ctypes.c_void_p)]


class DDPpoTrainMember(ctypes.Structure):
    """One learner of ``dd_ppo_train``: its two networks and its coefficients."""

    _fields_ = [("actor", DDPpoFusedNet), ("critic", DDPpoFusedNet), ("gamma", _D), ("lambda_", _D),
                ("clip_epsilon", _D), ("entropy_coef", _D), ("value_coef", _D), ("max_grad_norm", _D),
                ("shuffle_seed", ctypes.c_uint64)]


class DDPpoTrainIO(ctypes.Structure):
    _fields_ = [("table", ctypes.POINTER(DDPpoTrainMember)), ("members", _I), ("max_steps", _I),
                ("lanes_per_member", ctypes.c_int64), ("obs", ctypes.c_void_p), ("shaped_hist", ctypes.c_void_p),
                ("shaped_mode", _I), ("env_max_steps", _I), ("normalize", _I), ("num_epochs", _I),
                ("minibatch_size", _I), ("drop_last", _I), ("shuffle_epoch", ctypes.c_uint64),
                ("seed", ctypes.c_uint64), ("step", ctypes.c_int64), ("lengths", ctypes.c_void_p),
                ("ended", ctypes.c_void_p), ("episode_return", ctypes.c_void_p), ("landed", ctypes.c_void_p),
                ("record_reward", ctypes.c_void_p), ("record_done", ctypes.c_void_p),
                ("record_values", ctypes.c_void_p), ("record_returns", ctypes.c_void_p),
                ("record_advantages", ctypes.c_void_p), ("logs", ctypes.c_void_p), ("batch_logs", ctypes.c_void_p)]


def sampling_mode(temperature) -> int:
    """The ``DD_SAMPLE_*`` mode of a notebook ``temperature``: 1 is the plain
    Bernoulli draw, 0 greedy (``probs > 0.5``), any other positive finite value
    the tempered draw; anything else raises ``ValueError``."""
    try:
        t = float(temperature)
    except (TypeError, ValueError):
        raise ValueError(f"temperature must be a number, got {temperature!r}") from None
    if t == 0.0:
        return DD_SAMPLE_GREEDY
    if not (0.0 < t < float("inf")):
        raise ValueError(f"temperature must be 0 (greedy) or positive and finite, got {temperature!r}")
    return DD_SAMPLE_BERNOULLI if t == 1.0 else DD_SAMPLE_TEMPERED


#: every symbol include/dronestep.h declares, with its ctypes signature
EXPORTS = {
    "dd_config_default": (None, [ctypes.POINTER(DDConfig)]),
    "dd_step": (ctypes.c_int, [ctypes.POINTER(DDConfig), ctypes.POINTER(DDState),
                               ctypes.POINTER(DDStepIO), ctypes.c_int64, ctypes.c_void_p]),
    "dd_step_variant": (ctypes.c_int32, [ctypes.POINTER(DDConfig), ctypes.POINTER(DDState),
                                         ctypes.POINTER(DDStepIO), ctypes.c_int64]),
    "dd_rollout": (ctypes.c_int, [ctypes.POINTER(DDConfig), ctypes.POINTER(DDState),
                                  ctypes.POINTER(DDRolloutIO), ctypes.c_int64, ctypes.c_void_p]),
    "dd_rollout_kernel": (ctypes.c_int, [ctypes.POINTER(DDConfig), ctypes.POINTER(DDState),
                                         ctypes.POINTER(DDRolloutIO), ctypes.c_int64]),
    "dd_device_errors": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint32), _I]),
    "dd_reset": (ctypes.c_int, [ctypes.POINTER(DDConfig), ctypes.POINTER(DDState), ctypes.c_void_p,
                                ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "dd_shaped_reset": (ctypes.c_int, [ctypes.POINTER(DDConfig), ctypes.POINTER(DDState), ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "dd_write_obs": (ctypes.c_int, [ctypes.POINTER(DDConfig), ctypes.POINTER(DDState), ctypes.c_void_p,
                                    ctypes.c_int64, ctypes.c_void_p]),
    "dd_get_info": (ctypes.c_int, [ctypes.POINTER(DDConfig), ctypes.POINTER(DDState), ctypes.c_void_p,
                                   ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "dd_gae": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                              ctypes.c_int64, ctypes.c_int64, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]),
    "dd_compact_workspace": (ctypes.c_int64, [ctypes.c_int64]),
    "dd_compact": (ctypes.c_int, [ctypes.c_void_p, _I, ctypes.c_void_p, ctypes.c_void_p,
                                  ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "dd_mlp_packed_floats": (ctypes.c_int64, []),
    "dd_mlp_pack": (ctypes.c_int, [ctypes.POINTER(DDMlpParams), _I, ctypes.c_void_p, ctypes.c_void_p]),
    "dd_mlp_forward": (ctypes.c_int, [ctypes.c_void_p, _I, _I, ctypes.POINTER(DDMlpIO), ctypes.c_int64,
                                      ctypes.c_void_p]),
    "dd_policy_rollout": (ctypes.c_int, [ctypes.POINTER(DDConfig), ctypes.POINTER(DDState), ctypes.c_void_p, _I,
                                         ctypes.POINTER(DDPolicyRolloutIO), ctypes.c_int64, ctypes.c_void_p]),
    "dd_mlp_forward_sampled": (ctypes.c_int, [ctypes.c_void_p, _I, _I, ctypes.POINTER(DDMlpIO),
                                              ctypes.POINTER(DDSampling), ctypes.c_int64, ctypes.c_void_p]),
    "dd_policy_rollout_sampled": (ctypes.c_int, [ctypes.POINTER(DDConfig), ctypes.POINTER(DDState), ctypes.c_void_p,
                                                 _I, ctypes.POINTER(DDPolicyRolloutIO), ctypes.POINTER(DDSampling),
                                                 ctypes.POINTER(DDEpisodeStats), ctypes.c_int64, ctypes.c_void_p]),
    "dd_policy_evaluate_parts": (ctypes.c_int, [ctypes.POINTER(DDConfig), ctypes.POINTER(DDState), ctypes.c_void_p,
                                                _I, ctypes.POINTER(DDPolicyRolloutIO), ctypes.POINTER(DDSampling),
                                                ctypes.POINTER(DDEpisodeStats), ctypes.POINTER(DDRewardParts),
                                                ctypes.c_int64, ctypes.c_void_p]),
    "dd_policy_rollout_population": (ctypes.c_int, [ctypes.POINTER(DDConfig), ctypes.POINTER(DDState),
                                                    ctypes.c_void_p, _I, ctypes.c_int64, _I,
                                                    ctypes.POINTER(DDPolicyRolloutIO), ctypes.POINTER(DDSampling),
                                                    ctypes.POINTER(DDEpisodeStats), ctypes.c_int64, ctypes.c_void_p]),
    "dd_render": (ctypes.c_int, [ctypes.POINTER(DDConfig), ctypes.POINTER(DDState), ctypes.c_void_p,
                                 ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, _I,
                                 ctypes.c_void_p]),
    "dd_render_grid": (ctypes.c_int, [ctypes.POINTER(DDConfig), ctypes.POINTER(DDState), ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, _I, _I, ctypes.c_void_p, _I,
                                      ctypes.c_void_p]),
    "dd_step_bytes_per_env": (ctypes.c_int64, [_I, _I, _I]),
    "dd_error_string": (ctypes.c_char_p, [ctypes.c_int]),
    "dd_abi_version": (ctypes.c_int, []),
    "dd_build_info": (ctypes.c_char_p, []),
    "dd_selftest_sqrt": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "dd_stamp": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "dd_wall_clock_khz": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    "dd_device_alloc": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint64, _I]),
    "dd_device_free": (ctypes.c_int, [ctypes.c_void_p]),
    "dd_batch_workspace": (ctypes.c_int64, [ctypes.c_int64]),
    "dd_batch_plan": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(DDBatchLayout),
                                     ctypes.c_void_p, ctypes.c_void_p]),
    "dd_batch_gather": (ctypes.c_int, [ctypes.POINTER(DDBatchLayout), ctypes.POINTER(DDBatchGatherIO),
                                       ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]),
    "dd_batch_advantages": (ctypes.c_int, [ctypes.POINTER(DDBatchLayout), ctypes.POINTER(DDBatchAdvIO),
                                           ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]),
    "dd_batch_normalize": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "dd_episodes_workspace": (ctypes.c_int64, [ctypes.c_int64]),
    "dd_episodes_count": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, _I,
                                         ctypes.POINTER(DDEpisodeLayout), ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p]),
    "dd_episodes_fill": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, _I,
                                        ctypes.POINTER(DDEpisodeLayout), ctypes.c_void_p]),
    "dd_episodes_gather": (ctypes.c_int, [ctypes.POINTER(DDEpisodeLayout), ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.POINTER(DDBatchGatherIO), ctypes.c_int64, ctypes.c_int64,
                                          ctypes.c_void_p]),
    "dd_episodes_advantages": (ctypes.c_int, [ctypes.POINTER(DDEpisodeLayout), ctypes.POINTER(DDBatchAdvIO),
                                              ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]),
    "dd_mlp_evaluate_actions": (ctypes.c_int, [ctypes.c_void_p, _I, ctypes.POINTER(DDMlpEvalIO), ctypes.c_void_p]),
    "dd_ppo_loss_workspace": (ctypes.c_int64, []),
    "dd_ppo_losses": (ctypes.c_int, [ctypes.POINTER(DDPpoLossIO), ctypes.c_int64, ctypes.c_void_p,
                                     ctypes.c_void_p]),
    "dd_mlp_backward_workspace": (ctypes.c_int64, []),
    "dd_mlp_backward": (ctypes.c_int, [ctypes.POINTER(DDMlpParams), ctypes.POINTER(DDMlpBackwardIO), ctypes.c_int64,
                                       ctypes.c_void_p, ctypes.c_void_p]),
    "dd_adamw_state_bytes": (ctypes.c_int64, []),
    "dd_adamw_init": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                     ctypes.c_void_p]),
    "dd_adamw_step": (ctypes.c_int, [ctypes.POINTER(DDAdamWHyper), ctypes.POINTER(DDAdamWIO), ctypes.c_void_p]),
    "dd_pg_loss_workspace": (ctypes.c_int64, []),
    "dd_pg_losses": (ctypes.c_int, [ctypes.POINTER(DDPgLossIO), ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "dd_td_loss_workspace": (ctypes.c_int64, []),
    "dd_td_losses": (ctypes.c_int, [ctypes.POINTER(DDTdLossIO), ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "dd_shuffle_indices": (ctypes.c_int, [ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
                                          ctypes.c_void_p]),
    "dd_shuffle_rows": (ctypes.c_int, [ctypes.POINTER(DDShuffleIO), ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint64,
                                       ctypes.c_void_p]),
    "dd_ppo_update_fused_workspace": (ctypes.c_int64, []),
    "dd_ppo_update_fused": (ctypes.c_int, [ctypes.POINTER(DDPpoFusedIO), ctypes.c_void_p, ctypes.c_void_p]),
    "dd_ppo_update_population_workspace": (ctypes.c_int64, [_I]),
    "dd_ppo_update_population": (ctypes.c_int, [ctypes.POINTER(DDPpoPopulationIO), ctypes.c_void_p, ctypes.c_void_p]),
    "dd_actor_critic_train_workspace": (ctypes.c_int64, [_I]),
    "dd_actor_critic_train": (ctypes.c_int, [ctypes.POINTER(DDConfig), ctypes.POINTER(DDState),
                                             ctypes.POINTER(DDActorCriticIO), ctypes.c_int64, ctypes.c_void_p,
                                             ctypes.c_void_p]),
    "dd_reinforce_train_workspace": (ctypes.c_int64, [_I, ctypes.c_int64, _I]),
    "dd_reinforce_train": (ctypes.c_int, [ctypes.POINTER(DDConfig), ctypes.POINTER(DDState),
                                          ctypes.POINTER(DDReinforceIO), ctypes.c_int64, ctypes.c_void_p,
                                          ctypes.c_void_p]),
    "dd_ppo_train_workspace": (ctypes.c_int64, [_I, ctypes.c_int64, _I]),
    "dd_ppo_train": (ctypes.c_int, [ctypes.POINTER(DDConfig), ctypes.POINTER(DDState), ctypes.POINTER(DDPpoTrainIO),
                                    ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
}

#: symbols a timing-only lab build (tools/build_variants.sh) or an older
#: committed source built for an A/B run may lack
_LAB_OPTIONAL = ("dd_build_info", "dd_selftest_sqrt", "dd_rollout_kernel", "dd_step_variant", "dd_device_errors", "dd_stamp",
                 "dd_wall_clock_khz", "dd_device_alloc", "dd_device_free", "dd_mlp_forward_sampled",
                 "dd_policy_rollout_sampled", "dd_batch_workspace", "dd_batch_plan", "dd_batch_gather",
                 "dd_batch_advantages", "dd_batch_normalize", "dd_episodes_workspace", "dd_episodes_count",
                 "dd_episodes_fill", "dd_episodes_gather", "dd_episodes_advantages", "dd_mlp_evaluate_actions",
                 "dd_ppo_loss_workspace", "dd_ppo_losses", "dd_mlp_backward_workspace", "dd_mlp_backward",
                 "dd_adamw_state_bytes", "dd_adamw_init", "dd_adamw_step", "dd_pg_loss_workspace", "dd_pg_losses",
                 "dd_td_loss_workspace", "dd_td_losses", "dd_shuffle_indices", "dd_shuffle_rows",
                 "dd_policy_evaluate_parts", "dd_policy_rollout_population", "dd_render_grid",
                 "dd_ppo_update_fused_workspace", "dd_ppo_update_fused", "dd_ppo_update_population_workspace",
                 "dd_ppo_update_population", "dd_actor_critic_train_workspace", "dd_actor_critic_train",
                 "dd_reinforce_train_workspace", "dd_reinforce_train",
                 "dd_ppo_train_workspace", "dd_ppo_train")


class NativeLibraryError(RuntimeError):
    """The HIP extension is missing, stale or failed a call."""


_LIB = None
_LOCK = threading.Lock()


def library_path() -> str:
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "_native", "libdronestep.so")


def load(path: str, *, abi_versions=None) -> ctypes.CDLL:
    """Load a build of the library at ``path`` and bind the header's signatures.
    ``abi_versions``: the versions accepted (default: this header's only); A/B
    labs pass the two sides of a version bump whose signatures are unchanged."""
    if not os.path.exists(path):
        raise NativeLibraryError(
            f"HIP extension not built: {path} is missing. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` from the repo root.")
    try:
        handle = ctypes.CDLL(path)
    except OSError as exc:  # pragma: no cover - depends on the box
        raise NativeLibraryError(f"cannot load {path}: {exc}") from exc
    for name, (restype, argtypes) in EXPORTS.items():
        if name in _LAB_OPTIONAL and not hasattr(handle, name):
            continue
        fn = getattr(handle, name)
        fn.restype = restype
        fn.argtypes = argtypes
    if handle.dd_abi_version() not in (abi_versions or (DD_ABI_VERSION,)):
        raise NativeLibraryError(f"{path}: ABI version mismatch; rebuild it")
    return handle


def lib() -> ctypes.CDLL:
    """The product library ``_native/libdronestep.so`` (built by
    ``__graft_entry__.build()``); raises if it is absent."""
    global _LIB
    if _LIB is None:
        with _LOCK:
            if _LIB is None:
                _LIB = load(library_path())
    return _LIB


def check(code: int, what: str) -> None:
    """Raise :class:`NativeLibraryError` for a nonzero HIP status."""
    if code != 0:
        msg = lib().dd_error_string(code)
        raise NativeLibraryError(f"{what} failed: HIP error {code} ({msg.decode() if msg else '?'})")
