"""One-step actor-critic learners trained online, one launch per episode.

Actor_Critic_Basic.ipynb's training loop updates both networks after every
frame, and the next frame's actions come from the actor that was just updated,
so nothing can be collected ahead.  :func:`actor_critic_train` runs ``frames``
passes of its ``while not all(games_done)`` body (the actor's draw, the frame,
the critic's update, the actor's update) as one persistent launch
(``dd_actor_critic_train``, ``csrc/ac_fused.hip``) instead of about 25 launches
per frame, and :func:`actor_critic_train_population` does so for every member
of a :class:`LearnerPopulation` at once, member ``g`` on lanes ``[g L, (g + 1)
L)`` of one env.  Both leave the bits of the loop of launches
(:meth:`MlpNet.act`, :meth:`VecDroneEnv.step`, :func:`actor_critic_update`).
"""
from __future__ import annotations

import ctypes
from functools import partial
from typing import NamedTuple, Optional

import torch

from . import _args, abi, adamw
from .adamw import AdamW
from .policy import MlpNet
from .population import LearnerPopulation

__all__ = ["ActorCriticRun", "actor_critic_train", "actor_critic_train_population", "AC_LOG_KEYS"]

#: the rows of :attr:`ActorCriticRun.logs`
AC_LOG_KEYS = abi.AC_LOG_NAMES


class ActorCriticRun(NamedTuple):
    """What a training launch leaves, all on the device.  ``logs`` is float64
    ``[len(AC_LOG_KEYS), frames, members]``: per frame and member the
    ``actor_loss``, ``critic_loss``, ``mse``, ``value_reg``, ``count`` (the rows
    that trained), ``actor_grad_norm`` and ``critic_grad_norm`` (before
    clipping) of :func:`actor_critic_update`; :meth:`log` names a row."""
    logs: torch.Tensor
    obs: torch.Tensor                      # [N, 15]: env.obs, the observation after the last frame
    done_last: torch.Tensor                # uint8 [N]: the last frame's done; the next call's active0 is its complement
    reward: Optional[torch.Tensor] = None  # record=True: [frames, N], every frame's returned reward
    done: Optional[torch.Tensor] = None    # record=True: bool [frames, N], every frame's returned done

    def log(self, key: str) -> torch.Tensor:
        """``logs``' row ``key``, ``[frames, members]``."""
        return self.logs[AC_LOG_KEYS.index(key)]


def _check_reward_mode(env) -> None:
    if env.reward_mode not in ("engine", "notebook"):
        raise ValueError(f"reward_mode must be 'engine' or 'notebook', this env has {env.reward_mode!r}")


def actor_critic_train_population(env, pop: LearnerPopulation, frames: int, *, seed: int = 0, step: int = 0,
                                  gamma=0.99, value_reg=0.01, max_grad_norm=0.5, active0=None,
                                  record: bool = False) -> ActorCriticRun:
    """``frames`` frames of the one-step actor-critic loop for every member of
    ``pop`` in one launch.  Member ``g`` drives lanes ``[g L, (g + 1) L)`` of
    ``env`` (``L = env.num_envs / len(pop)``, ``1 <= L <= 128``), and is left
    bit for bit as this loop on an env of those lanes alone (``env_id_base +
    g L``) leaves it::

        obs = env's current observation; done_prev = ~active0 (zeros if None)
        for t in range(frames):
            state = obs.clone()
            actions, _ = actor.act(state, seed=seed, step=step + t, env_id_base=...)
            obs, reward, done, _ = env.step(actions)
            actor_critic_update(actor, critic, state, actions, reward, obs, done, actor_opt, critic_opt,
                                gamma=, value_reg=, max_grad_norm=, active=~done_prev)
            done_prev = done

    so the re-spawn frame of an ``auto_reset=True`` env does not train, nor do
    the lanes of a sticky env that were done before the frame.  That covers
    the logs (a frame with no active row logs NaN losses and zero norms, and
    its zero-gradient steps are taken), the parameters, moments, optimizer
    state blocks, packed images and gradient buffers, and the env's arrays and
    ``obs``.  Two calls chained through ``step=step + frames`` and
    ``active0=~run.done_last.bool()`` equal one call of twice the frames.

    ``gamma``, ``value_reg`` and ``max_grad_norm`` are a scalar or a list with
    one value per member; the optimizers carry each member's learning rate.
    ``env``: ``precision="f32"``, ``reward_mode`` ``"engine"`` or
    ``"notebook"`` (with the env's ``max_steps``), ``auto_reset`` on or off,
    any :class:`EnvConfig`.  ``frames`` is a host integer: there is no "until
    all done" on the device, a sticky env whose lanes have all finished takes
    masked steps.  ``record=True`` also returns every frame's reward and done.

    Every refusal is a ``ValueError`` before anything is launched, naming the
    member where one is at fault.  Runs on the current stream and reads nothing
    back; it cannot be captured into a graph (the members' table is uploaded
    from host memory at every call)."""
    if not isinstance(pop, LearnerPopulation):
        raise ValueError("pop must be a LearnerPopulation")
    lanes = _args.fused_env_lanes(env, pop, _check_reward_mode)
    members, n, dev = len(pop), env.num_envs, pop.device
    frames = int(frames)
    if frames < 1:
        raise ValueError(f"frames must be at least 1, got {frames}")
    scalars = _args.member_scalars(members, ("gamma", gamma, partial(_args.finite, "gamma")),
                                   ("value_reg", value_reg, partial(_args.finite, "value_reg")),
                                   ("max_grad_norm", max_grad_norm, _args.clip_norm))
    active0 = _args.active_mask(active0, n, dev)

    table = (abi.DDActorCriticMember * members)()
    for p, ((actor, critic, actor_opt, critic_opt), (g, reg, norm)) in enumerate(zip(pop, scalars)):
        table[p] = abi.DDActorCriticMember(adamw._fused_net(actor, actor_opt),
                                           adamw._fused_net(critic, critic_opt), g, reg, norm)
    if not env._obs_current:  # frame 0's policy input must be the current state's observation
        env.get_state()
    logs = torch.empty(abi.DD_AC_LOGS, frames, members, dtype=torch.float64, device=dev)
    done_last = torch.empty(n, dtype=torch.uint8, device=dev)
    rec_reward = torch.empty(frames, n, dtype=torch.float32, device=dev) if record else None
    rec_done = torch.empty(frames, n, dtype=torch.uint8, device=dev) if record else None
    notebook = env.reward_mode == "notebook"
    io = abi.DDActorCriticIO(
        table, members, frames, lanes, env.obs.data_ptr(), env.reward.data_ptr(), env._done.data_ptr(),
        env.shaped_hist.data_ptr() if notebook else None, env.shaped_reward.data_ptr() if notebook else None,
        env._shaped_done.data_ptr() if notebook else None, abi.DD_SHAPED_PPO, env.max_steps if notebook else 0,
        active0.data_ptr() if active0 is not None else None, done_last.data_ptr(),
        rec_reward.data_ptr() if record else None, rec_done.data_ptr() if record else None,
        int(seed) & (2 ** 64 - 1), int(step), logs.data_ptr())
    abi.check(pop._lib.dd_actor_critic_train(ctypes.byref(env._cfg), ctypes.byref(env._state), ctypes.byref(io), n,
                                             pop._workspace.data_ptr(), _args.stream_ptr(dev)),
              "dd_actor_critic_train")
    env._trained_in_place()
    return ActorCriticRun(logs, env.obs, done_last, rec_reward, rec_done.view(torch.bool) if record else None)


def actor_critic_train(env, actor: MlpNet, critic: MlpNet, actor_opt: AdamW, critic_opt: AdamW, frames: int, *,
                       seed: int = 0, step: int = 0, gamma: float = 0.99, value_reg: float = 0.01,
                       max_grad_norm: float = 0.5, active0=None, record: bool = False) -> ActorCriticRun:
    """:func:`actor_critic_train_population` for one learner that drives every
    lane of ``env`` (at most 128): ``frames`` frames of the notebook's loop in
    one launch, ``logs`` ``[len(AC_LOG_KEYS), frames, 1]``.  The population of
    one, with its workspace, is built on the first call and kept on
    ``actor_opt``."""
    pop = LearnerPopulation._of_one(actor_opt, "_ac_pop", (actor, critic, actor_opt, critic_opt))
    return actor_critic_train_population(env, pop, frames, seed=seed, step=step, gamma=gamma, value_reg=value_reg,
                                         max_grad_norm=max_grad_norm, active0=active0, record=record)
