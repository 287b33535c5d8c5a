"""REINFORCE learners trained on device, one launch per iteration.

One iteration of Policy_Gradients.ipynb's training loop is
:func:`collect_reinforce` (reset, rollout, the batch's plan, gather, returns
and normalisation) and :func:`reinforce_update` (score, loss, backward, clip,
AdamW, re-pack): about fifteen launches per learner, on batches of a few
thousand rows.  :func:`reinforce_train` runs it as the env's reset launch plus
one persistent launch (``dd_reinforce_train``, ``csrc/reinforce_fused.hip``),
and :func:`reinforce_train_population` does so for every member of a
:class:`ReinforcePopulation` at once, member ``g`` on lanes ``[g L, (g + 1)
L)`` of one env.  Both leave the bits of the loop of launches.
"""
from __future__ import annotations

import ctypes
from functools import partial
from typing import NamedTuple, Optional

import torch

from . import _args, abi, adamw
from .adamw import AdamW
from .policy import MlpNet
from .population import ReinforcePopulation

__all__ = ["ReinforceRun", "reinforce_train", "reinforce_train_population", "REINFORCE_LOG_KEYS"]

#: the rows of :attr:`ReinforceRun.logs`
REINFORCE_LOG_KEYS = abi.RF_LOG_NAMES


class ReinforceRun(NamedTuple):
    """What a training launch leaves, all on the device.  ``logs`` is float64
    ``[len(REINFORCE_LOG_KEYS), members]``: per member the ``loss`` and the
    ``grad_norm`` (before clipping) of :func:`reinforce_update`, the
    ``baseline`` and ``std`` of its batch and its ``rows``; :meth:`log` names
    a row.  The per-lane tensors are :class:`ReinforceBatch`'s."""
    logs: torch.Tensor
    lengths: torch.Tensor                      # int32 [N]: each lane's first episode
    ended: torch.Tensor                        # bool [N]
    episode_return: torch.Tensor               # float64 [N], sum(rewards)
    obs: torch.Tensor                          # [N, 15]: env.obs, the observation after the last frame
    reward: Optional[torch.Tensor] = None      # record=True: [max_steps, N], zeros after a lane's episode
    done: Optional[torch.Tensor] = None        # record=True: bool [max_steps, N]
    returns: Optional[torch.Tensor] = None     # record=True: [max_steps, N], the batch's returns at their frames
    advantages: Optional[torch.Tensor] = None  # record=True: [max_steps, N]

    def log(self, key: str) -> torch.Tensor:
        """``logs``' row ``key``, ``[members]``."""
        return self.logs[REINFORCE_LOG_KEYS.index(key)]


def _check_sticky(env) -> None:
    if env.config.auto_reset:
        raise ValueError("REINFORCE collects one episode per lane: the env needs auto_reset=False")


def reinforce_train_population(env, pop: ReinforcePopulation, max_steps: int = 300, *, seed: int = 0, step: int = 0,
                               gamma=0.99, max_grad_norm=0.5, normalize: bool = True,
                               record: bool = False) -> ReinforceRun:
    """One REINFORCE iteration for every member of ``pop``: ``env.reset()``,
    then one launch.  Member ``g`` drives lanes ``[g L, (g + 1) L)`` of ``env``
    (``L = env.num_envs / len(pop)``, ``1 <= L <= 128``), and is left bit for
    bit as this loop on an env of those lanes alone (``env_id_base + g L``, the
    same config and ``reward_mode``) leaves it::

        batch = collect_reinforce(env_g, actor, max_steps, seed=seed, step=step, gamma=gamma_g, normalize=normalize)
        upd = reinforce_update(actor, batch, opt, max_grad_norm=norm_g)

    That covers the logs (``upd.loss``, ``upd.grad_norm``, ``batch.baseline``,
    ``batch.std``), ``lengths``, ``ended`` and ``episode_return``, the
    parameters, both moments, the optimizer state block, the packed image and
    the gradient buffer, and the env's arrays and ``obs``.  ``record=True``
    also returns each lane's rewards, dones, returns and advantages at their
    frames, ``[max_steps, N]`` with zeros after the lane's episode.

    ``gamma`` and ``max_grad_norm`` are a scalar or a list with one value per
    member; the optimizers carry each member's learning rate.  ``env``:
    ``precision="f32"``, ``auto_reset=False`` (one episode per lane, as the
    notebook's ``collect_episodes``), any ``reward_mode`` (``"engine"``,
    ``"notebook"`` or ``"reinforce"``; the shaped ones with the env's
    ``max_steps`` timeout), any :class:`EnvConfig` otherwise.

    Every refusal is a ``ValueError`` before anything is launched, naming the
    member where one is at fault.  Runs on the current stream and reads nothing
    back; it cannot be captured into a graph (the members' table is uploaded
    from host memory at every call)."""
    if not isinstance(pop, ReinforcePopulation):
        raise ValueError("pop must be a ReinforcePopulation")
    lanes = _args.fused_env_lanes(env, pop, _check_sticky)
    members, n, dev = len(pop), env.num_envs, pop.device
    max_steps = int(max_steps)
    if max_steps < 1:
        raise ValueError(f"max_steps must be at least 1, got {max_steps}")
    if lanes * max_steps > abi.DD_REINFORCE_MAX_CELLS:
        raise ValueError(f"{lanes} lanes x {max_steps} frames per member; the fused training loop records at most "
                         f"{abi.DD_REINFORCE_MAX_CELLS} lane-frames")
    scalars = _args.member_scalars(members, ("gamma", gamma, partial(_args.finite, "gamma")),
                                   ("max_grad_norm", max_grad_norm, _args.clip_norm))

    table = (abi.DDReinforceMember * members)()
    for p, ((actor, opt), (g, norm)) in enumerate(zip(pop, scalars)):
        table[p] = abi.DDReinforceMember(adamw._fused_net(actor, opt), g, norm)
    env.reset()
    if not env._obs_current:  # frame 0's policy input must be the fresh state's observation
        env.get_state()
    logs = torch.empty(abi.DD_RF_LOGS, members, dtype=torch.float64, device=dev)
    lengths = torch.empty(n, dtype=torch.int32, device=dev)
    ended = torch.empty(n, dtype=torch.uint8, device=dev)
    episode_return = torch.empty(n, dtype=torch.float64, device=dev)
    rec = [torch.empty(max_steps, n, dtype=dt, device=dev) if record else None
           for dt in (torch.float32, torch.uint8, torch.float32, torch.float32)]
    ptr = [t.data_ptr() if record else None for t in rec]
    workspace = pop._workspace_for(lanes, max_steps)
    io = abi.DDReinforceIO(
        table, members, max_steps, lanes, env.obs.data_ptr(),
        env.shaped_hist.data_ptr() if env.reward_mode == "notebook" else None, env._shaped_mode,
        env.max_steps if env.reward_mode != "engine" else 0, 1 if normalize else 0, 0,
        int(seed) & (2 ** 64 - 1), int(step), lengths.data_ptr(), ended.data_ptr(), episode_return.data_ptr(),
        ptr[0], ptr[1], ptr[2], ptr[3], logs.data_ptr())
    abi.check(pop._lib.dd_reinforce_train(ctypes.byref(env._cfg), ctypes.byref(env._state), ctypes.byref(io), n,
                                          workspace.data_ptr(), _args.stream_ptr(dev)), "dd_reinforce_train")
    env._trained_in_place()
    return ReinforceRun(logs, lengths, ended.view(torch.bool), episode_return, env.obs, rec[0],
                        rec[1].view(torch.bool) if record else None, rec[2], rec[3])


def reinforce_train(env, actor: MlpNet, opt: AdamW, max_steps: int = 300, *, seed: int = 0, step: int = 0,
                    gamma: float = 0.99, max_grad_norm: float = 0.5, normalize: bool = True,
                    record: bool = False) -> ReinforceRun:
    """:func:`reinforce_train_population` for one learner that drives every
    lane of ``env`` (at most 128): one REINFORCE iteration, ``logs``
    ``[len(REINFORCE_LOG_KEYS), 1]``.  The population of one, with its
    workspace, is built on the first call and kept on ``opt``."""
    pop = ReinforcePopulation._of_one(opt, "_reinforce_pop", (actor, opt))
    return reinforce_train_population(env, pop, max_steps, seed=seed, step=step, gamma=gamma,
                                      max_grad_norm=max_grad_norm, normalize=normalize, record=record)
