"""PPO learners trained on device, one launch per iteration.

One iteration of Actor_Critic_PPO.ipynb's training cell is :func:`collect_ppo`
(reset, rollout, the batch's plan, gather, the critic's values, GAE and the
normalisation) and :func:`ppo_update` (``num_epochs`` of losses, backward,
clip and the two AdamW steps).  :func:`collect_ppo_population` and
:func:`ppo_update_population` run the rollout and the update for a sweep in one
launch each, but build every member's batch in a host loop between them.
:func:`ppo_train_population` runs the whole iteration as the env's reset launch
plus one persistent launch (``dd_ppo_train``, ``csrc/ppo_train_fused.hip``),
member ``g`` of a :class:`LearnerPopulation` on lanes ``[g L, (g + 1) L)`` of
one env, and :func:`ppo_train` does so for one learner.  Both leave the bits of
the loop of launches.
"""
from __future__ import annotations

import ctypes
from functools import partial
from typing import Dict, List, NamedTuple, Optional

import torch

from . import _args, abi, adamw
from .adamw import AdamW, PpoUpdate
from .policy import MlpNet
from .population import LearnerPopulation

__all__ = ["PpoRun", "ppo_train", "ppo_train_population", "ppo_iteration_data", "PPO_BATCH_LOG_KEYS"]

#: the rows of :attr:`PpoRun.batch_logs`
PPO_BATCH_LOG_KEYS = abi.PT_BATCH_LOG_NAMES


class PpoRun(NamedTuple):
    """What a training launch leaves, all on the device.

    ``logs`` is float64 ``[11, num_epochs, steps, members]``, the rows of
    ``adamw.LOG_KEYS``.  With the full batch ``steps`` is 1.  With
    ``minibatch_size=B`` it is ``ceil(L max_steps / B)``, the most a member can
    take: a member whose batch has fewer rows takes fewer steps, and the
    entries past its own are NaN.  ``batch_logs`` is float64
    ``[len(PPO_BATCH_LOG_KEYS), members]``: per member the ``rows`` of its
    batch and the ``adv_mean`` and ``adv_std`` of its raw advantages.
    :meth:`updates` gives each member's :class:`PpoUpdate`."""
    logs: torch.Tensor
    batch_logs: torch.Tensor
    lengths: torch.Tensor                      # int32 [N]: each lane's first episode
    ended: torch.Tensor                        # bool [N]
    landed: torch.Tensor                       # bool [N]: the lane's drone landed
    episode_return: torch.Tensor               # float64 [N], sum(rewards)
    obs: torch.Tensor                          # [N, 15]: env.obs, the observation after the last frame
    minibatch_size: Optional[int] = None
    drop_last: bool = False
    reward: Optional[torch.Tensor] = None      # record=True: [max_steps, N], zeros after a lane's episode
    done: Optional[torch.Tensor] = None        # record=True: bool [max_steps, N]
    values: Optional[torch.Tensor] = None      # record=True: [max_steps, N], the critic at the batch's rows
    returns: Optional[torch.Tensor] = None     # record=True: [max_steps, N]
    advantages: Optional[torch.Tensor] = None  # record=True: [max_steps, N]

    def batch_log(self, key: str) -> torch.Tensor:
        """``batch_logs``' row ``key``, ``[members]``."""
        return self.batch_logs[PPO_BATCH_LOG_KEYS.index(key)]

    def steps_taken(self) -> List[int]:
        """The steps per epoch each member took.  With ``minibatch_size`` this
        reads the members' row counts back (the one host read, on request)."""
        members = self.logs.shape[3]
        if self.minibatch_size is None:
            return [1] * members
        rows = [int(m) for m in self.batch_log("rows").tolist()]
        return [len(adamw.minibatch_ranges(m, min(self.minibatch_size, m), self.drop_last))
                if not (self.drop_last and m < self.minibatch_size) else 0 for m in rows]

    def updates(self) -> List[PpoUpdate]:
        """Member ``g``'s :class:`PpoUpdate`, as ``ppo_update`` returns it:
        ``logs[k]`` is ``[num_epochs]`` for the full batch and ``[num_epochs,
        steps_g]`` with ``minibatch_size`` (see :meth:`steps_taken`)."""
        out = []
        for g, steps in enumerate(self.steps_taken()):
            log = self.logs[:, :, :, g]
            if steps == 0:  # no minibatch (drop_last with fewer rows than one): empty logs, a NaN summary
                nan = torch.full((), float("nan"), dtype=log.dtype, device=log.device)
                out.append(PpoUpdate({k: log[i, :, :0] for i, k in enumerate(adamw.LOG_KEYS)},
                                     {k: nan for k in adamw.LOG_KEYS}))
                continue
            out.append(adamw._update_of(log[:, :, 0] if self.minibatch_size is None else log[:, :, :steps]))
        return out


def ppo_iteration_data(run: PpoRun) -> List[Dict[str, torch.Tensor]]:
    """The training cell's ``iteration_data`` per member, 0-d tensors on the
    run's device: ``success_rate`` (the share of the member's lanes that
    landed), ``avg_reward`` (the mean ``episode_return``), ``avg_steps`` (the
    mean episode length), and the epoch-averaged losses and ratio statistics
    of :attr:`PpoUpdate.summary` under their own names."""
    members = run.logs.shape[3]
    landed = run.landed.reshape(members, -1).to(torch.float64)
    returns = run.episode_return.reshape(members, -1)
    lengths = run.lengths.reshape(members, -1).to(torch.float64)
    out = []
    for g, upd in enumerate(run.updates()):
        data = {"success_rate": landed[g].mean(), "avg_reward": returns[g].mean(), "avg_steps": lengths[g].mean()}
        data.update(upd.summary)
        out.append(data)
    return out


def _check_sticky(env) -> None:
    if env.config.auto_reset:
        raise ValueError("PPO collects one episode per lane here: the env needs auto_reset=False")


def _seed(x) -> int:
    return int(x) & (2 ** 64 - 1)


def _coefficient(name, x) -> float:
    return _args.finite(name, x)


def _clip_epsilon(x) -> float:
    x = _args.finite("clip_epsilon", x)
    if x < 0.0:
        raise ValueError(f"clip_epsilon must not be negative, got {x!r}")
    return x


def _member_table(pop: LearnerPopulation, gamma, lambda_, clip_epsilon, entropy_coef, value_coef, max_grad_norm,
                  shuffle_seed):
    """The launch's member table: every member's networks and seven scalars."""
    members = len(pop)
    scalars = _args.member_scalars(
        members, ("gamma", gamma, partial(_args.finite, "gamma")), ("lambda_", lambda_, partial(_args.finite, "lambda_")),
        ("clip_epsilon", clip_epsilon, _clip_epsilon), ("entropy_coef", entropy_coef, partial(_coefficient, "entropy_coef")),
        ("value_coef", value_coef, partial(_coefficient, "value_coef")), ("max_grad_norm", max_grad_norm, _args.clip_norm),
        ("shuffle_seed", shuffle_seed, _seed))
    table = (abi.DDPpoTrainMember * members)()
    for p, ((actor, critic, actor_opt, critic_opt), s) in enumerate(zip(pop, scalars)):
        table[p] = abi.DDPpoTrainMember(adamw._fused_net(actor, actor_opt), adamw._fused_net(critic, critic_opt), *s)
    return table


def ppo_train_population(env, pop: LearnerPopulation, max_steps: int = 300, *, seed: int = 0, step: int = 0,
                         gamma=0.99, lambda_=0.95, normalize: bool = True, num_epochs: int = 4,
                         minibatch_size: Optional[int] = None, drop_last: bool = False, clip_epsilon=0.2,
                         entropy_coef=0.01, value_coef=0.5, max_grad_norm=0.5, shuffle_seed=0,
                         shuffle_epoch: int = 0, record: bool = False) -> PpoRun:
    """One PPO iteration for every member of ``pop``: ``env.reset()``, then one
    launch.  Member ``g`` drives lanes ``[g L, (g + 1) L)`` of ``env`` (``L =
    env.num_envs / len(pop)``, ``1 <= L <= 128``), and is left bit for bit as
    this loop on an env of those lanes alone (``env_id_base + g L``, the same
    config and ``reward_mode``) leaves it::

        batch = collect_ppo(env_g, actor, critic, max_steps, seed=seed, step=step, gamma=gamma_g,
                            lambda_=lambda_g, normalize=normalize)
        upd = ppo_update(actor, critic, batch, actor_opt, critic_opt, num_epochs=num_epochs,
                         minibatch_size=minibatch_size, drop_last=drop_last, clip_epsilon=..., entropy_coef=...,
                         value_coef=..., max_grad_norm=..., shuffle_seed=..., shuffle_epoch=shuffle_epoch,
                         fused=fits_fused(M, minibatch_size, drop_last))

    That covers every log of ``upd``, ``batch.adv_mean`` and ``batch.adv_std``,
    ``lengths``, ``ended`` and ``episode_return``, both networks' parameters,
    moments, optimizer state blocks, packed images and gradient buffers, and
    the env's arrays, ``obs`` and ``shaped_hist``.  ``record=True`` also
    returns each lane's rewards, dones, values, returns and advantages at their
    frames, ``[max_steps, N]`` with zeros after the lane's episode.

    ``minibatch_size=None`` is the notebook's own loop, ``num_epochs``
    full-batch steps; ``minibatch_size=B`` (at most 128) shuffles with the key
    ``(shuffle_seed, shuffle_epoch + e)`` and steps on every ``B`` rows.  Where
    ``ppo_update`` raises because a member's batch has no minibatch (``M < B``
    with ``drop_last``), that member takes no step here.  ``gamma``,
    ``lambda_``, ``clip_epsilon``, ``entropy_coef``, ``value_coef``,
    ``max_grad_norm`` and ``shuffle_seed`` are a scalar or a list with one value
    per member; the optimizers carry each member's learning rates.  ``env``:
    ``precision="f32"``, ``auto_reset=False``, any ``reward_mode``, any
    :class:`EnvConfig` otherwise.

    Every refusal is a ``ValueError`` before anything is launched, naming the
    member where one is at fault.  Runs on the current stream and reads nothing
    back; it cannot be captured into a graph (the members' table is uploaded
    from host memory at every call)."""
    if not isinstance(pop, LearnerPopulation):
        raise ValueError("pop must be a LearnerPopulation")
    lanes = _args.fused_env_lanes(env, pop, _check_sticky)
    members, n, dev = len(pop), env.num_envs, pop.device
    max_steps = int(max_steps)
    if max_steps < 1:
        raise ValueError(f"max_steps must be at least 1, got {max_steps}")
    if lanes * max_steps > abi.DD_REINFORCE_MAX_CELLS:
        raise ValueError(f"{lanes} lanes x {max_steps} frames per member; the fused training loop records at most "
                         f"{abi.DD_REINFORCE_MAX_CELLS} lane-frames")
    num_epochs = int(num_epochs)
    if num_epochs < 1:
        raise ValueError(f"num_epochs must be at least 1, got {num_epochs}")
    size = None if minibatch_size is None else int(minibatch_size)
    if size is not None and not 1 <= size <= abi.DD_PPO_FUSED_ROWS:
        raise ValueError(f"minibatch_size must be None (the full batch) or in [1, {abi.DD_PPO_FUSED_ROWS}] (one row "
                         f"tile of the backward), got {minibatch_size!r}")
    table = _member_table(pop, gamma, lambda_, clip_epsilon, entropy_coef, value_coef, max_grad_norm, shuffle_seed)

    env.reset()
    if not env._obs_current:  # frame 0's policy input must be the fresh state's observation
        env.get_state()
    steps = 1 if size is None else (lanes * max_steps + size - 1) // size
    logs = torch.empty(abi.DD_PPO_FUSED_LOGS, num_epochs, steps, members, dtype=torch.float64, device=dev)
    batch_logs = torch.empty(abi.DD_PT_BATCH_LOGS, members, dtype=torch.float64, device=dev)
    lengths = torch.empty(n, dtype=torch.int32, device=dev)
    ended = torch.empty(n, dtype=torch.uint8, device=dev)
    landed = torch.empty(n, dtype=torch.uint8, device=dev)
    episode_return = torch.empty(n, dtype=torch.float64, device=dev)
    rec = [torch.empty(max_steps, n, dtype=dt, device=dev) if record else None
           for dt in (torch.float32, torch.uint8, torch.float32, torch.float32, torch.float32)]
    ptr = [t.data_ptr() if record else None for t in rec]
    workspace = pop._train_workspace_for(lanes, max_steps)
    io = abi.DDPpoTrainIO(
        table, members, max_steps, lanes, env.obs.data_ptr(),
        env.shaped_hist.data_ptr() if env.reward_mode == "notebook" else None, env._shaped_mode,
        env.max_steps if env.reward_mode != "engine" else 0, 1 if normalize else 0, num_epochs,
        0 if size is None else size, 1 if drop_last else 0, _seed(shuffle_epoch), _seed(seed), int(step),
        lengths.data_ptr(), ended.data_ptr(), episode_return.data_ptr(), landed.data_ptr(), ptr[0], ptr[1], ptr[2],
        ptr[3], ptr[4], logs.data_ptr(), batch_logs.data_ptr())
    abi.check(pop._lib.dd_ppo_train(ctypes.byref(env._cfg), ctypes.byref(env._state), ctypes.byref(io), n,
                                    workspace.data_ptr(), _args.stream_ptr(dev)), "dd_ppo_train")
    env._trained_in_place()
    return PpoRun(logs, batch_logs, lengths, ended.view(torch.bool), landed.view(torch.bool), episode_return, env.obs,
                  size, bool(drop_last), rec[0], rec[1].view(torch.bool) if record else None, rec[2], rec[3], rec[4])


def ppo_train(env, actor: MlpNet, critic: MlpNet, actor_opt: AdamW, critic_opt: AdamW, max_steps: int = 300,
              **kw) -> PpoRun:
    """:func:`ppo_train_population` for one learner that drives every lane of
    ``env`` (at most 128): one PPO iteration, the logs' last dimension 1.  The
    keywords are :func:`ppo_train_population`'s.  The population of one, with
    its workspace, is built on the first call and kept on ``actor_opt``."""
    pop = LearnerPopulation._of_one(actor_opt, "_ppo_train_pop", (actor, critic, actor_opt, critic_opt))
    return ppo_train_population(env, pop, max_steps, **kw)
