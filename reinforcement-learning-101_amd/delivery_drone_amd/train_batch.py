"""PPO and REINFORCE training batches from rollout buffers, on device.

The stretch between a finished rollout and the tensors the notebooks' loss
functions take.  In the reference it is a host loop over episodes
(Actor_Critic_PPO.ipynb's training cell, "PHASE 2": stack the states, run the
critic, ``compute_gae``, ``returns = advantages + values``, then ``torch.cat``
and the batch normalisation; Policy_Gradients.ipynb's: ``compute_returns``,
the baseline and the same normalisation).  Here the input is one rollout as
:meth:`VecDroneEnv.policy_rollout` returns it, ``[frames, N]`` buffers in which
every lane's episode has its own length, and four stages of
``csrc/train_batch.hip`` build the ragged batch:

* plan: each lane's first-episode ``length`` (first done + 1, or ``frames``),
  ``ended`` and the row ``offset`` (exclusive scan; ``offset[N] = M``).  Row
  ``offset[i] + t`` of every flat tensor is lane ``i``'s frame ``t``:
  episode-major, the order of the notebook's ``torch.cat``.  The wrapper reads
  ``M`` once (the one synchronisation per batch) and allocates exact sizes.
* gather: ``states [M, 15]``, ``actions [M, 3]`` float (main, left, right),
  ``old_log_probs [M]``.
* advantages: ``compute_gae`` per episode on the critic's values of the ``M``
  gathered rows (bit for bit :func:`~delivery_drone_amd.gae` on the valid
  rows), or ``compute_returns`` in double; and ``sum(rewards)`` per episode.
* normalise: ``(a - mean) / (std + 1e-8)``, mean and unbiased std accumulated
  in double in a fixed order (the same bits on every run).  With fewer than
  two rows (``M < 2``) std and the normalised values are NaN, as torch's.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import torch

from . import _args, abi

__all__ = ["PpoBatch", "ReinforceBatch", "ppo_batch", "reinforce_batch", "collect_ppo",
           "PpoEpisodesBatch", "ReinforceEpisodesBatch", "ppo_episodes_batch", "reinforce_episodes_batch",
           "collect_ppo_steps"]


class PpoBatch(NamedTuple):
    states: Optional[torch.Tensor]         # [M, 15]
    actions: Optional[torch.Tensor]        # [M, 3] float32, 1.0 / 0.0 (main, left, right)
    old_log_probs: Optional[torch.Tensor]  # [M]
    advantages: torch.Tensor               # [M], normalised unless normalize=False
    returns: torch.Tensor                  # [M] = raw advantages + values
    values: torch.Tensor                   # [M], the critic on states
    lengths: torch.Tensor                  # [N] int32
    offsets: torch.Tensor                  # [N + 1] int64, offsets[N] = M
    ended: torch.Tensor                    # [N] bool
    episode_return: torch.Tensor           # [N] float64, sum(rewards)
    adv_mean: torch.Tensor                 # 0-d float64, of the raw advantages
    adv_std: torch.Tensor                  # 0-d float64, unbiased


class ReinforceBatch(NamedTuple):
    states: Optional[torch.Tensor]
    actions: Optional[torch.Tensor]
    returns: torch.Tensor                  # [M] discounted returns, float32
    advantages: torch.Tensor               # [M] (returns - baseline) / (std + 1e-8); returns with normalize=False
    baseline: torch.Tensor                 # 0-d float64, mean of returns
    std: torch.Tensor                      # 0-d float64, unbiased
    lengths: torch.Tensor
    offsets: torch.Tensor
    ended: torch.Tensor
    episode_return: torch.Tensor


def _ptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


def _rollout_buffer(t, shape, dtype, dev, what):
    """An optional [T, N(, 15)] rollout buffer: checked, never copied."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
        raise ValueError(f"{what} must be a tensor of shape {shape}, got "
                         f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    if t.device != dev:
        raise ValueError(f"{what} is on {t.device}, done on {dev}")
    if t.dtype != dtype and not (dtype == torch.uint8 and t.dtype == torch.bool):
        raise ValueError(f"{what} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    return t.view(torch.uint8) if t.dtype == torch.bool else t


class _PlanBase:
    """What the two layouts share: the check of ``done``, and gather, advantages
    and normalize around the subclass's entry points.  A subclass sets
    ``layout``, ``workspace`` and ``M``, and gives ``_gather(io)`` /
    ``_advantages(io)`` (the ABI calls), ``_episodes`` (entries of
    ``episode_return``) and ``_launch_empty`` (whether an ``M == 0`` batch is
    still launched)."""

    def __init__(self, done: torch.Tensor):
        if not isinstance(done, torch.Tensor) or done.dim() != 2:
            raise ValueError("done must be [T, N]")
        if done.device.type != "cuda":
            raise ValueError("training batches are built on the GPU; move the rollout to a CUDA/HIP device")
        if done.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"done must be bool or uint8, got {done.dtype}")
        if not done.is_contiguous():
            raise ValueError("done must be contiguous")
        self.T, self.n = (int(s) for s in done.shape)
        self.dev = done.device
        self.done = done.view(torch.uint8) if done.dtype == torch.bool else done
        self.lib = abi.lib()

    def gather(self, obs, actions, log_prob, tile_frames: int = 0):
        T, n, dev, M = self.T, self.n, self.dev, self.M
        obs = _rollout_buffer(obs, (T, n, abi.DD_OBS_DIM), torch.float32, dev, "obs")
        actions = _rollout_buffer(actions, (T, n), torch.uint8, dev, "actions")
        log_prob = _rollout_buffer(log_prob, (T, n), torch.float32, dev, "log_prob")
        states = torch.empty(M, abi.DD_OBS_DIM, dtype=torch.float32, device=dev) if obs is not None else None
        acts = torch.empty(M, 3, dtype=torch.float32, device=dev) if actions is not None else None
        lps = torch.empty(M, dtype=torch.float32, device=dev) if log_prob is not None else None
        if M > 0 or self._launch_empty:
            self._gather(abi.DDBatchGatherIO(_ptr(obs), _ptr(actions), _ptr(log_prob), _ptr(states), _ptr(acts),
                                             _ptr(lps), int(tile_frames), 0))
        return states, acts, lps

    def advantages(self, reward, mode, gamma, lambda_=0.0, values=None, bootstrap=None):
        T, n, dev, M = self.T, self.n, self.dev, self.M
        if not isinstance(reward, torch.Tensor) or reward.dtype not in (torch.float32, torch.float64):
            raise ValueError("reward must be a float32 or float64 tensor")
        reward = _rollout_buffer(reward, (T, n), reward.dtype, dev, "reward")
        adv = torch.empty(M, dtype=torch.float32, device=dev) if mode == abi.DD_BATCH_GAE else None
        ret = torch.empty(M, dtype=torch.float32, device=dev)
        ep = torch.empty(self._episodes, dtype=torch.float64, device=dev)
        if M > 0 or self._launch_empty:
            self._advantages(abi.DDBatchAdvIO(reward.data_ptr(),
                                              abi.DD_F64 if reward.dtype == torch.float64 else abi.DD_F32, mode,
                                              _ptr(values), _ptr(bootstrap), _ptr(adv), ret.data_ptr(), ep.data_ptr(),
                                              float(gamma), float(lambda_)))
        return adv, ret, ep

    def normalize(self, x: torch.Tensor, normalize: bool):
        """(mean, std, normalised x or x itself)."""
        stats = torch.empty(2, dtype=torch.float64, device=self.dev)
        out = torch.empty_like(x) if normalize else None
        abi.check(self.lib.dd_batch_normalize(_ptr(x) if self.M else None, _ptr(out) if self.M else None, self.M,
                                              stats[0:].data_ptr(), stats[1:].data_ptr(), self.workspace.data_ptr(),
                                              _args.stream_ptr(self.dev)), "dd_batch_normalize")
        return stats[0], stats[1], out if normalize else x


class _Plan(_PlanBase):
    """The layout of one rollout's batch and what the later stages need of it."""
    _launch_empty = True

    def __init__(self, done: torch.Tensor):
        super().__init__(done)
        n, dev = self.n, self.dev
        self.lengths = torch.empty(n, dtype=torch.int32, device=dev)
        self.offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
        self.ended = torch.empty(n, dtype=torch.uint8, device=dev)
        self.workspace = torch.empty(int(self.lib.dd_batch_workspace(n)) // 8, dtype=torch.int64, device=dev)
        self.layout = abi.DDBatchLayout(self.lengths.data_ptr(), self.offsets.data_ptr(), self.ended.data_ptr())
        abi.check(self.lib.dd_batch_plan(self.done.data_ptr(), self.T, n, ctypes.byref(self.layout),
                                         self.workspace.data_ptr(), _args.stream_ptr(dev)), "dd_batch_plan")
        self.M = int(self.offsets[n].item())  # the one synchronisation: the flat tensors' size
        self._episodes = n

    def _gather(self, io):
        abi.check(self.lib.dd_batch_gather(ctypes.byref(self.layout), ctypes.byref(io), self.T, self.n,
                                           _args.stream_ptr(self.dev)), "dd_batch_gather")

    def _advantages(self, io):
        abi.check(self.lib.dd_batch_advantages(ctypes.byref(self.layout), ctypes.byref(io), self.T, self.n,
                                               _args.stream_ptr(self.dev)), "dd_batch_advantages")


def _values(critic, rows: torch.Tensor, what: str) -> torch.Tensor:
    with torch.no_grad():
        v = critic(rows)
    if not isinstance(v, torch.Tensor) or v.numel() != rows.shape[0]:
        raise ValueError(f"critic({what}) must give one value per row")
    if v.device != rows.device:
        raise ValueError(f"critic({what}) is on {v.device}, the rollout on {rows.device}")
    return v.detach().reshape(-1).to(torch.float32).contiguous()


def ppo_batch(obs: torch.Tensor, actions: Optional[torch.Tensor], log_prob: Optional[torch.Tensor],
              reward: torch.Tensor, done: torch.Tensor, critic, bootstrap_obs: Optional[torch.Tensor] = None,
              gamma: float = 0.99, lambda_: float = 0.95, normalize: bool = True) -> PpoBatch:
    """The PPO notebook's "PHASE 2" over one rollout (each lane's first episode).

    ``obs [T, N, 15]`` float32, ``actions [T, N]`` uint8 bitmasks and
    ``log_prob [T, N]`` float32 (either may be ``None``, its output is then
    ``None``), ``reward [T, N]`` float32 or float64, ``done [T, N]`` bool or
    uint8: contiguous, on one GPU.  ``critic`` maps ``[rows, 15]`` to one
    value per row (an :class:`~delivery_drone_amd.MlpNet` with ``out_dim ==
    1``); it runs on the ``M`` gathered rows, and on ``bootstrap_obs [N, 15]``
    (the observation after the last frame, ``env.obs``; default: bootstrap 0)
    for the episodes that did not end.  ``normalize=False`` leaves
    ``advantages`` raw (``adv_mean`` / ``adv_std`` are still returned, so
    that several ranks can combine their statistics).  ``M < 2``: NaN.
    """
    plan = _Plan(done)
    if obs is None:
        raise ValueError("ppo_batch needs obs: the critic runs on the gathered states")
    states, acts, lps = plan.gather(obs, actions, log_prob)
    values = _values(critic, states, "states")
    bootstrap = None
    if bootstrap_obs is not None:
        b = _rollout_buffer(bootstrap_obs, (plan.n, abi.DD_OBS_DIM), torch.float32, plan.dev, "bootstrap_obs")
        bootstrap = _values(critic, b, "bootstrap_obs")
    raw, ret, ep = plan.advantages(reward, abi.DD_BATCH_GAE, gamma, lambda_, values=values, bootstrap=bootstrap)
    mean, std, adv = plan.normalize(raw, normalize)
    return PpoBatch(states, acts, lps, adv, ret, values, plan.lengths, plan.offsets, plan.ended.view(torch.bool), ep,
                    mean, std)


def reinforce_batch(obs: Optional[torch.Tensor], actions: Optional[torch.Tensor], reward: torch.Tensor,
                    done: torch.Tensor, gamma: float = 0.99, normalize: bool = True) -> ReinforceBatch:
    """The REINFORCE notebook's batch: ``compute_returns`` per episode (double,
    rounded to float32 once), ``baseline`` = their mean, ``advantages`` =
    ``(returns - baseline) / (std + 1e-8)`` (the notebook's baseline
    subtraction followed by its normalisation; ``normalize=False``: the
    returns themselves).  Buffers as :func:`ppo_batch`; ``obs`` and
    ``actions`` are optional."""
    plan = _Plan(done)
    states, acts, _ = plan.gather(obs, actions, None)
    _, ret, ep = plan.advantages(reward, abi.DD_BATCH_RETURNS, gamma)
    mean, std, adv = plan.normalize(ret, normalize)
    return ReinforceBatch(states, acts, ret, adv, mean, std, plan.lengths, plan.offsets,
                          plan.ended.view(torch.bool), ep)


def collect_ppo(env, actor, critic, max_steps: int = 300, seed: int = 0, step: int = 0, gamma: float = 0.99,
                lambda_: float = 0.95, normalize: bool = True) -> PpoBatch:
    """One PPO iteration's data: ``env.reset()``, ``env.policy_rollout(actor,
    max_steps, seed=seed, step=step)`` (``collect_episodes_ppo``), then
    :func:`ppo_batch` with ``env.obs`` as the bootstrap state."""
    env.reset()
    obs, acts, lp, reward, done = env.policy_rollout(actor, int(max_steps), seed=seed, step=step)
    return ppo_batch(obs, acts, lp, reward, done, critic, bootstrap_obs=env.obs, gamma=gamma, lambda_=lambda_,
                     normalize=normalize)


# ---- every episode of a rollout (csrc/train_batch_episodes.hip) --------------
#
# The stages above keep each lane's first episode.  On an ``auto_reset=True``
# env the later episodes are in the same ``[frames, N]`` buffers; the functions
# below batch all of them.  ``done`` alone decides (include/dronestep.h): frame
# ``t`` of a lane is dropped when the frame before it was done (``done[t - 1]``,
# or ``done_before`` for ``t == 0``): the re-spawn frame of an auto-reset env,
# every later frame of a sticky one.  An episode is a maximal run of kept
# frames; it is *ended* when its last frame is done, else *open* (cut by the end
# of the rollout; the lane's last).  Lanes ascend and a lane's episodes are in
# time order, so a lane's rows are its kept frames in frame order.

class PpoEpisodesBatch(NamedTuple):
    states: Optional[torch.Tensor]         # [M, 15]
    actions: Optional[torch.Tensor]        # [M, 3] float32, 1.0 / 0.0 (main, left, right)
    old_log_probs: Optional[torch.Tensor]  # [M]
    advantages: torch.Tensor               # [M], normalised unless normalize=False
    returns: torch.Tensor                  # [M] = raw advantages + values
    values: torch.Tensor                   # [M], the critic on states
    ep_lane: torch.Tensor                  # [E] int32
    ep_start: torch.Tensor                 # [E] int32, the frame of the episode's first row
    ep_lengths: torch.Tensor               # [E] int32
    ep_offsets: torch.Tensor               # [E + 1] int64, ep_offsets[E] = M
    ep_ended: torch.Tensor                 # [E] bool
    episode_return: torch.Tensor           # [E] float64, sum(rewards)
    lane_episode_offsets: torch.Tensor     # [N + 1] int64: lane i's episodes are [o[i], o[i + 1])
    lane_row_offsets: torch.Tensor         # [N + 1] int64: and its rows
    adv_mean: torch.Tensor                 # 0-d float64, of the raw advantages
    adv_std: torch.Tensor                  # 0-d float64, unbiased


class ReinforceEpisodesBatch(NamedTuple):
    states: Optional[torch.Tensor]
    actions: Optional[torch.Tensor]
    returns: torch.Tensor                  # [M] discounted returns, float32
    advantages: torch.Tensor               # [M] (returns - baseline) / (std + 1e-8); returns with normalize=False
    baseline: torch.Tensor                 # 0-d float64, mean of returns
    std: torch.Tensor                      # 0-d float64, unbiased
    ep_lane: torch.Tensor
    ep_start: torch.Tensor
    ep_lengths: torch.Tensor
    ep_offsets: torch.Tensor
    ep_ended: torch.Tensor
    episode_return: torch.Tensor
    lane_episode_offsets: torch.Tensor
    lane_row_offsets: torch.Tensor


class _EpisodePlan(_PlanBase):
    """The episode layout of one rollout and what the later stages need of it."""
    _launch_empty = False

    def __init__(self, done: torch.Tensor, done_before: Optional[torch.Tensor] = None, drop_open: bool = False):
        super().__init__(done)
        T, n, dev, lib = self.T, self.n, self.dev, self.lib
        self.done_before = _rollout_buffer(done_before, (n,), torch.uint8, dev, "done_before")
        self.flags = abi.DD_EPISODES_DROP_OPEN if drop_open else 0
        self.lane_episode = torch.empty(n + 1, dtype=torch.int64, device=dev)
        self.lane_row = torch.empty(n + 1, dtype=torch.int64, device=dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        size = max(int(lib.dd_episodes_workspace(n)), int(lib.dd_batch_workspace(n)))
        self.workspace = torch.empty(size // 8, dtype=torch.int64, device=dev)
        self.layout = abi.DDEpisodeLayout(self.lane_episode.data_ptr(), self.lane_row.data_ptr())
        abi.check(lib.dd_episodes_count(_ptr(self.done), _ptr(self.done_before), T, n, self.flags,
                                        ctypes.byref(self.layout), totals.data_ptr(), self.workspace.data_ptr(),
                                        _args.stream_ptr(dev)), "dd_episodes_count")
        self.E, self.M = E, M = tuple(int(v) for v in totals.tolist())  # the one synchronisation: the flat tensors' size
        self._episodes = E
        self.ep_lane = torch.empty(E, dtype=torch.int32, device=dev)
        self.ep_start = torch.empty(E, dtype=torch.int32, device=dev)
        self.ep_length = torch.empty(E, dtype=torch.int32, device=dev)
        self.ep_ended = torch.empty(E, dtype=torch.uint8, device=dev)
        self.ep_offset = torch.zeros(1, dtype=torch.int64, device=dev) if E == 0 else \
            torch.empty(E + 1, dtype=torch.int64, device=dev)
        if E > 0:  # an empty tensor has no address to pass
            self.layout = abi.DDEpisodeLayout(self.lane_episode.data_ptr(), self.lane_row.data_ptr(),
                                              self.ep_lane.data_ptr(), self.ep_start.data_ptr(),
                                              self.ep_length.data_ptr(), self.ep_ended.data_ptr(),
                                              self.ep_offset.data_ptr())
            abi.check(lib.dd_episodes_fill(self.done.data_ptr(), _ptr(self.done_before), T, n, self.flags,
                                           ctypes.byref(self.layout), _args.stream_ptr(dev)), "dd_episodes_fill")

    def _gather(self, io):
        abi.check(self.lib.dd_episodes_gather(ctypes.byref(self.layout), self.done.data_ptr(),
                                              _ptr(self.done_before), ctypes.byref(io), self.T, self.n,
                                              _args.stream_ptr(self.dev)), "dd_episodes_gather")

    def _advantages(self, io):
        abi.check(self.lib.dd_episodes_advantages(ctypes.byref(self.layout), ctypes.byref(io), self.T, self.n,
                                                  _args.stream_ptr(self.dev)), "dd_episodes_advantages")

    def records(self):
        return (self.ep_lane, self.ep_start, self.ep_length, self.ep_offset, self.ep_ended.view(torch.bool))


def ppo_episodes_batch(obs: torch.Tensor, actions: Optional[torch.Tensor], log_prob: Optional[torch.Tensor],
                       reward: torch.Tensor, done: torch.Tensor, critic,
                       bootstrap_obs: Optional[torch.Tensor] = None, done_before: Optional[torch.Tensor] = None,
                       gamma: float = 0.99, lambda_: float = 0.95, normalize: bool = True) -> PpoEpisodesBatch:
    """The PPO notebook's "PHASE 2" over every episode of one rollout.

    Buffers as :func:`ppo_batch` (checked, never copied).  ``done_before [N]``
    bool or uint8: the lanes' done flags before the rollout (default: none
    done); a lane that was done spends frame 0 re-spawning, which is no row.
    ``critic`` runs on the ``M`` gathered rows and on ``bootstrap_obs [N, 15]``
    (``env.obs`` after the rollout; default: bootstrap 0), whose value follows
    the last frame of a lane's open episode; an ended episode bootstraps 0, as
    the training cell's ``dones[-1] = True``.  With no row at all (``M == 0``)
    every flat tensor is empty and the statistics are NaN, as ``M < 2`` gives.
    """
    plan = _EpisodePlan(done, done_before)
    if obs is None:
        raise ValueError("ppo_episodes_batch needs obs: the critic runs on the gathered states")
    states, acts, lps = plan.gather(obs, actions, log_prob)
    values = _values(critic, states, "states") if plan.M > 0 else states.new_empty(0)
    bootstrap = None
    if bootstrap_obs is not None:
        b = _rollout_buffer(bootstrap_obs, (plan.n, abi.DD_OBS_DIM), torch.float32, plan.dev, "bootstrap_obs")
        bootstrap = _values(critic, b, "bootstrap_obs") if plan.n > 0 else None
    raw, ret, ep = plan.advantages(reward, abi.DD_BATCH_GAE, gamma, lambda_, values=values, bootstrap=bootstrap)
    mean, std, adv = plan.normalize(raw, normalize)
    return PpoEpisodesBatch(states, acts, lps, adv, ret, values, *plan.records(), ep, plan.lane_episode,
                            plan.lane_row, mean, std)


def reinforce_episodes_batch(obs: Optional[torch.Tensor], actions: Optional[torch.Tensor], reward: torch.Tensor,
                             done: torch.Tensor, done_before: Optional[torch.Tensor] = None, gamma: float = 0.99,
                             normalize: bool = True, drop_open: bool = True) -> ReinforceEpisodesBatch:
    """The REINFORCE notebook's batch over every episode of one rollout:
    ``compute_returns`` per episode, then the baseline and the normalisation as
    :func:`reinforce_batch`.  ``drop_open`` (default) leaves the episodes that
    the end of the rollout cut out of the batch, rows and records: a
    discounted return that misses its later rewards is no return.  An episode
    that began before the rollout and ends in it stays."""
    plan = _EpisodePlan(done, done_before, drop_open=bool(drop_open))
    states, acts, _ = plan.gather(obs, actions, None)
    _, ret, ep = plan.advantages(reward, abi.DD_BATCH_RETURNS, gamma)
    mean, std, adv = plan.normalize(ret, normalize)
    return ReinforceEpisodesBatch(states, acts, ret, adv, mean, std, *plan.records(), ep, plan.lane_episode,
                                  plan.lane_row)


def collect_ppo_steps(env, actor, critic, frames: int, seed: int = 0, step: int = 0, gamma: float = 0.99,
                      lambda_: float = 0.95, normalize: bool = True) -> PpoEpisodesBatch:
    """``frames`` more frames of an ``auto_reset=True`` env as one PPO batch:
    the fixed-horizon collection (the notebook's ``rollout_steps``).  Does
    *not* reset the env: called in a loop with ``step`` advanced by ``frames``,
    each call continues the lanes' running episodes (their first rows) and
    bootstraps the ones it cuts from ``env.obs``.  The lanes that are done when
    the call starts re-spawn in frame 0; they are read from the env's status
    (``DD_ST_DONE``: what the kernels re-spawn by, and, unlike ``env.done``,
    kept current by ``policy_rollout``)."""
    if not env.config.auto_reset:
        raise ValueError("collect_ppo_steps batches every episode of a rollout that re-spawns its lanes: the env "
                         "needs auto_reset=True (collect_ppo plays one episode per lane on a sticky-done env)")
    done_before = (env.status & abi.DD_ST_DONE).ne(0).to(torch.uint8)
    obs, acts, lp, reward, done = env.policy_rollout(actor, int(frames), seed=seed, step=step)
    return ppo_episodes_batch(obs, acts, lp, reward, done, critic, bootstrap_obs=env.obs, done_before=done_before,
                              gamma=gamma, lambda_=lambda_, normalize=normalize)
