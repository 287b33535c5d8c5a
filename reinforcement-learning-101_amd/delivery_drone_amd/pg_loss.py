"""The REINFORCE and one-step actor-critic learners, on device.

Policy_Gradients.ipynb's training cell from ``returns_tensor = ...`` to
``optimizer.step()`` is :func:`reinforce_update` on a :class:`ReinforceBatch`
(:func:`collect_reinforce` builds one); one pass of Actor_Critic_Basic.ipynb's
``while not all(games_done)`` body, its critic update and then its actor
update, is :func:`actor_critic_update`.  Both chain launches that exist
(:meth:`MlpNet.evaluate_actions`, the critic's forward, :meth:`MlpNet.backward`
with the notebooks' ``clip_grad_norm_``, :class:`AdamW`) around the two
elementwise stages of ``csrc/pg_loss.hip``: ``dd_pg_losses``, the
score-function loss ``-(log_prob * w).mean()`` both notebooks share (``w`` the
normalised advantage, or the detached TD error) with its gradient at the
actor's logits, and ``dd_td_losses``, the TD target, error, critic loss and its
gradient at the critic's value.

``active`` (bool or uint8 ``[M]``) masks rows out of every mean without
compacting them, which would need a count on the host: a masked row's gradient
rows are exactly 0, so it adds nothing to a parameter gradient, and the number
of active rows is counted on the device.  Every scalar is a 0-d float64 device
tensor summed in double over a reduction tree of fixed shape; nothing is read
back to the host, and both update functions capture as one linear graph.
Rows, masks and batches are checked by ``_args``, in :func:`ppo_losses`' words;
gradients go into the optimizers' own buffers (:meth:`AdamW.grad_buffer`).
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import torch

from . import _args, abi
from .adamw import AdamW
from .policy import MlpNet
from .train_batch import ReinforceBatch, reinforce_batch

__all__ = ["ReinforceLosses", "reinforce_losses", "ReinforceUpdate", "reinforce_update", "collect_reinforce",
           "TdLosses", "td_losses", "ActorCriticUpdate", "actor_critic_update"]


class ReinforceLosses(NamedTuple):
    loss: torch.Tensor                     # 0-d float64: -(log_probs * advantages).mean()
    log_probs: torch.Tensor                # [M] float32, the actor's log-probability of the actions taken
    probs: torch.Tensor                    # [M, 3] float32, the actor on states
    grad_logits: Optional[torch.Tensor]    # [M, 3] float32: d loss / d the actor's pre-Sigmoid outputs


class ReinforceUpdate(NamedTuple):
    """What the training cell prints, 0-d float64 device tensors."""
    loss: torch.Tensor
    grad_norm: torch.Tensor                # before clipping, clip_grad_norm_'s return
    baseline: torch.Tensor                 # the batch's: mean of the returns
    std: torch.Tensor                      # the batch's: unbiased std of the returns


class TdLosses(NamedTuple):
    critic_loss: torch.Tensor              # 0-d float64: mse + value_reg
    mse: torch.Tensor                      # 0-d float64: (td_errors ** 2).mean()
    value_reg: torch.Tensor                # 0-d float64: value_reg * (values ** 2).mean()
    count: torch.Tensor                    # 0-d float64: the active rows
    td_targets: torch.Tensor               # [M] float32: r + gamma V(s') (1 - done)
    td_errors: torch.Tensor                # [M] float32: td_targets - V(s)
    values: torch.Tensor                   # [M] float32, the critic on states
    next_values: torch.Tensor              # [M] float32, the critic on next_states
    grad_values: Optional[torch.Tensor]    # [M] float32: d critic_loss / d the critic's output


class ActorCriticUpdate(NamedTuple):
    actor_loss: torch.Tensor               # 0-d float64
    critic_loss: torch.Tensor              # 0-d float64
    td_errors: torch.Tensor                # [M] float32, from the critic before its step
    actor_grad_norm: torch.Tensor          # 0-d float64, before clipping
    critic_grad_norm: torch.Tensor


def _score_losses(actor, states, actions, weights, active, grads, what):
    """evaluate_actions, then dd_pg_losses: (result, log_prob, probs, grad_logits)."""
    if not isinstance(actor, MlpNet) or actor.out_dim != 3:
        raise ValueError(f"{what} needs an MlpNet actor (out_dim 3)")
    dev = actor.device
    m = _args.states_rows(states, what)
    w = _args.row_tensor(weights, m, dev, "advantages" if what == "reinforce_losses" else "td_errors")
    active = _args.active_mask(active, m, dev)
    lp, _, probs = actor.evaluate_actions(states, actions, probs=True)
    actions = actions.contiguous()
    lib = actor._lib
    result = torch.empty(abi.DD_PG_RESULTS, dtype=torch.float64, device=dev)
    g_logits = torch.empty(m, 3, dtype=torch.float32, device=dev) if grads else None
    workspace = torch.empty(int(lib.dd_pg_loss_workspace()) // 8, dtype=torch.int64, device=dev)
    io = abi.DDPgLossIO(lp.data_ptr(), probs.data_ptr(), actions.data_ptr(), _args.action_format(actions), 0,
                        w.data_ptr(), active.data_ptr() if active is not None else None, result.data_ptr(),
                        g_logits.data_ptr() if grads else None)
    abi.check(lib.dd_pg_losses(ctypes.byref(io), m, workspace.data_ptr(), _args.stream_ptr(dev)), "dd_pg_losses")
    return result, lp, probs, g_logits


def reinforce_losses(actor, states, actions=None, advantages=None, *, grads: bool = False) -> ReinforceLosses:
    """``loss = -(log_probs_tensor * advantages).mean()`` of the REINFORCE
    notebook's training cell, with an :class:`MlpNet` actor scoring the actions
    that were taken.

    ``states [M, 15]`` float32; ``actions`` uint8 ``[M]`` bitmasks or float32
    ``[M, 3]``; ``advantages [M]``: on the actor's GPU.  A
    :class:`ReinforceBatch` or :class:`ReinforceEpisodesBatch` may stand in
    place of the three tensors.  ``grads=True`` adds the gradient of ``loss``
    at the actor's pre-Sigmoid outputs, where :meth:`MlpNet.backward` starts.
    ``M == 0`` raises.  Runs on the current stream and reads nothing back."""
    states, actions, advantages, _ = _args.reinforce_columns(states, actions, advantages)
    result, lp, probs, g_logits = _score_losses(actor, states, actions, advantages, None, grads, "reinforce_losses")
    return ReinforceLosses(result[abi.DD_PG_LOSS], lp, probs, g_logits)


def reinforce_update(actor: MlpNet, batch, opt: AdamW, *, max_grad_norm: float = 0.5) -> ReinforceUpdate:
    """The REINFORCE notebook's training cell from ``returns_tensor = ...`` to
    ``optimizer.step()`` on a :class:`ReinforceBatch` or
    :class:`ReinforceEpisodesBatch` (which holds the returns, the baseline and
    the twice-normalised advantages): ``reinforce_losses(grads=True)``,
    ``actor.backward`` with the cell's ``clip_grad_norm_(..., max_grad_norm)``
    into the optimizer's gradient buffer, ``opt.step``.  ``baseline`` and
    ``std`` are the batch's.  Runs on the current stream and reads nothing back
    for either ``compute``; a refused ``f16x3`` step shows in ``opt.status()``."""
    if not isinstance(opt, AdamW) or opt.net is not actor:
        raise ValueError("opt must be the AdamW that optimizes actor")
    states, actions, advantages, batch = _args.reinforce_columns(batch)
    if batch is None:
        raise ValueError("reinforce_update takes a ReinforceBatch or a ReinforceEpisodesBatch")
    result, _, _, g_logits = _score_losses(actor, states, actions, advantages, None, True, "reinforce_losses")
    _, norm = actor.backward(states, g_logits, max_norm=max_grad_norm, out=opt.grad_buffer())
    opt.step(opt.grad_buffer())
    return ReinforceUpdate(result[abi.DD_PG_LOSS], norm, batch.baseline, batch.std)


def collect_reinforce(env, actor, max_steps: int = 300, seed: int = 0, step: int = 0, gamma: float = 0.99,
                      normalize: bool = True) -> ReinforceBatch:
    """One REINFORCE iteration's data: ``env.reset()``,
    ``env.policy_rollout(actor, max_steps, seed=seed, step=step)``
    (``collect_episodes``), then :func:`reinforce_batch` on each lane's first
    episode.  The twin of :func:`collect_ppo`."""
    env.reset()
    obs, acts, _, reward, done = env.policy_rollout(actor, int(max_steps), seed=seed, step=step)
    return reinforce_batch(obs, acts, reward, done, gamma=gamma, normalize=normalize)


def td_losses(critic, states, rewards, next_states, dones, *, gamma: float = 0.99, value_reg: float = 0.01,
              active=None, grads: bool = False) -> TdLosses:
    """The critic stage of the actor-critic notebook's update:
    ``values = critic(states)``, ``next_values = critic(next_states)`` (under
    ``no_grad``), ``td_targets = rewards + gamma * next_values * (1 - dones)``,
    ``td_errors = td_targets - values``, ``critic_loss = (td_errors **
    2).mean() + value_reg * (values ** 2).mean()``.

    ``states``, ``next_states`` ``[M, 15]`` float32; ``rewards``, ``dones``
    ``[M]`` (any real or bool dtype; ``dones`` nonzero = the episode ended):
    on the critic's GPU.  Both forwards run on the critic's weights as they are
    at the call.  ``active``: see the module docstring; a masked row's
    ``td_targets`` and ``td_errors`` are 0.  ``grads=True`` adds the gradient of
    ``critic_loss`` at the critic's output.  ``M == 0`` raises; with no active
    row the scalars are NaN.  Runs on the current stream and reads nothing back."""
    if not isinstance(critic, MlpNet) or critic.out_dim != 1:
        raise ValueError("td_losses needs an MlpNet critic (out_dim 1)")
    gamma, value_reg = _args.finite("gamma", gamma), _args.finite("value_reg", value_reg)
    dev = critic.device
    m = _args.states_rows(states, "td_losses")
    if not isinstance(next_states, torch.Tensor) or tuple(next_states.shape) != tuple(states.shape):
        raise ValueError(f"next_states must have states' shape {tuple(states.shape)}")
    r = _args.row_tensor(rewards, m, dev, "rewards")
    d = _args.row_tensor(dones, m, dev, "dones")
    active = _args.active_mask(active, m, dev)
    values, next_values = critic(states), critic(next_states)
    lib = critic._lib
    result = torch.empty(abi.DD_TD_RESULTS, dtype=torch.float64, device=dev)
    targets = torch.empty(m, dtype=torch.float32, device=dev)
    errors = torch.empty(m, dtype=torch.float32, device=dev)
    g_values = torch.empty(m, dtype=torch.float32, device=dev) if grads else None
    workspace = torch.empty(int(lib.dd_td_loss_workspace()) // 8, dtype=torch.int64, device=dev)
    io = abi.DDTdLossIO(values.data_ptr(), next_values.data_ptr(), r.data_ptr(), d.data_ptr(),
                        active.data_ptr() if active is not None else None, gamma, value_reg,
                        targets.data_ptr(), errors.data_ptr(), result.data_ptr(),
                        g_values.data_ptr() if grads else None)
    abi.check(lib.dd_td_losses(ctypes.byref(io), m, workspace.data_ptr(), _args.stream_ptr(dev)), "dd_td_losses")
    return TdLosses(result[abi.DD_TD_CRITIC_LOSS], result[abi.DD_TD_MSE], result[abi.DD_TD_VALUE_REG],
                    result[abi.DD_TD_COUNT], targets, errors, values, next_values, g_values)


def actor_critic_update(actor: MlpNet, critic: MlpNet, states, actions, rewards, next_states, dones,
                        actor_opt: AdamW, critic_opt: AdamW, *, gamma: float = 0.99, value_reg: float = 0.01,
                        max_grad_norm: float = 0.5, active=None) -> ActorCriticUpdate:
    """One pass of the actor-critic notebook's ``while not all(games_done)``
    body on one frame's transitions, in the notebook's order:

    1. :func:`td_losses` from the critic before its update;
    2. the critic's backward, ``clip_grad_norm_(..., max_grad_norm)`` and step;
    3. ``actor_loss = -(log_probs * td_errors.detach()).mean()`` with the
       actor as it is at the call (the notebook's ``log_probs`` were sampled
       with these weights, so scoring ``actions`` again gives their bits);
    4. the actor's backward, clip and step.

    ``actions`` as :meth:`MlpNet.act` returns them (uint8 bitmasks) or float32
    ``[M, 3]``; the other arguments as :func:`td_losses`.  ``active`` masks rows
    that must not train: the re-spawn frame after a done on an
    ``auto_reset=True`` env (``active = ~done_prev``), the finished lanes of a
    sticky one.  With no active row the losses are NaN and every gradient is
    0, and the two optimizer steps are still taken (zero-gradient steps: weight
    decay and the decaying moments move the parameters); ending the loop is the
    caller's job.  Runs on the current stream and reads nothing back."""
    if not isinstance(actor_opt, AdamW) or not isinstance(critic_opt, AdamW) or actor_opt.net is not actor \
            or critic_opt.net is not critic:
        raise ValueError("actor_opt must optimize actor and critic_opt critic")
    if critic.device != actor.device:
        raise ValueError(f"the actor is on {actor.device}, the critic on {critic.device}")
    td = td_losses(critic, states, rewards, next_states, dones, gamma=gamma, value_reg=value_reg, active=active,
                   grads=True)
    _, n_critic = critic.backward(states, td.grad_values, max_norm=max_grad_norm, out=critic_opt.grad_buffer())
    critic_opt.step(critic_opt.grad_buffer())
    result, _, _, g_logits = _score_losses(actor, states, actions, td.td_errors, active, True, "actor_critic_update")
    _, n_actor = actor.backward(states, g_logits, max_norm=max_grad_norm, out=actor_opt.grad_buffer())
    actor_opt.step(actor_opt.grad_buffer())
    return ActorCriticUpdate(result[abi.DD_PG_LOSS], td.critic_loss, td.td_errors, n_actor, n_critic)
