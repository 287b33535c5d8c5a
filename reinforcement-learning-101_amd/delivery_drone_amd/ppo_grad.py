"""PHASE 3 of the PPO notebook's training cell up to the optimizer step, on device.

``ppo_grads`` is one :func:`ppo_losses` with ``grads=True`` (the losses and
the gradient of ``total_loss`` at the two networks' outputs) and one
:meth:`MlpNet.backward` per network (``csrc/mlp_backward.hip``): the
``.grad`` of every parameter of ``DroneGamerBoi`` and ``DroneTeacherBoi`` that
the notebook's ``total_loss.backward()`` leaves, after its
``clip_grad_norm_(network.parameters(), max_grad_norm)`` per network.  Nothing
is read back to the host; what remains for torch is the AdamW step.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional

import torch

from .ppo_loss import PpoLosses, ppo_losses

__all__ = ["PpoGrads", "ppo_grads"]


class PpoGrads(NamedTuple):
    losses: PpoLosses                      # ppo_losses(..., grads=True)
    actor: Dict[str, torch.Tensor]         # STATE_DICT_KEYS -> float32 gradient, views into one flat buffer
    critic: Dict[str, torch.Tensor]
    actor_grad_norm: torch.Tensor          # 0-d float64: the L2 norm before clipping, clip_grad_norm_'s return
    critic_grad_norm: torch.Tensor


def ppo_grads(actor, critic, states, actions=None, old_log_probs=None, advantages=None, returns=None,
              clip_epsilon: float = 0.2, entropy_coef: float = 0.01, value_coef: float = 0.5, *,
              max_grad_norm: Optional[float] = None) -> PpoGrads:
    """``compute_ppo_losses(...)["total_loss"].backward()`` and the two
    ``clip_grad_norm_`` calls of the training cell, with :class:`MlpNet`
    networks.  Arguments as :func:`ppo_losses` (a batch may stand in place of
    the five tensors); ``max_grad_norm`` as :meth:`MlpNet.backward`'s
    ``max_norm`` (``None``: no clipping).  Runs on the current stream."""
    losses = ppo_losses(actor, critic, states, actions, old_log_probs, advantages, returns, clip_epsilon,
                        entropy_coef, value_coef, grads=True)
    rows = states.states if not isinstance(states, torch.Tensor) else states
    g_actor, n_actor = actor.backward(rows, losses.grad_logits, max_norm=max_grad_norm)
    g_critic, n_critic = critic.backward(rows, losses.grad_values, max_norm=max_grad_norm)
    return PpoGrads(losses, g_actor, g_critic, n_actor, n_critic)
