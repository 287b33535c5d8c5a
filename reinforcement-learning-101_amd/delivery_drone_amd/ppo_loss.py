"""The PPO notebook's losses and head gradients, on device.

``compute_ppo_losses`` (Actor_Critic_PPO.ipynb, the cell after
``collect_episodes_ppo``) on a training batch, as three launches:
:meth:`MlpNet.evaluate_actions` (the actor on ``states``, scoring the actions
that were taken), the critic's forward, and ``dd_ppo_losses``
(``csrc/ppo_loss.hip``): the clipped surrogate, the value loss, the entropy
bonus, the ratio statistics the training cell logs every epoch, and, with
``grads=True``, the gradient of ``total_loss`` at the two networks' outputs
(the actor's pre-Sigmoid logits and the critic's value), which is where a
backward pass through the networks starts.  Every scalar is a 0-d float64
device tensor summed in double over a reduction tree of fixed shape: the same
bits on every run and every device, and nothing is read back to the host.
"""
from __future__ import annotations

import ctypes
from typing import Dict, NamedTuple, Optional

import torch

from . import _args, abi

__all__ = ["PpoLosses", "ppo_losses"]


class PpoLosses(NamedTuple):
    total_loss: torch.Tensor               # 0-d float64: policy_loss + value_coef value_loss - entropy_coef entropy
    policy_loss: torch.Tensor              # 0-d float64: -mean(min(r A, clip(r) A))
    value_loss: torch.Tensor               # 0-d float64: mean((v - R)^2)
    entropy: torch.Tensor                  # 0-d float64: dist.entropy().mean()
    ratio_stats: Dict[str, torch.Tensor]   # 0-d float64: mean, min, max, std (unbiased), clipped_frac
    new_log_probs: torch.Tensor            # [M] float32
    ratio: torch.Tensor                    # [M] float32: exp(new_log_probs - old_log_probs)
    values: torch.Tensor                   # [M] float32, the critic on states
    grad_logits: Optional[torch.Tensor]    # [M, 3] float32: d total_loss / d the actor's pre-Sigmoid outputs
    grad_values: Optional[torch.Tensor]    # [M] float32: d total_loss / d the critic's output
    probs: torch.Tensor                    # [M, 3] float32, the actor on states
    row_entropy: torch.Tensor              # [M] float32: each row's three factor entropies, summed


def ppo_losses(actor, critic, states, actions=None, old_log_probs=None, advantages=None, returns=None,
               clip_epsilon: float = 0.2, entropy_coef: float = 0.01, value_coef: float = 0.5, *,
               grads: bool = False) -> PpoLosses:
    """``compute_ppo_losses(policy, critic, states, actions, old_log_probs,
    advantages, returns, clip_epsilon, entropy_coef, value_coef)`` with
    :class:`MlpNet` networks.

    ``states [M, 15]`` float32; ``actions`` uint8 ``[M]`` bitmasks or float32
    ``[M, 3]``; ``old_log_probs``, ``advantages``, ``returns`` ``[M]``: on the
    actor's GPU.  A :class:`PpoBatch` or :class:`PpoEpisodesBatch` may stand
    in place of the five tensors (``ppo_losses(actor, critic, batch)``).
    ``M == 0`` raises: a mean over no rows has no value.  Runs on the current
    stream and reads nothing back.
    """
    states, actions, old_log_probs, advantages, returns = _args.ppo_columns(states, actions, old_log_probs,
                                                                            advantages, returns)
    _args.check_actor_critic(actor, critic)
    clip_epsilon, entropy_coef, value_coef = _args.ppo_coefficients(clip_epsilon, entropy_coef, value_coef)
    dev = actor.device
    m = _args.states_rows(states, "ppo_losses")
    old = _args.row_tensor(old_log_probs, m, dev, "old_log_probs")
    adv = _args.row_tensor(advantages, m, dev, "advantages")
    ret = _args.row_tensor(returns, m, dev, "returns")
    lp, ent, probs = actor.evaluate_actions(states, actions, probs=True)
    values = critic(states)
    actions = actions.contiguous()
    lib = actor._lib
    result = torch.empty(abi.DD_PPO_RESULTS, dtype=torch.float64, device=dev)
    ratio = torch.empty(m, dtype=torch.float32, device=dev)
    g_logits = torch.empty(m, 3, dtype=torch.float32, device=dev) if grads else None
    g_values = torch.empty(m, dtype=torch.float32, device=dev) if grads else None
    workspace = torch.empty(int(lib.dd_ppo_loss_workspace()) // 8, dtype=torch.int64, device=dev)
    io = abi.DDPpoLossIO(lp.data_ptr(), ent.data_ptr(), probs.data_ptr(), values.data_ptr(), old.data_ptr(),
                         adv.data_ptr(), ret.data_ptr(), actions.data_ptr(), _args.action_format(actions), 0,
                         clip_epsilon, entropy_coef, value_coef, result.data_ptr(), ratio.data_ptr(),
                         g_logits.data_ptr() if grads else None, g_values.data_ptr() if grads else None)
    abi.check(lib.dd_ppo_losses(ctypes.byref(io), m, workspace.data_ptr(), _args.stream_ptr(dev)), "dd_ppo_losses")
    stats = {"mean": result[abi.DD_PPO_RATIO_MEAN], "min": result[abi.DD_PPO_RATIO_MIN],
             "max": result[abi.DD_PPO_RATIO_MAX], "std": result[abi.DD_PPO_RATIO_STD],
             "clipped_frac": result[abi.DD_PPO_CLIPPED_FRAC]}
    return PpoLosses(result[abi.DD_PPO_TOTAL_LOSS], result[abi.DD_PPO_POLICY_LOSS], result[abi.DD_PPO_VALUE_LOSS],
                     result[abi.DD_PPO_ENTROPY], stats, lp, ratio, values, g_logits, g_values, probs, ent)
