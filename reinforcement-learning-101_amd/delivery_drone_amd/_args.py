"""The learner wrappers' argument layer: the one copy of every check and
unpacking step that more than one module needs, so that two entry points
cannot disagree on what they refuse or in which words.  Every refusal is a
``ValueError`` on the host, before any launch; no tensor's values are read.
Imported as a module (``from . import _args``), so the import order is free.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import abi, train_batch


def stream_ptr(device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def some_rows(m: int, what: str) -> int:
    if m == 0:
        raise ValueError(f"{what} needs at least one row: a mean over no rows has no value")
    return m


def states_rows(states, what: str) -> int:
    """``M`` of a loss function's ``states [M, 15]``; ``M == 0`` raises."""
    if not isinstance(states, torch.Tensor) or states.dim() != 2:
        raise ValueError(f"states must be [M, {abi.DD_OBS_DIM}]")
    return some_rows(int(states.shape[0]), what)


def row_tensor(t, m, dev, what):
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != (m,):
        raise ValueError(f"{what} must be a tensor of shape ({m},), got "
                         f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    if t.device != dev:
        raise ValueError(f"{what} is on {t.device}, states on {dev}")
    return t.detach().to(torch.float32).contiguous()


def active_mask(active, m, dev):
    if active is None:
        return None
    if (not isinstance(active, torch.Tensor) or tuple(active.shape) != (m,)
            or active.dtype not in (torch.bool, torch.uint8)):
        raise ValueError(f"active must be a bool or uint8 tensor of shape ({m},)")
    if active.device != dev:
        raise ValueError(f"active is on {active.device}, states on {dev}")
    active = active.contiguous()
    return active.view(torch.uint8) if active.dtype == torch.bool else active


def column(name, t, m, dev):
    """A PPO batch's column (a ``ShuffledBatch`` field name) as the kernels read it, or None."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a tensor or None, got {type(t).__name__}")
    if t.device != dev:
        raise ValueError(f"{name} is on {t.device}, the batch on {dev}")
    shape = tuple(t.shape)
    if name == "actions":
        if (t.dtype, shape) in ((torch.uint8, (m,)), (torch.float32, (m, 3))):
            return t.detach().contiguous()
        raise ValueError(f"actions must be uint8 [{m}] bitmasks or float32 [{m}, 3], got {t.dtype} {shape}")
    want = (m, abi.DD_OBS_DIM) if name == "states" else (m,)
    if shape != want:
        raise ValueError(f"{name} must have shape {want}, got {shape}")
    return t.detach().to(torch.float32).contiguous()


def action_format(actions) -> int:
    """The ``DD_ACT_*`` of an action tensor that was checked already."""
    return abi.DD_ACT_BITMASK if actions.dtype == torch.uint8 else abi.DD_ACT_F32X3


def finite(name, x) -> float:
    if not math.isfinite(float(x)):
        raise ValueError(f"{name} must be finite, got {x!r}")
    return float(x)


def ppo_coefficients(clip_epsilon, entropy_coef, value_coef):
    coefficients = (finite("clip_epsilon", clip_epsilon), finite("entropy_coef", entropy_coef),
                    finite("value_coef", value_coef))
    if coefficients[0] < 0.0:
        raise ValueError(f"clip_epsilon must not be negative, got {clip_epsilon!r}")
    return coefficients


def clip_norm(max_norm) -> float:
    """``MlpNet.backward``'s ``max_norm`` as the kernels take it: 0 for None (no clipping)."""
    if max_norm is None:
        return 0.0
    if math.isnan(float(max_norm)):
        raise ValueError("max_norm must not be NaN")
    return float(max_norm)


def per_member(name: str, value, members: int) -> list:
    """A scalar for every member, or one value per member."""
    if isinstance(value, (tuple, list)):
        if len(value) != members:
            raise ValueError(f"{name}: {len(value)} values for {members} members")
        return list(value)
    return [value] * members


def member_scalars(members: int, *triples) -> list:
    """A population call's per-member scalars: ``(name, value, check)`` triples
    in, ``value`` a scalar or one per member; out, for every member the tuple of
    its ``check(value)`` in the triples' order.  A refusal names the member."""
    per = [per_member(name, value, members) for name, value, _ in triples]
    scalars = []
    for p in range(members):
        try:
            scalars.append(tuple(check(values[p]) for (_, _, check), values in zip(triples, per)))
        except ValueError as exc:
            raise ValueError(f"member {p}: {exc}") from None
    return scalars


def fused_env_lanes(env, pop, own_check) -> int:
    """What a fused training launch needs of ``env``: the lanes per member of
    ``pop``.  ``own_check(env)`` is the caller's own refusal, made between the
    checks of the env itself and those of its lanes."""
    from .vec_env import VecDroneEnv  # vec_env imports this module
    if not isinstance(env, VecDroneEnv):
        raise ValueError("env must be a VecDroneEnv")
    if env.device != pop.device:
        raise ValueError(f"the env is on {env.device}, the learners on {pop.device}")
    if env.precision != "f32":
        raise ValueError(f"the fused training loop steps precision='f32' envs only, this one is {env.precision!r}")
    if env.ping_pong:
        raise ValueError("the fused training loop steps an env in place: ping_pong=True is not supported")
    own_check(env)
    members, n = len(pop), env.num_envs
    lanes = n // members
    if lanes * members != n or lanes < 1:
        raise ValueError(f"{n} lanes do not split into {members} equal groups, one per member")
    if lanes > abi.DD_PPO_FUSED_ROWS:
        raise ValueError(f"member 0: {lanes} lanes per member; the fused training loop takes at most "
                         f"{abi.DD_PPO_FUSED_ROWS} (one row tile of the backward)")
    return lanes


def check_out(t, shape, dtype, dev, what) -> None:
    """A caller's output buffer.  ``what`` opens the message as the call site
    words it ("out must be a contiguous float32 tensor")."""
    if (not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype != dtype
            or not t.is_contiguous() or t.device != dev):
        raise ValueError(f"{what} of shape {tuple(shape)} on {dev}")


def batch_five(batch):
    """The five tensors of a PpoBatch or PpoEpisodesBatch (any may be None); None for anything else."""
    if isinstance(batch, (train_batch.PpoBatch, train_batch.PpoEpisodesBatch)):
        return tuple(batch[:5])
    return None


def ppo_columns(states, actions=None, old_log_probs=None, advantages=None, returns=None):
    """The five tensors from a PPO batch in ``states``' place, or as given."""
    five = batch_five(states)
    if five is None:
        return states, actions, old_log_probs, advantages, returns
    if any(t is not None for t in (actions, old_log_probs, advantages, returns)):
        raise ValueError("pass a batch or the five tensors, not both")
    if any(t is None for t in five[:3]):
        raise ValueError("the batch was built without obs, actions or log_prob")
    return five


def reinforce_columns(states, actions=None, advantages=None):
    """``(states, actions, advantages, batch)`` from a REINFORCE batch in ``states``' place, or as given and None."""
    if not isinstance(states, (train_batch.ReinforceBatch, train_batch.ReinforceEpisodesBatch)):
        return states, actions, advantages, None
    if actions is not None or advantages is not None:
        raise ValueError("pass a batch or the three tensors, not both")
    if states.states is None or states.actions is None:
        raise ValueError("the batch was built without obs or actions")
    return states.states, states.actions, states.advantages, states


def check_actor_critic(actor, critic) -> None:
    if getattr(actor, "out_dim", None) != 3 or getattr(critic, "out_dim", None) != 1:
        raise ValueError("ppo_losses needs an MlpNet actor (out_dim 3) and an MlpNet critic (out_dim 1)")
    if critic.device != actor.device:
        raise ValueError(f"the actor is on {actor.device}, the critic on {critic.device}")
