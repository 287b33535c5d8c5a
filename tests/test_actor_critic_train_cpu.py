"""No GPU: the argument errors of actor_critic_train and
actor_critic_train_population (delivery_drone_amd/actor_critic.py) and the
per-member broadcasting of their scalars.

The wrappers' checks read a network's ``out_dim``, ``device``, ``compute`` and
``_lib``, an optimizer's ``net``, and an env's ``device``, ``precision``,
``ping_pong``, ``reward_mode`` and ``num_envs`` only, so the members and envs
here are objects made without their constructors (which need a GPU).  Every
refusal comes before anything is allocated or launched: a stand-in has no buffer
a launch could use, so a check that came too late would fail on a missing
attribute instead of raising the ValueError.
"""
import pytest
import torch

import delivery_drone_amd
from delivery_drone_amd import (AC_LOG_KEYS, ActorCriticRun, AdamW, LearnerPopulation, MlpNet, VecDroneEnv, abi,
                                actor_critic_train, actor_critic_train_population)
from delivery_drone_amd import actor_critic as ac

CPU = torch.device("cpu")
LIB = object()


def net(out_dim, compute="f32", device=CPU, lib=LIB):
    n = object.__new__(MlpNet)
    n.out_dim, n.compute, n.device, n._lib = out_dim, compute, device, lib
    return n


def opt(network):
    o = object.__new__(AdamW)
    o.net = network
    return o


def member(compute=("f32", "f32"), **kw):
    actor, critic = net(3, compute[0], **kw), net(1, compute[1], **kw)
    return (actor, critic, opt(actor), opt(critic))


def population(count):
    """A LearnerPopulation of stand-in members, without its device-side parts."""
    pop = object.__new__(LearnerPopulation)
    pop._members = tuple(member() for _ in range(count))
    pop.device, pop._lib = CPU, LIB
    return pop


def env(n, precision="f32", ping_pong=False, reward_mode="engine", device=CPU):
    e = object.__new__(VecDroneEnv)
    e.num_envs, e.precision, e.ping_pong, e.reward_mode, e.device = n, precision, ping_pong, reward_mode, device
    return e


def test_the_names_are_exported():
    for name in ("ActorCriticRun", "actor_critic_train", "actor_critic_train_population", "AC_LOG_KEYS"):
        assert name in delivery_drone_amd.__all__ and hasattr(delivery_drone_amd, name), name
    assert AC_LOG_KEYS == ("actor_loss", "critic_loss", "mse", "value_reg", "count", "actor_grad_norm",
                           "critic_grad_norm") == abi.AC_LOG_NAMES
    run = ActorCriticRun(torch.arange(7 * 2 * 3, dtype=torch.float64).view(7, 2, 3), None, None)
    assert run.reward is None and run.done is None
    assert torch.equal(run.log("count"), run.logs[4]) and tuple(run.log("mse").shape) == (2, 3)


def test_env_refusals():
    pop = population(3)
    with pytest.raises(ValueError, match="pop must be a LearnerPopulation"):
        actor_critic_train_population(env(192), [member()], 5)
    with pytest.raises(ValueError, match="env must be a VecDroneEnv"):
        actor_critic_train_population(object(), pop, 5)
    with pytest.raises(ValueError, match="the env is on meta, the learners on cpu"):
        actor_critic_train_population(env(192, device=torch.device("meta")), pop, 5)
    with pytest.raises(ValueError, match="precision='f32' envs only, this one is 'f64'"):
        actor_critic_train_population(env(192, precision="f64"), pop, 5)
    with pytest.raises(ValueError, match="ping_pong=True is not supported"):
        actor_critic_train_population(env(192, ping_pong=True), pop, 5)
    with pytest.raises(ValueError, match="reward_mode must be 'engine' or 'notebook', this env has 'reinforce'"):
        actor_critic_train_population(env(192, reward_mode="reinforce"), pop, 5)
    for n in (191, 193, 2, 0):
        with pytest.raises(ValueError, match=f"{n} lanes do not split into 3 equal groups"):
            actor_critic_train_population(env(n), pop, 5)
    with pytest.raises(ValueError, match="member 0: 129 lanes per member; .* at most 128"):
        actor_critic_train_population(env(3 * 129), pop, 5)
    for frames in (0, -2):
        with pytest.raises(ValueError, match=f"frames must be at least 1, got {frames}"):
            actor_critic_train_population(env(192), pop, frames)


def test_scalar_refusals_name_the_member():
    pop, e = population(3), env(3 * 128, reward_mode="notebook")
    for name in ("gamma", "value_reg", "max_grad_norm"):
        with pytest.raises(ValueError, match=f"{name}: 2 values for 3 members"):
            actor_critic_train_population(e, pop, 5, **{name: [0.1, 0.2]})
    with pytest.raises(ValueError, match="member 1: gamma must be finite, got nan"):
        actor_critic_train_population(e, pop, 5, gamma=[0.99, float("nan"), 0.9])
    with pytest.raises(ValueError, match="member 2: value_reg must be finite, got inf"):
        actor_critic_train_population(e, pop, 5, value_reg=[0.0, 0.01, float("inf")])
    with pytest.raises(ValueError, match="member 0: max_norm must not be NaN"):
        actor_critic_train_population(e, pop, 5, max_grad_norm=float("nan"))
    with pytest.raises(ValueError, match=r"active must be a bool or uint8 tensor of shape \(384,\)"):
        actor_critic_train_population(e, pop, 5, active0=torch.ones(383, dtype=torch.bool))
    with pytest.raises(ValueError, match="active must be a bool or uint8 tensor"):
        actor_critic_train_population(e, pop, 5, active0=torch.ones(384))
    with pytest.raises(ValueError, match="active is on meta"):
        actor_critic_train_population(e, pop, 5, active0=torch.ones(384, dtype=torch.bool, device="meta"))


def test_the_single_call_is_a_population_of_one():
    good = member()
    with pytest.raises(ValueError, match="^actor_opt must optimize actor and critic_opt critic"):
        actor_critic_train(env(64), good[0], good[1], good[3], good[2], 5)
    with pytest.raises(ValueError, match="^actor_opt and critic_opt must be AdamW"):
        actor_critic_train(env(64), good[0], good[1], None, good[3], 5)
    with pytest.raises(ValueError, match=r"^ppo_losses needs an MlpNet actor \(out_dim 3\)"):
        actor_critic_train(env(64), good[1], good[0], good[3], good[2], 5)
    for compute, name in ((("f16x3", "f32"), "actor"), (("f32", "f16x3"), "critic")):
        with pytest.raises(ValueError, match=f"compute='f32' networks only, the {name} is compute='f16x3'"):
            actor_critic_train(env(64), *member(compute), 5)


def test_per_member_scalars_reach_the_table(monkeypatch):
    """A scalar goes to every member, a list to its own: the descriptors the launch would be handed, recorded
    as they are built (the stand-in env has no buffers, so the call ends there)."""
    seen = []

    class Recorded(abi.DDActorCriticMember):
        def __init__(self, actor, critic, gamma, value_reg, max_grad_norm):
            super().__init__(actor, critic, gamma, value_reg, max_grad_norm)
            seen.append((gamma, value_reg, max_grad_norm))

    monkeypatch.setattr(ac.adamw, "_fused_net", lambda network, optimizer: abi.DDPpoFusedNet())
    monkeypatch.setattr(ac.abi, "DDActorCriticMember", Recorded)
    pop, e = population(3), env(3 * 64)
    with pytest.raises(AttributeError, match="_obs_current"):  # every check passed; the env's buffers come next
        actor_critic_train_population(e, pop, 5, gamma=[0.99, 0.9, 0.95], value_reg=0.0, max_grad_norm=[0.5, None, 2],
                                      active0=torch.ones(192, dtype=torch.uint8))
    assert seen == [(0.99, 0.0, 0.5), (0.9, 0.0, 0.0), (0.95, 0.0, 2.0)]  # None: no clipping, the kernels' 0
    del seen[:]
    with pytest.raises(AttributeError, match="_obs_current"):
        actor_critic_train_population(e, pop, 5)
    assert seen == [(0.99, 0.01, 0.5)] * 3
