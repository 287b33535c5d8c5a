"""No GPU: the argument errors of reinforce_train, reinforce_train_population and
ReinforcePopulation (delivery_drone_amd/reinforce.py, population.py) and the
per-member broadcasting of their scalars.

The wrappers' checks read a network's ``out_dim``, ``device``, ``compute`` and
``_lib``, an optimizer's ``net``, and an env's ``device``, ``precision``,
``ping_pong``, ``config.auto_reset`` and ``num_envs`` only, so the members and
envs here are objects made without their constructors (which need a GPU).
Every refusal comes before anything is allocated or launched: a stand-in has no
buffer a launch could use, so a check that came too late would fail on a missing
attribute instead of raising the ValueError.
"""
import pytest
import torch

import delivery_drone_amd
from delivery_drone_amd import (REINFORCE_LOG_KEYS, AdamW, EnvConfig, MlpNet, ReinforcePopulation, ReinforceRun,
                                VecDroneEnv, abi, reinforce_train, reinforce_train_population)
from delivery_drone_amd import reinforce as rf

CPU = torch.device("cpu")
LIB = object()


def net(out_dim=3, compute="f32", device=CPU, lib=LIB):
    n = object.__new__(MlpNet)
    n.out_dim, n.compute, n.device, n._lib = out_dim, compute, device, lib
    return n


def opt(network):
    o = object.__new__(AdamW)
    o.net = network
    return o


def member(**kw):
    actor = net(**kw)
    return (actor, opt(actor))


def population(count):
    """A ReinforcePopulation of stand-in members, without its device-side parts."""
    pop = object.__new__(ReinforcePopulation)
    pop._members = tuple(member() for _ in range(count))
    pop.device, pop._lib = CPU, LIB
    return pop


def env(n, precision="f32", ping_pong=False, reward_mode="reinforce", device=CPU, auto_reset=False):
    e = object.__new__(VecDroneEnv)
    e.num_envs, e.precision, e.ping_pong, e.reward_mode, e.device = n, precision, ping_pong, reward_mode, device
    e.config = EnvConfig(auto_reset=auto_reset)
    return e


def test_the_names_are_exported():
    for name in ("ReinforcePopulation", "ReinforceRun", "reinforce_train", "reinforce_train_population",
                 "REINFORCE_LOG_KEYS"):
        assert name in delivery_drone_amd.__all__ and hasattr(delivery_drone_amd, name), name
    assert REINFORCE_LOG_KEYS == ("loss", "grad_norm", "baseline", "std", "rows") == abi.RF_LOG_NAMES
    run = ReinforceRun(torch.arange(5 * 3, dtype=torch.float64).view(5, 3), None, None, None, None)
    assert run.reward is None and run.done is None and run.returns is None and run.advantages is None
    assert torch.equal(run.log("std"), run.logs[3]) and tuple(run.log("rows").shape) == (3,)


def test_population_refusals_name_the_member(monkeypatch):
    good = member()
    with pytest.raises(ValueError, match="needs at least one member"):
        ReinforcePopulation([])
    with pytest.raises(ValueError, match=r"member 1: expected \(actor, opt\)"):
        ReinforcePopulation([good, (good[0],)])
    with pytest.raises(ValueError, match="member 1: the actor must be an MlpNet with out_dim 3"):
        ReinforcePopulation([good, member(out_dim=1)])
    with pytest.raises(ValueError, match="member 0: opt must be an AdamW optimizer"):
        ReinforcePopulation([(good[0], None)])
    with pytest.raises(ValueError, match="member 2: opt must be the AdamW that optimizes actor"):
        ReinforcePopulation([good, member(), (net(), good[1])])
    with pytest.raises(ValueError, match="member 1: .*compute='f32' networks only, the actor is compute='f16x3'"):
        ReinforcePopulation([good, member(compute="f16x3")])
    with pytest.raises(ValueError, match="member 1: its actor is in the population already"):
        ReinforcePopulation([good, good])
    with pytest.raises(ValueError, match="member 1: on meta, member 0 on cpu"):
        ReinforcePopulation([good, member(device=torch.device("meta"))])
    with pytest.raises(ValueError, match="member 1: uses another build of the library than member 0"):
        ReinforcePopulation([good, member(lib=object())])


def test_env_refusals():
    pop = population(3)
    with pytest.raises(ValueError, match="pop must be a ReinforcePopulation"):
        reinforce_train_population(env(192), [member()], 5)
    with pytest.raises(ValueError, match="env must be a VecDroneEnv"):
        reinforce_train_population(object(), pop, 5)
    with pytest.raises(ValueError, match="the env is on meta, the learners on cpu"):
        reinforce_train_population(env(192, device=torch.device("meta")), pop, 5)
    with pytest.raises(ValueError, match="precision='f32' envs only, this one is 'f64'"):
        reinforce_train_population(env(192, precision="f64"), pop, 5)
    with pytest.raises(ValueError, match="ping_pong=True is not supported"):
        reinforce_train_population(env(192, ping_pong=True), pop, 5)
    with pytest.raises(ValueError, match="one episode per lane: the env needs auto_reset=False"):
        reinforce_train_population(env(192, auto_reset=True), pop, 5)
    for n in (191, 193, 2, 0):
        with pytest.raises(ValueError, match=f"{n} lanes do not split into 3 equal groups"):
            reinforce_train_population(env(n), pop, 5)
    with pytest.raises(ValueError, match="member 0: 129 lanes per member; .* at most 128"):
        reinforce_train_population(env(3 * 129), pop, 5)
    for max_steps in (0, -2):
        with pytest.raises(ValueError, match=f"max_steps must be at least 1, got {max_steps}"):
            reinforce_train_population(env(192), pop, max_steps)
    with pytest.raises(ValueError, match="records at most 16777216 lane-frames"):
        reinforce_train_population(env(3 * 128), pop, (1 << 17) + 1)


def test_scalar_refusals_name_the_member():
    pop, e = population(3), env(3 * 128)
    for name in ("gamma", "max_grad_norm"):
        with pytest.raises(ValueError, match=f"{name}: 2 values for 3 members"):
            reinforce_train_population(e, pop, 5, **{name: [0.1, 0.2]})
    with pytest.raises(ValueError, match="member 1: gamma must be finite, got nan"):
        reinforce_train_population(e, pop, 5, gamma=[0.99, float("nan"), 0.9])
    with pytest.raises(ValueError, match="member 2: gamma must be finite, got inf"):
        reinforce_train_population(e, pop, 5, gamma=[0.99, 0.9, float("inf")])
    with pytest.raises(ValueError, match="member 0: max_norm must not be NaN"):
        reinforce_train_population(e, pop, 5, max_grad_norm=float("nan"))


def test_the_single_call_is_a_population_of_one():
    good = member()
    with pytest.raises(ValueError, match="^opt must be the AdamW that optimizes actor"):
        reinforce_train(env(64), net(), good[1], 5)
    with pytest.raises(ValueError, match="^opt must be an AdamW optimizer"):
        reinforce_train(env(64), good[0], None, 5)
    with pytest.raises(ValueError, match="^the actor must be an MlpNet with out_dim 3"):
        reinforce_train(env(64), *member(out_dim=1), 5)
    with pytest.raises(ValueError, match="compute='f32' networks only, the actor is compute='f16x3'"):
        reinforce_train(env(64), *member(compute="f16x3"), 5)


def test_per_member_scalars_reach_the_table(monkeypatch):
    """A scalar goes to every member, a list to its own: the descriptors the launch would be handed, recorded
    as they are built (the stand-in env has no buffers, so the call ends at its reset)."""
    seen = []

    class Recorded(abi.DDReinforceMember):
        def __init__(self, actor, gamma, max_grad_norm):
            super().__init__(actor, gamma, max_grad_norm)
            seen.append((gamma, max_grad_norm))

    monkeypatch.setattr(rf.adamw, "_fused_net", lambda network, optimizer: abi.DDPpoFusedNet())
    monkeypatch.setattr(rf.abi, "DDReinforceMember", Recorded)
    pop, e = population(3), env(3 * 6)
    with pytest.raises(AttributeError):  # every check passed; the env's reset comes next
        reinforce_train_population(e, pop, 300, gamma=[0.99, 0.9, 0.95], max_grad_norm=[0.5, None, 2])
    assert seen == [(0.99, 0.5), (0.9, 0.0), (0.95, 2.0)]  # None: no clipping, the kernels' 0
    del seen[:]
    with pytest.raises(AttributeError):
        reinforce_train_population(e, pop, 300)
    assert seen == [(0.99, 0.5)] * 3
