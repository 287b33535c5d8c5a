"""No GPU: the argument errors of ppo_train and ppo_train_population
(delivery_drone_amd/ppo_train.py), the per-member scalars that land in the
launch's table, and the metrics helper on hand-made tensors.

The wrappers' checks read a network's ``out_dim``, ``device``, ``compute`` and
``_lib``, an optimizer's ``net``, and an env's ``device``, ``precision``,
``ping_pong``, ``config.auto_reset`` and ``num_envs`` only, so the members and
envs here are objects made without their constructors (which need a GPU).
Every refusal comes before anything is allocated or launched: a stand-in has no
buffer a launch could use, so a check that came too late would fail on a missing
attribute instead of raising the ValueError.
"""
import sys

import pytest
import torch

import delivery_drone_amd
from delivery_drone_amd import (PPO_BATCH_LOG_KEYS, AdamW, EnvConfig, LearnerPopulation, MlpNet, PpoRun,
                                ReinforcePopulation, VecDroneEnv, abi, adamw, ppo_iteration_data, ppo_train,
                                ppo_train_population)

pt = sys.modules["delivery_drone_amd.ppo_train"]  # the module: the package's attribute of that name is the function

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


def member(compute="f32"):
    actor, critic = net(3, compute), net(1, compute)
    return (actor, critic, opt(actor), opt(critic))


def population(count):
    """A LearnerPopulation of stand-in members, without its device-side parts."""
    pop = object.__new__(LearnerPopulation)
    pop._members = tuple(member() for _ in range(count))
    pop.device, pop._lib = CPU, LIB
    return pop


def env(n, precision="f32", ping_pong=False, reward_mode="notebook", device=CPU, auto_reset=False):
    e = object.__new__(VecDroneEnv)
    e.num_envs, e.precision, e.ping_pong, e.reward_mode, e.device = n, precision, ping_pong, reward_mode, device
    e.config = EnvConfig(auto_reset=auto_reset)
    return e


def test_the_names_are_exported():
    for name in ("PpoRun", "ppo_train", "ppo_train_population", "ppo_iteration_data", "PPO_BATCH_LOG_KEYS"):
        assert name in delivery_drone_amd.__all__ and hasattr(delivery_drone_amd, name), name
    assert PPO_BATCH_LOG_KEYS == ("rows", "adv_mean", "adv_std") == abi.PT_BATCH_LOG_NAMES
    assert len(adamw.LOG_KEYS) == abi.DD_PPO_FUSED_LOGS


def test_env_and_population_refusals():
    pop = population(3)
    with pytest.raises(ValueError, match="pop must be a LearnerPopulation"):
        ppo_train_population(env(192), object.__new__(ReinforcePopulation), 5)
    with pytest.raises(ValueError, match="pop must be a LearnerPopulation"):
        ppo_train_population(env(192), [member()], 5)
    with pytest.raises(ValueError, match="env must be a VecDroneEnv"):
        ppo_train_population(object(), pop, 5)
    with pytest.raises(ValueError, match="precision='f32' envs only, this one is 'f64'"):
        ppo_train_population(env(192, precision="f64"), pop, 5)
    with pytest.raises(ValueError, match="one episode per lane here: the env needs auto_reset=False"):
        ppo_train_population(env(192, auto_reset=True), pop, 5)
    for n in (191, 193, 2, 0):
        with pytest.raises(ValueError, match=f"{n} lanes do not split into 3 equal groups"):
            ppo_train_population(env(n), pop, 5)
    with pytest.raises(ValueError, match="member 0: 129 lanes per member; .* at most 128"):
        ppo_train_population(env(3 * 129), pop, 5)
    for max_steps in (0, -2):
        with pytest.raises(ValueError, match=f"max_steps must be at least 1, got {max_steps}"):
            ppo_train_population(env(192), pop, max_steps)
    with pytest.raises(ValueError, match="records at most"):
        ppo_train_population(env(3 * 128), pop, abi.DD_REINFORCE_MAX_CELLS // 128 + 1)
    with pytest.raises(ValueError, match="num_epochs must be at least 1, got 0"):
        ppo_train_population(env(192), pop, 5, num_epochs=0)
    for size in (129, 0, -4):
        with pytest.raises(ValueError, match=r"minibatch_size must be None \(the full batch\) or in \[1, 128\]"):
            ppo_train_population(env(192), pop, 5, minibatch_size=size)


def test_f16x3_networks_are_refused():
    with pytest.raises(ValueError, match="member 1: .*compute='f32' networks only, the actor is compute='f16x3'"):
        LearnerPopulation([member(), member(compute="f16x3")])
    with pytest.raises(ValueError, match="^a population update runs compute='f32' networks only"):
        ppo_train(env(6), *member(compute="f16x3"), 5)  # the single call speaks of the learner, not of "member 0"


def test_per_member_scalars_are_checked():
    pop = population(3)
    for name in ("gamma", "lambda_", "clip_epsilon", "entropy_coef", "value_coef", "max_grad_norm", "shuffle_seed"):
        with pytest.raises(ValueError, match=f"{name}: 2 values for 3 members"):
            ppo_train_population(env(192), pop, 5, **{name: [1, 2]})
    for name in ("gamma", "lambda_", "clip_epsilon", "entropy_coef", "value_coef"):
        with pytest.raises(ValueError, match=f"member 2: {name} must be finite"):
            ppo_train_population(env(192), pop, 5, **{name: [0.5, 0.5, float("inf")]})
    with pytest.raises(ValueError, match="member 1: clip_epsilon must not be negative"):
        ppo_train_population(env(192), pop, 5, clip_epsilon=[0.2, -0.1, 0.2])
    with pytest.raises(ValueError, match="member 0: max_norm must not be NaN"):
        ppo_train_population(env(192), pop, 5, max_grad_norm=float("nan"))


def test_the_scalars_land_in_the_table(monkeypatch):
    monkeypatch.setattr(adamw, "_fused_net", lambda network, optimizer: abi.DDPpoFusedNet())
    pop = population(3)
    table = pt._member_table(pop, [0.99, 0.9, 0.95], 0.95, [0.2, 0.1, 0.3], 0.01, [0.5, 1.0, 0.25],
                             [0.5, None, float("inf")], [0, 7, -1])
    assert [m.gamma for m in table] == [0.99, 0.9, 0.95]
    assert [m.lambda_ for m in table] == [0.95] * 3
    assert [m.clip_epsilon for m in table] == [0.2, 0.1, 0.3]
    assert [m.entropy_coef for m in table] == [0.01] * 3
    assert [m.value_coef for m in table] == [0.5, 1.0, 0.25]
    assert [m.max_grad_norm for m in table] == [0.5, 0.0, float("inf")]  # None: no clipping
    assert [m.shuffle_seed for m in table] == [0, 7, 2 ** 64 - 1]


def hand_made_run(minibatch_size, drop_last=False):
    """Two members of two lanes; with minibatches of 4 rows member 0 (10 rows) takes 3 steps an epoch (2 with
    drop_last) and member 1 (3 rows) one (none with drop_last)."""
    steps = 1 if minibatch_size is None else 3
    logs = torch.full((11, 2, steps, 2), float("nan"), dtype=torch.float64)
    taken = [1, 1] if minibatch_size is None else ([2, 0] if drop_last else [3, 1])
    for g, s in enumerate(taken):
        logs[:, :, :s, g] = torch.arange(11 * 2 * s, dtype=torch.float64).view(11, 2, s) + 100 * g
    batch_logs = torch.tensor([[10.0, 3.0], [0.5, 0.25], [1.0, 2.0]], dtype=torch.float64)
    return PpoRun(logs, batch_logs, torch.tensor([7, 3, 1, 2], dtype=torch.int32),
                  torch.tensor([True, True, True, False]), torch.tensor([True, False, False, False]),
                  torch.tensor([10.0, -30.0, 1.0, 2.0], dtype=torch.float64), torch.zeros(4, 15), minibatch_size,
                  drop_last), taken


@pytest.mark.parametrize("minibatch_size, drop_last", [(None, False), (4, False), (4, True)])
def test_updates_and_iteration_data_on_hand_made_tensors(minibatch_size, drop_last):
    run, taken = hand_made_run(minibatch_size, drop_last)
    assert run.reward is None and run.values is None
    assert run.steps_taken() == taken
    assert torch.equal(run.batch_log("adv_std"), torch.tensor([1.0, 2.0], dtype=torch.float64))
    updates = run.updates()
    data = ppo_iteration_data(run)
    assert len(updates) == len(data) == 2
    for g, upd in enumerate(updates):
        want_shape = (2,) if minibatch_size is None else (2, taken[g])
        for i, key in enumerate(adamw.LOG_KEYS):
            assert tuple(upd.logs[key].shape) == want_shape
            assert torch.equal(upd.logs[key], run.logs[i, :, :taken[g], g].reshape(want_shape))
            if taken[g]:
                assert not torch.isnan(upd.logs[key]).any()
        if taken[g]:
            assert data[g]["policy_loss"] == upd.logs["policy_loss"].mean()
            assert data[g]["ratio_max"] == upd.logs["ratio_max"].max()
    assert data[0]["success_rate"].item() == 0.5 and data[1]["success_rate"].item() == 0.0
    assert data[0]["avg_reward"].item() == -10.0 and data[1]["avg_reward"].item() == 1.5
    assert data[0]["avg_steps"].item() == 5.0 and data[1]["avg_steps"].item() == 1.5
