"""GPU: a population of actors in one fused launch
(dd_policy_rollout_population, ActorPopulation) against the single-actor path
(dd_policy_rollout / dd_policy_rollout_sampled), which the other suites pin to
the oracle and to the two-kernel host loop.

Bounds: none for the rollouts.  The contract is equality, bit for bit
(torch.equal), with P single-actor calls on P envs of L lanes whose
env_id_base is the big env's plus g L: every returned buffer column-wise, the
final observation, and every field of state_dict().  population_summary is
compared with float64 means taken on the host (numpy: sum / L): exactly for
the two integer columns (their sums are exact in float64 and both sides divide
once, correctly rounded), and for the two float columns within
2 L 2^-53 sum|x| / L: two float64 summations in different orders, (L - 1) u
sum|x| each (Higham, Accuracy and Stability, eq. 4.4), and the two quotients'
roundings, u |mean| <= u sum|x| / L each.

Shapes: P in {1, 2, 3} x L in {1, 31, 32, 33, 255, 256, 257, 260}: a tail
inside a wave (1, 31, 33), a full wave (32), a tail inside a block (255, 257,
260), more than one block per member (257, 260), L % 4 != 0 (the scalar row
stores; the groups start at lanes that are no multiple of 4) and L % 4 == 0
(32, 256, 260: the 16-byte row stores).  24 frames.  The other axes (storage,
compute, physics, reward mode / auto-reset, temperature, probs_used) rotate
over the 24 cases; test_matrix_covers_every_axis asserts that each value and
the pairings that select a code path occur."""
import os

import numpy as np
import pytest
import torch
from torch import nn

from delivery_drone_amd import ActorPopulation, EnvConfig, MlpNet, VecDroneEnv, population_summary

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MEMBERS = (1, 2, 3)
LANES = (1, 31, 32, 33, 255, 256, 257, 260)
STORAGE = ("f32", "f64")
COMPUTE = ("f32", "f16x3")
PHYSICS = {"reference": {}, "gravity": dict(gravity=0.31)}  # a changed constant: the physics come from the call
# (reward_mode, auto_reset, max_steps): the first truncates and re-spawns lanes well inside the 24 frames
SCENARIOS = (("notebook", True, 7), ("reinforce", False, 300), ("engine", False, 300), ("reinforce", True, 9),
             ("notebook", False, 300), ("engine", True, 300))
TEMPERATURES = (1.0, 0, 0.5)
FRAMES, SPAWN_SEED, ENV_ID_BASE, DRAW_SEED, STEP0 = 24, 4, 1000, 9, 3
FIELDS = ("x", "y", "vx", "vy", "angle", "omega", "fuel", "px", "py", "total_reward", "status", "steps", "episode")


def _cases():
    cases = []
    for i, (p, lanes) in enumerate((p, lanes) for p in MEMBERS for lanes in LANES):
        j = i // len(LANES)  # shifts the rotations between the three passes over LANES
        storage = STORAGE[(i + j) % 2]
        compute = COMPUTE[(i // 2 + j) % 2]
        physics = tuple(PHYSICS)[(i // 4 + j) % 2]
        mode, auto_reset, cap = SCENARIOS[(i + 2 * j) % len(SCENARIOS)]
        temperature = TEMPERATURES[(i + j) % 3]
        used = temperature != 1.0 or i % 2 == 0  # temperature 1 without probs_used: the collection kernel is the yardstick
        cases.append((p, lanes, storage, compute, physics, mode, auto_reset, cap, temperature, used))
    return cases


def _id(c):
    return f"P{c[0]}-L{c[1]}-{c[2]}-{c[3]}-{c[4]}-{c[5]}-{'auto' if c[6] else 'sticky'}-T{c[8]}{'-used' if c[9] else ''}"


CASES = _cases()


def test_matrix_covers_every_axis():
    seen = lambda k: {c[k] for c in CASES}  # noqa: E731
    assert seen(0) == set(MEMBERS) and seen(1) == set(LANES)
    assert seen(2) == set(STORAGE) and seen(3) == set(COMPUTE) and seen(4) == set(PHYSICS)
    assert {(c[5], c[6], c[7]) for c in CASES} == set(SCENARIOS)
    assert seen(8) == set(TEMPERATURES) and seen(9) == {True, False}
    # the eight kernels: storage x compute x physics, each with more than one member
    assert {(c[2], c[3], c[4]) for c in CASES if c[0] > 1} == {(s, c, p) for s in STORAGE for c in COMPUTE
                                                               for p in PHYSICS}
    # both row-store paths with more than one member, and a second block per member
    assert {c[1] % 4 == 0 for c in CASES if c[0] > 1} == {True, False}
    assert any(c[0] > 1 and c[1] > 256 for c in CASES)


def _golden(prefix):
    w = np.load(os.path.join(HERE, "golden", "policy.npz"))
    return {k[len(prefix):]: torch.from_numpy(w[k]) for k in w.files if k.startswith(prefix)}


def _random_actor_sd(seed):
    """A seeded torch-default initialisation of the notebooks' actor (inside
    the f16x3 operand ranges, which MlpNet checks), each with another bias on
    the three thrusters so that the members' episodes differ."""
    torch.manual_seed(seed)
    net = nn.Sequential(nn.Linear(15, 128), nn.LayerNorm(128), nn.ReLU(), nn.Linear(128, 128), nn.LayerNorm(128),
                        nn.ReLU(), nn.Linear(128, 64), nn.LayerNorm(64), nn.ReLU(), nn.Linear(64, 3))
    with torch.no_grad():
        net[9].bias.copy_(torch.tensor([-1.0, 0.0, 0.0]) + 0.25 * seed * torch.tensor([1.0, -1.0, 0.5]))
    return net.state_dict()


@pytest.fixture(scope="module")
def state_dicts():
    """Member 0: the notebook's trained actor (tests/golden/policy.npz); the rest seeded."""
    sds = [_golden("actor."), _random_actor_sd(1), _random_actor_sd(2), _random_actor_sd(3)]
    assert sds[0], "policy.npz holds no actor"
    return sds


@pytest.fixture(scope="module")
def actors(gpu_device, state_dicts):
    """compute -> three actors with different weights (never re-loaded: the tests that do build their own)."""
    return {c: [MlpNet(sd, device=gpu_device, compute=c) for sd in state_dicts[:3]] for c in COMPUTE}


def make_env(dev, n, base, *, storage="f32", physics="reference", mode="engine", auto_reset=False, cap=300):
    cfg = EnvConfig(randomize_drone=True, auto_reset=auto_reset, seed=SPAWN_SEED, **PHYSICS[physics])
    env = VecDroneEnv(n, device=dev, config=cfg, precision=storage, reward_mode=mode, max_steps=cap, env_id_base=base)
    env.reset()
    return env


def rollout(env, actor, temperature, used, frames=FRAMES):
    n, dev = env.num_envs, env.device
    kw = {}
    if env.reward_mode != "engine":
        kw = dict(engine_reward_out=torch.full((frames, n), float("nan"), dtype=env.float_dtype, device=dev),
                  engine_done_out=torch.full((frames, n), 7, dtype=torch.uint8, device=dev))
    if used:
        kw["probs_used_out"] = torch.full((frames, n, 3), float("nan"), device=dev)
    obs, acts, lp, rew, done = env.policy_rollout(actor, frames, seed=DRAW_SEED, step=STEP0, temperature=temperature,
                                                  **kw)
    out = {"obs": obs, "actions": acts, "log_prob": lp, "reward": rew, "done": done}
    out.update({k[:-len("_out")]: v for k, v in kw.items()})
    return out


def assert_group_equals(big_out, big_env, lanes, small_out, small_env, what):
    """The big launch's lane columns `lanes` against a single-actor launch on those lanes alone."""
    for key, want in small_out.items():
        got = big_out[key][:, lanes]
        assert got.dtype == want.dtype and torch.equal(got, want), f"{what}: {key}"  # NaN != NaN: equal means none
    assert torch.equal(big_env.obs[lanes], small_env.obs), f"{what}: env.obs"
    big_sd, small_sd = big_env.state_dict(), small_env.state_dict()
    assert sorted(big_sd) == sorted(small_sd)
    for f in small_sd:
        got = big_sd[f][:, lanes] if f == "shaped_hist" else big_sd[f][lanes]
        want = small_sd[f]
        if f == "shaped_hist":  # NaN marks "no previous frame": compare the bits
            got, want = got.contiguous().view(torch.int64), want.contiguous().view(torch.int64)
        assert torch.equal(got, want), f"{what}: state {f}"


@pytest.mark.parametrize("p,lanes,storage,compute,physics,mode,auto_reset,cap,temperature,used", CASES,
                         ids=[_id(c) for c in CASES])
def test_population_rollout_equals_single_actor_rollouts(actors, gpu_device, p, lanes, storage, compute, physics, mode,
                                                         auto_reset, cap, temperature, used):
    members = actors[compute][:p]
    pop = ActorPopulation(members)
    kw = dict(storage=storage, physics=physics, mode=mode, auto_reset=auto_reset, cap=cap)
    big = make_env(gpu_device, p * lanes, ENV_ID_BASE, **kw)
    got = rollout(big, pop, temperature, used)
    assert got["obs"].shape == (FRAMES, p * lanes, 15) and got["reward"].dtype == big.float_dtype
    ended = False
    for g in range(p):
        assert pop.lanes(big, g) == slice(g * lanes, (g + 1) * lanes)
        small = make_env(gpu_device, lanes, ENV_ID_BASE + g * lanes, **kw)
        want = rollout(small, members[g], temperature, used)  # P == 1: policy_rollout(actor) on the same lanes
        assert_group_equals(got, big, pop.lanes(big, g), want, small, f"member {g}")
        ended |= bool(want["done"].any()) and int(small.episode.max()) > 1
    if auto_reset and cap < FRAMES:  # every lane is truncated at the cap at the latest
        assert ended, "no lane of the single-actor runs ended and re-spawned"


def test_members_get_different_results(actors, gpu_device):
    """The yardstick itself tells the members apart: the same lanes under two
    members' weights differ, so a launch that read one image for every group
    could not pass the matrix."""
    a, b = actors["f32"][0], actors["f32"][1]
    one, two = make_env(gpu_device, 64, ENV_ID_BASE), make_env(gpu_device, 64, ENV_ID_BASE)
    ra, rb = rollout(one, a, 0, True), rollout(two, b, 0, True)
    assert not torch.equal(ra["probs_used"], rb["probs_used"]) and not torch.equal(ra["actions"], rb["actions"])


@pytest.mark.parametrize("compute,mode,storage", [("f16x3", "notebook", "f32"), ("f32", "engine", "f64")])
def test_evaluate_policy_and_summary(actors, gpu_device, compute, mode, storage):
    p, lanes, cap, chunk, temperature, seed = 3, 33, 40, 16, 0.5, 13
    members = actors[compute]
    pop = ActorPopulation(members)
    big = make_env(gpu_device, p * lanes, ENV_ID_BASE, storage=storage, mode=mode)
    got = big.evaluate_policy(pop, max_steps=cap, temperature=temperature, seed=seed, frames_per_launch=chunk)
    assert sorted(got) == ["crashed", "final_fuel", "landed", "steps", "total_reward"]
    summary = population_summary(got, p)
    assert sorted(summary) == ["mean_final_fuel", "mean_reward", "mean_steps", "success_rate"]
    for v in summary.values():
        assert v.shape == (p,) and v.device == gpu_device
    finished = 0
    for g in range(p):
        small = make_env(gpu_device, lanes, ENV_ID_BASE + g * lanes, storage=storage, mode=mode)
        want = small.evaluate_policy(members[g], max_steps=cap, temperature=temperature, seed=seed,
                                     frames_per_launch=chunk)
        for key in want:
            assert got[key].dtype == want[key].dtype and torch.equal(got[key][pop.lanes(big, g)], want[key]), (g, key)
        assert torch.equal(big.obs[pop.lanes(big, g)], small.obs)
        for f in FIELDS:
            assert torch.equal(getattr(big, f)[pop.lanes(big, g)], getattr(small, f)), (g, f)
        finished += int((want["landed"] | want["crashed"]).sum())
        host = {k: v.cpu().numpy().astype(np.float64) for k, v in want.items()}
        assert float(summary["success_rate"][g]) == host["landed"].mean()
        assert float(summary["mean_steps"][g]) == host["steps"].mean()
        for name, key in (("mean_reward", "total_reward"), ("mean_final_fuel", "final_fuel")):
            tol = 2 * lanes * 2.0 ** -53 * np.abs(host[key]).sum() / lanes
            print(f"member {g} {name}: {float(summary[name][g])!r} host {host[key].mean()!r} bound {tol:.3g}")
            assert abs(float(summary[name][g]) - host[key].mean()) <= tol, (g, name)
    assert finished > 0, "no episode of the single-actor evaluations ended inside the cap"


def test_new_weights_are_seen_by_the_same_population(gpu_device, state_dicts):
    """load_state_dict re-packs into the same buffer: the table built once
    still points at it, so member 1 plays its new weights at the next launch
    and members 0 and 2 are untouched."""
    p, lanes = 3, 33
    members = [MlpNet(sd, device=gpu_device, compute="f16x3") for sd in state_dicts[:3]]
    pop = ActorPopulation(members)
    table, address = pop.table.clone(), members[1].packed.data_ptr()
    before = rollout(make_env(gpu_device, p * lanes, ENV_ID_BASE), pop, 0.5, True)
    members[1].load_state_dict(state_dicts[3])
    assert members[1].packed.data_ptr() == address and torch.equal(pop.table, table)
    big = make_env(gpu_device, p * lanes, ENV_ID_BASE)
    after = rollout(big, pop, 0.5, True)
    for g in (0, 2):
        for key in before:
            assert torch.equal(after[key][:, pop.lanes(big, g)], before[key][:, pop.lanes(big, g)]), (g, key)
    fresh = MlpNet(state_dicts[3], device=gpu_device, compute="f16x3")
    small = make_env(gpu_device, lanes, ENV_ID_BASE + lanes)
    assert_group_equals(after, big, pop.lanes(big, 1), rollout(small, fresh, 0.5, True), small, "member 1 reloaded")
    assert not torch.equal(after["probs_used"][:, pop.lanes(big, 1)], before["probs_used"][:, pop.lanes(big, 1)])


def test_population_argument_errors(actors, gpu_device):
    f32, split = actors["f32"], actors["f16x3"]
    critic = MlpNet(_golden("critic."), device=gpu_device)
    assert critic.out_dim == 1
    with pytest.raises(ValueError, match="out_dim 3"):
        ActorPopulation([f32[0], critic])
    with pytest.raises(ValueError, match="compute"):
        ActorPopulation([f32[0], split[1]])
    with pytest.raises(ValueError):
        ActorPopulation([])
    with pytest.raises(ValueError, match="out_dim 3"):
        ActorPopulation([f32[0], "not an actor"])
    pop = ActorPopulation(f32[:2])
    assert len(pop) == 2 and pop[0] is f32[0] and pop[-1] is f32[1] and list(pop) == f32[:2]
    odd = make_env(gpu_device, 7, ENV_ID_BASE, mode="notebook")
    with pytest.raises(ValueError, match="equal groups"):
        odd.policy_rollout(pop, 4)
    with pytest.raises(ValueError, match="equal groups"):
        odd.evaluate_policy(pop, max_steps=4)
    with pytest.raises(ValueError, match="equal groups"):
        pop.lanes(odd, 0)
    even = make_env(gpu_device, 8, ENV_ID_BASE, mode="notebook")
    with pytest.raises(ValueError, match="components"):
        even.evaluate_policy(pop, max_steps=4, components=True)
    with pytest.raises(IndexError):
        pop.lanes(even, 2)
    assert pop.lanes(even, -1) == slice(4, 8)
