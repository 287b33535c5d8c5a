"""GPU: reinforce_train / reinforce_train_population (dd_reinforce_train,
csrc/reinforce_fused.hip) against the loop of launches it replaces.

The reference of every case is, per member, this loop on twins of its actor and
optimizer and on a twin env of its lanes alone (env_id_base at the group's
start):

    batch = collect_reinforce(env_g, actor, max_steps, seed=, step=, gamma=gamma_g, normalize=)
    upd = reinforce_update(actor, batch, opt, max_grad_norm=norm_g)

Nothing is approximate: the five logs, lengths, ended, episode_return, the
returns and advantages scattered to [frames, N], the flat parameters, both
moments, the optimizer's state block, the packed image and the gradient buffer,
every state array of the env and its obs are compared on bit patterns (a NaN,
which the loop gives for the std and the advantages of a one-row batch, equals
a NaN).
"""
import pytest
import torch

import adamw_ref
import golden_data as gd
from delivery_drone_amd import (REINFORCE_LOG_KEYS, AdamW, EnvConfig, MlpNet, ReinforcePopulation, VecDroneEnv,
                                collect_reinforce, reinforce_train, reinforce_train_population, reinforce_update)

pytestmark = pytest.mark.gpu

ENV_FIELDS = gd.FLOAT_FIELDS + ("status", "steps", "episode", "obs")
# strong gravity: a random actor's drone is on the ground, the pad or out of bounds within a few dozen frames
FAST = EnvConfig(gravity=3.0, randomize_drone=True, randomize_platform=True, seed=5)
# the reference physics, the pad far below the spawn: in three frames no drone gets anywhere, so only a
# timeout ends an episode
CALM = EnvConfig(randomize_platform=False, seed=7)
# drones that hover for ever: no gravity, no thrust, no fuel burnt
HOVER = EnvConfig(randomize_platform=False, gravity=0.0, main_thrust_power=0.0, side_thrust_power=0.0, fuel_main=0.0,
                  fuel_side=0.0, seed=3)
# spawns from the top of the world to below the ground: some drones crash in their first frame
RAGGED = EnvConfig(randomize_drone=True, randomize_platform=True, drone_y_min=50, drone_y_max=640, seed=9)


@pytest.fixture(scope="module")
def nets():
    return gd.policy_fixture()[1]


def make_member(nets, dev, p=0, lr_scale=1.0):
    sd = {k: torch.as_tensor(v).clone() for k, v in nets["actor"].items()}
    sd["9.bias"] = sd["9.bias"] + 0.125 * (p % 8)
    actor = MlpNet(sd, device=dev)
    return actor, AdamW(actor, lr=adamw_ref.NOTEBOOK_LR["actor"] * lr_scale)


def bits(t):
    t = t.detach().contiguous()
    return t.view({torch.float64: torch.int64, torch.float32: torch.int32}.get(t.dtype, t.dtype))


def same(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.is_floating_point():
        nan = torch.isnan(a)
        return torch.equal(nan, torch.isnan(b)) and torch.equal(bits(a)[~nan], bits(b)[~nan])
    return torch.equal(a, b)


def training_state(member):
    actor, opt = member
    return {"params": actor.flat_parameters(), "packed": actor.packed, "exp_avg": opt.exp_avg,
            "exp_avg_sq": opt.exp_avg_sq, "state": opt._state, "grads": opt.grad_buffer()}


def assert_same_training(ours, twin, where):
    mine, theirs = training_state(ours), training_state(twin)
    for name in mine:
        assert same(mine[name], theirs[name]), (where, name, int((bits(mine[name]) != bits(theirs[name])).sum()))


def assert_same_env(env, group, single, where):
    fields = ENV_FIELDS + (("shaped_hist",) if single.reward_mode == "notebook" else ())
    for name in fields:
        t = getattr(env, name)
        assert same(t[:, group] if name == "shaped_hist" else t[group], getattr(single, name)), (where, name)


def scattered(batch, column, frames):
    """A batch's flat column at its frames: [frames, L], zeros after a lane's episode."""
    lanes = batch.lengths.numel()
    lengths = batch.lengths.long()
    lane = torch.repeat_interleave(torch.arange(lanes, device=column.device), lengths)
    frame = torch.arange(column.numel(), device=column.device) - torch.repeat_interleave(batch.offsets[:-1], lengths)
    out = torch.zeros(frames, lanes, dtype=column.dtype, device=column.device)
    out[frame, lane] = column
    return out


def run_case(nets, dev, members, lanes, frames, *, cfg=FAST, env_kw=None, gamma=0.99, max_grad_norm=0.5, lr=None,
             normalize=True, seed=11, step=3, iterations=1, single_call=False):
    """The launch on fresh learners and a fresh env against the loop on twins; everything compared.  Returns
    the last run, its batches, the population and the env."""
    env_kw = env_kw or {}
    lr = lr or [1.0] * members
    ours = [make_member(nets, dev, p, lr[p]) for p in range(members)]
    twins = [make_member(nets, dev, p, lr[p]) for p in range(members)]
    pop = None if single_call else ReinforcePopulation(ours)
    env = VecDroneEnv(members * lanes, device=dev, config=cfg, **env_kw)
    singles = [VecDroneEnv(lanes, device=dev, config=cfg, env_id_base=g * lanes, **env_kw) for g in range(members)]
    per = lambda v, g: v[g] if isinstance(v, (list, tuple)) else v
    for it in range(iterations):
        at = step + it * frames
        if single_call:
            run = reinforce_train(env, *ours[0], frames, seed=seed, step=at, gamma=gamma, max_grad_norm=max_grad_norm,
                                  normalize=normalize, record=True)
        else:
            run = reinforce_train_population(env, pop, frames, seed=seed, step=at, gamma=gamma,
                                             max_grad_norm=max_grad_norm, normalize=normalize, record=True)
        assert tuple(run.logs.shape) == (len(REINFORCE_LOG_KEYS), members) and run.logs.dtype == torch.float64
        assert run.obs is env.obs
        batches = []
        for g, (actor, opt) in enumerate(twins):
            where = (it, g)
            group = slice(g * lanes, (g + 1) * lanes)
            batch = collect_reinforce(singles[g], actor, frames, seed=seed, step=at, gamma=per(gamma, g),
                                      normalize=normalize)
            upd = reinforce_update(actor, batch, opt, max_grad_norm=per(max_grad_norm, g))
            rows = torch.tensor(float(batch.returns.numel()), dtype=torch.float64, device=dev)
            for key, want in zip(REINFORCE_LOG_KEYS, (upd.loss, upd.grad_norm, batch.baseline, batch.std, rows)):
                got = run.log(key)[g]
                assert same(got, want.reshape(())), (where, key, got.item(), want.item())
            assert same(run.lengths[group], batch.lengths), where
            assert same(run.ended[group], batch.ended), where
            assert same(run.episode_return[group], batch.episode_return), where
            assert same(run.returns[:, group], scattered(batch, batch.returns, frames)), where
            assert same(run.advantages[:, group], scattered(batch, batch.advantages, frames)), where
            done = run.done[:, group]
            assert torch.equal(done.sum(0) > 0, batch.ended) and int(done.sum(0).max()) <= 1, where
            assert_same_training(ours[g], twins[g], where)
            assert_same_env(env, group, singles[g], where)
            assert opt.step_count() == it + 1 == ours[g][1].step_count()
            batches.append(batch)
    return run, batches, (pop, ours, twins), (env, singles)


@pytest.mark.parametrize("lanes, frames", [(1, 2), (3, 40), (33, 40), (128, 40)])
def test_one_member_lane_counts(nets, gpu_device, lanes, frames):
    """A single lane on two frames, a ragged wave, a wave boundary, the full tile."""
    run_case(nets, gpu_device, 1, lanes, frames)


@pytest.mark.parametrize("lanes, frames", [(127, 1), (64, 2), (43, 3)])
def test_rows_around_one_tile(nets, gpu_device, lanes, frames):
    """M = 127, 128 and 129 rows: only the timeout ends an episode, so M = lanes x frames."""
    run, batches, _, _ = run_case(nets, gpu_device, 1, lanes, frames, cfg=CALM,
                                  env_kw=dict(reward_mode="reinforce", max_steps=frames))
    assert batches[0].returns.numel() == lanes * frames == int(run.log("rows")[0].item())
    assert bool(batches[0].ended.all())


@pytest.mark.parametrize("mode", ["engine", "notebook", "reinforce"])
def test_ragged_episodes_in_every_reward_mode(nets, gpu_device, mode):
    """Lanes end on different frames: some in their first, some at the shaped modes' timeout (the engine's
    reward has none: there the longest episode is cut by the end of the rollout)."""
    env_kw = dict(reward_mode=mode) if mode == "engine" else dict(reward_mode=mode, max_steps=12)
    run, batches, _, (env, _) = run_case(nets, gpu_device, 1, 96, 14, cfg=RAGGED, env_kw=env_kw)
    lengths = batches[0].lengths
    assert int(lengths.min()) == 1 and len(set(lengths.tolist())) > 2
    if mode == "engine":
        assert int(lengths.max()) == 14 and not bool(batches[0].ended.all())
    else:
        assert int(lengths.max()) == 12 and bool(batches[0].ended.all())
        assert bool((env.steps == 12).any())  # a lane reached the timeout


def test_without_normalisation(nets, gpu_device):
    run, batches, _, _ = run_case(nets, gpu_device, 1, 33, 40, normalize=False)
    assert same(batches[0].advantages, batches[0].returns)


def test_three_members_with_their_own_hyperparameters(nets, gpu_device):
    run, _, _, _ = run_case(nets, gpu_device, 3, 20, 40, gamma=[0.99, 0.9, 0.95], max_grad_norm=[0.5, None, 0.05],
                            lr=[1.0, 3.0, 0.3])
    assert len(set(run.log("loss").tolist())) == 3


def test_more_members_than_compute_units(nets, gpu_device):
    run_case(nets, gpu_device, 260, 1, 4)


def test_three_chained_iterations(nets, gpu_device):
    run_case(nets, gpu_device, 2, 33, 30, iterations=3, env_kw=dict(reward_mode="reinforce", max_steps=25))


def test_the_packed_images_are_current_after_an_update(nets, gpu_device):
    """The next population rollout runs the updated actors."""
    _, _, (pop, _, twins), (env, singles) = run_case(nets, gpu_device, 3, 20, 40)
    env.reset()
    obs, acts, lp, reward, done = env.policy_rollout(pop.actors, 6, seed=4, step=50)
    for g, (actor, _) in enumerate(twins):
        group = slice(g * 20, (g + 1) * 20)
        singles[g].reset()
        want = singles[g].policy_rollout(actor, 6, seed=4, step=50)
        for got, w in zip((obs, acts, lp, reward, done), want):
            assert same(got[:, group], w), g


def test_the_single_call_is_the_population_of_one(nets, gpu_device):
    run, _, _, _ = run_case(nets, gpu_device, 1, 33, 40, single_call=True)
    other, _, _, _ = run_case(nets, gpu_device, 1, 33, 40)
    assert all(same(a, b) for a, b in zip(run, other))


def test_blocks_that_take_two_tiles(nets, gpu_device):
    """M = 128 x 257 = 32,896 rows > 256 x 128: block 0 of the backward's 256 takes tiles 0 and 256.
    Measured on an MI355X: 0.06 s, the loop included."""
    run, batches, _, _ = run_case(nets, gpu_device, 1, 128, 257, cfg=HOVER,
                                  env_kw=dict(reward_mode="reinforce", max_steps=257))
    assert batches[0].returns.numel() == 128 * 257 > 256 * 128
