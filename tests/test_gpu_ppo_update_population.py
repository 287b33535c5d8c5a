"""GPU: ppo_update_population (dd_ppo_update_population,
csrc/ppo_fused_population.hip) against single ppo_update(fused=True) calls.

The reference of every case is, for each member, one ppo_update(...,
fused=True) with that member's arguments on twins of its networks and
optimizers.  Nothing is approximate: for every member the eleven logs, the
summary, both flat parameter buffers, both packed images, both optimizers'
moments, device state blocks and gradient buffers are compared on bit patterns
(int32 / int64 views, so NaN logs compare by their bits too).

Networks and rows are those of tests/test_gpu_ppo_fused.py: the policy
fixture's actor and critic (member p's last-layer biases shifted by p, so that
the members differ), the ppo_loss fixture's 203 rows rolled by the member's
index and repeated to M.
"""
import numpy as np
import pytest
import torch

import adamw_ref
import golden_data as gd
from delivery_drone_amd import (AdamW, EnvConfig, LearnerPopulation, MlpNet, VecDroneEnv, collect_ppo,
                                collect_ppo_population, ppo_update, ppo_update_population)
from delivery_drone_amd.adamw import LOG_KEYS, minibatch_ranges

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15   # both keys above 2^32: their high halves count
EPOCH = (7 << 32) + 3
COLUMNS = ("states", "actions", "old_log_probs", "advantages", "returns")
COEF = dict(clip_epsilon=0.2, entropy_coef=0.01, value_coef=0.5, max_grad_norm=0.5)


@pytest.fixture(scope="module")
def nets():
    return gd.policy_fixture()[1]


@pytest.fixture(scope="module")
def rows():
    return gd.npz("ppo_loss/losses.npz")


def make_batch(rows, m, dev, p=0, actions="f32x3"):
    five = [np.ascontiguousarray(np.resize(np.roll(rows[k], -7 * p, axis=0), (m,) + rows[k].shape[1:]))
            for k in COLUMNS]
    if actions == "bitmask":  # the same actions as dd_step's uint8 bitmask
        a = five[1] != 0.0
        five[1] = (a[:, 0] + 2 * a[:, 1] + 4 * a[:, 2]).astype(np.uint8)
    elif actions == "any_nonzero":  # a pressed thruster is any value but 0
        five[1] = (five[1] * np.array([0.5, -2.0, 3.0], np.float32)).astype(np.float32)
        assert set(np.unique(five[1])) - {0.0, 1.0}
    return tuple(torch.as_tensor(t, device=dev) for t in five)


def make_member(nets, dev, p, lr_scale=1.0):
    sd = {tag: {k: torch.as_tensor(v).clone() for k, v in nets[tag].items()} for tag in ("actor", "critic")}
    for tag in sd:
        sd[tag]["9.bias"] = sd[tag]["9.bias"] + 0.125 * p
    actor, critic = MlpNet(sd["actor"], device=dev), MlpNet(sd["critic"], device=dev)
    return (actor, critic, AdamW(actor, lr=adamw_ref.NOTEBOOK_LR["actor"] * lr_scale),
            AdamW(critic, lr=adamw_ref.NOTEBOOK_LR["critic"] * lr_scale))


def bits(t):
    """A float tensor's bit patterns; any other tensor as it is."""
    t = t.detach().contiguous()
    return t.view({torch.float64: torch.int64, torch.float32: torch.int32}.get(t.dtype, t.dtype))


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def training_state(member):
    actor, critic, a_opt, c_opt = member
    out = {"actor.params": actor.flat_parameters(), "critic.params": critic.flat_parameters(),
           "actor.packed": actor.packed, "critic.packed": critic.packed}
    for tag, o in (("actor", a_opt), ("critic", c_opt)):
        out.update({f"{tag}.exp_avg": o.exp_avg, f"{tag}.exp_avg_sq": o.exp_avg_sq, f"{tag}.state": o._state,
                    f"{tag}.grads": o.grad_buffer()})
    return out


def assert_same_member(p, ours, twin, got, want, shape):
    assert tuple(got.logs) == LOG_KEYS and set(got.summary) == set(want.summary)
    for key in LOG_KEYS:
        assert tuple(got.logs[key].shape) == shape and got.logs[key].dtype == torch.float64, (p, key)
        assert same(got.logs[key], want.logs[key]), (p, key, got.logs[key].tolist(), want.logs[key].tolist())
        assert same(got.summary[key], want.summary[key]), (p, key)
    mine, theirs = training_state(ours), training_state(twin)
    for name in mine:
        assert same(mine[name], theirs[name]), (p, name, int((bits(mine[name]) != bits(theirs[name])).sum()))


def per_member(value, p):
    return value[p] if isinstance(value, list) else value


def run_case(nets, rows, dev, ms, *, actions=None, lr_scales=None, **kw):
    """The population call on len(ms) fresh members against one fused call per twin; every member compared."""
    count = len(ms)
    actions = actions or ["f32x3"] * count
    lr_scales = lr_scales or [1.0] * count
    ours = [make_member(nets, dev, p, lr_scales[p]) for p in range(count)]
    twins = [make_member(nets, dev, p, lr_scales[p]) for p in range(count)]
    batches = [make_batch(rows, m, dev, p, actions[p]) for p, m in enumerate(ms)]
    pop = LearnerPopulation(ours)
    got = ppo_update_population(pop, batches, **kw)
    assert len(got) == count
    size, drop_last, epochs = kw.get("minibatch_size"), kw.get("drop_last", False), kw.get("num_epochs", 4)
    for p in range(count):
        single = {k: per_member(v, p) for k, v in kw.items()}
        want = ppo_update(*twins[p][:2], batches[p], *twins[p][2:], fused=True, **single)
        steps = None if size is None else len(minibatch_ranges(ms[p], size, drop_last))
        assert_same_member(p, ours[p], twins[p], got[p], want, (epochs,) if steps is None else (epochs, steps))
        assert ours[p][2].step_count() == epochs * (steps or 1) == ours[p][3].step_count()
    return ours, got


def test_ragged_members(nets, rows, gpu_device):
    """Tail minibatches of 3, 2 and 8 rows, one, three and four steps an epoch, the permutation's smallest
    domains; a learning rate, a clip range and a shuffle seed per member."""
    _, got = run_case(nets, rows, gpu_device, (3, 130, 200), lr_scales=[1.0, 0.5, 2.0], num_epochs=2,
                      minibatch_size=64, clip_epsilon=[0.2, 0.1, 0.3], shuffle_seed=[SEED, 3, 2**64 - 1],
                      shuffle_epoch=EPOCH, entropy_coef=0.01, value_coef=0.5, max_grad_norm=0.5)
    assert [tuple(g.logs["total_loss"].shape) for g in got] == [(2, 1), (2, 3), (2, 4)]
    # the second epoch saw another order and other weights
    assert not same(got[2].logs["policy_grad_norm"][0], got[2].logs["policy_grad_norm"][1])


def test_full_batch_no_shuffle_odd_population(nets, rows, gpu_device):
    """m = 1: ratio_std is NaN; 32 and 33: the wave tile's edge; 128: the full tile."""
    _, got = run_case(nets, rows, gpu_device, (1, 32, 33, 128, 64), num_epochs=2, **COEF)
    assert bool(torch.isnan(got[0].logs["ratio_std"]).all())
    assert not bool(torch.isnan(got[1].logs["ratio_std"]).any())


def test_action_formats(nets, rows, gpu_device):
    run_case(nets, rows, gpu_device, (70, 70), actions=["bitmask", "any_nonzero"], num_epochs=1, minibatch_size=64,
             shuffle_seed=5, **COEF)


def test_more_blocks_than_cus(nets, rows, gpu_device):
    """260 workgroups at one per CU: the later ones start when a CU is free, and nothing waits on them."""
    assert torch.cuda.get_device_properties(gpu_device).multi_processor_count < 260
    run_case(nets, rows, gpu_device, (4,) * 130, num_epochs=1, minibatch_size=4, shuffle_seed=list(range(130)),
             **COEF)


def test_drop_last(nets, rows, gpu_device):
    _, got = run_case(nets, rows, gpu_device, (64, 100), num_epochs=2, minibatch_size=32, drop_last=True,
                      shuffle_seed=9, shuffle_epoch=4, **COEF)
    assert [tuple(g.logs["value_loss"].shape) for g in got] == [(2, 2), (2, 3)]


def test_the_loop_closes(nets, gpu_device):
    """Population rollout, per-member batches, one population update, and the next population rollout on the
    new weights, against the same per member: collect_ppo on a 64-lane env whose env_id_base is the group's
    start, ppo_update(fused=True), policy_rollout."""
    members, lanes, frames, base = 3, 64, 40, 1000
    cfg = EnvConfig(randomize_drone=True, seed=4)
    ours = [make_member(nets, gpu_device, p) for p in range(members)]
    twins = [make_member(nets, gpu_device, p) for p in range(members)]
    kw = dict(num_epochs=2, minibatch_size=64, shuffle_epoch=6, **COEF)
    seeds = [11, 12, 13]

    pop = LearnerPopulation(ours)
    env = VecDroneEnv(members * lanes, device=gpu_device, config=cfg, env_id_base=base)
    batches = collect_ppo_population(env, pop, frames, seed=9, step=3)
    got = ppo_update_population(pop, batches, shuffle_seed=seeds, **kw)
    env.reset()
    after = env.policy_rollout(pop.actors, frames, seed=10, step=5)

    for p in range(members):
        single = VecDroneEnv(lanes, device=gpu_device, config=cfg, env_id_base=base + p * lanes)
        batch = collect_ppo(single, twins[p][0], twins[p][1], frames, seed=9, step=3)
        for name, mine, theirs in zip(batch._fields, batches[p], batch):
            assert same(mine, theirs), (p, name)
        want = ppo_update(*twins[p][:2], batch, *twins[p][2:], fused=True, shuffle_seed=seeds[p], **kw)
        steps = len(minibatch_ranges(batch.states.shape[0], 64))
        assert_same_member(p, ours[p], twins[p], got[p], want, (2, steps))
        single.reset()
        alone = single.policy_rollout(twins[p][0], frames, seed=10, step=5)
        group = pop.actors.lanes(env, p)
        for mine, theirs in zip(after, alone):
            assert same(mine[:, group], theirs), p
        assert same(env.obs[group], single.obs), p
