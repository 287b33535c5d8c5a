"""GPU: the shaped tail of a frame (frame.h shaped_tail and the copy ac_fused.hip keeps) agrees across the three
kernels that run it, on a case no single kernel's file covers: lanes that end on their own, lanes that run into
the env's max_steps timeout un-landed, sticky frames after either, and (auto_reset) the re-spawn frame.

Every learner steps with lr = 0 and weight_decay = 0, so each path runs the same weights on every frame and
draws the same actions (keys (seed; env id, step + frame)).  The reference is env.policy_rollout of the same
actors on a twin env; rewards, dones and the reward history are compared on bit patterns.

The spawn seed was chosen on the CPU with oracle/pyloop.py: with seed 324, lane 6 of the first fifteen lands in
its first frame under every constant action and the other fourteen are still flying after eight frames, so with
max_steps = 8 the reference shows both endings (asserted below, not assumed).
"""
import pytest
import torch

import golden_data as gd
from delivery_drone_amd import (AdamW, EnvConfig, LearnerPopulation, MlpNet, ReinforcePopulation, VecDroneEnv, abi,
                                actor_critic_train_population, reinforce_train, reinforce_train_population)

pytestmark = pytest.mark.gpu

SEED, STEP = 11, 3
TIMEOUT = 8           # the env's max_steps
FRAMES = TIMEOUT + 3  # sticky frames (or re-spawned ones) after every lane's first ending


@pytest.fixture(scope="module")
def nets():
    return gd.policy_fixture()[1]


def net(nets, tag, dev, p=0):
    sd = {k: torch.as_tensor(v).clone() for k, v in nets[tag].items()}
    sd["9.bias"] = sd["9.bias"] + 0.125 * p
    return MlpNet(sd, device=dev)


def frozen(network):
    return AdamW(network, lr=0.0, weight_decay=0.0)


def bits(t):
    t = t.detach().contiguous()
    return t.view({torch.float64: torch.int64, torch.float32: torch.int32}.get(t.dtype, t.dtype))


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def test_three_kernels_one_tail(nets):
    dev = torch.device("cuda", 0)
    members, lanes = 3, 5
    n = members * lanes
    kw = dict(device=dev, reward_mode="notebook", max_steps=TIMEOUT)
    sticky = EnvConfig(randomize_drone=True, randomize_platform=True, seed=324)
    again = EnvConfig(randomize_drone=True, randomize_platform=True, seed=324, auto_reset=True)

    rf_pop = ReinforcePopulation([(a, frozen(a)) for a in (net(nets, "actor", dev, p) for p in range(members))])
    ac_members = []
    for p in range(members):
        actor, critic = net(nets, "actor", dev, p), net(nets, "critic", dev, p)
        ac_members.append((actor, critic, frozen(actor), frozen(critic)))
    ac_pop = LearnerPopulation(ac_members)
    images = [m[0].packed.clone() for m in ac_members]

    # the reference: policy_rollout of the same actors on twin envs
    ref = {}
    for name, cfg in (("sticky", sticky), ("again", again)):
        twin = VecDroneEnv(n, config=cfg, **kw)
        twin.reset()
        _, _, _, reward, done = twin.policy_rollout(ac_pop.actors, FRAMES, seed=SEED, step=STEP)
        ref[name] = (reward, done, twin)
    reward, done, twin = ref["sticky"]
    first = torch.where(done.any(0), done.int().argmax(0), torch.full((n,), FRAMES, device=dev))  # the ending frame
    flagged = (twin.status & (abi.DD_ST_LANDED | abi.DD_ST_CRASHED)) != 0
    assert bool(((first < TIMEOUT - 1) & flagged).any()), "no lane ended on its own before the timeout"
    timed_out = (first == TIMEOUT - 1) & ~flagged
    assert bool(timed_out.any()), "no lane timed out un-landed"
    assert bool((first < FRAMES).all())  # every lane ended: the frames after are sticky ones

    # reinforce_fused.hip, sticky
    env = VecDroneEnv(n, config=sticky, **kw)
    run = reinforce_train_population(env, rf_pop, FRAMES, seed=SEED, step=STEP, record=True)
    assert torch.equal(run.lengths.long(), first + 1) and bool(run.ended.all())
    recorded = torch.arange(FRAMES, device=dev)[:, None] < run.lengths[None, :]  # zeros after a lane's episode
    assert same(run.reward[recorded], reward[recorded]) and torch.equal(run.done[recorded], done[recorded])
    assert same(env.shaped_hist, twin.shaped_hist)

    # ac_fused.hip, sticky and re-spawning
    for name, cfg in (("sticky", sticky), ("again", again)):
        reward, done, twin = ref[name]
        env = VecDroneEnv(n, config=cfg, **kw)
        env.reset()
        run = actor_critic_train_population(env, ac_pop, FRAMES, seed=SEED, step=STEP, record=True)
        assert same(run.reward, reward) and torch.equal(run.done, done), name
        assert same(env.shaped_hist, twin.shaped_hist), name
    assert bool(ref["again"][2].episode.max() > 1)  # the re-spawn frame was played

    # lr = 0 held: every path ran the same weights on every frame
    for (actor, _), (ac_actor, _, _, _), image in zip(rf_pop, ac_pop, images):
        assert same(actor.packed, image) and same(ac_actor.packed, image)


def test_reinforce_shape_two_ragged_waves(nets):
    """reward_mode="reinforce" on 33 lanes: two waves of the forward, the second with one live row."""
    dev = torch.device("cuda", 0)
    n = 33
    cfg = EnvConfig(randomize_drone=True, randomize_platform=True, seed=324)
    kw = dict(device=dev, config=cfg, reward_mode="reinforce", max_steps=TIMEOUT)
    actor, twin_actor = net(nets, "actor", dev), net(nets, "actor", dev)
    twin = VecDroneEnv(n, **kw)
    twin.reset()
    _, _, _, reward, done = twin.policy_rollout(twin_actor, FRAMES, seed=SEED, step=STEP)
    env = VecDroneEnv(n, **kw)
    run = reinforce_train(env, actor, frozen(actor), FRAMES, seed=SEED, step=STEP, record=True)
    first = torch.where(done.any(0), done.int().argmax(0), torch.full((n,), FRAMES - 1, device=dev))
    assert torch.equal(run.lengths.long(), first + 1) and torch.equal(run.ended, done.any(0))
    recorded = torch.arange(FRAMES, device=dev)[:, None] < run.lengths[None, :]
    assert same(run.reward[recorded], reward[recorded]) and torch.equal(run.done[recorded], done[recorded])
    assert same(actor.packed, twin_actor.packed)
