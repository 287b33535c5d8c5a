"""GPU: actor_critic_train / actor_critic_train_population (dd_actor_critic_train,
csrc/ac_fused.hip) against the loop of launches it replaces.

The reference of every case is, per member, this loop on twins of its networks
and optimizers and on a twin env of its lanes alone:

    state = obs.clone(); actions, _ = actor.act(state, seed, step + t, env_id_base)
    obs, reward, done, _ = env.step(actions)
    actor_critic_update(..., active=~done_prev); done_prev = done

Nothing is approximate: the seven logs of every frame, both flat parameter
buffers, both packed images, both optimizers' moments, device state blocks and
gradient buffers, every state array of the env, its obs and step outputs, and
the recorded reward and done are compared on bit patterns (integer views, so
NaN logs and the NaN of a fresh reward history compare by their bits too).
"""
import pytest
import torch

import adamw_ref
import config_field_cases as cfc
import golden_data as gd
from delivery_drone_amd import (AC_LOG_KEYS, AdamW, EnvConfig, LearnerPopulation, MlpNet, VecDroneEnv,
                                actor_critic_train, actor_critic_train_population, actor_critic_update,
                                td_losses)

pytestmark = pytest.mark.gpu

ENV_FIELDS = gd.FLOAT_FIELDS + ("status", "steps", "episode", "obs", "reward", "_done")
SHAPED_FIELDS = ("shaped_hist", "shaped_reward", "_shaped_done")
CFG = EnvConfig(randomize_drone=True, randomize_platform=True, auto_reset=True, seed=5)
HYPER = dict(gamma=0.99, value_reg=0.01, max_grad_norm=0.5)


@pytest.fixture(scope="module")
def nets():
    return gd.policy_fixture()[1]


def make_member(nets, dev, p=0, lr_scale=1.0, actor_ln_eps=1e-5):
    sd = {tag: {k: torch.as_tensor(v).clone() for k, v in nets[tag].items()} for tag in ("actor", "critic")}
    for tag in sd:
        sd[tag]["9.bias"] = sd[tag]["9.bias"] + 0.125 * (p % 8)
    actor, critic = MlpNet(sd["actor"], device=dev, ln_eps=actor_ln_eps), MlpNet(sd["critic"], device=dev)
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


def env_fields(env):
    return ENV_FIELDS + (SHAPED_FIELDS if env.reward_mode == "notebook" else ())


def lanes_of(env, name, group):
    t = getattr(env, name)
    return t[:, group] if name == "shaped_hist" else t[group]


def loop(env, member, frames, *, seed, step, gamma, value_reg, max_grad_norm, active0=None):
    """The loop of launches on one member: (logs [7, frames], reward [frames, L], done [frames, L], done_last)."""
    actor, critic, a_opt, c_opt = member
    n, dev = env.num_envs, env.device
    obs = env.obs if env._obs_current else env.get_state()
    done_prev = torch.zeros(n, dtype=torch.bool, device=dev) if active0 is None else ~active0.bool()
    logs = torch.empty(len(AC_LOG_KEYS), frames, dtype=torch.float64, device=dev)
    rewards, dones = [], []
    for t in range(frames):
        state = obs.clone()
        actions, _ = actor.act(state, seed=seed, step=step + t, env_id_base=env.env_id_base)
        obs, reward, done, _ = env.step(actions)
        active = ~done_prev
        # the update returns critic_loss alone: its parts and the count from the same stage on the critic
        # before its step (launches that write nothing the update reads)
        td = td_losses(critic, state, reward, obs, done, gamma=gamma, value_reg=value_reg, active=active)
        up = actor_critic_update(actor, critic, state, actions, reward, obs, done, a_opt, c_opt, gamma=gamma,
                                 value_reg=value_reg, max_grad_norm=max_grad_norm, active=active)
        assert same(td.critic_loss, up.critic_loss)
        for i, v in enumerate((up.actor_loss, up.critic_loss, td.mse, td.value_reg, td.count, up.actor_grad_norm,
                               up.critic_grad_norm)):
            logs[i, t] = v
        rewards.append(reward.clone())
        dones.append(done.clone())
        done_prev = done.clone()
    return logs, torch.stack(rewards), torch.stack(dones), done_prev.to(torch.uint8)


def assert_same_logs(got, want, where):
    """got [7, frames] of one member against the loop's."""
    for i, key in enumerate(AC_LOG_KEYS):
        assert same(got[i], want[i]), (where, key, got[i].tolist(), want[i].tolist())


def assert_same_training(ours, twin, where):
    mine, theirs = training_state(ours), training_state(twin)
    for name in mine:
        assert same(mine[name], theirs[name]), (where, name, int((bits(mine[name]) != bits(theirs[name])).sum()))


def assert_same_env(env, group, single, where):
    for name in env_fields(single):
        assert same(lanes_of(env, name, group), getattr(single, name)), (where, name)


def run_single(nets, dev, lanes, frames, *, cfg=CFG, env_kw=None, member_kw=None, active0=None, seed=11, step=3,
               **hyper):
    """actor_critic_train on a fresh learner and env against the loop on twins; everything compared."""
    hyper = {**HYPER, **hyper}
    env_kw = env_kw or {}
    ours, twin = make_member(nets, dev, **(member_kw or {})), make_member(nets, dev, **(member_kw or {}))
    env = VecDroneEnv(lanes, device=dev, config=cfg, **env_kw)
    single = VecDroneEnv(lanes, device=dev, config=cfg, **env_kw)
    env.reset()
    single.reset()
    run = actor_critic_train(env, *ours, frames, seed=seed, step=step, active0=active0, record=True, **hyper)
    want_logs, want_reward, want_done, want_last = loop(single, twin, frames, seed=seed, step=step, active0=active0,
                                                        **hyper)
    assert tuple(run.logs.shape) == (len(AC_LOG_KEYS), frames, 1) and run.logs.dtype == torch.float64
    assert_same_logs(run.logs[:, :, 0], want_logs, lanes)
    assert_same_training(ours, twin, lanes)
    assert_same_env(env, slice(0, lanes), single, lanes)
    assert run.obs is env.obs and same(run.obs, single.obs)
    assert same(run.reward, want_reward) and same(run.done, want_done) and same(run.done_last, want_last)
    assert ours[2].step_count() == frames == ours[3].step_count()
    return run, ours, env


@pytest.mark.parametrize("lanes", [1, 5, 33, 64, 128])
def test_one_member_row_counts(nets, gpu_device, lanes):
    """A single row, a ragged wave, a wave boundary, half tiles and the full tile."""
    run, _, _ = run_single(nets, gpu_device, lanes, 6)
    assert run.log("count")[0, 0].item() == lanes and bool(torch.isfinite(run.logs).all())


def test_auto_reset_notebook_timeouts(nets, gpu_device):
    """Every lane still flying at frame 4 times out there: the -500, done in the TD target, and the masked
    re-spawn frame are certain to occur."""
    lanes = 64
    run, _, env = run_single(nets, gpu_device, lanes, 12, env_kw=dict(reward_mode="notebook", max_steps=4))
    count = run.log("count")[:, 0]
    assert count[0].item() == lanes and bool((count < lanes).any())
    assert count[4].item() < lanes                 # the lanes that timed out at frame 3 re-spawn at frame 4
    assert bool(run.done[3].any()) and bool((run.reward[3] < -400).any())
    assert int(env.episode.min()) >= 2 and bool(torch.isfinite(run.logs).all())


def test_sticky_env_past_the_last_done(nets, gpu_device):
    """auto_reset off: after frame 3 every lane is done, the frames are all masked (NaN losses, zero norms),
    and the zero-gradient steps still move the parameters as the loop's do."""
    lanes, frames = 64, 7
    cfg = CFG.replace(auto_reset=False)
    run, ours, _ = run_single(nets, gpu_device, lanes, frames, cfg=cfg,
                              env_kw=dict(reward_mode="notebook", max_steps=4))
    assert bool(run.done[3:].all())
    for t in range(4, frames):
        assert run.log("count")[t, 0].item() == 0
        for key in ("actor_loss", "critic_loss", "mse", "value_reg"):
            assert bool(torch.isnan(run.log(key)[t, 0])), (t, key)
        assert run.log("actor_grad_norm")[t, 0].item() == 0.0 == run.log("critic_grad_norm")[t, 0].item()
    assert bool((run.reward[4:] == 0).all())
    # one more masked frame moves the parameters (weight decay, the decaying moments)
    before = ours[2].params.clone()
    env = VecDroneEnv(lanes, device=gpu_device, config=cfg, reward_mode="notebook", max_steps=4)
    env.reset()
    actor_critic_train(env, *ours, 1, active0=torch.zeros(lanes, dtype=torch.bool, device=gpu_device))
    assert not torch.equal(before, ours[2].params)


@pytest.mark.parametrize("field", [None, "gravity", "platform_speed"])
def test_engine_reward_and_a_config_field(nets, gpu_device, field):
    """The engine's reward, no max_steps; the reference world (compiled-in constants) and two off it."""
    cfg = CFG if field is None else cfc.config(cfc.BY_FIELD[field])
    run, _, _ = run_single(nets, gpu_device, 64, 8, cfg=cfg)
    assert bool(torch.isfinite(run.logs).all())


def test_three_members_on_one_env(nets, gpu_device):
    """A sweep: lr, gamma, value_reg and max_grad_norm per member, env_id_base set; each member against the loop
    on its own 64-lane env at env_id_base + g L."""
    members, lanes, frames, base = 3, 64, 8, 1000
    lr = [1.0, 0.5, 2.0]
    hyper = dict(gamma=[0.99, 0.9, 0.95], value_reg=[0.01, 0.0, 0.1], max_grad_norm=[0.5, 1e-3, 1e6])
    kw = dict(reward_mode="notebook", max_steps=5)
    ours = [make_member(nets, gpu_device, p, lr[p]) for p in range(members)]
    twins = [make_member(nets, gpu_device, p, lr[p]) for p in range(members)]
    pop = LearnerPopulation(ours)
    env = VecDroneEnv(members * lanes, device=gpu_device, config=CFG, env_id_base=base, **kw)
    env.reset()
    run = actor_critic_train_population(env, pop, frames, seed=7, step=2, record=True, **hyper)
    assert tuple(run.logs.shape) == (len(AC_LOG_KEYS), frames, members)
    for p in range(members):
        single = VecDroneEnv(lanes, device=gpu_device, config=CFG, env_id_base=base + p * lanes, **kw)
        single.reset()
        want = loop(single, twins[p], frames, seed=7, step=2, **{k: v[p] for k, v in hyper.items()})
        group = slice(p * lanes, (p + 1) * lanes)
        assert_same_logs(run.logs[:, :, p], want[0], p)
        assert_same_training(ours[p], twins[p], p)
        assert_same_env(env, group, single, p)
        assert same(run.reward[:, group], want[1]) and same(run.done[:, group], want[2]), p
        assert same(run.done_last[group], want[3]), p
    assert not same(run.logs[:, :, 0], run.logs[:, :, 1])


def test_more_blocks_than_cus(nets, gpu_device):
    """260 workgroups at one per CU: the later ones start when a CU is free, and nothing waits on them."""
    members, lanes, frames = 260, 4, 2
    assert torch.cuda.get_device_properties(gpu_device).multi_processor_count < members
    ours = [make_member(nets, gpu_device, p) for p in range(members)]
    twins = [make_member(nets, gpu_device, p) for p in range(members)]
    env = VecDroneEnv(members * lanes, device=gpu_device, config=CFG)
    env.reset()
    run = actor_critic_train_population(env, LearnerPopulation(ours), frames, seed=3, **HYPER)
    for p in range(members):
        single = VecDroneEnv(lanes, device=gpu_device, config=CFG, env_id_base=p * lanes)
        single.reset()
        want = loop(single, twins[p], frames, seed=3, step=0, **HYPER)
        assert_same_logs(run.logs[:, :, p], want[0], p)
        assert_same_training(ours[p], twins[p], p)
        assert_same_env(env, slice(p * lanes, (p + 1) * lanes), single, p)


@pytest.mark.parametrize("max_grad_norm,clips", [(1e-3, True), (1e6, False)])
def test_clip_and_no_clip(nets, gpu_device, max_grad_norm, clips):
    run, _, _ = run_single(nets, gpu_device, 33, 4, max_grad_norm=max_grad_norm)
    norms = torch.stack([run.log("actor_grad_norm"), run.log("critic_grad_norm")])
    assert bool((norms > max_grad_norm).all()) == clips and bool((norms < max_grad_norm).all()) != clips


def test_ln_eps_and_active0(nets, gpu_device):
    """An actor with ln_eps = 1e-3, and a first frame in which only some lanes train."""
    lanes = 64
    active0 = (torch.arange(lanes, device=gpu_device) % 3 != 0)
    run, _, _ = run_single(nets, gpu_device, lanes, 4, member_kw=dict(actor_ln_eps=1e-3), active0=active0)
    assert run.log("count")[0, 0].item() == int(active0.sum()) < lanes
    assert run.log("count")[1, 0].item() == lanes - int(run.done[0].sum())  # frame 0's mask is not carried on


def test_two_chained_calls_equal_one(nets, gpu_device):
    lanes, k = 64, 6
    kw = dict(reward_mode="notebook", max_steps=4)
    once, twice = make_member(nets, gpu_device), make_member(nets, gpu_device)
    env1 = VecDroneEnv(lanes, device=gpu_device, config=CFG, **kw)
    env2 = VecDroneEnv(lanes, device=gpu_device, config=CFG, **kw)
    env1.reset()
    env2.reset()
    whole = actor_critic_train(env1, *once, 2 * k, seed=5, step=10, record=True, **HYPER)
    first = actor_critic_train(env2, *twice, k, seed=5, step=10, record=True, **HYPER)
    second = actor_critic_train(env2, *twice, k, seed=5, step=10 + k, active0=~first.done_last.bool(), record=True,
                                **HYPER)
    assert same(torch.cat([first.logs, second.logs], dim=1), whole.logs)
    assert same(torch.cat([first.reward, second.reward]), whole.reward)
    assert same(torch.cat([first.done, second.done]), whole.done) and same(second.done_last, whole.done_last)
    assert_same_training(twice, once, "chained")
    assert_same_env(env2, slice(0, lanes), env1, "chained")
    assert bool((whole.log("count")[:, 0] < lanes).any())  # the hand-over crossed masked frames' neighbourhood


def test_refusals_launch_nothing(nets, gpu_device):
    member = make_member(nets, gpu_device)
    half = make_member(nets, gpu_device)
    split = (MlpNet(nets["actor"], device=gpu_device, compute="f16x3"), half[1])
    split = split + (AdamW(split[0]), half[3])
    env = VecDroneEnv(64, device=gpu_device, config=CFG)
    env.reset()
    before = {k: v.clone() for k, v in training_state(member).items()}
    env_before = {name: getattr(env, name).clone() for name in ENV_FIELDS}
    bad_envs = [(VecDroneEnv(64, device=gpu_device, config=CFG, precision="f64"), "precision='f32'"),
                (VecDroneEnv(64, device=gpu_device, config=CFG, ping_pong=True), "ping_pong"),
                (VecDroneEnv(64, device=gpu_device, config=CFG, reward_mode="reinforce"), "reward_mode"),
                (VecDroneEnv(129, device=gpu_device, config=CFG), "member 0: 129 lanes per member")]
    for bad, match in bad_envs:
        with pytest.raises(ValueError, match=match):
            actor_critic_train(bad, *member, 3)
        assert int(bad.steps.max()) == 0
    with pytest.raises(ValueError, match="frames must be at least 1"):
        actor_critic_train(env, *member, 0)
    with pytest.raises(ValueError, match="member 0: gamma must be finite"):
        actor_critic_train(env, *member, 3, gamma=float("nan"))
    with pytest.raises(ValueError, match="member 0: max_norm must not be NaN"):
        actor_critic_train(env, *member, 3, max_grad_norm=float("nan"))
    with pytest.raises(ValueError, match="active must be a bool or uint8 tensor of shape"):
        actor_critic_train(env, *member, 3, active0=torch.ones(63, dtype=torch.bool, device=gpu_device))
    with pytest.raises(ValueError, match="compute='f32' networks only, the actor is compute='f16x3'"):
        actor_critic_train(env, *split, 3)
    with pytest.raises(ValueError, match="65 lanes do not split into 2 equal groups"):
        actor_critic_train_population(VecDroneEnv(65, device=gpu_device, config=CFG),
                                      LearnerPopulation([member, half]), 3)
    for name, t in training_state(member).items():
        assert same(t, before[name]), name
    for name in ENV_FIELDS:
        assert same(getattr(env, name), env_before[name]), name
    assert member[2].step_count() == 0 == member[3].step_count() and split[2].step_count() == 0
