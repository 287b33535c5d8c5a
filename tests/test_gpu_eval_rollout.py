"""GPU: dd_policy_rollout_sampled.  The fused rollout with the notebooks'
temperature / greedy action selection equals the two-kernel host loop
`actor.act(env.obs, temperature=T); env.step(a)` bit for bit, and
VecDroneEnv.evaluate_policy (per-lane episode statistics, no per-frame
buffers) equals the same loop's bookkeeping.  97 lanes: three 32-drone tiles
and a tail; both computes; the engine reward and both notebook rewards."""
import ctypes

import pytest
import torch
from torch import nn

from delivery_drone_amd import EnvConfig, MlpNet, VecDroneEnv, abi

pytestmark = pytest.mark.gpu

N = 97
COMPUTE = ("f32", "f16x3")
MODES = ("engine", "notebook", "reinforce")
# evaluate_policy's episodes: with this policy, spawn seed and cap the host
# loop alone shows lanes that ended (crashed or landed) and lanes still flying
# at the cap, for every compute, reward mode and temperature below (asserted
# in the test, so neither exit can silently go uncovered)
EVAL_SEED, EVAL_MAX_STEPS = 5, 50


@pytest.fixture(scope="module")
def actors(gpu_device):
    torch.manual_seed(0)
    net = nn.Sequential(nn.Linear(15, 128), nn.LayerNorm(128), nn.ReLU(), nn.Linear(128, 128), nn.LayerNorm(128),
                        nn.ReLU(), nn.Linear(128, 64), nn.LayerNorm(64), nn.ReLU(), nn.Linear(64, 3))
    with torch.no_grad():  # the main engine fires less often: longer, more varied episodes
        net[9].bias.copy_(torch.tensor([-1.0, 0.0, 0.0]))
    return {c: MlpNet(net.state_dict(), device=gpu_device, compute=c) for c in COMPUTE}


def make_env(dev, mode, *, auto_reset, seed, max_steps):
    return VecDroneEnv(N, device=dev, config=EnvConfig(randomize_drone=True, auto_reset=auto_reset, seed=seed),
                       reward_mode=mode, max_steps=max_steps, env_id_base=1000)


@pytest.mark.parametrize("temperature", [0, 0.3])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("compute", COMPUTE)
def test_sampled_rollout_equals_act_step_loop(actors, gpu_device, compute, mode, temperature):
    frames, seed, step = 40, 9, 3
    net = actors[compute]
    fused = make_env(gpu_device, mode, auto_reset=True, seed=4, max_steps=25)
    ref = make_env(gpu_device, mode, auto_reset=True, seed=4, max_steps=25)
    fused.reset()
    ref.reset()
    used = torch.full((frames, N, 3), float("nan"), device=gpu_device)
    obs, acts, lp, rew, done = fused.policy_rollout(net, frames, seed=seed, step=step, temperature=temperature,
                                                    probs_used_out=used)
    for k in range(frames):
        assert torch.equal(obs[k], ref.obs), k
        r_used = torch.empty(N, 3, device=gpu_device)
        a, r_lp = net.act(ref.obs, seed=seed, step=step + k, env_id_base=ref.env_id_base, temperature=temperature,
                          probs_used_out=r_used)
        _, r, d, _ = ref.step(a)
        assert torch.equal(acts[k], a) and torch.equal(lp[k], r_lp) and torch.equal(used[k], r_used), k
        assert torch.equal(rew[k], r) and torch.equal(done[k], d), k
    assert torch.equal(fused.obs, ref.obs)
    for f in ("x", "y", "vx", "vy", "angle", "omega", "fuel", "px", "py", "total_reward", "status", "steps",
              "episode"):
        assert torch.equal(getattr(fused, f), getattr(ref, f)), f
    if mode != "engine":  # the notebooks' 25-frame cap: episodes ended and re-spawned inside the launch
        assert bool(done.any()) and int(fused.episode.max()) > 1


def host_episode(net, env, max_steps, temperature, seed):
    """The notebooks' evaluate_policy for every lane of a sticky-done env, on
    the two kernels: per lane, the float64 sum in frame order of the rewards
    step() returned up to and including the frame that ended its episode."""
    dev, n = env.device, env.num_envs
    total = torch.zeros(n, dtype=torch.float64, device=dev)
    steps = torch.zeros(n, dtype=torch.int32, device=dev)
    landed = torch.zeros(n, dtype=torch.bool, device=dev)
    crashed = torch.zeros(n, dtype=torch.bool, device=dev)
    fuel = env.fuel.clone()
    alive = torch.ones(n, dtype=torch.bool, device=dev)
    for k in range(max_steps):
        a, _ = net.act(env.obs, seed=seed, step=k, env_id_base=env.env_id_base, temperature=temperature)
        _, r, d, info = env.step(a)
        total = torch.where(alive, total + r.double(), total)
        steps += alive.to(torch.int32)
        fuel = torch.where(alive, env.fuel, fuel)
        ended = alive & d
        landed |= ended & info["landed"]
        crashed |= ended & info["crashed"]
        alive = alive & ~d
    return {"total_reward": total, "steps": steps, "landed": landed, "crashed": crashed, "final_fuel": fuel}


def assert_same_results(got, want):
    assert sorted(got) == ["crashed", "final_fuel", "landed", "steps", "total_reward"]
    assert got["total_reward"].dtype == torch.float64
    for key in want:
        assert torch.equal(got[key], want[key]), key


@pytest.mark.parametrize("temperature", [0, 0.3])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("compute", COMPUTE)
def test_evaluate_policy_equals_host_loop(actors, gpu_device, compute, mode, temperature):
    net = actors[compute]
    # the reference env never truncates (max_steps 0): the notebooks' evaluation has no timeout penalty
    ref = make_env(gpu_device, mode, auto_reset=False, seed=EVAL_SEED, max_steps=0)
    ref.reset()
    want = host_episode(net, ref, EVAL_MAX_STEPS, temperature, seed=13)
    ended = want["landed"] | want["crashed"]
    print(f"evaluate_policy {compute} {mode} T={temperature}: ended {int(ended.sum())} of {N}, "
          f"at the cap {int((want['steps'] == EVAL_MAX_STEPS).sum())}")
    assert bool(ended.any()), "no lane ended: the early exit is not covered"
    assert bool((~ended & (want["steps"] == EVAL_MAX_STEPS)).any()), "no lane ran to max_steps"
    assert bool((want["steps"][ended] < EVAL_MAX_STEPS).any())
    env = make_env(gpu_device, mode, auto_reset=False, seed=EVAL_SEED, max_steps=300)  # its own cap is not applied
    got = env.evaluate_policy(net, max_steps=EVAL_MAX_STEPS, temperature=temperature, seed=13)
    assert_same_results(got, want)
    assert torch.equal(env.obs, ref.obs) and torch.equal(env.status, ref.status)


@pytest.mark.parametrize("mode", ["engine", "notebook"])
def test_evaluate_policy_chunked_launches(actors, gpu_device, mode):
    net = actors["f16x3"]
    one = make_env(gpu_device, mode, auto_reset=False, seed=EVAL_SEED, max_steps=300)
    many = make_env(gpu_device, mode, auto_reset=False, seed=EVAL_SEED, max_steps=300)
    a = one.evaluate_policy(net, max_steps=EVAL_MAX_STEPS, temperature=0.3, seed=2)
    b = many.evaluate_policy(net, max_steps=EVAL_MAX_STEPS, temperature=0.3, seed=2, frames_per_launch=7)
    assert_same_results(b, a)
    assert torch.equal(one.obs, many.obs)
    assert int(a["steps"].min()) < EVAL_MAX_STEPS == int(a["steps"].max())


def test_statistics_only_launch_writes_nothing_else(actors, gpu_device):
    """With DDEpisodeStats and NULL per-frame buffers the launch writes the
    four statistics arrays (and the state and obs_final) only: they sit in
    one arena between guard bands, which stay intact."""
    net = actors["f32"]
    env = make_env(gpu_device, "engine", auto_reset=False, seed=EVAL_SEED, max_steps=300)
    twin = make_env(gpu_device, "engine", auto_reset=False, seed=EVAL_SEED, max_steps=300)
    want = twin.evaluate_policy(net, max_steps=EVAL_MAX_STEPS, temperature=0.3, seed=6)
    env.reset()
    guard = 4096
    sizes = [8 * N, 4 * N, N, 4 * N]  # ep_return f64, ep_steps i32, ep_status u8, ep_fuel f32
    offs, pos = [], guard
    for sz in sizes:
        offs.append(pos)
        pos = (pos + sz + guard + 255) // 256 * 256
    arena = torch.full((pos + guard,), 0xA5, dtype=torch.uint8, device=gpu_device)
    assert arena.data_ptr() % 8 == 0
    views = [arena[o:o + sz] for o, sz in zip(offs, sizes)]
    for v in views[:3]:
        v.zero_()
    views[3].view(torch.float32).copy_(env.fuel)
    before = arena.clone()
    stats = abi.DDEpisodeStats(*[v.data_ptr() for v in views])
    sampling = abi.DDSampling(abi.DD_SAMPLE_TEMPERED, 0.3, None)
    io = abi.DDPolicyRolloutIO()
    io.obs0 = io.obs_final = env.obs.data_ptr()
    io.seed, io.step, io.frames = 6, 0, EVAL_MAX_STEPS
    io.shaped_mode = abi.DD_SHAPED_PPO
    abi.check(abi.lib().dd_policy_rollout_sampled(ctypes.byref(env._cfg), ctypes.byref(env._state),
                                                  net.packed.data_ptr(), abi.DD_MLP_F32, ctypes.byref(io),
                                                  ctypes.byref(sampling), ctypes.byref(stats), N, None), "eval")
    torch.cuda.synchronize()
    keep = torch.ones_like(arena, dtype=torch.bool)
    for o, sz in zip(offs, sizes):
        keep[o:o + sz] = False
    assert torch.equal(arena[keep], before[keep])  # the guard bands
    assert torch.equal(views[0].view(torch.float64), want["total_reward"])
    assert torch.equal(views[1].view(torch.int32), want["steps"])
    assert torch.equal((views[2] & abi.DD_ST_LANDED) != 0, want["landed"])
    assert torch.equal((views[2] & abi.DD_ST_CRASHED) != 0, want["crashed"])
    assert torch.equal(views[3].view(torch.float32), want["final_fuel"])
    assert torch.equal(env.obs, twin.obs) and torch.equal(env.status, twin.status)
    # ep_status: the status of the frame that ended the episode (sticky afterwards), 0 for a lane still flying
    done = (twin.status & abi.DD_ST_DONE) != 0
    assert torch.equal(views[2], torch.where(done, twin.status, torch.zeros_like(twin.status)))


def test_evaluate_policy_needs_sticky_done(actors, gpu_device):
    env = make_env(gpu_device, "engine", auto_reset=True, seed=1, max_steps=300)
    with pytest.raises(ValueError, match="auto_reset"):
        env.evaluate_policy(actors["f32"])
    sticky = make_env(gpu_device, "engine", auto_reset=False, seed=1, max_steps=300)
    with pytest.raises(ValueError):
        sticky.evaluate_policy(actors["f32"], temperature=-1.0)
