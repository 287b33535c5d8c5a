"""GPU: the per-lane episode statistics of dd_policy_rollout_sampled
(DDEpisodeStats) against the CPU oracle, and the promises of
include/dronestep.h that VecDroneEnv never exercises.  Every launch goes
through the C ABI with the four statistics pointers AND the per-frame
buffers set.

Reference: the launch's recorded actions replayed frame by frame on an
OracleEnv of the same config, precision and env id base (its spawn is
bit-equal to the GPU's: test_gpu_parity.py), with `step` / `step_shaped`; the
PPO reward's [2, N] history starts from the env's shaped_hist after reset.
The oracle's statistics are formed in numpy float64.

Bounds, all taken from what the suite already allows between the kernels and
the oracle (test_gpu_parity.py, test_gpu_rollout.py):
* done[k], ep_steps, ep_status (landed / crashed with it) : exact.
* ep_fuel: exact.  Fuel only ever loses whole units (2 main, 1 side) from 1000.
* reward[k]: gd.f32_close(got, ref, 1.0) with f32 storage (1 float32 ulp of
  the oracle's value), f64_close(got, ref) of test_gpu_parity.py with f64
  storage (4 double ulps + 1e-12).
* ep_return: |ep_return - the oracle's float64 sum| <= the sum of those
  per-frame allowances over the frames the lane counted (`allowance` below is
  the same two formulas).  Both sides add in frame order in double; with equal
  rewards the sums are equal, and the rounding of a double addition (half an
  ulp of a partial sum) is far inside an allowance.
* ep_return / ep_steps against the same launch's own reward[k] / done[k]
  (float64 sum in frame order up to and including the first done frame), the
  sticky-done twin of an auto_reset env, the host loop with max_steps, and
  the carry-in sums: bit for bit.

Coverage conditions (some lane landed, some crashed within the cap, some ran
to the cap, some episode ended before it) are asserted on the oracle's replay, or on the host loop where
that is the reference.  Tempered cases draw with DRAW_SEED.

The argument error "a DDEpisodeStats with one to three pointers set" is
covered, for all fourteen subsets, by tests/test_eval_abi.py."""
import ctypes

import numpy as np
import pytest
import torch

import golden_data as gd
from delivery_drone_amd import abi
from oracle import oracle as ora
from test_gpu_eval_matrix import ENV_ID_BASE, assert_covered, make_env
from test_gpu_eval_rollout import actors  # noqa: F401 - a fixture
from test_gpu_parity import f64_close, host

pytestmark = pytest.mark.gpu

N, CAP = 515, 50
DRAW_SEED = 13
STAT_KEYS = ("ret", "steps", "status", "fuel")
STATE_FIELDS = gd.FLOAT_FIELDS + ("status", "steps", "episode")


def new_stats(env):
    """Zeroed accumulators, as evaluate_policy starts them."""
    n, dev = env.num_envs, env.device
    return {"ret": torch.zeros(n, dtype=torch.float64, device=dev),
            "steps": torch.zeros(n, dtype=torch.int32, device=dev),
            "status": torch.zeros(n, dtype=torch.uint8, device=dev), "fuel": env.fuel.clone()}


def launch(env, net, frames, temperature, seed, stats, *, max_steps=0, obs_final="env"):
    """dd_policy_rollout_sampled with statistics and actions / reward / done
    (engine_reward / engine_done too in the notebook modes) recorded."""
    n, dev = env.num_envs, env.device
    out = {"actions": torch.full((frames, n), 0xEE, dtype=torch.uint8, device=dev),
           "reward": torch.full((frames, n), float("nan"), dtype=env.float_dtype, device=dev),
           "done": torch.full((frames, n), 0xEE, dtype=torch.uint8, device=dev)}
    io = abi.DDPolicyRolloutIO()
    io.obs0 = env.obs.data_ptr()
    io.obs_final = env.obs.data_ptr() if isinstance(obs_final, str) else \
        (obs_final.data_ptr() if obs_final is not None else None)
    if env.reward_mode != "engine":
        out["engine_reward"] = torch.full_like(out["reward"], float("nan"))
        out["engine_done"] = torch.full_like(out["done"], 0xEE)
        io.engine_reward, io.engine_done = out["engine_reward"].data_ptr(), out["engine_done"].data_ptr()
    if frames > 0:
        io.actions, io.reward, io.done = out["actions"].data_ptr(), out["reward"].data_ptr(), out["done"].data_ptr()
    io.seed, io.step, io.frames, io.max_steps = seed, 0, frames, max_steps
    io.shaped_hist = env.shaped_hist.data_ptr() if env.shaped_hist is not None else None
    io.shaped_mode = env._shaped_mode
    sampling = abi.DDSampling(abi.sampling_mode(temperature), float(temperature), None)
    st = abi.DDEpisodeStats(*[stats[k].data_ptr() for k in STAT_KEYS])
    compute = {"f32": abi.DD_MLP_F32, "f16x3": abi.DD_MLP_F16X3}[net.compute]
    abi.check(abi.lib().dd_policy_rollout_sampled(ctypes.byref(env._cfg), ctypes.byref(env._state),
                                                  net.packed.data_ptr(), compute, ctypes.byref(io),
                                                  ctypes.byref(sampling), ctypes.byref(st), n, env._stream()),
              "dd_policy_rollout_sampled")
    torch.cuda.synchronize()
    return out


def episode_of(reward, done, total0=None, steps0=None, alive0=None):
    """First-episode return and length from a launch's own [frames, N]
    buffers: the float64 sum in frame order of reward[k], up to and including
    the first frame whose done[k] is set.  Optionally from carried-in values."""
    frames, n = reward.shape
    total = torch.zeros(n, dtype=torch.float64, device=reward.device) if total0 is None else total0.clone()
    steps = torch.zeros(n, dtype=torch.int32, device=reward.device) if steps0 is None else steps0.clone()
    alive = torch.ones(n, dtype=torch.bool, device=reward.device) if alive0 is None else alive0.clone()
    for k in range(frames):
        total = torch.where(alive, total + reward[k].double(), total)
        steps = steps + alive.to(torch.int32)
        alive = alive & (done[k] == 0)
    return total, steps


def allowance(ref, storage):
    """The per-frame reward allowance as an array: the right-hand sides of
    gd.f32_close(., ref, 1.0) and of test_gpu_parity.f64_close(., ref)."""
    ref = np.asarray(ref, np.float64)
    if storage == "f64":
        return 4 * np.spacing(np.abs(ref)) + 1e-12
    return 1.0 * gd.ulp32(ref)


def reward_close(got, ref, storage):
    return f64_close(got, ref) if storage == "f64" else gd.f32_close(got, ref, 1.0)


def oracle_replay(env, actions, hist0, max_steps):
    """The recorded actions on the C oracle; per-frame outputs and the
    statistics of each lane's first episode, in numpy float64."""
    frames, n = actions.shape
    mode, storage = env.reward_mode, env.precision
    o = ora.OracleEnv(n, precision=storage, config=env.config, env_id_base=env.env_id_base)
    o.reset()
    hist = np.ascontiguousarray(hist0, dtype=np.float64).copy() if mode == "notebook" else None
    rep = {k: np.zeros((frames, n), np.float64) for k in ("reward", "engine_reward")}
    rep.update({k: np.zeros((frames, n), bool) for k in ("done", "engine_done")})
    total, bound = np.zeros(n), np.zeros(n)
    steps, status = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    fuel, alive = o.fuel.copy(), np.ones(n, bool)
    for k in range(frames):
        if mode == "engine":
            _, r, d, _ = o.step(actions[k])
            sr, sd = r, d
        else:
            _, r, d, _, sr, sd = o.step_shaped(actions[k], hist, max_steps, mode)
        rep["reward"][k], rep["done"][k], rep["engine_reward"][k], rep["engine_done"][k] = sr, sd, r, d
        total = np.where(alive, total + sr.astype(np.float64), total)
        bound = np.where(alive, bound + allowance(sr, storage), bound)
        steps += alive
        fuel = np.where(alive, o.fuel, fuel)
        status = np.where(alive & sd, o.status | abi.DD_ST_DONE, status).astype(np.uint8)
        alive = alive & ~sd
    rep.update(ret=total, bound=bound, steps=steps, status=status, fuel=fuel)
    return rep


def oracle_results(rep):
    """The oracle's statistics under evaluate_policy's keys (for assert_covered)."""
    return {"landed": torch.as_tensor((rep["status"] & abi.DD_ST_LANDED) != 0),
            "crashed": torch.as_tensor((rep["status"] & abi.DD_ST_CRASHED) != 0),
            "steps": torch.as_tensor(rep["steps"])}


def check_vs_oracle(env, out, stats, hist0, max_steps, what):
    """Per-frame outputs and statistics of one launch against its replay."""
    storage = env.precision
    rep = oracle_replay(env, host(out["actions"]), hist0, max_steps)
    np.testing.assert_array_equal(host(out["done"]), rep["done"].astype(np.uint8), err_msg=what)
    ok = reward_close(host(out["reward"]), rep["reward"], storage)
    assert ok.all(), (what, "reward", np.argwhere(~ok)[:5])
    if "engine_reward" in out:
        np.testing.assert_array_equal(host(out["engine_done"]), rep["engine_done"].astype(np.uint8), err_msg=what)
        ok = reward_close(host(out["engine_reward"]), rep["engine_reward"], storage)
        assert ok.all(), (what, "engine_reward", np.argwhere(~ok)[:5])
    np.testing.assert_array_equal(host(stats["steps"]), rep["steps"], err_msg=what)
    np.testing.assert_array_equal(host(stats["status"]), rep["status"], err_msg=what)
    assert stats["fuel"].dtype == env.float_dtype
    np.testing.assert_array_equal(host(stats["fuel"]), rep["fuel"], err_msg=what)
    err = np.abs(host(stats["ret"]) - rep["ret"])
    print(f"{what}: worst |ep_return - oracle| {err.max():.3e}, its bound {rep['bound'][err.argmax()]:.3e}; "
          f"smallest bound {rep['bound'].min():.3e}")
    assert (err <= rep["bound"]).all(), (what, np.flatnonzero(err > rep["bound"])[:5])
    return rep


def assert_own_buffers(out, stats, what):
    total, steps = episode_of(out["reward"], out["done"])
    assert torch.equal(stats["ret"], total), what
    assert torch.equal(stats["steps"], steps), what


def _oracle_cases():
    cases = []
    for i, storage in enumerate(("f32", "f64")):
        for j, physics in enumerate(("reference", "wind")):
            for m, mode in enumerate(("engine", "notebook", "reinforce")):
                for t, temperature in enumerate((0, 0.3)):
                    compute = ("f32", "f16x3")[(i + j + m + t) % 2]
                    cases.append(pytest.param(storage, compute, physics, mode, temperature,
                                              id=f"{storage}-{compute}-{physics}-{mode}-T{temperature}"))
    return cases


@pytest.mark.parametrize("storage,compute,physics,mode,temperature", _oracle_cases())
def test_statistics_equal_the_oracles_episode(actors, gpu_device, storage, compute, physics, mode, temperature):
    what = f"eval vs oracle {storage} {compute} {physics} {mode} T={temperature}"
    net = actors[compute]
    env = make_env(gpu_device, N, storage, physics, mode, auto_reset=False, max_steps=300)
    env.reset()
    hist0 = host(env.shaped_hist) if mode == "notebook" else None
    stats = new_stats(env)
    out = launch(env, net, CAP, temperature, DRAW_SEED, stats)
    rep = check_vs_oracle(env, out, stats, hist0, 0, what)
    assert_covered(oracle_results(rep), CAP, what)
    assert_own_buffers(out, stats, what)
    landed = (rep["status"] & abi.DD_ST_LANDED) != 0
    if mode != "engine":  # the notebook rewards' landing terminal is in the lanes' returns
        assert (rep["reward"][rep["steps"][landed] - 1, np.flatnonzero(landed)] > 400).all()


AUTO_CASES = [pytest.param("f32", "f16x3", "reference", id="f32-f16x3-reference"),
              pytest.param("f64", "f32", "wind", id="f64-f32-wind")]


@pytest.mark.parametrize("mode,io_max_steps", [("engine", 0), ("notebook", 25)])
@pytest.mark.parametrize("storage,compute,physics", AUTO_CASES)
def test_statistics_on_an_auto_reset_env(actors, gpu_device, storage, compute, physics, mode, io_max_steps):
    """'Its first episode is counted once, whatever the env does after it':
    on an auto_reset env the four arrays equal those of a sticky-done twin,
    while the per-frame rewards go on into the next episodes."""
    frames, net = 60, actors[compute]
    auto = make_env(gpu_device, N, storage, physics, mode, auto_reset=True, max_steps=300)
    sticky = make_env(gpu_device, N, storage, physics, mode, auto_reset=False, max_steps=300)
    outs, stats = {}, {}
    for name, env in (("auto", auto), ("sticky", sticky)):
        env.reset()
        stats[name] = new_stats(env)
        outs[name] = launch(env, net, frames, 0.3, DRAW_SEED, stats[name], max_steps=io_max_steps)
    for k in STAT_KEYS:
        assert torch.equal(stats["auto"][k], stats["sticky"][k]), k
    assert_own_buffers(outs["auto"], stats["auto"], "auto_reset")
    assert_own_buffers(outs["sticky"], stats["sticky"], "sticky")
    assert int(auto.episode.max()) > 1 and int(sticky.episode.max()) == 1
    ended = (stats["sticky"]["status"] & abi.DD_ST_DONE) != 0
    assert bool(ended.any())
    if io_max_steps:  # every lane ended by the cap and re-spawned inside the launch
        assert bool(ended.all()) and int(auto.episode.min()) > 1 and int(stats["sticky"]["steps"].max()) == io_max_steps
    # frames up to the one that ended the first episode agree; two frames later the
    # re-spawned lane is flying again (the frame in between is the spawn: reward 0)
    k = torch.arange(frames, device=gpu_device)[:, None]
    last = (stats["sticky"]["steps"] - 1)[None, :]
    first_episode = k <= last
    assert torch.equal(outs["auto"]["reward"][first_episode], outs["sticky"]["reward"][first_episode])
    later = ended[None, :] & (k > last + 1)
    assert bool(later.any())
    assert bool((outs["sticky"]["reward"][later] == 0).all())
    changing = (outs["auto"]["reward"] != 0) & later
    assert bool(changing.any(dim=0)[ended & (stats["sticky"]["steps"] < frames - 2)].all())


TIMEOUT_CASES = [pytest.param("f32", "f32", "reference", 0, id="f32-f32-reference-T0"),
                 pytest.param("f64", "f16x3", "wind", 0.3, id="f64-f16x3-wind-T0.3")]


def host_loop(net, env, frames, temperature, seed):
    """The statistics on the two kernels: act + step on a sticky-done env,
    the env's own max_steps timeout included."""
    n, dev = env.num_envs, env.device
    st = new_stats(env)
    alive = torch.ones(n, dtype=torch.bool, device=dev)
    for k in range(frames):
        a, _ = net.act(env.obs, seed=seed, step=k, env_id_base=env.env_id_base, temperature=temperature)
        _, r, d, _ = env.step(a)
        st["ret"] = torch.where(alive, st["ret"] + r.double(), st["ret"])
        st["steps"] = st["steps"] + alive.to(torch.int32)
        st["fuel"] = torch.where(alive, env.fuel, st["fuel"])
        st["status"] = torch.where(alive & d, env.status | abi.DD_ST_DONE, st["status"])
        alive = alive & ~d
    return st


@pytest.mark.parametrize("mode", ["notebook", "reinforce"])
@pytest.mark.parametrize("storage,compute,physics,temperature", TIMEOUT_CASES)
def test_statistics_with_the_collection_timeout(actors, gpu_device, storage, compute, physics, temperature, mode):
    """io->max_steps = 25 next to the statistics: the timeout ends the episode
    through the notebook's done, with its -500 in the return."""
    frames, cap, net = 40, 25, actors[compute]
    what = f"timeout {storage} {compute} {physics} {mode} T={temperature}"
    ref = make_env(gpu_device, N, storage, physics, mode, auto_reset=False, max_steps=cap)
    ref.reset()
    want = host_loop(net, ref, frames, temperature, DRAW_SEED)
    timed_out = (want["steps"] == cap) & (want["status"] == abi.DD_ST_DONE)
    print(f"{what}: timed out {int(timed_out.sum())}, ended earlier {int((want['steps'] < cap).sum())}")
    assert bool(timed_out.any()) and bool((want["steps"] < cap).any())
    assert int(want["steps"].max()) == cap
    # the cap of the call applies, not the env's own
    env = make_env(gpu_device, N, storage, physics, mode, auto_reset=False, max_steps=300)
    env.reset()
    hist0 = host(env.shaped_hist) if mode == "notebook" else None
    stats = new_stats(env)
    out = launch(env, net, frames, temperature, DRAW_SEED, stats, max_steps=cap)
    for k in STAT_KEYS:
        assert torch.equal(stats[k], want[k]), k
    for f in STATE_FIELDS:
        assert torch.equal(getattr(env, f), getattr(ref, f)), f
    assert torch.equal(env.obs, ref.obs)
    assert_own_buffers(out, stats, what)
    # a lane still flying at frame 25: that frame carries the -500 and the done, and nothing after it counts
    assert bool((out["reward"][cap - 1][timed_out] < -400).all()) and bool((out["done"][cap - 1][timed_out] == 1).all())
    assert bool((out["reward"][cap:] == 0).all()) and bool((out["done"][cap:] == 1).all())
    rep = check_vs_oracle(env, out, stats, hist0, cap, what)
    o_timed = (rep["steps"] == cap) & (rep["status"] == abi.DD_ST_DONE)
    assert o_timed.any() and (rep["steps"] < cap).any()
    assert (rep["reward"][cap - 1][o_timed] < -400).all()


CARRY_CASES = [pytest.param("f32", "f32", "reference", "engine", id="f32-f32-reference-engine"),
               pytest.param("f64", "f16x3", "moving", "reinforce", id="f64-f16x3-moving-reinforce")]


@pytest.mark.parametrize("storage,compute,physics,mode", CARRY_CASES)
def test_statistics_carry_in(actors, gpu_device, storage, compute, physics, mode):
    """The accumulators are in/out: a lane whose ep_status carries DD_ST_DONE
    is left alone, the others add this launch's episode to what they held."""
    net = actors[compute]
    env = make_env(gpu_device, N, storage, physics, mode, auto_reset=False, max_steps=300)
    twin = make_env(gpu_device, N, storage, physics, mode, auto_reset=False, max_steps=300)
    env.reset()
    twin.reset()
    zero = new_stats(twin)
    out_t = launch(twin, net, CAP, 0.3, DRAW_SEED, zero)
    assert_own_buffers(out_t, zero, "zero-started twin")
    assert_covered({"landed": (zero["status"] & abi.DD_ST_LANDED) != 0,
                    "crashed": (zero["status"] & abi.DD_ST_CRASHED) != 0, "steps": zero["steps"]}, CAP,
                   f"carry-in twin {storage} {compute} {physics} {mode}")
    lane = torch.arange(N, device=gpu_device)
    closed = lane % 3 == 1  # these lanes' episodes ended in an earlier launch
    pre = new_stats(env)
    pre["ret"].copy_(lane.double() * 0.37 - 40.1)
    pre["steps"].copy_((7 + lane % 5).to(torch.int32))
    pre["status"][closed] = abi.DD_ST_DONE | abi.DD_ST_CRASHED
    pre["fuel"][closed] = 123.0
    before = {k: v.clone() for k, v in pre.items()}
    out_e = launch(env, net, CAP, 0.3, DRAW_SEED, pre)
    for k in ("actions", "reward", "done"):  # the lanes themselves play the same frames
        assert torch.equal(out_e[k], out_t[k]), k
    for f in STATE_FIELDS:
        assert torch.equal(getattr(env, f), getattr(twin, f)), f
    for k in STAT_KEYS:
        assert torch.equal(pre[k][closed], before[k][closed]), k
    total, steps = episode_of(out_t["reward"], out_t["done"], before["ret"], before["steps"])
    assert torch.equal(pre["ret"][~closed], total[~closed])
    assert torch.equal(pre["steps"][~closed], steps[~closed])
    assert torch.equal(pre["steps"][~closed], (before["steps"] + zero["steps"])[~closed])
    assert torch.equal(pre["status"][~closed], zero["status"][~closed])
    assert torch.equal(pre["fuel"][~closed], zero["fuel"][~closed])


NO_FRAMES_CASES = [pytest.param("f32", "f16x3", "reference", id="f32-f16x3-reference"),
                   pytest.param("f64", "f32", "gravity", id="f64-f32-gravity")]


@pytest.mark.parametrize("storage,compute,physics", NO_FRAMES_CASES)
def test_no_frames_with_statistics(actors, gpu_device, storage, compute, physics):
    """frames = 0: with obs_final the accumulators come back unchanged and the
    observation is written from the state; with obs_final NULL nothing is."""
    net = actors[compute]
    env = make_env(gpu_device, N, storage, physics, "notebook", auto_reset=False, max_steps=300)
    twin = make_env(gpu_device, N, storage, physics, "notebook", auto_reset=False, max_steps=300)
    env.reset()
    twin.reset()
    lane = torch.arange(N, device=gpu_device)
    stats = new_stats(env)
    stats["ret"].copy_(lane.double() * 1.25 + 0.1)
    stats["steps"].copy_((3 + lane % 11).to(torch.int32))
    stats["status"].copy_((lane % 2).to(torch.uint8) * (abi.DD_ST_DONE | abi.DD_ST_LANDED))
    stats["fuel"].copy_(1000 - lane % 17)
    before = {k: v.clone() for k, v in stats.items()}
    state = {f: getattr(env, f).clone() for f in STATE_FIELDS}
    obs0, hist = env.obs.clone(), env.shaped_hist.clone()

    def unchanged():
        return (all(torch.equal(stats[k], before[k]) for k in STAT_KEYS)
                and all(torch.equal(getattr(env, f), state[f]) for f in STATE_FIELDS)
                and torch.equal(env.obs, obs0)
                and torch.equal(env.shaped_hist.view(torch.int64), hist.view(torch.int64)))

    launch(env, net, 0, 0.3, DRAW_SEED, stats, obs_final=None)
    assert unchanged()
    final = torch.full((N, 15), float("nan"), device=gpu_device)
    launch(env, net, 0, 0.3, DRAW_SEED, stats, obs_final=final)
    assert unchanged()
    assert torch.equal(final, obs0) and torch.equal(final, twin.get_state())
