"""GPU: dd_step at the batch sizes and done-lane patterns where a wave takes
another path through the step kernel, against the C oracle.

What varies per wave in step_tile / finish_lane (csrc/step.hip):
* the observation flush: a wave whose 64 rows all exist and whose rows are
  16-byte aligned takes flush_obs_wave_full (unrolled), every other wave the
  general flush_obs_wave (a ragged batch's last wave; any wave when the
  stepped range starts at a lane that is no multiple of 4);
* the done lanes' branch: re-spawn (auto_reset) or sticky, skipped by waves
  with no done lane; the live lanes' frame, skipped by waves with none.

Sizes: 1 and 63 (one partial wave), 64 (one full wave in a partial tile), 65,
256 and 512 (whole tiles: every wave full), 257 (one lane over).  Done-lane
patterns, written into `status` before the first step: none, all, lane 0,
lane 63, lane 64 (the second wave's first), alternating, one per wave.  Three
consecutive steps, so a lane re-spawns and then flies; every sixteenth lane
starts just above the ground and crashes on the first step, so episodes end
(done_idx) and, under auto_reset, lanes the kernel itself marked done re-spawn.

The headline combination (f32, engine reward, in place, obs written, no
done_idx, random spawn, auto_reset) runs every size x pattern; every other
value of each axis (sticky, f64, notebook / reinforce reward, ping-pong, no
obs, done_idx, fixed spawn) runs every pattern at 257 lanes, the size with
both kinds of wave.

Bounds, as tests/test_gpu_step_matrix.py's anchors (imported): done, status,
steps, episode, fuel exact; the other fields and rewards reward_close (1 f32
ulp / 4 f64 ulps + 1e-12); obs within 1 f32 ulp of the oracle's double row;
the PPO history's NaN slots equal and its values reward_close in f64.  Paths
that must not change a result are compared bit for bit: ping-pong, done_idx
and no-obs against the plain run; 256 lanes alone against the first 256 of
257; a range starting at lane 1 (unaligned rows) against the whole batch."""
import functools

import numpy as np
import pytest
import torch

import golden_data as gd
from delivery_drone_amd import EnvConfig, VecDroneEnv
from oracle import oracle as ora
from test_gpu_eval_oracle import reward_close
from test_gpu_notebook_rollout import bits_equal
from test_gpu_parity import host

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 256, 257, 512)
N_MAX, PRE_FRAMES, FRAMES, CAP = 512, 48, 3, 300
ENV_ID_BASE = (1 << 33) + 5
STATE_FIELDS = gd.FLOAT_FIELDS + ("status", "steps", "episode")
EXACT_FIELDS = ("fuel", "status", "steps", "episode")
PATTERNS = {
    "none": lambda lane: np.zeros(lane.size, bool),
    "all": lambda lane: np.ones(lane.size, bool),
    "lane0": lambda lane: lane == 0,
    "lane63": lambda lane: lane == 63,
    "lane64": lambda lane: lane == 64,
    "alternating": lambda lane: lane % 2 == 1,
    "one_per_wave": lambda lane: lane % 64 == (lane // 64) * 7 % 64,
}
HEADLINE = dict(auto_reset=True, storage="f32", mode="engine", ping_pong=False, write_obs=True, done_idx=False,
                randomize=True)
AXES = [dict(auto_reset=False), dict(storage="f64"), dict(mode="notebook"), dict(mode="reinforce"),
        dict(mode="notebook", auto_reset=False), dict(ping_pong=True), dict(write_obs=False), dict(done_idx=True),
        dict(randomize=False), dict(storage="f64", ping_pong=True, done_idx=True)]


def config_for(auto_reset, randomize):
    return EnvConfig(randomize_drone=randomize, randomize_platform=randomize, auto_reset=auto_reset, seed=7)


@functools.lru_cache(maxsize=None)
def flying_state(storage, randomize):
    """N_MAX lanes (keyed by env id: the first n are the n-lane batch) after
    PRE_FRAMES random frames on the oracle, and the test's actions."""
    o = ora.OracleEnv(N_MAX, precision=storage, config=config_for(True, randomize), env_id_base=ENV_ID_BASE)
    o.reset()
    rng = np.random.default_rng(3)
    for a in rng.integers(0, 8, (PRE_FRAMES, N_MAX)).astype(np.uint8):
        o.step(a)
    st = o.state_dict()
    st["status"][:] = 0  # (a lane that ended in the warm-up flies on: the pattern alone says who is done)
    low = np.arange(N_MAX) % 16 == 4  # falling fast just above the ground: these crash on the first step
    st["y"][low], st["vy"][low] = 545.0, 8.0
    return st, rng.integers(0, 8, (FRAMES, N_MAX)).astype(np.uint8)


def start_state(n, pattern, storage, randomize):
    st, acts = flying_state(storage, randomize)
    st = {k: v[:n].copy() for k, v in st.items()}
    st["status"][PATTERNS[pattern](np.arange(n))] = gd.ST_DONE | gd.ST_CRASHED
    return st, acts[:, :n]


def make_env(dev, n, *, auto_reset, storage, mode, ping_pong, randomize, **_):
    return VecDroneEnv(n, device=dev, config=config_for(auto_reset, randomize), precision=storage, reward_mode=mode,
                       max_steps=CAP, env_id_base=ENV_ID_BASE, ping_pong=ping_pong)


def run_gpu(dev, n, pattern, lanes=None, **case):
    """FRAMES steps; per frame the outputs, every state field, the history,
    the done_idx set.  lanes: step only that range (rows then start there)."""
    st, acts = start_state(n, pattern, case["storage"], case["randomize"])
    env = make_env(dev, n, **case)
    env.load_state_dict({f: torch.as_tensor(v) for f, v in st.items()})
    rec = {"hist0": host(env.shaped_hist).copy() if case["mode"] == "notebook" else None, "frames": []}
    sl = lanes or slice(0, n)
    for t in range(FRAMES):
        env.obs.fill_(-7.0)
        obs, r, d, info = env.step(torch.as_tensor(acts[t, sl], device=dev), collect_done_idx=case["done_idx"],
                                   write_obs=case["write_obs"], lanes=lanes)
        if lanes is not None:  # (the whole buffers, so that lane indices are the batch's)
            r, d = env.reward, env.done
        f = {"obs": env.obs.clone(), "reward": r.clone(), "done": d.clone()}
        if case["mode"] != "engine":
            f.update(engine_reward=info["engine_reward"].clone(), engine_done=info["engine_done"].clone())
        if case["done_idx"]:
            f["done_idx"] = np.sort(host(info["done_idx"]))
        f["state"] = {k: getattr(env, k).clone() for k in STATE_FIELDS}
        if env.shaped_hist is not None:
            f["state"]["shaped_hist"] = env.shaped_hist.clone()
        rec["frames"].append(f)
    return rec


_ORACLE = {}


def run_oracle(n, pattern, hist0, *, auto_reset, storage, mode, randomize, **_):
    key = (n, pattern, auto_reset, storage, mode, randomize)
    if key not in _ORACLE:
        st, acts = start_state(n, pattern, storage, randomize)
        o = ora.OracleEnv(n, precision=storage, config=config_for(auto_reset, randomize), env_id_base=ENV_ID_BASE)
        o.load_state_dict(st)
        hist = np.ascontiguousarray(hist0, np.float64).copy() if mode == "notebook" else None
        frames = []
        for t in range(FRAMES):
            before = o.status.copy()
            if mode == "engine":
                _, r, d, obs64 = o.step(acts[t])
                f = {"reward": r, "done": d}
            else:
                _, r, d, obs64, sr, sd = o.step_shaped(acts[t], hist, CAP, mode)
                f = {"reward": sr, "done": sd, "engine_reward": r, "engine_done": d}
            f["obs"] = obs64
            f["ended"] = np.flatnonzero(((before & gd.ST_DONE) == 0) & ((o.status & gd.ST_DONE) != 0))
            f["state"] = o.state_dict()
            if hist is not None:
                f["state"]["shaped_hist"] = hist.copy()
            frames.append({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in f.items()})
        _ORACLE[key] = frames
    return _ORACLE[key]


def assert_matches_oracle(rec, want, case, what):
    storage = case["storage"]
    for t, (g, w) in enumerate(zip(rec["frames"], want)):
        at = f"{what} frame {t}"
        for name in ("done", "engine_done"):
            if name in w:
                np.testing.assert_array_equal(host(g[name]), w[name], err_msg=f"{at} {name}")
        for name in ("reward", "engine_reward"):
            if name in w:
                ok = reward_close(host(g[name]), w[name], storage)
                assert ok.all(), (at, name, np.flatnonzero(~ok)[:5])
        for f in STATE_FIELDS:
            got, ref = host(g["state"][f]), w["state"][f]
            if f in EXACT_FIELDS:
                np.testing.assert_array_equal(got, ref, err_msg=f"{at} {f}")
            else:
                ok = reward_close(got, ref, storage)
                assert ok.all(), (at, f, np.flatnonzero(~ok)[:5])
        if case["write_obs"]:
            ok = gd.f32_close(host(g["obs"]), w["obs"], 1.0)
            assert ok.all(), (at, "obs", np.argwhere(~ok)[:5])
        else:
            assert (host(g["obs"]) == -7.0).all(), (at, "obs written with write_obs=False")
        if "shaped_hist" in w["state"]:
            got, ref = host(g["state"]["shaped_hist"]), w["state"]["shaped_hist"]
            np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=f"{at} history NaN slots")
            assert reward_close(np.nan_to_num(got), np.nan_to_num(ref), "f64").all(), (at, "shaped_hist")
        if case["done_idx"]:
            np.testing.assert_array_equal(g["done_idx"], w["ended"], err_msg=f"{at} done_idx")


def assert_same_bits(got, want, what, lanes=slice(None), skip=()):
    for t, (g, w) in enumerate(zip(got["frames"], want["frames"])):
        for k in w:
            if k in skip or k == "done_idx" or k not in g:
                continue
            pairs = w[k].items() if k == "state" else [(k, w[k])]
            for name, ref in pairs:
                have = g[k][name] if k == "state" else g[k]
                assert bits_equal(have[..., lanes] if name != "obs" else have[lanes],
                                  ref[..., lanes] if name != "obs" else ref[lanes]), f"{what}: {name} frame {t}"


def check(dev, n, pattern, case):
    what = f"n={n} {pattern} " + " ".join(f"{k}={v}" for k, v in case.items() if HEADLINE[k] != v)
    rec = run_gpu(dev, n, pattern, **case)
    assert_matches_oracle(rec, run_oracle(n, pattern, rec["hist0"], **case), case, what)
    return rec


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_headline_combination(gpu_device, n, pattern):
    rec = check(gpu_device, n, pattern, HEADLINE)
    if pattern == "all":  # every lane re-spawned on the first step, and flew on the next
        assert (host(rec["frames"][0]["state"]["steps"]) == 0).all()
        assert (host(rec["frames"][1]["state"]["steps"]) == 1).all()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("axis", AXES, ids=lambda a: ",".join(f"{k}={v}" for k, v in a.items()))
def test_each_axis(gpu_device, axis, pattern):
    case = {**HEADLINE, **axis}
    rec = check(gpu_device, 257, pattern, case)
    if case["done_idx"] and pattern != "all":  # (all: no live lane, the list must be empty)
        assert sum(len(f["done_idx"]) for f in rec["frames"]) >= 8, "too few episodes ended for done_idx to be checked"
    if case["ping_pong"] or case["done_idx"] or not case["write_obs"]:  # these change no result
        plain = run_gpu(gpu_device, 257, pattern, **{**case, "ping_pong": False, "done_idx": False, "write_obs": True})
        assert_same_bits(rec, plain, f"{axis} {pattern}", skip=() if case["write_obs"] else ("obs",))


@pytest.mark.parametrize("pattern", PATTERNS)
def test_whole_tiles_equal_the_ragged_batch(gpu_device, pattern):
    """256 lanes (every wave full) against the first 256 of 257 (and the 257th's wave partial)."""
    assert_same_bits(run_gpu(gpu_device, 256, pattern, **HEADLINE), run_gpu(gpu_device, 257, pattern, **HEADLINE),
                     pattern, lanes=slice(0, 256))


@pytest.mark.parametrize("pattern", ["none", "alternating", "one_per_wave"])
def test_unaligned_rows_equal_the_aligned_ones(gpu_device, pattern):
    """Lanes 1..256 of 257 stepped as a range: four full waves whose rows start
    4 bytes off a 16-byte boundary (the general flush), against the whole batch."""
    part = run_gpu(gpu_device, 257, pattern, lanes=slice(1, 257), **HEADLINE)
    assert_same_bits(part, run_gpu(gpu_device, 257, pattern, **HEADLINE), pattern, lanes=slice(1, 257))
