"""GPU: every world constant a call supplies, moved alone off config.py's
value, through every path that evaluates a frame.

The cases and the state set are tests/config_field_cases.py's: one entry per
EnvConfig field a kernel reads (44), 515 lanes placed so that one frame
reaches every predicate, at most 3 frames.  tests/test_config_fields_cpu.py
shows on the oracle that each entry changes the compared outputs on at least
8 lanes, so a kernel that read csrc/frame.h's reference_config() for an
entry's field where it should read the call's DDConfig fails that entry.

Anchor (test_step_reset_and_obs_equal_the_oracle): dd_reset, dd_write_obs and
the in-place bitmask dd_step against the C oracle under the same config, f32
and f64 storage, the engine's and both notebooks' rewards; one frame from the
loaded states and a second that re-spawns the lanes the first one ended.
Bounds, test_gpu_parity.test_vs_oracle_same_precision's and
test_gpu_thresholds': done, status, steps and episode equal; f64 fields and
rewards within 4 ulps + 1e-12 (f64_close), f32 ones within 1 float32 ulp
(gd.f32_close(., ., 1.0)); every obs row within 1 float32 ulp of the oracle's
double row; the engine's terminal rewards equal.

Every other path, bit for bit (integer views) against that step loop under
the same entry, the kernel matrices' contract: dd_rollout flushed (515 lanes)
and held (512), 3 frames and one more step; dd_policy_rollout with a fixed
random actor in f32 and f16x3 against the host loop of actor.act + env.step;
evaluate_policy against that loop's episode statistics, and with
components=True against it (REINFORCE: every statistic; PPO: all but the
total, whose prev_state differs by design) and against the oracle's replay
with test_gpu_reward_parts' bounds.  evaluate_policy starts from reset(), so
within its 3 frames only the entries that act right after a spawn are live
(the scales, the world size and max_fuel, which reach the actor's input and
calc_reward, among them).

Kernel family: under an entry that leaves the reference world no call may
take a kernel with the constants compiled in.  The calls that can tell report
it: a 512-lane engine-reward step is "fast" exactly under reference physics,
a 512-lane engine-reward rollout "split".  The twelve spawn entries keep the
reference physics (spawn ranges always come from the call), so their 512-lane
steps do run the compiled-in kernels, headline kernel included."""
import numpy as np
import pytest
import torch

import config_field_cases as cf
import golden_data as gd
from delivery_drone_amd import VecDroneEnv
from oracle import oracle as ora
from test_gpu_eval_oracle import reward_close
from test_gpu_eval_rollout import actors, assert_same_results  # noqa: F401 - actors is a fixture
from test_gpu_notebook_rollout import bits_equal
from test_gpu_parity import host
from test_gpu_reward_parts import replay as parts_replay
from test_gpu_step_matrix import STATE_FIELDS, run_steps

pytestmark = pytest.mark.gpu

STORAGE = ("f32", "f64")
MODES = ("engine", "notebook", "reinforce")
ENTRY = pytest.mark.parametrize("e", cf.ENTRIES, ids=cf.entry_id)
EVAL_T, EVAL_SEED = 0.3, 13


def make_env(dev, e, storage, mode, n=cf.N, max_steps=cf.MAX_STEPS, **switches):
    return VecDroneEnv(n, device=dev, config=cf.config(e, **switches), precision=storage, reward_mode=mode,
                       max_steps=max_steps)


def load(env, storage):
    st, acts = cf.state_set(storage, env.num_envs)
    env.load_state_dict({f: torch.as_tensor(st[f]) for f in STATE_FIELDS})
    return torch.as_tensor(acts, device=env.device)


def assert_physics_family(e, env, what):
    """A 512-lane engine-reward call under an entry off the reference world."""
    if e.physics and env.num_envs == cf.N_HELD and env.reward_mode == "engine":
        if env.last_step_kernel is not None:
            assert env.last_step_kernel == "generic", f"{what}: dd_step took the compiled-in headline kernel"
        if env.last_rollout_kernel is not None:
            assert env.last_rollout_kernel == "held", f"{what}: dd_rollout took {env.last_rollout_kernel}"


@ENTRY
def test_step_reset_and_obs_equal_the_oracle(gpu_device, e):
    for storage in STORAGE:
        for mode in MODES:
            what = f"{e.field}={e.value} {storage} {mode}"
            env = make_env(gpu_device, e, storage, mode)
            o = ora.OracleEnv(cf.N, precision=storage, config=env.config)
            ok = gd.f32_close(host(env.reset()), o.reset()[1], 1.0)  # dd_reset
            assert ok.all(), (what, "reset obs", np.argwhere(~ok)[:5])
            for f in STATE_FIELDS:
                np.testing.assert_array_equal(host(getattr(env, f)), getattr(o, f), err_msg=f"{what} reset {f}")
            acts = load(env, storage)
            o.load_state_dict(cf.state_set(storage)[0])
            ok = gd.f32_close(host(env.get_state()), o.get_state()[1], 1.0)  # dd_write_obs
            assert ok.all(), (what, "obs of the loaded state", np.argwhere(~ok)[:5])
            hist0 = None
            if mode == "notebook":  # the restarted history: this state's distance / world_width, no prev_state
                hist0 = host(env.shaped_hist).copy()
                assert reward_close(hist0[0], o.get_state()[1][:, 9], "f64").all() and np.isnan(hist0[1]).all(), what
            rec = run_steps(env, acts, cf.ANCHOR_FRAMES)
            want = cf.oracle_frames(env.config, storage, mode, hist0=hist0)
            for t, w in enumerate(want):
                for k in ("done", "engine_done"):
                    if k in rec["out"]:
                        np.testing.assert_array_equal(host(rec["out"][k][t]), w[k], err_msg=f"{what} frame {t} {k}")
                for f in ("status", "steps", "episode"):
                    np.testing.assert_array_equal(host(rec["state"][f][t]), w[f], err_msg=f"{what} frame {t} {f}")
                for f in gd.FLOAT_FIELDS:
                    ok = reward_close(host(rec["state"][f][t]), w[f], storage)
                    assert ok.all(), (what, t, f, np.flatnonzero(~ok)[:5])
                ok = gd.f32_close(host(rec["out"]["obs"][t]), w["obs"], 1.0)
                assert ok.all(), (what, t, "obs", np.argwhere(~ok)[:5])
                for k in ("reward", "engine_reward"):
                    if k in rec["out"]:
                        ok = reward_close(host(rec["out"][k][t]), w[k], storage)
                        assert ok.all(), (what, t, k, np.flatnonzero(~ok)[:5])
                engine = host(rec["out"]["engine_reward" if mode != "engine" else "reward"][t]).astype(np.float64)
                term = w["engine_done"]  # ended on this frame (auto_reset: a lane done before re-spawns, not done)
                np.testing.assert_array_equal(engine[term], w["engine_reward"][term].astype(np.float64),
                                              err_msg=f"{what} frame {t} terminal rewards")
                if mode == "notebook":
                    got = host(rec["state"]["shaped_hist"][t])
                    np.testing.assert_array_equal(np.isnan(got), np.isnan(w["shaped_hist"]), err_msg=what)
                    assert reward_close(np.nan_to_num(got), np.nan_to_num(w["shaped_hist"]), "f64").all(), (what, t)


def _assert_frames_equal(out, want, frames, what):
    assert set(out) == set(want), what
    for k, w in want.items():
        assert out[k].dtype == w.dtype, (what, k)
        for t in range(frames):
            assert bits_equal(out[k][t], w[t]), f"{what}: {k} differs first at frame {t}"


@ENTRY
def test_rollout_equals_the_step_loop(gpu_device, e):
    for n, kind in ((cf.N, "flushed"), (cf.N_HELD, "held")):
        for storage in STORAGE:
            for mode in MODES:
                what = f"{e.field}={e.value} {storage} {mode} {kind}"
                loop, roll = (make_env(gpu_device, e, storage, mode, n) for _ in range(2))
                acts = load(loop, storage)
                load(roll, storage)
                want = run_steps(loop, acts, cf.FRAMES + 1)
                assert_physics_family(e, loop, what)
                dev = gpu_device
                out = {"obs": torch.full((cf.FRAMES, n, 15), float("nan"), device=dev),
                       "reward": torch.full((cf.FRAMES, n), float("nan"), dtype=roll.float_dtype, device=dev),
                       "done": torch.full((cf.FRAMES, n), 0xEE, dtype=torch.uint8, device=dev)}
                kw = {}
                if mode != "engine":
                    out["engine_reward"] = torch.full_like(out["reward"], float("nan"))
                    out["engine_done"] = torch.full_like(out["done"], 0xEE)
                    kw = dict(engine_reward_out=out["engine_reward"], engine_done_out=out["engine_done"])
                roll.rollout(acts[:cf.FRAMES].contiguous(), obs_out=out["obs"], reward_out=out["reward"],
                             done_out=out["done"], **kw)
                expect = "split" if (kind == "held" and mode == "engine" and not e.physics) else kind
                if not (expect == "split" and roll.last_rollout_kernel == "held"):  # (fewer CUs than blocks: no split)
                    assert roll.last_rollout_kernel == expect, (what, roll.last_rollout_kernel)
                assert_physics_family(e, roll, what)
                for k in ("done", "engine_done"):
                    if k in out:
                        out[k] = out[k].view(torch.bool)
                _assert_frames_equal(out, want["out"], cf.FRAMES, what)
                for f, w in want["state"].items():
                    assert bits_equal(getattr(roll, f), w[cf.FRAMES - 1]), f"{what}: {f} after the launch"
                got = run_steps(roll, acts[cf.FRAMES:], 1)  # reads the history the rollout wrote back
                for part in ("out", "state"):
                    for k, w in want[part].items():
                        assert bits_equal(got[part][k][0], w[cf.FRAMES]), f"{what}: {part} {k} of the next step"


def host_loop(net, env, frames, temperature, seed):
    """actor.act + env.step on the env's current state: per-frame outputs,
    the actions, and the first episode's statistics as evaluate_policy keeps
    them (test_gpu_eval_rollout.host_episode's bookkeeping)."""
    dev, n = env.device, env.num_envs
    rows = {k: [] for k in ("obs", "actions", "log_prob", "reward", "done")}
    total = torch.zeros(n, dtype=torch.float64, device=dev)
    steps = torch.zeros(n, dtype=torch.int32, device=dev)
    landed = torch.zeros(n, dtype=torch.bool, device=dev)
    crashed = torch.zeros(n, dtype=torch.bool, device=dev)
    fuel = env.fuel.clone()
    alive = torch.ones(n, dtype=torch.bool, device=dev)
    obs = env.get_state()
    for k in range(frames):
        rows["obs"].append(obs.clone())
        a, lp = net.act(obs, seed=seed, step=k, env_id_base=env.env_id_base, temperature=temperature)
        obs, r, d, info = env.step(a)
        for name, v in (("actions", a), ("log_prob", lp), ("reward", r), ("done", d)):
            rows[name].append(v.clone())
        total = torch.where(alive, total + r.double(), total)
        steps += alive.to(torch.int32)
        fuel = torch.where(alive, env.fuel, fuel)
        ended = alive & d
        landed |= ended & info["landed"]
        crashed |= ended & info["crashed"]
        alive = alive & ~d
    stats = {"total_reward": total, "steps": steps, "landed": landed, "crashed": crashed, "final_fuel": fuel}
    return {k: torch.stack(v) for k, v in rows.items()}, stats


@ENTRY
def test_policy_rollout_equals_the_host_loop(actors, gpu_device, e):
    for compute, net in actors.items():
        for storage in STORAGE:
            for mode in MODES:
                what = f"{e.field}={e.value} {compute} {storage} {mode}"
                loop, fused = (make_env(gpu_device, e, storage, mode) for _ in range(2))
                load(loop, storage)
                load(fused, storage)
                want, _ = host_loop(net, loop, cf.FRAMES, 1.0, seed=8)
                got = dict(zip(("obs", "actions", "log_prob", "reward", "done"),
                               fused.policy_rollout(net, cf.FRAMES, seed=8)))
                _assert_frames_equal(got, want, cf.FRAMES, what)
                assert bits_equal(fused.obs, loop.obs), what
                for f in STATE_FIELDS:
                    assert bits_equal(getattr(fused, f), getattr(loop, f)), (what, f)
                if mode == "notebook":
                    assert bits_equal(fused.shaped_hist, loop.shaped_hist), what


@ENTRY
def test_evaluate_policy_equals_the_host_loop(actors, gpu_device, e):
    for compute, net in actors.items():
        for storage in STORAGE:
            for mode in MODES:
                what = f"{e.field}={e.value} {compute} {storage} {mode}"
                # (the reference env never truncates: the notebooks' evaluation has no timeout penalty)
                ref = make_env(gpu_device, e, storage, mode, max_steps=0, auto_reset=False)
                ref.reset()
                rows, want = host_loop(net, ref, cf.FRAMES, EVAL_T, EVAL_SEED)
                env = make_env(gpu_device, e, storage, mode, auto_reset=False)
                got = env.evaluate_policy(net, max_steps=cf.FRAMES, temperature=EVAL_T, seed=EVAL_SEED)
                assert_same_results(got, want)
                assert bits_equal(env.obs, ref.obs), what
                for f in STATE_FIELDS:
                    assert bits_equal(getattr(env, f), getattr(ref, f)), (what, f)
                if mode == "engine":
                    continue
                env = make_env(gpu_device, e, storage, mode, auto_reset=False)
                got = env.evaluate_policy(net, max_steps=cf.FRAMES, temperature=EVAL_T, seed=EVAL_SEED,
                                          components=True)
                parts = got.pop("components")
                assert bits_equal(parts["total"], got["total_reward"]), what
                for key in want:  # PPO: the notebook's evaluation passes prev_state one frame back, the loop two
                    if not (mode == "notebook" and key == "total_reward"):
                        assert torch.equal(got[key], want[key]), (what, "components=True", key)
                assert bits_equal(env.obs, ref.obs), what
                rep = parts_replay(env, host(rows["actions"]))  # the oracle, calc_reward restated on its obs64
                sums = np.stack([host(v) for v in parts.values()], axis=1)
                bad = np.abs(sums - rep["sum"]) > rep["bound"]
                assert not bad.any(), (what, "components", np.argwhere(bad)[:5])
                np.testing.assert_array_equal(host(got["steps"]), rep["steps"], err_msg=what)
                np.testing.assert_array_equal(host(got["final_fuel"]), rep["fuel"], err_msg=what)
