"""GPU: every dd_step kernel, step_kernel / step_pp_kernel<T, AFMT, kRef,
kShape> (72), each with auto_reset on and off.  The cases and the template
arguments they select come from tests/test_kernel_matrix_cpu.py, which pins
them to the build's kernel names; the ids name the template arguments.

Two tiers, as tests/test_gpu_eval_matrix.py / test_gpu_eval_oracle.py.

Anchors (test_anchor_equals_the_oracle): the in-place bitmask kernel of each
storage x physics (the PHYSICS table of test_gpu_eval_matrix.py) x reward
mode, replayed frame by frame on the C oracle (OracleEnv.step / step_shaped,
same config, precision and env id base; the PPO history seeded from the env,
as test_gpu_eval_oracle.oracle_replay does).  Bounds, all imported:
* done, shaped done, status, steps, episode, fuel: exact.
* every other state field, reward, engine reward, shaped reward:
  test_gpu_eval_oracle.reward_close, i.e. gd.f32_close(., ., 1.0) with f32
  storage and test_gpu_parity.f64_close (4 ulps + 1e-12) with f64.  No shaped
  case needed test_gpu_parity.py's older, wider shaped bound.
* obs: gd.f32_close(., ., 1.0) against the oracle's double row.
The worst measured error of each group is printed next to its bound.

Every other kernel (test_kernel_equals_its_anchor): f32x3, u8x3 and ping-pong
in every combination, bit for bit (integer views, so NaN history slots
compare) against the anchor of the same storage, physics, mode and
auto_reset, after every frame: obs, reward, done, the engine's reward and
done in the notebook modes, every state field and the PPO history.  A
ping-pong env's fields are read after each of the 42 steps, so both an odd
and an even number of swaps are compared.

Sizes: 515 lanes = two full 256-lane blocks and a 3-lane tail wave (the
partial flush_obs_wave); 41 frames (odd, past the 25-frame cap of the
notebook modes, so the timeout and the re-spawn happen inside) and one more.

Starting states (start_state): even lanes are env.reset() spawns
(randomize_drone), odd lanes come from threshold_states.generate(config=the
case's), loaded into env and oracle alike, so landings and crashes happen on
frame 1.  40 % of the threshold lanes and every eighth spawn lane start at
steps = cap - 1: near-pad ones land on the cap frame (no -500), mid-air ones
take the -500 on frame 1.  generate placed states for all four physics.

Coverage conditions, asserted on the oracle's replay and printed as counts:
some lane landed; some crashed; notebook modes: some lane timed out mid-air
(-500) and some landed exactly on the cap frame; auto_reset: some lane
re-spawned (PPO: and its history restarted); otherwise some lane sat sticky
done for two frames or more.  Seeds were picked with the oracle alone
(STATE_SEED, ACTION_SEED; the first ones tried met every condition in every
anchor).  Thinnest counts over the 48 anchors at 515 lanes: THINNEST below
(at least 29 lanes for the rarest condition, landing on the cap frame).

Action values (test_action_values): each format x storage, 1 and 5 frames,
with bitmask bytes from all of 0..255, f32x3 entries from {0, -0, 1, -1, 0.5,
2^-149, inf, NaN} and u8x3 entries from {0, 1, 2, 128, 255}, bit for bit
against the bitmask kernel fed oracle.bitmask of the same array (numpy's
!= 0; for bitmask bytes its low three bits, the ones the header defines)."""
import functools

import numpy as np
import pytest
import torch

import golden_data as gd
import threshold_states
from delivery_drone_amd import EnvConfig, VecDroneEnv
from oracle import oracle as ora
from test_gpu_eval_matrix import ENV_ID_BASE, PHYSICS, STORAGE
from test_gpu_eval_oracle import allowance, reward_close
from test_gpu_notebook_rollout import bits_equal
from test_gpu_parity import host
from test_kernel_matrix_cpu import STEP_FORMATS, is_anchor, step_id, step_matrix

pytestmark = pytest.mark.gpu

N, N_ALL, FRAMES, CAP = 515, 520, 41, 25
SPAWN_SEED, STATE_SEED, ACTION_SEED = 5, 11, 17
PHILOX_SEED, PHILOX_STEP = 23, 29  # the rollout's in-kernel stream: crosses the 32-step block inside the launch
STATE_FIELDS = gd.FLOAT_FIELDS + ("status", "steps", "episode")
EXACT_FIELDS = ("fuel", "status", "steps", "episode")
# thinnest coverage counts over the 48 anchors (515 lanes, 41 frames), from the oracle alone; episode ends and
# re-spawns are counted per lane and frame, sticky lanes per lane
THINNEST = {"rng": "landed 100 (f32 moving notebook sticky), crashed 77, timed out mid-air 327, landed on the cap "
                   "frame 32 (f32 reference notebook), re-spawned 226 (PPO history restarted 832), sticky 223",
            "philox": "landed 93, crashed 76, timed out mid-air 334, landed on the cap frame 29, re-spawned 213, "
                      "sticky 210"}


def config_for(physics, auto_reset):
    return EnvConfig(randomize_drone=True, auto_reset=auto_reset, seed=SPAWN_SEED, **PHYSICS[physics])


def make_env(dev, n, storage, physics, mode, auto_reset, ping_pong=False):
    return VecDroneEnv(n, device=dev, config=config_for(physics, auto_reset), precision=storage, reward_mode=mode,
                       max_steps=CAP, env_id_base=ENV_ID_BASE, ping_pong=ping_pong)


@functools.lru_cache(maxsize=None)
def start_state(storage, physics):
    """(state of N_ALL lanes as numpy arrays, frame-0 actions of the threshold
    lanes, threshold mask).  Lanes are keyed by env id: the first 515 of the
    520 are the 515-lane batch."""
    cfg = config_for(physics, False)
    o = ora.OracleEnv(N_ALL, precision=storage, config=cfg, env_id_base=ENV_ID_BASE)
    o.reset()
    st = {k: np.asarray(v, np.float64 if k in gd.FLOAT_FIELDS else v.dtype).copy() for k, v in o.state_dict().items()}
    th, acts, _, _ = threshold_states.generate(N_ALL, storage, seed=STATE_SEED, config=cfg)
    lane = np.arange(N_ALL)
    odd = lane % 2 == 1
    for f in gd.FLOAT_FIELDS + ("status",):
        st[f][odd] = th[f][odd]
    rng = np.random.default_rng(STATE_SEED + 1)
    at_cap = rng.random(N_ALL) < 0.4
    early = rng.integers(0, 20, N_ALL)
    st["steps"][odd] = np.where(at_cap, CAP - 1, early)[odd]
    st["steps"][lane % 8 == 0] = CAP - 1
    return st, acts, odd


@functools.lru_cache(maxsize=None)
def action_stream(storage, physics, stream):
    """[FRAMES + 1, N_ALL] uint8 bitmasks: "rng" (the threshold lanes' first
    action is the one their state was placed for) or "philox" (the documented
    host stream of DD_ACT_PHILOX, golden_data.philox_actions_np)."""
    if stream == "philox":
        return gd.philox_actions_np(PHILOX_SEED, ENV_ID_BASE, N_ALL, PHILOX_STEP, FRAMES + 1)
    _, acts0, odd = start_state(storage, physics)
    a = np.random.default_rng(ACTION_SEED).integers(0, 8, (FRAMES + 1, N_ALL)).astype(np.uint8)
    a[0, odd] = acts0[odd]
    return a


def load_start(env, storage, physics):
    """reset(), whose spawn must be the oracle's, then the threshold lanes."""
    st, _, odd = start_state(storage, physics)
    n = env.num_envs
    env.reset()
    even = torch.as_tensor(~odd[:n], device=env.device)
    for f in ("x", "y", "px", "py", "fuel", "episode"):
        want = torch.as_tensor(st[f][:n], device=env.device).to(getattr(env, f).dtype)
        assert torch.equal(getattr(env, f)[even], want[even]), f
    env.load_state_dict({f: torch.as_tensor(st[f][:n]) for f in STATE_FIELDS})


def encode(acts, fmt):
    """A uint8 bitmask tensor in the given action format (0 / 1 entries)."""
    if fmt == "bitmask":
        return acts
    a = torch.stack([(acts >> k) & 1 for k in range(3)], dim=-1)
    return a.float() if fmt == "f32x3" else a.to(torch.uint8)


def run_steps(env, actions, count):
    """`count` step() calls; every output and every state field after each."""
    out, state = {}, {}
    shaped = env.reward_mode != "engine"
    for t in range(count):
        obs, r, d, info = env.step(actions[t])
        frame = {"obs": obs, "reward": r, "done": d}
        if shaped:
            frame.update(engine_reward=info["engine_reward"], engine_done=info["engine_done"])
        for k, v in frame.items():
            out.setdefault(k, []).append(v.clone())
        for f in STATE_FIELDS:
            state.setdefault(f, []).append(getattr(env, f).clone())
        if env.shaped_hist is not None:
            state.setdefault("shaped_hist", []).append(env.shaped_hist.clone())
    return {"out": {k: torch.stack(v) for k, v in out.items()}, "state": {k: torch.stack(v) for k, v in state.items()}}


_ANCHORS = {}


def anchor_record(dev, storage, physics, mode, auto_reset, n=N, stream="rng"):
    """The in-place bitmask step loop of one config (FRAMES + 1 frames),
    computed once: the kernel test_anchor_equals_the_oracle ties to the
    oracle.  Lanes are keyed by env id, so a 520-lane record must contain the
    515-lane one, which is asserted here."""
    key = (storage, physics, mode, auto_reset, n, stream)
    if key not in _ANCHORS:
        env = make_env(dev, n, storage, physics, mode, auto_reset)
        load_start(env, storage, physics)
        hist0 = host(env.shaped_hist).copy() if mode == "notebook" else None
        acts = torch.as_tensor(action_stream(storage, physics, stream)[:, :n], device=dev)
        rec = run_steps(env, acts, FRAMES + 1)
        rec["hist0"] = hist0
        if n != N:
            small = anchor_record(dev, storage, physics, mode, auto_reset, N, stream)
            for part in ("out", "state"):
                for k, v in small[part].items():
                    assert bits_equal(rec[part][k][..., :N, :] if k == "obs" else rec[part][k][..., :N], v), (part, k)
        _ANCHORS[key] = rec
    return _ANCHORS[key]


_REPLAYS = {}


def oracle_replay(storage, physics, mode, auto_reset, n=N, stream="rng", hist0=None):
    """The same frames on the C oracle: per-frame outputs and state in numpy,
    and the coverage counts.  hist0: the env's PPO history after load_start
    (None: from the oracle's own observation, for runs without a GPU)."""
    key = (storage, physics, mode, auto_reset, n, stream)
    if key in _REPLAYS:
        return _REPLAYS[key]
    st, _, _ = start_state(storage, physics)
    o = ora.OracleEnv(n, precision=storage, config=config_for(physics, auto_reset), env_id_base=ENV_ID_BASE)
    o.load_state_dict({f: st[f][:n] for f in STATE_FIELDS})
    hist = None
    if mode == "notebook":
        if hist0 is None:
            hist0 = np.stack([o.get_state()[1][:, 9], np.full(n, np.nan)])
        hist = np.ascontiguousarray(hist0, dtype=np.float64).copy()
    acts = action_stream(storage, physics, stream)[:, :n]
    out = {k: [] for k in ("obs", "reward", "done", "engine_reward", "engine_done")}
    state = {f: [] for f in STATE_FIELDS + ("shaped_hist",)}
    for k in range(FRAMES + 1):
        if mode == "engine":
            _, r, d, obs64 = o.step(acts[k])
            sr, sd = r, d
        else:
            _, r, d, obs64, sr, sd = o.step_shaped(acts[k], hist, CAP, mode)
        for name, v in (("obs", obs64), ("reward", sr), ("done", sd), ("engine_reward", r), ("engine_done", d)):
            out[name].append(np.array(v))
        for f in STATE_FIELDS:
            state[f].append(getattr(o, f).copy())
        state["shaped_hist"].append(hist.copy() if hist is not None else np.zeros((2, n)))
    rep = {"out": {k: np.stack(v) for k, v in out.items()}, "state": {k: np.stack(v) for k, v in state.items()}}
    rep["coverage"] = coverage(rep, st["status"][:n], mode, auto_reset)
    _REPLAYS[key] = rep
    return rep


def coverage(rep, status0, mode, auto_reset):
    """Counts of the coverage conditions over the first FRAMES frames of an oracle replay."""
    status, steps = rep["state"]["status"][:FRAMES], rep["state"]["steps"][:FRAMES]
    before = np.concatenate([status0[None], status[:-1]])
    was_done = (before & gd.ST_DONE) != 0
    ended = ~was_done & ((status & gd.ST_DONE) != 0)
    landed, crashed = ended & ((status & gd.ST_LANDED) != 0), ended & ((status & gd.ST_CRASHED) != 0)
    c = {"landed": int(landed.sum()), "crashed": int(crashed.sum())}
    if mode != "engine":
        midair = ended & ~landed & ~crashed & (steps >= CAP)
        assert (rep["out"]["reward"][:FRAMES][midair] < -400).all()  # the -500
        on_cap = landed & (steps >= CAP)
        assert (rep["out"]["reward"][:FRAMES][on_cap] > 0).all()  # the landing terminal, no -500
        c.update(timed_out_midair=int(midair.sum()), landed_on_cap=int(on_cap.sum()))
    if auto_reset:
        c["respawned"] = int(was_done.sum())
        if mode == "notebook":  # the history restarts: this frame's distance, prev_state None
            h = rep["state"]["shaped_hist"][:FRAMES]
            restarted = was_done & np.isnan(h[:, 1]) & np.isfinite(h[:, 0])
            assert (restarted == was_done).all()
            c["history_restarted"] = int(restarted.sum())
    else:
        c["sticky_two_frames"] = int((was_done.sum(axis=0) >= 2).sum())
    return c


def assert_covered(c, what):
    print(f"{what}: " + ", ".join(f"{k} {v}" for k, v in c.items()))
    for k, v in c.items():
        assert v > 0, f"{what}: no lane {k.replace('_', ' ')}"


def first_difference(got, want):
    """Index of the first frame whose bits differ, or None."""
    for t in range(want.shape[0]):
        if not bits_equal(got[t], want[t]):
            return t
    return None


def assert_same_record(got, want, what, frames=FRAMES + 1):
    for part in ("out", "state"):
        assert set(got[part]) == set(want[part]), (what, part)
        for k, w in want[part].items():
            g = got[part][k]
            assert g.dtype == w.dtype and g.shape[1:] == w.shape[1:], (what, part, k)
            if not bits_equal(g[:frames], w[:frames]):
                raise AssertionError(f"{what}: {part} {k} differs first at frame {first_difference(g, w)}")


def _share(got, ref, storage):
    """The worst |got - ref| as a share of what reward_close allows there (<= 1 passes)."""
    ref = np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.nanmax(np.abs(np.asarray(got, np.float64) - ref) / allowance(ref, storage), initial=0.0))


ANCHORS = [c for c in step_matrix() if is_anchor(c)]
OTHERS = [c for c in step_matrix() if not is_anchor(c)]


@pytest.mark.parametrize("auto_reset", [True, False], ids=["auto_reset", "sticky"])
@pytest.mark.parametrize("case", ANCHORS, ids=step_id)
def test_anchor_equals_the_oracle(gpu_device, case, auto_reset):
    storage, physics, mode = case.storage, case.physics, case.mode
    what = f"{step_id(case)} {'auto_reset' if auto_reset else 'sticky'}"
    rec = anchor_record(gpu_device, storage, physics, mode, auto_reset)
    rep = oracle_replay(storage, physics, mode, auto_reset, hist0=rec["hist0"])
    assert_covered(rep["coverage"], what)
    worst = {}
    for name in ("done", "engine_done"):
        if name in rec["out"]:
            np.testing.assert_array_equal(host(rec["out"][name]), rep["out"][name], err_msg=f"{what} {name}")
    for f in EXACT_FIELDS:
        np.testing.assert_array_equal(host(rec["state"][f]), rep["state"][f], err_msg=f"{what} {f}")
    for name in ("reward", "engine_reward"):
        if name in rec["out"]:
            got = host(rec["out"][name])
            worst[name] = _share(got, rep["out"][name], storage)
            ok = reward_close(got, rep["out"][name], storage)
            assert ok.all(), (what, name, worst[name], np.argwhere(~ok)[:5])
    for f in gd.FLOAT_FIELDS:
        if f not in EXACT_FIELDS:
            got = host(rec["state"][f])
            worst[f] = _share(got, rep["state"][f], storage)
            ok = reward_close(got, rep["state"][f], storage)
            assert ok.all(), (what, f, worst[f], np.argwhere(~ok)[:5])
    obs = host(rec["out"]["obs"])
    worst["obs"] = _share(obs, rep["out"]["obs"], "f32")
    ok = gd.f32_close(obs, rep["out"]["obs"], 1.0)
    assert ok.all(), (what, "obs", worst["obs"], np.argwhere(~ok)[:5])
    if mode == "notebook":  # the ring the oracle keeps in double: the same slots, NaN where it has none
        got, want = host(rec["state"]["shaped_hist"]), rep["state"]["shaped_hist"]
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
        assert reward_close(np.nan_to_num(got), np.nan_to_num(want), "f64").all(), (what, "shaped_hist")
    top = max(worst, key=worst.get)
    print(f"{what}: worst error {worst[top]:.2f} of its bound ({top}; "
          f"{'4 f64 ulps + 1e-12' if storage == 'f64' else '1 f32 ulp'}), obs {worst['obs']:.2f} of 1 f32 ulp")


@pytest.mark.parametrize("auto_reset", [True, False], ids=["auto_reset", "sticky"])
@pytest.mark.parametrize("case", OTHERS, ids=step_id)
def test_kernel_equals_its_anchor(gpu_device, case, auto_reset):
    what = f"{step_id(case)} {'auto_reset' if auto_reset else 'sticky'}"
    want = anchor_record(gpu_device, case.storage, case.physics, case.mode, auto_reset)
    assert_covered(oracle_replay(case.storage, case.physics, case.mode, auto_reset, hist0=want["hist0"])["coverage"],
                   what)
    env = make_env(gpu_device, N, case.storage, case.physics, case.mode, auto_reset, ping_pong=case.ping_pong)
    load_start(env, case.storage, case.physics)
    acts = torch.as_tensor(action_stream(case.storage, case.physics, "rng")[:, :N], device=gpu_device)
    got = run_steps(env, encode(acts, case.fmt), FRAMES + 1)
    assert_same_record(got, want, what)


# --------------------------------------------------------------------------
# action values
# --------------------------------------------------------------------------
F32_VALUES = np.array([0.0, -0.0, 1.0, -1.0, 0.5, 2.0 ** -149, np.inf, np.nan], np.float32)
U8_VALUES = np.array([0, 1, 2, 128, 255], np.uint8)


def unusual_actions(fmt, frames, n, seed=3):
    """(the actions in `fmt`, the bitmask the formats' "nonzero = on" gives)."""
    rng = np.random.default_rng(seed)
    if fmt == "bitmask":
        a = rng.integers(0, 256, (frames, n)).astype(np.uint8)
        assert (a > 7).any()
        return a, a & 7  # bit0 main, bit1 left, bit2 right: the bits the header defines
    values = F32_VALUES if fmt == "f32x3" else U8_VALUES
    idx = rng.integers(0, values.size, (frames, n, 3))
    assert np.unique(idx).size == values.size  # every value is drawn
    a = values[idx]
    bits = np.stack([ora.bitmask(a[k]) for k in range(frames)])
    return a, bits


@pytest.mark.parametrize("frames", [1, 5])
@pytest.mark.parametrize("storage", STORAGE)
@pytest.mark.parametrize("fmt", STEP_FORMATS)
def test_action_values(gpu_device, fmt, storage, frames):
    a, bits = unusual_actions(fmt, frames, N)
    if fmt == "f32x3":  # NaN and the subnormal are on, -0.0 is off
        sub, nan, negz = a.view(np.uint32) == 1, np.isnan(a), a.view(np.uint32) == 0x80000000
        on = np.stack([(bits >> k) & 1 for k in range(3)], axis=-1).astype(bool)
        assert on[sub].all() and on[nan].all() and not on[negz].any() and sub.any() and nan.any() and negz.any()
    envs = [make_env(gpu_device, N, storage, "reference", "engine", True) for _ in range(2)]
    for e in envs:
        e.reset()
    got = run_steps(envs[0], torch.as_tensor(a, device=gpu_device), frames)
    want = run_steps(envs[1], torch.as_tensor(bits, device=gpu_device), frames)
    assert_same_record(got, want, f"{fmt} {storage} {frames} frames", frames)
