"""GPU: every dd_rollout kernel, rollout_kernel<T, AFMT, kRef, kHeld, kShape,
kSplit> (104), each with auto_reset on and off.  The cases and the template
arguments they select come from tests/test_kernel_matrix_cpu.py, which pins
them to the build's kernel names; the ids name the template arguments.

Reference: the step loop of the same env config, which dd_rollout promises to
equal bit for bit: test_gpu_step_matrix.anchor_record, the in-place bitmask
dd_step kernel that test_anchor_equals_the_oracle ties to the C oracle at 515
lanes (a 520-lane record is asserted to contain the 515-lane one; lanes are
keyed by env id).  It is computed once per (storage, physics, mode,
auto_reset, lanes, action stream).  Philox cases: the step loop is fed the
documented host stream (golden_data.philox_actions_np, pinned to
oracle.philox4x32_10 by tests/test_philox_np.py), never another Philox launch;
action_step = 29, so the 32-step block boundary is crossed inside the launch.

Bounds: none, every comparison is on bits (integer views: NaN history slots):
obs, reward, done per frame, the engine's reward and done in the notebook
modes (engine_reward_out / engine_done_out), every state field and the PPO
history after the launch, and one more step() on both sides, which reads the
history the rollout wrote back.  Output buffers start as NaN / 0xEE, so a row
the kernel leaves unwritten fails.

Kernel kind: each case asserts that env.last_rollout_kernel is the kind the
CPU mapping (rollout_kind, from the buffers' actual addresses) predicts, so a
case cannot pass on another kernel.  Flushed: 515 lanes (n % 4 != 0; two full
blocks and a 3-lane tail wave).  Held: 520 lanes (a third block of 8 lanes),
kernel="single" where "auto" would split.  Split: 520 lanes, 3 blocks, under
any CU count.  test_other_routes_to_flushed adds, at 520 lanes, an obs_out
that is only 4-byte aligned and a bitmask action tensor that starts 1 byte
into its storage.

Frames, states, cap and coverage conditions are the step matrix's (41 frames,
cap 25, test_gpu_step_matrix.start_state; counts asserted on the oracle's
replay of the case's own action stream and printed; thinnest:
test_gpu_step_matrix.THINNEST).  test_few_frames runs 1, 2 and 3 frames (the
by-two loop's tail; action prefetches past the buffer's end) on a held and a
flushed shaped non-reference kernel, with the unusual action values of
test_gpu_step_matrix.unusual_actions in f32x3 and u8x3, against the step loop
fed oracle.bitmask of the same arrays."""
import pytest
import torch

from test_gpu_step_matrix import (CAP, FRAMES, PHILOX_SEED, PHILOX_STEP, action_stream, anchor_record,  # noqa: F401
                                  assert_covered, assert_same_record, bits_equal, encode, load_start, make_env,
                                  oracle_replay, run_steps, unusual_actions)
from test_kernel_matrix_cpu import RolloutCase, rollout_id, rollout_kernel_for, rollout_kind, rollout_matrix

pytestmark = pytest.mark.gpu


def launch(env, case, actions, frames, *, obs_out=None):
    """One rollout() with sentinel-filled buffers; asserts the kernel kind the
    CPU mapping predicts from the buffers' addresses.  Returns the outputs
    under run_steps' names."""
    n, dev = env.num_envs, env.device
    obs = torch.full((frames, n, 15), float("nan"), device=dev) if obs_out is None else obs_out
    out = {"obs": obs, "reward": torch.full((frames, n), float("nan"), dtype=env.float_dtype, device=dev),
           "done": torch.full((frames, n), 0xEE, dtype=torch.uint8, device=dev)}
    kw = {}
    if env.reward_mode != "engine":
        out["engine_reward"] = torch.full_like(out["reward"], float("nan"))
        out["engine_done"] = torch.full_like(out["done"], 0xEE)
        kw = dict(engine_reward_out=out["engine_reward"], engine_done_out=out["engine_done"])
    if actions is None:
        kw.update(frames=frames, action_seed=PHILOX_SEED, action_step=PHILOX_STEP)
    env.rollout(actions, obs_out=obs, reward_out=out["reward"], done_out=out["done"], kernel=case.kernel, **kw)
    key = rollout_kernel_for(case)
    predicted = rollout_kind(key.ref, key.shape, case.fmt, actions.data_ptr() if actions is not None else 0,
                             obs.data_ptr(), n, kernel=case.kernel)
    assert env.last_rollout_kernel == predicted, (env.last_rollout_kernel, predicted)
    if predicted == "split":
        env.check_device_errors()  # a hand-over that ran out of polls
    for k in ("done", "engine_done"):
        if k in out:
            out[k] = out[k].view(torch.bool)
    return out, predicted


def assert_rollout_equals_steps(env, out, want, frames, extra_action, what):
    """The launch's outputs, the state it left, and one more step()."""
    assert set(out) == set(want["out"]), what
    for k, w in want["out"].items():
        assert out[k].dtype == w.dtype, (what, k)
        for t in range(frames):
            assert bits_equal(out[k][t], w[t]), f"{what}: {k} differs first at frame {t}"
    for f, w in want["state"].items():
        assert bits_equal(getattr(env, f), w[frames - 1]), f"{what}: {f} after the launch"
    got = run_steps(env, extra_action[None], 1)
    for part in ("out", "state"):
        for k, w in want[part].items():
            assert bits_equal(got[part][k][0], w[frames]), f"{what}: {part} {k} of the step after the launch"


@pytest.mark.parametrize("auto_reset", [True, False], ids=["auto_reset", "sticky"])
@pytest.mark.parametrize("case", rollout_matrix(), ids=rollout_id)
def test_rollout_equals_the_step_loop(gpu_device, case, auto_reset):
    what = f"{rollout_id(case)} {'auto_reset' if auto_reset else 'sticky'}"
    stream = "philox" if case.fmt == "philox" else "rng"
    want = anchor_record(gpu_device, case.storage, case.physics, case.mode, auto_reset, case.n, stream)
    assert_covered(oracle_replay(case.storage, case.physics, case.mode, auto_reset, case.n, stream,
                                 hist0=want["hist0"])["coverage"], what)
    env = make_env(gpu_device, case.n, case.storage, case.physics, case.mode, auto_reset)
    load_start(env, case.storage, case.physics)
    bits = torch.as_tensor(action_stream(case.storage, case.physics, stream)[:, :case.n], device=gpu_device)
    actions = None if case.fmt == "philox" else encode(bits[:FRAMES], case.fmt).contiguous()
    out, kind = launch(env, case, actions, FRAMES)
    assert kind == case.kind
    assert_rollout_equals_steps(env, out, want, FRAMES, bits[FRAMES], what)


ROUTE_CASES = [RolloutCase("f32", "bitmask", "reference", "engine", "flushed", 520, "auto"),  # else the split kernel
               RolloutCase("f64", "bitmask", "gravity", "reinforce", "flushed", 520, "auto"),
               RolloutCase("f64", "u8x3", "wind", "notebook", "flushed", 520, "auto")]
# (only the bitmask format's dword loads need an aligned action buffer)
ROUTES = [pytest.param(c, r, id=f"{rollout_id(c)}-{r}") for c in ROUTE_CASES
          for r in ("obs_4_byte_aligned", "actions_1_byte_in") if r == "obs_4_byte_aligned" or c.fmt == "bitmask"]


@pytest.mark.parametrize("auto_reset", [True, False], ids=["auto_reset", "sticky"])
@pytest.mark.parametrize("case,route", ROUTES)
def test_other_routes_to_flushed(gpu_device, case, route, auto_reset):
    what = f"{rollout_id(case)} {route}"
    n = case.n
    want = anchor_record(gpu_device, case.storage, case.physics, case.mode, auto_reset, n)
    env = make_env(gpu_device, n, case.storage, case.physics, case.mode, auto_reset)
    load_start(env, case.storage, case.physics)
    bits = torch.as_tensor(action_stream(case.storage, case.physics, "rng")[:, :n], device=gpu_device)
    actions, obs_out = encode(bits[:FRAMES], case.fmt).contiguous(), None
    if route == "obs_4_byte_aligned":
        buf = torch.full((FRAMES * n * 15 + 4,), float("nan"), device=gpu_device)
        obs_out = buf[1:1 + FRAMES * n * 15].view(FRAMES, n, 15)
        assert obs_out.data_ptr() % 16 == 4 and obs_out.is_contiguous()
    else:
        raw = torch.zeros(FRAMES * n + 1, dtype=torch.uint8, device=gpu_device)
        raw[1:] = actions.reshape(-1)
        actions = raw[1:].view(FRAMES, n)
        assert actions.data_ptr() % 4 == 1 and actions.is_contiguous()
    out, kind = launch(env, case, actions, FRAMES, obs_out=obs_out)
    assert kind == "flushed"
    assert_rollout_equals_steps(env, out, want, FRAMES, bits[FRAMES], what)
    if obs_out is not None:  # nothing outside the view was written
        assert bool(torch.isnan(buf[:1]).all()) and bool(torch.isnan(buf[1 + FRAMES * n * 15:]).all())


FEW_CASES = [RolloutCase("f64", "f32x3", "wind", "notebook", "held", 520, "auto"),
             RolloutCase("f64", "u8x3", "wind", "notebook", "held", 520, "auto"),
             RolloutCase("f32", "f32x3", "gravity", "reinforce", "flushed", 515, "auto"),
             RolloutCase("f32", "u8x3", "gravity", "reinforce", "flushed", 515, "auto")]


@pytest.mark.parametrize("frames", [1, 2, 3])
@pytest.mark.parametrize("case", FEW_CASES, ids=rollout_id)
def test_few_frames(gpu_device, case, frames):
    what = f"{rollout_id(case)} {frames} frames"
    roll, loop = (make_env(gpu_device, case.n, case.storage, case.physics, case.mode, True) for _ in range(2))
    for e in (roll, loop):
        load_start(e, case.storage, case.physics)
    a, bits = unusual_actions(case.fmt, frames + 1, case.n, seed=frames)
    bits = torch.as_tensor(bits, device=gpu_device)
    want = run_steps(loop, bits, frames + 1)
    actions = torch.as_tensor(a[:frames], device=gpu_device).contiguous()
    out, kind = launch(roll, case, actions, frames)
    assert kind == case.kind
    assert_rollout_equals_steps(roll, out, want, frames, bits[frames], what)
