"""GPU: dd_step's headline-shape kernel (csrc/step_fast.hip) against the
generic kernel, bit for bit, and the host's choice between the two.

Reference: the generic kernel itself (csrc/step.hip, held to the oracle by
tests/test_gpu_step_matrix.py and tests/test_gpu_step_wave_paths.py).  Two
envs with the same seed, state and actions step FRAMES frames; one call has
the headline shape and takes the fast kernel, the other is forced onto the
generic kernel by its call shape alone (collect_done_idx=True, or obs rows
written into a view that starts one row into its buffer, 60 bytes: no
16-byte alignment).  Bounds: none.  After every frame every state field, obs,
reward and done are equal in every bit (torch.equal on the floats' bit
patterns).

Sizes: 256 (one tile), 1,024 (one block per XCD-sized group), 4,096 with
env_id_base != 0.  FRAMES = 300: a drone falls to the ground in under 100
frames, so most waves re-spawn lanes several times (asserted).  Two starting
states at 1,024: one with every lane of a wave (lanes 64..127) done, so the
first step runs a wave with no live lane, and one with no lane done.

Dispatch, through VecDroneEnv.last_step_kernel (dd_step_variant of the call
just made): each departure from the headline shape takes the generic kernel,
the headline shape the fast one, up to and including 262,144 lanes (the residency
bound, csrc/step_tile.h kStepFastMaxLanes) and not beyond."""
import ctypes

import pytest
import torch

import golden_data as gd
from delivery_drone_amd import EnvConfig, VecDroneEnv, abi
from test_gpu_notebook_rollout import bits_equal

pytestmark = pytest.mark.gpu

FRAMES = 300
STATE_FIELDS = gd.FLOAT_FIELDS + ("status", "steps", "episode")
MAX_FAST = 1 << 18


def headline_config(**kw):
    return EnvConfig(**{**dict(randomize_drone=True, randomize_platform=True, auto_reset=True, seed=11), **kw})


def make_pair(dev, n, storage, env_id_base=0):
    envs = [VecDroneEnv(n, device=dev, config=headline_config(), precision=storage, env_id_base=env_id_base)
            for _ in range(2)]
    for e in envs:
        e.reset()
    return envs


def step_generic(env, acts, force, bufs):
    """One step that the call's shape alone sends to the generic kernel."""
    if force == "done_idx":
        obs, r, d, _ = env.step(acts, collect_done_idx=True)
    else:  # rows written one row into a larger buffer: 60 bytes off, not 16-byte aligned
        obs, r, d, _ = env.step(acts, out=(bufs[0][1:], bufs[1], bufs[2]))
    return obs, r, d


def run_pair(dev, n, storage, force, env_id_base=0, start=None):
    fast, gen = make_pair(dev, n, storage, env_id_base)
    if start is not None:
        for e in (fast, gen):
            sd = e.state_dict()
            start(sd)
            e.load_state_dict(sd)
    bufs = (torch.empty(n + 1, abi.DD_OBS_DIM, device=dev), torch.empty(n, device=dev, dtype=fast.float_dtype),
            torch.empty(n, device=dev, dtype=torch.bool))
    g = torch.Generator(device=dev).manual_seed(5)
    acts = torch.randint(0, 8, (FRAMES, n), device=dev, dtype=torch.uint8, generator=g)
    episode0 = fast.episode.clone()
    for t in range(FRAMES):
        fo, fr, fd, _ = fast.step(acts[t])
        assert fast.last_step_kernel == "fast", t
        go, gr, gd_ = step_generic(gen, acts[t], force, bufs)
        assert gen.last_step_kernel == "generic", t
        assert bits_equal(fo, go), f"obs frame {t}"
        assert bits_equal(fr, gr), f"reward frame {t}"
        assert torch.equal(fd, gd_), f"done frame {t}"
        for f in STATE_FIELDS:
            assert bits_equal(getattr(fast, f), getattr(gen, f)), f"{f} frame {t}"
    respawned = (fast.episode > episode0).view(-1, 64).any(dim=1).float().mean().item()
    assert respawned > 0.5, f"only {respawned:.0%} of the waves re-spawned a lane"
    return fast


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("n,force,env_id_base", [(256, "done_idx", 0), (1024, "offset_obs", 0),
                                                 (4096, "done_idx", (1 << 33) + 5)],
                         ids=["256", "1024", "4096-env_id_base"])
def test_fast_kernel_equals_generic(gpu_device, n, force, env_id_base, storage):
    run_pair(gpu_device, n, storage, force, env_id_base)


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_a_wave_with_every_lane_done(gpu_device, storage):
    def start(sd):
        sd["status"][64:128] = gd.ST_DONE | gd.ST_CRASHED
        assert bool((sd["status"][64:128] & gd.ST_DONE).all()) and not bool((sd["status"][:64] & gd.ST_DONE).any())
    fast = run_pair(gpu_device, 1024, storage, "done_idx", start=start)
    assert bool((fast.episode[64:128] >= 1).all())


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_no_lane_done_at_the_start(gpu_device, storage):
    def start(sd):
        assert not bool((sd["status"] & gd.ST_DONE).any())
    run_pair(gpu_device, 1024, storage, "offset_obs", start=start)


# --------------------------------------------------------------------------
# dispatch
# --------------------------------------------------------------------------
def stepped(dev, n=512, cfg=None, acts3=False, lanes=None, **kw):
    """An env after one step of the given call shape."""
    step_kw = {k: kw.pop(k) for k in ("write_obs", "collect_done_idx") if k in kw}
    env = VecDroneEnv(n, device=dev, config=cfg or headline_config(), **kw)
    env.reset()
    count = n if lanes is None else lanes.stop - lanes.start
    a = torch.zeros((count, 3) if acts3 else (count,), device=dev, dtype=torch.float32 if acts3 else torch.uint8)
    env.step(a, lanes=lanes, **step_kw)
    torch.cuda.synchronize(dev)
    return env


def test_headline_shape_takes_the_fast_kernel(gpu_device):
    assert VecDroneEnv(512, device=gpu_device, config=headline_config()).last_step_kernel is None
    assert stepped(gpu_device).last_step_kernel == "fast"
    assert stepped(gpu_device, precision="f64").last_step_kernel == "fast"
    assert stepped(gpu_device, lanes=slice(256, 512)).last_step_kernel == "fast"  # rows 256.. start 16-byte aligned


OFF_HEADLINE = {
    "n=257": dict(n=257),
    "obs_4_bytes_off": dict(lanes=slice(1, 257)),  # 256 lanes whose rows start 60 bytes in: 4 bytes off a boundary
    "write_obs=False": dict(write_obs=False),
    "collect_done_idx": dict(collect_done_idx=True),
    "auto_reset=False": dict(cfg=headline_config(auto_reset=False)),
    "randomize_drone=False": dict(cfg=headline_config(randomize_drone=False)),
    "randomize_platform=False": dict(cfg=headline_config(randomize_platform=False)),
    "ping_pong": dict(ping_pong=True),
    "notebook_reward": dict(reward_mode="notebook"),
    "reinforce_reward": dict(reward_mode="reinforce"),
    "gravity=0.25": dict(cfg=headline_config(gravity=0.25)),
    "f32x3_actions": dict(acts3=True),
}


@pytest.mark.parametrize("case", list(OFF_HEADLINE.values()), ids=list(OFF_HEADLINE))
def test_every_other_shape_takes_the_generic_kernel(gpu_device, case):
    assert stepped(gpu_device, **case).last_step_kernel == "generic"


def test_empty_batch_takes_the_generic_kernel(gpu_device):
    env = stepped(gpu_device)
    k = abi.lib().dd_step_variant(ctypes.byref(env._cfg), ctypes.byref(env._state), ctypes.byref(env._io), 0)
    assert k == abi.DD_STEP_GENERIC


def test_residency_bound(gpu_device):
    """262,144 lanes still take the fast kernel; one tile more reports the generic one."""
    assert stepped(gpu_device, n=MAX_FAST).last_step_kernel == "fast"
    assert stepped(gpu_device, n=MAX_FAST + 256).last_step_kernel == "generic"
