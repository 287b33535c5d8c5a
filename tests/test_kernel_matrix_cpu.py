"""CPU: the dd_step / dd_rollout kernel matrix, and its name-set check
against the build.

dd_step compiles to step_kernel / step_pp_kernel<T, AFMT, kRef, kShape> (72
kernels), dd_rollout to rollout_kernel<T, AFMT, kRef, kHeld, kShape, kSplit>
(104).  This module restates, in Python, the host dispatch that picks one of
them from a call's run-time values (csrc/step.hip step_chunks, csrc/rollout.hip
rollout_chunks / rollout_kernel_for / launch_rollout, csrc/launch.h shape_of,
csrc/frame.h uses_reference_physics), enumerates the cases the GPU matrix
tests run (step_matrix, rollout_matrix) and maps each case to the template
arguments it must select (step_kernel_for, rollout_kernel_for).
tests/test_gpu_step_matrix.py and tests/test_gpu_rollout_matrix.py
parametrise over the same functions, so a kernel with no case, or a case that
names no kernel, fails here without a GPU.

Reference: the build itself.  The kernel symbols are read from the
`.amdhsa_kernel` lines of the built _native/step.s and _native/rollout.s and
their template arguments from the mangled name's I...E run; nothing else of
the assembly is read.  Bounds: none, the two name sets must be equal (72 and
104).  A missing .s is a failure: the session fixture builds it."""
import os
import re
from collections import namedtuple

import pytest

from delivery_drone_amd import EnvConfig
from test_gpu_eval_matrix import MODES, PHYSICS, STORAGE

NATIVE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "reinforcement-learning-101_amd",
                      "delivery_drone_amd", "_native")

# include/dronestep.h DD_ACT_*, csrc/frame.h kShape*
ACT = {"bitmask": 0, "f32x3": 1, "u8x3": 2, "philox": 3}
SHAPE = {"engine": 0, "notebook": 1, "reinforce": 2}
ACT_NAME = {v: k for k, v in ACT.items()}
SHAPE_NAME = {0: "none", 1: "ppo", 2: "reinforce"}
STEP_FORMATS = ("bitmask", "f32x3", "u8x3")
ROLLOUT_FORMATS = STEP_FORMATS + ("philox",)
OTHER_PHYSICS = tuple(p for p in PHYSICS if p != "reference")

# the fields uses_reference_physics compares: DDConfig gravity .. angle_scale (every double) but wind_x / wind_y
_PHYSICS_FIELDS = ("gravity", "drag", "angular_drag", "main_thrust_power", "side_thrust_power", "fuel_main",
                   "fuel_side", "max_fuel", "drone_half_height", "dt", "platform_half_width", "platform_half_height",
                   "platform_speed", "platform_min_x", "platform_max_x", "max_landing_velocity", "max_landing_angle",
                   "world_width", "world_height", "oob_margin", "ground_level", "reward_step", "reward_landing",
                   "reward_crash", "reward_out_of_fuel", "reward_out_of_bounds", "shaping_offset", "shaping_scale",
                   "vel_scale", "angle_scale")

StepKey = namedtuple("StepKey", "name T afmt ref shape")
RolloutKey = namedtuple("RolloutKey", "T afmt ref held shape split")
StepCase = namedtuple("StepCase", "storage fmt physics mode ping_pong")
RolloutCase = namedtuple("RolloutCase", "storage fmt physics mode kind n kernel")


def uses_reference_physics(cfg: EnvConfig) -> bool:
    """csrc/frame.h: the world constants folded into the instruction stream
    apply when no switch is on and every constant is the default's double."""
    if cfg.wind_enabled or cfg.platform_moving:
        return False
    ref = EnvConfig()
    return all(float(getattr(cfg, f)) == float(getattr(ref, f)) for f in _PHYSICS_FIELDS)


def shape_of(mode: str, has_hist: bool, has_shaped_reward: bool = False) -> int:
    """csrc/launch.h shape_of: REINFORCE's reward by its mode, PPO's when a
    history (dd_step: or shaped_reward) pointer is set, else none.  `mode` is
    VecDroneEnv's reward_mode: "engine" and "notebook" both send DD_SHAPED_PPO."""
    if mode == "reinforce":
        return SHAPE["reinforce"]
    return SHAPE["notebook"] if has_hist or has_shaped_reward else SHAPE["engine"]


def config_of(physics: str, **switches) -> EnvConfig:
    return EnvConfig(**PHYSICS[physics], **switches)


def step_kernel_for(case: StepCase) -> StepKey:
    """step_chunks: with_bool(ref), with_value(shape), with_value(action
    format), and launch_step's `state_out` switch."""
    ref = uses_reference_physics(config_of(case.physics))
    # VecDroneEnv passes the history in "notebook" mode only, shaped_reward in both notebook modes
    shape = shape_of(case.mode, case.mode == "notebook", case.mode != "engine")
    return StepKey("step_pp_kernel" if case.ping_pong else "step_kernel", case.storage, ACT[case.fmt], ref, shape)


def rollout_kind(ref: bool, shape: int, fmt: str, actions_addr: int, obs_addr: int, n: int, *, write_obs=True,
                 kernel="auto", blocks_fit=True) -> str:
    """rollout_kernel_for: held needs every frame row 16-byte aligned (obs
    aligned, n % 4 == 0) and, for bitmask actions, a 4-byte aligned action
    buffer; split is the held path of the reference world with the engine
    reward, observations written, unless kernel="single" or the launch has
    more blocks than the device has CUs (`blocks_fit`)."""
    held = obs_addr % 16 == 0 and n % 4 == 0 and (fmt != "bitmask" or actions_addr % 4 == 0)
    if ref and shape == SHAPE["engine"] and held and write_obs and obs_addr != 0 and kernel != "single" and blocks_fit:
        return "split"
    return "held" if held else "flushed"


def rollout_kernel_for(case: RolloutCase) -> RolloutKey:
    """rollout_chunks + launch_rollout: the kind picks kHeld / kSplit, the
    rest as dd_step (the history pointer alone decides PPO's shape)."""
    ref = uses_reference_physics(config_of(case.physics))
    shape = shape_of(case.mode, case.mode == "notebook")
    split = case.kind == "split"
    assert not split or (ref and shape == SHAPE["engine"]), case
    return RolloutKey(case.storage, ACT[case.fmt], ref, case.kind != "flushed", shape, split)


def _other(*axes) -> str:
    """The non-reference physics of a non-anchor case: spread over the three."""
    return OTHER_PHYSICS[sum(hash_free(a) for a in axes) % len(OTHER_PHYSICS)]


def hash_free(a) -> int:
    return sum(str(a).encode())  # (str hashes are salted per process: case ids must not move)


def step_matrix():
    """Every dd_step case: the anchors (in-place bitmask) under all four
    physics, every other kernel under the reference physics and one other."""
    cases = []
    for storage in STORAGE:
        for mode in MODES:
            for fmt in STEP_FORMATS:
                for pp in (False, True):
                    anchor = fmt == "bitmask" and not pp
                    for physics in (tuple(PHYSICS) if anchor else ("reference", _other(storage, mode, fmt, pp))):
                        cases.append(StepCase(storage, fmt, physics, mode, pp))
    return cases


def is_anchor(case: StepCase) -> bool:
    return case.fmt == "bitmask" and not case.ping_pong


def rollout_matrix():
    """Every dd_rollout case.  Flushed: 515 lanes (n % 4 != 0).  Held: 520
    lanes, kernel="single" where "auto" would take the split kernel.  Split:
    520 lanes (3 blocks, under any CU count), reference physics, engine reward."""
    cases = []
    for storage in STORAGE:
        for mode in MODES:
            for fmt in ROLLOUT_FORMATS:
                for kind in ("flushed", "held"):
                    for physics in ("reference", _other(storage, mode, fmt, kind)):
                        would_split = kind == "held" and physics == "reference" and mode == "engine"
                        cases.append(RolloutCase(storage, fmt, physics, mode, kind, 515 if kind == "flushed" else 520,
                                                 "single" if would_split else "auto"))
                if mode == "engine":
                    cases.append(RolloutCase(storage, fmt, "reference", mode, "split", 520, "auto"))
    return cases


def step_id(case: StepCase) -> str:
    k = step_kernel_for(case)
    return (f"{k.name}<{k.T},{ACT_NAME[k.afmt]},{'kRef' if k.ref else 'call'},{SHAPE_NAME[k.shape]}>"
            f"-{case.physics}")


def rollout_id(case: RolloutCase) -> str:
    k = rollout_kernel_for(case)
    return (f"rollout_kernel<{k.T},{ACT_NAME[k.afmt]},{'kRef' if k.ref else 'call'},"
            f"{'held' if k.held else 'flushed'},{SHAPE_NAME[k.shape]},{'split' if k.split else 'single'}>"
            f"-{case.physics}")


# --------------------------------------------------------------------------
# the build's kernel names
# --------------------------------------------------------------------------
_KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+_ZN2dd\d+(step_kernel|step_pp_kernel|rollout_kernel)I([fd])((?:L[ib]\d+E)+)E")


def built_kernels(unit: str):
    """[(kernel name, storage, template values...)] of one unit's device
    assembly, from its .amdhsa_kernel lines."""
    path = os.path.join(NATIVE, unit + ".s")
    assert os.path.exists(path), f"{path} is missing: the build (make, run by the session fixture) writes it"
    found = []
    with open(path) as f:
        for line in f:
            if ".amdhsa_kernel" not in line:
                continue
            m = _KERNEL.match(line)
            assert m, f"unparsed kernel symbol in {unit}.s: {line.strip()}"
            args = [int(v) if t == "i" else bool(int(v)) for t, v in re.findall(r"L([ib])(\d+)E", m.group(3))]
            found.append((m.group(1), {"f": "f32", "d": "f64"}[m.group(2)], *args))
    return found


def test_step_kernels_equal_the_matrix():
    built = built_kernels("step")
    assert all(len(b) == 5 for b in built), [b for b in built if len(b) != 5]
    names = {StepKey(*b) for b in built}
    assert len(built) == len(names) == 72, len(built)
    keys = {step_kernel_for(c) for c in step_matrix()}
    assert keys == names, (sorted(keys - names), sorted(names - keys))


def test_rollout_kernels_equal_the_matrix():
    built = built_kernels("rollout")
    assert all(b[0] == "rollout_kernel" and len(b) == 7 for b in built), [b for b in built if len(b) != 7]
    names = {RolloutKey(*b[1:]) for b in built}
    assert len(built) == len(names) == 104, len(built)
    keys = {rollout_kernel_for(c) for c in rollout_matrix()}
    assert keys == names, (sorted(keys - names), sorted(names - keys))


def test_matrix_cases_are_distinct_and_name_their_kernel():
    for cases, ident in ((step_matrix(), step_id), (rollout_matrix(), rollout_id)):
        ids = [ident(c) for c in cases]
        assert len(set(ids)) == len(ids)
    assert sum(is_anchor(c) for c in step_matrix()) == 24


def test_reference_physics_rule():
    assert uses_reference_physics(EnvConfig(randomize_drone=True, auto_reset=True, seed=9))
    assert uses_reference_physics(EnvConfig(wind_x=0.05))  # wind off: its components are not compared
    for p in OTHER_PHYSICS:
        assert not uses_reference_physics(config_of(p)), p
    assert not uses_reference_physics(EnvConfig(angle_scale=180.0, vel_scale=10.5))
    assert not uses_reference_physics(EnvConfig(angle_scale=90.0))  # the observation's column 4 divides by it


@pytest.mark.parametrize("case", rollout_matrix(), ids=rollout_id)
def test_rollout_case_predicts_its_kind(case):
    """With aligned buffers a case's lane count and `kernel` choice give the kind it names."""
    k = rollout_kernel_for(case)
    assert rollout_kind(k.ref, k.shape, case.fmt, 4096, 4096, case.n, kernel=case.kernel) == case.kind
    # the two other routes to flushed at 520 lanes
    assert rollout_kind(k.ref, k.shape, case.fmt, 4096, 4100, 520, kernel=case.kernel) == "flushed"
    aligned = rollout_kind(k.ref, k.shape, case.fmt, 4096, 4096, 520, kernel=case.kernel)
    assert aligned in ("held", "split")
    assert rollout_kind(k.ref, k.shape, case.fmt, 4097, 4096, 520, kernel=case.kernel) == \
        ("flushed" if case.fmt == "bitmask" else aligned)
