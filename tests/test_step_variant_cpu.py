"""CPU: dd_step_variant, the host's choice between dd_step's two kernel
families (csrc/step_tile.h step_variant_of, used by step.hip's step_chunks).

The fast kernel (csrc/step_fast.hip) hard-wires the headline shape; a call
that differs from it in any one respect must take the generic matrix.  Host
logic only: the pointers are made-up addresses and are never dereferenced.
Reference: the rule as include/dronestep.h states it.  Bounds: none, the
answers are exact."""
import ctypes
import dataclasses
import re

import pytest

from delivery_drone_amd import EnvConfig, abi
from test_abi import HEADER, _state

HEADLINE_CFG = EnvConfig(randomize_drone=True, randomize_platform=True, auto_reset=True, seed=0)
N = 262_144
MAX_FAST = 1 << 18  # csrc/step_tile.h kStepFastMaxLanes


def headline_io():
    io = abi.DDStepIO()
    io.actions, io.reward, io.done = 4096, 8192, 12288
    io.obs = 1 << 20  # 16-byte aligned
    io.action_format = abi.DD_ACT_BITMASK
    io.shaped_mode = abi.DD_SHAPED_PPO
    return io


def variant(cfg=HEADLINE_CFG, io=None, n=N, precision=abi.DD_F32):
    c = cfg.to_abi()
    st = _state(4096, precision)
    return abi.lib().dd_step_variant(ctypes.byref(c), ctypes.byref(st), ctypes.byref(io or headline_io()), n)


def test_exported_and_declared():
    header = open(HEADER).read()
    assert re.search(r"int32_t\s+dd_step_variant\s*\(", header)
    assert abi.EXPORTS["dd_step_variant"][0] is ctypes.c_int32
    assert (abi.DD_STEP_GENERIC, abi.DD_STEP_FAST) == (0, 1)
    assert abi.DD_ABI_VERSION == 13 and abi.lib().dd_abi_version() == 13  # an addition only


@pytest.mark.parametrize("precision", [abi.DD_F32, abi.DD_F64])
def test_headline_shape_takes_the_fast_kernel(precision):
    assert variant(precision=precision) == abi.DD_STEP_FAST
    assert variant(n=256, precision=precision) == abi.DD_STEP_FAST
    assert variant(n=MAX_FAST, precision=precision) == abi.DD_STEP_FAST


@pytest.mark.parametrize("n", [0, 1, 255, 257, N + 64, MAX_FAST + 256, 16_777_216])
def test_other_sizes_take_the_generic_kernel(n):
    """No whole tiles, an empty batch, or a batch past the residency bound."""
    assert variant(n=n) == abi.DD_STEP_GENERIC


@pytest.mark.parametrize("switch", ["auto_reset", "randomize_drone", "randomize_platform"])
def test_each_switch_off_takes_the_generic_kernel(switch):
    assert variant(cfg=dataclasses.replace(HEADLINE_CFG, **{switch: False})) == abi.DD_STEP_GENERIC


@pytest.mark.parametrize("change", [dict(gravity=0.25), dict(wind_enabled=True), dict(platform_moving=True),
                                    dict(max_fuel=500.0)], ids=lambda c: next(iter(c)))
def test_non_reference_physics_takes_the_generic_kernel(change):
    assert variant(cfg=dataclasses.replace(HEADLINE_CFG, **change)) == abi.DD_STEP_GENERIC


def test_spawn_ranges_and_seed_stay_on_the_fast_kernel():
    """They come from the call, not from the kernel's constants."""
    cfg = dataclasses.replace(HEADLINE_CFG, seed=12345, drone_x_min=200, drone_x_max=300, platform_y_lo=300)
    assert variant(cfg=cfg) == abi.DD_STEP_FAST


def _with(**fields):
    io = headline_io()
    for k, v in fields.items():
        setattr(io, k, v)
    return io


@pytest.mark.parametrize("fields", [
    dict(obs=None),                                     # write_obs=False
    dict(obs=(1 << 20) + 4),                            # rows 4 bytes off a 16-byte boundary
    dict(obs=(1 << 20) + 60),                           # a one-row-offset view
    dict(done_idx=4096, done_count=8192),               # collect_done_idx
    dict(state_out=4096),                               # ping-pong
    dict(action_format=abi.DD_ACT_F32X3),
    dict(action_format=abi.DD_ACT_U8X3),
    dict(shaped_hist=4096, shaped_reward=4096, shaped_done=4096),   # the PPO notebook reward
    dict(shaped_mode=abi.DD_SHAPED_REINFORCE, shaped_reward=4096, shaped_done=4096),
], ids=lambda f: ",".join(f))
def test_each_call_shape_off_the_headline_takes_the_generic_kernel(fields):
    assert variant(io=_with(**fields)) == abi.DD_STEP_GENERIC


def test_done_count_alone_keeps_the_fast_kernel():
    """dd_step only clears done_count; without done_idx no kernel reads it."""
    assert variant(io=_with(done_count=8192)) == abi.DD_STEP_FAST


def test_invalid_arguments():
    lib = abi.lib()
    c, st, io = HEADLINE_CFG.to_abi(), _state(4096), headline_io()
    assert lib.dd_step_variant(None, ctypes.byref(st), ctypes.byref(io), N) == -1
    assert lib.dd_step_variant(ctypes.byref(c), None, ctypes.byref(io), N) == -1
    assert lib.dd_step_variant(ctypes.byref(c), ctypes.byref(st), None, N) == -1
    assert lib.dd_step_variant(ctypes.byref(c), ctypes.byref(st), ctypes.byref(io), -1) == -1
    assert lib.dd_step_variant(ctypes.byref(c), ctypes.byref(st), ctypes.byref(io), 2**31) == -1
