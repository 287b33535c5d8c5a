"""CPU: ABI 13's action-selection and episode-statistics surface
(DDSampling, DDEpisodeStats, dd_mlp_forward_sampled,
dd_policy_rollout_sampled): struct layouts, exports, and the argument errors,
each refused before any GPU work (fake pointers throughout)."""
import ctypes
import math
import os
import re
import subprocess

import pytest

from delivery_drone_amd import abi
from delivery_drone_amd.config import EnvConfig

EINVAL = 1  # hipErrorInvalidValue


def _state(precision=abi.DD_F32):
    p = ctypes.c_void_p(8)
    return abi.DDState(p, p, p, p, p, p, p, p, p, p, p, p, p, 0, precision, 0)


def test_struct_layouts_and_version():
    assert ctypes.sizeof(abi.DDSampling) == 4 + 4 + 8
    assert abi.DDSampling.probs_used.offset == 8
    assert ctypes.sizeof(abi.DDEpisodeStats) == 4 * 8
    assert (abi.DD_SAMPLE_BERNOULLI, abi.DD_SAMPLE_TEMPERED, abi.DD_SAMPLE_GREEDY) == (0, 1, 2)
    assert abi.DD_ABI_VERSION == 13 and abi.lib().dd_abi_version() == 13
    # the structs that were there before keep their layouts
    assert ctypes.sizeof(abi.DDPolicyRolloutIO) == 7 * 8 + 8 + 8 + 4 + 4 + 3 * 8 + 8
    assert ctypes.sizeof(abi.DDMlpIO) == 4 * 8 + 3 * 8


def test_new_exports_are_present():
    out = subprocess.run(["nm", "-D", "--defined-only", abi.library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (dd_[a-z0-9_]+)$", out, flags=re.M))
    assert {"dd_mlp_forward_sampled", "dd_policy_rollout_sampled"} <= exported
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(repo, "include", "dronestep.h")).read()
    for name in ("DDSampling", "DDEpisodeStats", "DD_SAMPLE_TEMPERED", "dd_mlp_forward_sampled",
                 "dd_policy_rollout_sampled"):
        assert name in header, name


def test_sampling_mode_mapping():
    assert abi.sampling_mode(1.0) == abi.DD_SAMPLE_BERNOULLI
    assert abi.sampling_mode(0) == abi.DD_SAMPLE_GREEDY
    assert abi.sampling_mode(0.3) == abi.DD_SAMPLE_TEMPERED
    assert abi.sampling_mode(2.0) == abi.DD_SAMPLE_TEMPERED
    for bad in (-1.0, float("nan"), float("inf"), -0.5, "hot", None):
        with pytest.raises(ValueError):
            abi.sampling_mode(bad)


BAD_SAMPLINGS = [(3, 1.0), (-1, 1.0), (abi.DD_SAMPLE_TEMPERED, 0.0), (abi.DD_SAMPLE_TEMPERED, -0.5),
                 (abi.DD_SAMPLE_TEMPERED, math.nan), (abi.DD_SAMPLE_TEMPERED, math.inf)]


def test_forward_sampled_argument_errors_without_gpu():
    lib = abi.lib()
    io = abi.DDMlpIO(8, 8, 8, 8, 0, 0, 0)

    def run(sampling, out_dim=3, packed=16, compute=abi.DD_MLP_F32, n=4, io_=io):
        return lib.dd_mlp_forward_sampled(packed, compute, out_dim, ctypes.byref(io_) if io_ is not None else None,
                                          ctypes.byref(sampling) if sampling is not None else None, n, None)

    for mode, t in BAD_SAMPLINGS:  # an unknown mode; TEMPERED with T not finite or <= 0
        assert run(abi.DDSampling(mode, t, None)) == EINVAL, (mode, t)
        assert run(abi.DDSampling(mode, t, None), n=0) == EINVAL, (mode, t)  # checked before the empty batch returns
    critic_io = abi.DDMlpIO(8, 8, None, None, 0, 0, 0)
    for mode in (abi.DD_SAMPLE_BERNOULLI, abi.DD_SAMPLE_TEMPERED, abi.DD_SAMPLE_GREEDY):  # sampling with out_dim 1
        assert run(abi.DDSampling(mode, 0.5, None), out_dim=1, io_=critic_io) == EINVAL
    ok = abi.DDSampling(abi.DD_SAMPLE_TEMPERED, 0.5, None)
    # the old entry point's own checks still hold through the new one
    assert run(ok, io_=None) == EINVAL
    assert run(ok, n=-1) == EINVAL
    assert run(ok, compute=5) == EINVAL
    assert run(ok, out_dim=2) == EINVAL
    assert run(ok, packed=None) == EINVAL
    assert run(ok, packed=8) == EINVAL  # 16-byte fragments
    assert run(ok, n=0) == 0  # a valid call on an empty batch: nothing to do
    assert run(None, n=0) == 0  # sampling NULL: dd_mlp_forward


def test_policy_rollout_sampled_argument_errors_without_gpu():
    lib = abi.lib()
    cfg = EnvConfig().to_abi()
    io = abi.DDPolicyRolloutIO()
    io.obs0 = io.reward = io.done = 8
    io.frames = 4

    def run(sampling=None, stats=None, packed=16, compute=abi.DD_MLP_F16X3, n=4):
        return lib.dd_policy_rollout_sampled(ctypes.byref(cfg), ctypes.byref(_state()), packed, compute,
                                             ctypes.byref(io), ctypes.byref(sampling) if sampling is not None else None,
                                             ctypes.byref(stats) if stats is not None else None, n, None)

    for mode, t in BAD_SAMPLINGS:
        assert run(abi.DDSampling(mode, t, None)) == EINVAL, (mode, t)
        assert run(abi.DDSampling(mode, t, None), n=0) == EINVAL, (mode, t)
    # a DDEpisodeStats with some but not all pointers set
    for k in range(1, 15):
        ptrs = [8 if (k >> j) & 1 else None for j in range(4)]
        assert run(stats=abi.DDEpisodeStats(*ptrs)) == EINVAL, ptrs
    full = abi.DDEpisodeStats(8, 8, 8, 8)
    ok = abi.DDSampling(abi.DD_SAMPLE_GREEDY, 0.0, None)
    assert run(ok, full, packed=None) == EINVAL
    assert run(ok, full, packed=8) == EINVAL
    assert run(ok, full, compute=7) == EINVAL
    assert run(ok, full, n=-1) == EINVAL
    io.reward = io.done = None  # per-frame buffers are optional only with the statistics
    assert run(ok, None) == EINVAL
    assert run(None, abi.DDEpisodeStats()) == EINVAL  # all four NULL: no statistics
    assert run(ok, full, n=0) == 0
    io.frames = 0
    assert run(ok, full) == 0  # no frames and no final observation wanted: nothing to do
    io.frames = -1
    assert run(ok, full) == EINVAL
