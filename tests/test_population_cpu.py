"""CPU: dd_policy_rollout_population's host side (no GPU).

* abi.py binds the export with the header's signature, argument by argument;
* the header still says DD_ABI_VERSION 13 (the entry point is an addition) and
  states the contract; the built library exports the symbol;
* every argument error comes back as hipErrorInvalidValue before any GPU work
  (fake pointers throughout, as tests/test_eval_abi.py): the table's, the
  grouping's, and each of dd_policy_rollout_sampled's own;
* population_summary on a synthetic result (host tensors; exact means)."""
import ctypes
import math
import os
import re
import subprocess

import pytest
import torch

from delivery_drone_amd import abi, population_summary
from delivery_drone_amd.config import EnvConfig

EINVAL = 1  # hipErrorInvalidValue
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "dronestep.h")
NAME = "dd_policy_rollout_population"

# the C parameter types of the declaration -> what abi.py must bind
C_TO_CTYPES = {
    "const DDConfig *": ctypes.POINTER(abi.DDConfig), "const DDState *": ctypes.POINTER(abi.DDState),
    "const float *const *": ctypes.c_void_p, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64,
    "const DDPolicyRolloutIO *": ctypes.POINTER(abi.DDPolicyRolloutIO),
    "const DDSampling *": ctypes.POINTER(abi.DDSampling), "const DDEpisodeStats *": ctypes.POINTER(abi.DDEpisodeStats),
    "void *": ctypes.c_void_p,
}


def header_text(comments=True):
    text = open(HEADER).read()
    return text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_abi_binds_the_headers_signature():
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", header_text(comments=False))
    assert m, "the header does not declare " + NAME
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    types = [re.sub(r"\s*\b\w+$", "", p).strip() for p in params]  # drop the parameter's name
    names = [re.search(r"(\w+)$", p).group(1) for p in params]
    assert names == ["cfg", "st", "packed_table", "members", "lanes_per_member", "compute", "io", "sampling", "stats",
                     "n", "stream"]
    restype, argtypes = abi.EXPORTS[NAME]
    assert restype is ctypes.c_int
    assert argtypes == [C_TO_CTYPES[t] for t in types], types


def test_abi_version_stays_13_and_the_contract_is_written_down():
    header = header_text()
    assert re.search(r"#define\s+DD_ABI_VERSION\s+13\b", header)
    assert abi.DD_ABI_VERSION == 13 and abi.lib().dd_abi_version() == 13
    body = " ".join(re.sub(r"\n \* ?", " ", header).split())  # comment lines joined, their leading " * " dropped
    for text in ("members == 1 is dd_policy_rollout_sampled exactly", "bit for bit", "env_id_base + g L",
                 "DEVICE memory", "copies no weight", "not 8-byte-aligned packed_table", "members < 1",
                 "lanes_per_member < 1", "members * lanes_per_member != n"):
        assert text in body, text


def test_library_exports_the_symbol():
    out = subprocess.run(["nm", "-D", "--defined-only", abi.library_path()], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r"\bT " + NAME + "$", out, flags=re.M)
    assert hasattr(abi.lib(), NAME)


def _state(precision=abi.DD_F32):
    p = ctypes.c_void_p(8)
    return abi.DDState(p, p, p, p, p, p, p, p, p, p, p, p, p, 0, precision, 0)


def _io(frames=4, **kw):
    io = abi.DDPolicyRolloutIO()
    io.obs0 = io.reward = io.done = 8
    io.frames = frames
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def _run(table=64, members=2, lanes=3, n=6, compute=abi.DD_MLP_F16X3, io=None, sampling=None, stats=None, cfg=True,
         state=None):
    c = EnvConfig().to_abi()
    st = state if state is not None else _state()
    io = io if io is not None else _io()
    return abi.lib().dd_policy_rollout_population(
        ctypes.byref(c) if cfg else None, ctypes.byref(st), table, members, lanes, compute, ctypes.byref(io),
        ctypes.byref(sampling) if sampling is not None else None, ctypes.byref(stats) if stats is not None else None,
        n, None)


def test_table_and_grouping_errors_without_gpu():
    assert _run(table=None) == EINVAL
    assert _run(table=None, n=0) == EINVAL
    for misaligned in (1, 4, 68, 71):  # an array of pointers: 8-byte aligned
        assert _run(table=misaligned) == EINVAL, misaligned
        assert _run(table=misaligned, n=0) == EINVAL, misaligned
    for members in (0, -1, -2**31):
        assert _run(members=members) == EINVAL, members
        assert _run(members=members, n=0) == EINVAL, members
    for lanes in (0, -1, -2**63):
        assert _run(lanes=lanes) == EINVAL, lanes
        assert _run(lanes=lanes, n=0) == EINVAL, lanes
    # members * lanes_per_member != n, for n > 0
    for members, lanes, n in ((2, 3, 5), (2, 3, 7), (2, 3, 3), (3, 2, 4), (1, 5, 6), (2, 7, 6), (4, 2, 6),
                              (2, 2**62, 6), (2**31 - 1, 2**62, 6), (2, 2**63 - 1, 2**63 - 2)):
        assert _run(members=members, lanes=lanes, n=n) == EINVAL, (members, lanes, n)


def test_every_error_of_the_sampled_rollout_without_gpu():
    assert _run(cfg=False) == EINVAL
    assert _run(state=abi.DDState()) == EINVAL  # null SoA pointers
    assert _run(state=_state(precision=7)) == EINVAL
    assert _run(n=-1) == EINVAL
    assert _run(n=-6) == EINVAL
    assert _run(compute=5) == EINVAL
    assert _run(io=_io(frames=-1)) == EINVAL
    assert _run(io=_io(obs0=None)) == EINVAL  # frame 0's policy input is required
    assert _run(io=_io(reward=None)) == EINVAL  # per-frame buffers are optional only next to the statistics
    assert _run(io=_io(done=None)) == EINVAL
    assert _run(io=_io(engine_reward=8)) == EINVAL  # both or neither, and only in notebook mode
    assert _run(io=_io(engine_reward=8, engine_done=8)) == EINVAL
    assert _run(io=_io(shaped_mode=5)) == EINVAL
    for mode, t in ((3, 1.0), (-1, 1.0), (abi.DD_SAMPLE_TEMPERED, 0.0), (abi.DD_SAMPLE_TEMPERED, -0.5),
                    (abi.DD_SAMPLE_TEMPERED, math.nan), (abi.DD_SAMPLE_TEMPERED, math.inf)):
        assert _run(sampling=abi.DDSampling(mode, t, None)) == EINVAL, (mode, t)
        assert _run(sampling=abi.DDSampling(mode, t, None), n=0) == EINVAL, (mode, t)
    for k in range(1, 15):  # DDEpisodeStats: all four pointers or none
        ptrs = [8 if (k >> j) & 1 else None for j in range(4)]
        assert _run(stats=abi.DDEpisodeStats(*ptrs)) == EINVAL, ptrs


def test_nothing_to_do_without_gpu():
    """n == 0 and frames == 0 (with no final observation wanted) return before
    any launch, as they do in dd_policy_rollout_sampled."""
    assert _run(n=0) == 0
    assert _run(n=0, members=1, lanes=1) == 0
    assert _run(io=_io(frames=0)) == 0
    assert _run(io=_io(frames=0), members=1, lanes=6) == 0
    assert _run(io=_io(frames=0, reward=None, done=None)) == 0


def test_population_summary_on_a_synthetic_result():
    members, lanes = 3, 4
    n = members * lanes
    landed = torch.tensor([1, 0, 0, 1, 0, 0, 0, 0, 1, 1, 1, 1], dtype=torch.bool)
    res = {"landed": landed, "crashed": ~landed,
           "steps": torch.arange(n, dtype=torch.int32) * 3,
           "total_reward": torch.arange(n, dtype=torch.float64) * 0.25 - 1.0,   # sums exact in float64
           "final_fuel": torch.arange(n, dtype=torch.float32) * 0.5}
    got = population_summary(res, members)
    assert sorted(got) == ["mean_final_fuel", "mean_reward", "mean_steps", "success_rate"]
    for v in got.values():
        assert v.shape == (members,) and v.dtype == torch.float64
    assert got["success_rate"].tolist() == [0.5, 0.0, 1.0]
    assert got["mean_steps"].tolist() == [4.5, 16.5, 28.5]
    assert got["mean_reward"].tolist() == [-0.625, 0.375, 1.375]
    assert got["mean_final_fuel"].tolist() == [0.75, 2.75, 4.75]
    with pytest.raises(ValueError):
        population_summary(res, 5)
    with pytest.raises(ValueError):
        population_summary(res, 0)
