"""CPU: the training-batch surface without a GPU.  The NumPy restatement
(tests/train_batch_ref.py) against the notebooks' own results
(tests/golden/train_batch/ragged.npz), the fixture's regeneration, and the C
ABI of csrc/train_batch.hip: struct layouts, exports, argument errors (fake
pointers throughout; every error is returned before any launch)."""
import ctypes
import filecmp
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import train_batch_ref as ref
from delivery_drone_amd import abi
import delivery_drone_amd
import delivery_drone_amd.train_batch as tb

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "train_batch")
REF = os.environ.get("RL101_REFERENCE", "/root/reference")
EINVAL = 1  # hipErrorInvalidValue


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "ragged.npz"))


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "Actor_Critic_PPO.ipynb")),
                    reason="reference checkout absent")
def test_fixture_regenerates_byte_identically(tmp_path):
    subprocess.run([sys.executable, "-B", os.path.join(GOLDEN, "make_train_batch_golden.py"), "--out", str(tmp_path)],
                   check=True, capture_output=True, timeout=300)
    assert os.listdir(tmp_path) == ["ragged.npz"]
    assert filecmp.cmp(tmp_path / "ragged.npz", os.path.join(GOLDEN, "ragged.npz"), shallow=False)
    assert os.path.getsize(os.path.join(GOLDEN, "ragged.npz")) < 100 * 1024


def test_fixture_covers_the_edge_lengths(g):
    T = g["done"].shape[0]
    ln, e = g["length"], g["ended"]
    assert T == 37 and 1 in ln and 2 in ln
    assert ((ln == T) & (e == 1)).any() and ((ln == T) & (e == 0) & (g["bootstrap"] != 0)).any()
    assert np.abs(g["reward"]).max() > 500.0 and (g["reward"] == -500.0).any()


def test_plan_matches_the_notebook_episodes(g):
    ln, off, e = ref.plan(g["done"])
    assert ln.dtype == np.int32 and off.dtype == np.int64 and e.dtype == np.uint8
    assert np.array_equal(ln, g["length"]) and np.array_equal(e, g["ended"])
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(g["length"])]))
    assert off[-1] == len(g["gae_advantages"])


def test_gae_and_returns_are_bit_equal_to_the_notebooks(g):
    ln, off, e = ref.plan(g["done"])
    values = ref.gather(g["values"], ln)
    adv, ret = ref.gae_flat(g["reward"], values, ln, off, e, g["bootstrap"], float(g["gamma"]), float(g["lam"]))
    assert np.array_equal(adv, g["gae_advantages"]) and np.array_equal(ret, g["gae_returns"])
    assert np.array_equal(ref.returns_flat(g["reward"], ln, off, float(g["gamma"])), g["reinforce_returns"])
    assert np.array_equal(ref.episode_return(g["reward"], ln), g["episode_return"])
    # the reward as float32 storage: the same GAE (compute_gae rounds it first)
    adv32, _ = ref.gae_flat(g["reward"].astype(np.float32), values, ln, off, e, g["bootstrap"], float(g["gamma"]),
                            float(g["lam"]))
    assert np.array_equal(adv32, adv)


def test_normalised_values_match_the_notebooks_float32(g):
    """The notebooks normalise in float32 (torch's mean / std of a float32
    tensor), the restatement in float64.  Measured on this fixture (826 rows,
    CPU torch): max |notebook - restatement| = 2^-22 = 2.38e-7 for both the
    PPO advantages (max |value| 2.42) and the REINFORCE ones (1.76), i.e. 2
    float32 ulps of the largest values.  That deviation is the float32
    reduction's, a property of the reference; it is the bound here."""
    bound = 2.0 ** -22
    for raw, want in ((g["gae_advantages"], g["gae_normalized"]), (g["reinforce_returns"], g["reinforce_normalized"])):
        _, _, out = ref.normalize(raw)
        assert out.dtype == np.float32
        assert np.abs(out.astype(np.float64) - want.astype(np.float64)).max() <= bound
    mean, std, _ = ref.normalize(g["reinforce_returns"])
    assert abs(mean - float(g["reinforce_baseline"])) <= np.spacing(np.float32(abs(mean)))
    assert abs(std - float(g["reinforce_std"])) <= np.spacing(np.float32(std))
    m1, s1, o1 = ref.normalize(np.array([3.0], dtype=np.float32))  # M < 2: NaN, as torch.std's
    assert m1 == 3.0 and np.isnan(s1) and np.isnan(o1).all()


def test_gather_helpers():
    x = np.arange(12).reshape(4, 3)
    ln = np.array([2, 4, 1], dtype=np.int32)
    flat = ref.gather(x, ln)
    assert flat.tolist() == [0, 3, 1, 4, 7, 10, 2]
    assert ref.scatter(flat, ln, 4, fill=-1)[:, 0].tolist() == [0, 3, -1, -1]
    assert ref.actions_f32([0, 1, 2, 4, 7]).tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]]


# ---- the C ABI ---------------------------------------------------------------

def test_struct_layouts_match_the_header():
    assert ctypes.sizeof(abi.DDBatchLayout) == 3 * 8
    assert ctypes.sizeof(abi.DDBatchGatherIO) == 6 * 8 + 4 + 4
    assert abi.DDBatchGatherIO.tile_frames.offset == 48
    assert ctypes.sizeof(abi.DDBatchAdvIO) == 8 + 4 + 4 + 5 * 8 + 2 * 8
    assert abi.DDBatchAdvIO.mode.offset == 12 and abi.DDBatchAdvIO.gamma.offset == 56
    assert (abi.DD_BATCH_GAE, abi.DD_BATCH_RETURNS) == (0, 1)
    header = open(os.path.join(os.path.dirname(HERE), "include", "dronestep.h")).read()
    for cls in (abi.DDBatchLayout, abi.DDBatchGatherIO, abi.DDBatchAdvIO):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cls.__name__, cls.__name__), header, flags=re.S).group(1)
        names = re.findall(r"(\w+);", body)
        assert names == [n.rstrip("_") if n != "_pad" else n for n, _ in cls._fields_], cls.__name__
    assert "#define DD_BATCH_GAE 0" in header and "#define DD_BATCH_RETURNS 1" in header
    assert abi.DD_ABI_VERSION == 13  # additions only


def test_library_exports_the_new_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", abi.library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (dd_[a-z0-9_]+)$", out, flags=re.M))
    assert {"dd_batch_workspace", "dd_batch_plan", "dd_batch_gather", "dd_batch_advantages",
            "dd_batch_normalize"} <= exported
    assert {"ppo_batch", "reinforce_batch", "collect_ppo"} <= set(delivery_drone_amd.__all__)
    assert delivery_drone_amd.ppo_batch is tb.ppo_batch


def test_workspace_size():
    lib = abi.lib()
    assert lib.dd_batch_workspace(0) == lib.dd_batch_workspace(1) == 8 * 1024  # the statistics' partial sums
    assert lib.dd_batch_workspace(256 * 1024) == 8 * 1024
    assert lib.dd_batch_workspace(256 * 1024 + 1) == 8 * 1025  # one int64 per 256-lane tile


def test_plan_argument_errors_without_gpu():
    lib = abi.lib()
    lay = abi.DDBatchLayout(8, 8, 8)

    def plan(done=8, T=4, n=4, layout=lay, ws=8):
        return lib.dd_batch_plan(done, T, n, ctypes.byref(layout) if layout is not None else None, ws, None)

    assert plan(done=None) == EINVAL
    assert plan(T=-1) == EINVAL
    assert plan(n=-1) == EINVAL
    assert plan(T=2 ** 31) == EINVAL
    assert plan(n=2 ** 31) == EINVAL
    assert plan(layout=None) == EINVAL
    assert plan(ws=None) == EINVAL
    for k in range(3):
        ptrs = [8, 8, 8]
        ptrs[k] = None
        assert plan(layout=abi.DDBatchLayout(*ptrs)) == EINVAL, k


def test_gather_argument_errors_without_gpu():
    lib = abi.lib()
    lay = abi.DDBatchLayout(8, 8, 8)

    def gather(io, T=4, n=4, layout=lay):
        return lib.dd_batch_gather(ctypes.byref(layout) if layout is not None else None,
                                   ctypes.byref(io) if io is not None else None, T, n, None)

    full = (16, 16, 16, 16, 16, 16)
    assert gather(None) == EINVAL
    assert gather(abi.DDBatchGatherIO(*full, 0, 0), layout=None) == EINVAL
    assert gather(abi.DDBatchGatherIO(*full, 0, 0), layout=abi.DDBatchLayout(8, None, 8)) == EINVAL
    assert gather(abi.DDBatchGatherIO(*full, 0, 0), T=-1) == EINVAL
    assert gather(abi.DDBatchGatherIO(*full, 0, 0), n=-1) == EINVAL
    for k in range(6):  # an input without its output, an output without its input
        ptrs = list(full)
        ptrs[k] = None
        assert gather(abi.DDBatchGatherIO(*ptrs, 0, 0)) == EINVAL, k
    for frames in (-8, 4, 12, 32):
        assert gather(abi.DDBatchGatherIO(*full, frames, 0)) == EINVAL, frames
    assert gather(abi.DDBatchGatherIO(*full, 16, 0), T=0) == 0  # nothing to gather
    assert gather(abi.DDBatchGatherIO(*full, 8, 0), n=0) == 0
    assert gather(abi.DDBatchGatherIO(None, None, None, None, None, None, 0, 0)) == 0


def test_advantages_argument_errors_without_gpu():
    lib = abi.lib()
    lay = abi.DDBatchLayout(8, 8, 8)

    def adv(T=4, n=4, layout=lay, io_none=False, **kw):
        f = dict(reward=8, precision=abi.DD_F32, mode=abi.DD_BATCH_GAE, values=8, bootstrap=None, advantages=8,
                 returns=8, episode_return=8, gamma=0.99, lambda_=0.95)
        f.update(kw)
        io = abi.DDBatchAdvIO(*[f[name] for name, _ in abi.DDBatchAdvIO._fields_])
        return lib.dd_batch_advantages(ctypes.byref(layout) if layout is not None else None,
                                       None if io_none else ctypes.byref(io), T, n, None)

    assert adv(io_none=True) == EINVAL
    assert adv(layout=None) == EINVAL
    assert adv(layout=abi.DDBatchLayout(None, 8, 8)) == EINVAL
    assert adv(T=-1) == EINVAL
    assert adv(n=-1) == EINVAL
    assert adv(mode=2) == EINVAL and adv(mode=-1) == EINVAL
    assert adv(precision=2) == EINVAL and adv(precision=-1) == EINVAL
    assert adv(values=None) == EINVAL  # GAE needs the critic's values
    assert adv(advantages=None) == EINVAL
    assert adv(reward=None) == EINVAL
    assert adv(mode=abi.DD_BATCH_RETURNS, returns=None) == EINVAL
    assert adv(mode=abi.DD_BATCH_RETURNS, reward=None, values=None, advantages=None) == EINVAL
    assert adv(mode=2, n=0) == EINVAL  # checked before the empty batch returns
    assert adv(n=0) == 0
    assert adv(mode=abi.DD_BATCH_RETURNS, values=None, advantages=None, n=0) == 0


def test_normalize_argument_errors_without_gpu():
    lib = abi.lib()
    assert lib.dd_batch_normalize(None, 8, 4, 8, 8, 8, None) == EINVAL
    assert lib.dd_batch_normalize(8, 8, -1, 8, 8, 8, None) == EINVAL
    assert lib.dd_batch_normalize(8, 8, 4, None, 8, 8, None) == EINVAL
    assert lib.dd_batch_normalize(8, 8, 4, 8, None, 8, None) == EINVAL
    assert lib.dd_batch_normalize(8, 8, 4, 8, 8, None, None) == EINVAL


def test_python_wrappers_check_before_the_gpu():
    import torch
    done = torch.zeros(4, 3, dtype=torch.bool)
    with pytest.raises(ValueError, match="GPU"):
        tb.reinforce_batch(None, None, torch.zeros(4, 3), done)
    with pytest.raises(ValueError, match=r"\[T, N\]"):
        tb.reinforce_batch(None, None, torch.zeros(4), torch.zeros(4, dtype=torch.bool))
