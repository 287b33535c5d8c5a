"""CPU: the every-episode training batch without a GPU.  The NumPy restatement
(tests/episodes_ref.py) against the notebooks' own results on a rollout with
several episodes per lane (tests/golden/train_batch_episodes/multi.npz), the
fixture's regeneration and coverage, and the C ABI of
csrc/train_batch_episodes.hip: struct layout, exports, the workspace size,
argument errors (fake pointers throughout; every error is returned before any
launch)."""
import ctypes
import filecmp
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import episodes_ref as eref
from delivery_drone_amd import abi
import delivery_drone_amd
import delivery_drone_amd.train_batch as tb

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "train_batch_episodes")
REF = os.environ.get("RL101_REFERENCE", "/root/reference")
EINVAL = 1  # hipErrorInvalidValue


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "multi.npz"))


@pytest.fixture(scope="module")
def lay(g):
    return eref.layout(g["done"], g["done_before"])


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "Actor_Critic_PPO.ipynb")),
                    reason="reference checkout absent")
def test_fixture_regenerates_byte_identically(tmp_path):
    subprocess.run([sys.executable, "-B", os.path.join(GOLDEN, "make_episodes_golden.py"), "--out", str(tmp_path)],
                   check=True, capture_output=True, timeout=300)
    assert os.listdir(tmp_path) == ["multi.npz"]
    assert filecmp.cmp(tmp_path / "multi.npz", os.path.join(GOLDEN, "multi.npz"), shallow=False)
    assert os.path.getsize(os.path.join(GOLDEN, "multi.npz")) < 100 * 1024


def test_fixture_covers_the_listed_lanes(g, lay):
    assert g["done"].shape == (37, 40)
    cases = eref.covered_cases(g["done"], g["done_before"], lay, g["reward"], g["bootstrap"])
    assert all(cases.values()), [k for k, v in cases.items() if not v]


def test_layout_matches_the_generators_episodes(g, lay):
    for name, dtype in (("lane_episode", np.int64), ("lane_row", np.int64), ("ep_lane", np.int32),
                        ("ep_start", np.int32), ("ep_length", np.int32), ("ep_ended", np.uint8),
                        ("ep_offset", np.int64)):
        assert lay[name].dtype == dtype, name
    for name in ("ep_lane", "ep_start", "ep_length", "ep_ended"):
        assert np.array_equal(lay[name], g[name]), name
    assert np.array_equal(lay["ep_offset"], np.concatenate([[0], np.cumsum(g["ep_length"])]))
    assert lay["lane_row"][-1] == lay["ep_offset"][-1] == len(g["gae_advantages"])
    assert lay["lane_episode"][-1] == len(g["ep_lane"])
    # the issue's row formula: row(i, t) = lane_row[i] + kept frames of lane i before t
    kept = eref.kept_frames(g["done"], g["done_before"])
    rank = np.cumsum(kept, axis=0) - kept
    assert np.array_equal(lay["lane_row"][lay["row_lane"]] + rank[lay["row_t"], lay["row_lane"]],
                          np.arange(len(lay["row_t"])))
    assert kept[lay["row_t"], lay["row_lane"]].all() and len(lay["row_t"]) == kept.sum()
    # without the open episodes: the same records less the open ones
    closed = eref.layout(g["done"], g["done_before"], drop_open=True)
    keep = g["ep_ended"] != 0
    assert 0 < keep.sum() < len(keep)
    for name in ("ep_lane", "ep_start", "ep_length", "ep_ended"):
        assert np.array_equal(closed[name], g[name][keep]), name


def test_gae_and_returns_are_bit_equal_to_the_notebooks(g, lay):
    gamma, lam = float(g["gamma"]), float(g["lam"])
    values = eref.gather(g["values"], lay)
    adv, ret = eref.gae_flat(g["reward"], values, lay, g["bootstrap"], gamma, lam)
    assert np.array_equal(adv, g["gae_advantages"]) and np.array_equal(ret, g["gae_returns"])
    assert np.array_equal(eref.returns_flat(g["reward"], lay, gamma), g["reinforce_returns"])
    assert np.array_equal(eref.episode_return(g["reward"], lay), g["episode_return"])
    closed = eref.layout(g["done"], g["done_before"], drop_open=True)
    assert np.array_equal(eref.returns_flat(g["reward"], closed, gamma), g["closed_returns"])
    assert np.array_equal(eref.episode_return(g["reward"], closed), g["episode_return"][g["ep_ended"] != 0])
    # the reward as float32 storage: the same GAE (compute_gae rounds it first)
    adv32, _ = eref.gae_flat(g["reward"].astype(np.float32), values, lay, g["bootstrap"], gamma, lam)
    assert np.array_equal(adv32, adv)
    # the bootstrap matters to open episodes only
    adv0, _ = eref.gae_flat(g["reward"], values, lay, None, gamma, lam)
    differs = adv0 != adv
    open_rows = np.repeat(lay["ep_ended"] == 0, lay["ep_length"])
    assert differs.any() and not differs[~open_rows].any()


def test_normalised_values_match_the_notebooks_float32(g, lay):
    """The notebooks normalise in float32, the restatement in float64; the
    bound is test_train_batch_cpu.py's 2^-22, a measured property of the
    reference's float32 reduction there.  Measured on this fixture (CPU torch;
    this test prints the figures): max |notebook - restatement| = 2^-22 =
    2.38e-7 for the PPO advantages (1,327 rows, max |value| 2.33), 2^-23 =
    1.19e-7 for the REINFORCE returns over all episodes (1,327 rows, 1.65)
    and over the ended ones (844 rows, 1.50): within the same bound."""
    bound = 2.0 ** -22
    closed = eref.layout(g["done"], g["done_before"], drop_open=True)
    assert closed["ep_offset"][-1] == len(g["closed_returns"])
    for name, raw, want in (("gae", g["gae_advantages"], g["gae_normalized"]),
                            ("reinforce", g["reinforce_returns"], g["reinforce_normalized"]),
                            ("closed", g["closed_returns"], g["closed_normalized"])):
        _, _, out = eref.normalize(raw)
        err = np.abs(out.astype(np.float64) - want.astype(np.float64)).max()
        print(f"{name}: rows {len(raw)}, max |notebook - restatement| = {err:.3e}, max |value| {np.abs(want).max():.3f}")
        assert out.dtype == np.float32 and err <= bound
    for raw, base, std in ((g["reinforce_returns"], g["reinforce_baseline"], g["reinforce_std"]),
                           (g["closed_returns"], g["closed_baseline"], g["closed_std"])):
        mean, sd, _ = eref.normalize(raw)
        assert abs(mean - float(base)) <= np.spacing(np.float32(abs(mean)))
        assert abs(sd - float(std)) <= np.spacing(np.float32(sd))


def test_layout_edges():
    z = eref.layout(np.zeros((0, 3), dtype=np.uint8))
    assert z["lane_episode"].tolist() == [0, 0, 0, 0] and z["ep_offset"].tolist() == [0]
    one = eref.layout(np.array([[0, 1, 1]], dtype=np.uint8), np.array([0, 0, 1], dtype=np.uint8))
    assert one["ep_lane"].tolist() == [0, 1] and one["ep_ended"].tolist() == [0, 1]
    assert one["lane_row"].tolist() == [0, 1, 2, 2]
    drop = eref.layout(np.array([[0, 1, 1]], dtype=np.uint8), np.array([0, 0, 1], dtype=np.uint8), drop_open=True)
    assert drop["ep_lane"].tolist() == [1] and drop["lane_row"].tolist() == [0, 0, 1, 1]


# ---- the C ABI ---------------------------------------------------------------

def test_struct_layout_matches_the_header():
    assert ctypes.sizeof(abi.DDEpisodeLayout) == 7 * 8
    assert abi.DDEpisodeLayout.ep_offset.offset == 48
    assert abi.DD_EPISODES_DROP_OPEN == 1
    header = open(os.path.join(os.path.dirname(HERE), "include", "dronestep.h")).read()
    body = re.search(r"typedef struct DDEpisodeLayout \{(.*?)\} DDEpisodeLayout;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+);", body) == [n for n, _ in abi.DDEpisodeLayout._fields_]
    assert re.findall(r"(\w+) \*\w+;", body) == ["int64_t", "int64_t", "int32_t", "int32_t", "int32_t", "uint8_t",
                                                   "int64_t"]
    assert "#define DD_EPISODES_DROP_OPEN 1" in header
    assert abi.DD_ABI_VERSION == 13 and "#define DD_ABI_VERSION 13" in header  # additions only


NEW_EXPORTS = {"dd_episodes_workspace", "dd_episodes_count", "dd_episodes_fill", "dd_episodes_gather",
               "dd_episodes_advantages"}


def test_library_exports_the_new_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", abi.library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (dd_[a-z0-9_]+)$", out, flags=re.M))
    assert NEW_EXPORTS <= exported and NEW_EXPORTS <= set(abi.EXPORTS)
    assert abi.lib().dd_abi_version() == 13
    names = {"ppo_episodes_batch", "reinforce_episodes_batch", "collect_ppo_steps"}
    assert names <= set(delivery_drone_amd.__all__) and names <= set(tb.__all__)
    assert delivery_drone_amd.ppo_episodes_batch is tb.ppo_episodes_batch
    assert tb.PpoEpisodesBatch._fields[6:14] == ("ep_lane", "ep_start", "ep_lengths", "ep_offsets", "ep_ended",
                                                 "episode_return", "lane_episode_offsets", "lane_row_offsets")


def test_workspace_size():
    lib = abi.lib()
    assert lib.dd_episodes_workspace(0) == lib.dd_episodes_workspace(1) == lib.dd_episodes_workspace(256) == 16
    assert lib.dd_episodes_workspace(257) == 32  # two int64 per 256-lane tile
    assert lib.dd_episodes_workspace(256 * 1024 + 1) == 16 * 1025
    assert lib.dd_batch_workspace(256 * 1024) == 8 * 1024  # unchanged


def _layout(**kw):
    f = dict(lane_episode=8, lane_row=8, ep_lane=8, ep_start=8, ep_length=8, ep_ended=8, ep_offset=8)
    f.update(kw)
    return abi.DDEpisodeLayout(*[f[name] for name, _ in abi.DDEpisodeLayout._fields_])


def test_count_argument_errors_without_gpu():
    lib = abi.lib()

    def count(done=8, before=None, T=4, n=4, flags=0, layout=_layout(), totals=8, ws=8):
        return lib.dd_episodes_count(done, before, T, n, flags, ctypes.byref(layout) if layout is not None else None,
                                     totals, ws, None)

    assert count(done=None) == EINVAL
    assert count(T=-1) == EINVAL and count(n=-1) == EINVAL
    assert count(T=2 ** 31) == EINVAL and count(n=2 ** 31) == EINVAL
    assert count(flags=2) == EINVAL and count(flags=-1) == EINVAL and count(flags=3) == EINVAL
    assert count(layout=None) == EINVAL
    assert count(layout=_layout(lane_episode=None)) == EINVAL
    assert count(layout=_layout(lane_row=None)) == EINVAL
    assert count(totals=None) == EINVAL
    assert count(ws=None) == EINVAL
    assert count(flags=2, n=0) == EINVAL  # checked before the empty batch returns


def test_fill_argument_errors_without_gpu():
    lib = abi.lib()

    def fill(done=8, before=None, T=4, n=4, flags=abi.DD_EPISODES_DROP_OPEN, layout=_layout()):
        return lib.dd_episodes_fill(done, before, T, n, flags, ctypes.byref(layout) if layout is not None else None,
                                    None)

    assert fill(done=None) == EINVAL
    assert fill(T=-1) == EINVAL and fill(n=-1) == EINVAL and fill(T=2 ** 31) == EINVAL
    assert fill(flags=2) == EINVAL
    assert fill(layout=None) == EINVAL
    for name, _ in abi.DDEpisodeLayout._fields_:
        assert fill(layout=_layout(**{name: None})) == EINVAL, name
    assert fill(T=0) == 0 and fill(n=0) == 0  # an empty batch
    assert fill(flags=4, n=0) == EINVAL


def test_gather_argument_errors_without_gpu():
    lib = abi.lib()
    full = (16, 16, 16, 16, 16, 16)

    def gather(io, done=8, T=4, n=4, layout=_layout(ep_lane=None, ep_start=None, ep_length=None, ep_ended=None,
                                                    ep_offset=None)):
        return lib.dd_episodes_gather(ctypes.byref(layout) if layout is not None else None, done, None,
                                      ctypes.byref(io) if io is not None else None, T, n, None)

    assert gather(None) == EINVAL
    assert gather(abi.DDBatchGatherIO(*full, 0, 0), layout=None) == EINVAL
    assert gather(abi.DDBatchGatherIO(*full, 0, 0), layout=_layout(lane_row=None)) == EINVAL
    assert gather(abi.DDBatchGatherIO(*full, 0, 0), done=None) == EINVAL
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

    def adv(T=4, n=4, layout=_layout(), io_none=False, **kw):
        f = dict(reward=8, precision=abi.DD_F32, mode=abi.DD_BATCH_GAE, values=8, bootstrap=None, advantages=8,
                 returns=8, episode_return=8, gamma=0.99, lambda_=0.95)
        f.update(kw)
        io = abi.DDBatchAdvIO(*[f[name] for name, _ in abi.DDBatchAdvIO._fields_])
        return lib.dd_episodes_advantages(ctypes.byref(layout) if layout is not None else None,
                                          None if io_none else ctypes.byref(io), T, n, None)

    assert adv(io_none=True) == EINVAL
    assert adv(layout=None) == EINVAL
    for name, _ in abi.DDEpisodeLayout._fields_:
        assert adv(layout=_layout(**{name: None})) == EINVAL, name
    assert adv(T=-1) == EINVAL and adv(n=-1) == EINVAL
    assert adv(mode=2) == EINVAL and adv(mode=-1) == EINVAL
    assert adv(precision=2) == EINVAL and adv(precision=-1) == EINVAL
    assert adv(values=None) == EINVAL  # GAE needs the critic's values
    assert adv(advantages=None) == EINVAL
    assert adv(reward=None) == EINVAL
    assert adv(mode=abi.DD_BATCH_RETURNS, returns=None) == EINVAL
    assert adv(mode=abi.DD_BATCH_RETURNS, reward=None, values=None, advantages=None) == EINVAL
    assert adv(mode=2, n=0) == EINVAL  # checked before the empty batch returns
    assert adv(n=0) == 0 and adv(T=0) == 0
    assert adv(mode=abi.DD_BATCH_RETURNS, values=None, advantages=None, n=0) == 0


def test_python_wrappers_check_before_the_gpu():
    import torch
    done = torch.zeros(4, 3, dtype=torch.bool)
    with pytest.raises(ValueError, match="GPU"):
        tb.reinforce_episodes_batch(None, None, torch.zeros(4, 3), done)
    with pytest.raises(ValueError, match=r"\[T, N\]"):
        tb.reinforce_episodes_batch(None, None, torch.zeros(4), torch.zeros(4, dtype=torch.bool))

    class Env:
        class config:
            auto_reset = False

    with pytest.raises(ValueError, match="collect_ppo"):
        tb.collect_ppo_steps(Env(), None, None, 8)
