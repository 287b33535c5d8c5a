"""CPU: the reward components' host side (no GPU).

* tests/reward_parts_ref.py (the NumPy float64 restatement of both notebooks'
  calc_reward, whole dict) against tests/golden/reward_parts/reward_parts.npz,
  which holds what the notebooks' own cells returned.  Bound: none, equality
  per slot, the bound tests/test_oracle_golden.py applies to the two totals
  (np.testing.assert_array_equal against the notebook's values).
* the fixture's branch coverage, slot 7 against the re-added slots bit for bit,
  the PPO notebook's time-penalty quirk in numbers;
* where the reference checkout is present, the notebooks' cells run again;
* DDRewardParts' layout, DD_REWARD_PARTS, the header's text, and every argument
  error of dd_policy_evaluate_parts, each refused before any GPU work (fake
  pointers throughout, as tests/test_eval_abi.py);
* notebook_rewards() on a synthetic result, with plot_accumulated_rewards'
  cumulative sums (the notebook's arithmetic, without matplotlib)."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_data as gd
import reward_parts_ref as rp
from delivery_drone_amd import abi, notebook_rewards
from delivery_drone_amd.config import EnvConfig

EINVAL = 1  # hipErrorInvalidValue
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("RL101_REFERENCE", "/root/reference")
GENERATOR = os.path.join(REPO, "tests", "golden", "reward_parts", "make_reward_parts_golden.py")


@pytest.fixture(scope="module")
def rec():
    return gd.npz(os.path.join("reward_parts", "reward_parts.npz"))


def test_names_are_the_notebooks_keys(rec):
    assert tuple(rec["names_ppo"]) == rp.PPO_NAMES == abi.REWARD_PART_NAMES["notebook"]
    assert tuple(rec["names_reinforce"]) == rp.REINFORCE_NAMES == abi.REWARD_PART_NAMES["reinforce"]
    assert bool(rec["basic_equals_ppo"])  # Actor_Critic_Basic.ipynb's cell gave the PPO notebook's values


def test_restatement_equals_the_notebooks_values_per_slot(rec):
    got = rp.ppo_parts(rec["states"], rec["prev_dist"])
    for j, name in enumerate(rp.PPO_NAMES):
        np.testing.assert_array_equal(got[:, j], rec["ppo"][:, j], err_msg=f"PPO {name}")
    got = rp.reinforce_parts(rec["states"])
    for j, name in enumerate(rp.REINFORCE_NAMES):
        np.testing.assert_array_equal(got[:, j], rec["reinforce"][:, j], err_msg=f"REINFORCE {name}")
    assert np.array_equal(rp.parts("notebook", rec["states"], rec["prev_dist"]), rp.ppo_parts(rec["states"],
                                                                                             rec["prev_dist"]))


def test_fixture_takes_every_branch(rec):
    cov = rp.coverage(rec["states"], rec["prev_dist"])
    print(cov)
    assert not [k for k, v in cov.items() if v == 0]
    # prev_state present from frame 0: the first recorded frame of an episode has a prev_dist
    assert not math.isnan(rec["prev_dist"][0]) and np.isnan(rec["prev_dist"]).sum() == 1
    # the branch outcomes are in the recorded values too
    ppo, rf = rec["ppo"], rec["reinforce"]
    assert (ppo[:, 1] == -2.0).any() and (ppo[:, 1] == 5.0).any() and ((ppo[:, 1] > 0) & (ppo[:, 1] < 5)).any()
    assert (ppo[:, 2] == -1.0).any() and (ppo[:, 2] == -0.3).any()
    assert (ppo[:, 6] > 800).any() and (ppo[:, 6] == -200).any() and (ppo[:, 6] == -300).any()
    assert (rf[:, 6] > 500).any() and (rf[:, 2] == 0.5).any() and (rf[:, 1] > 0).any()
    assert (ppo[:, 3] < 0).any() and (ppo[:, 5] < 0).any() and (ppo[:, 4] < 0).any()


def test_total_is_the_slots_re_added_bit_for_bit(rec):
    ppo, rf = rec["ppo"], rec["reinforce"]
    total = np.zeros(len(ppo)) + -0.5
    for j in range(1, 7):
        total = total + ppo[:, j]
    np.testing.assert_array_equal(total, ppo[:, 7])
    total = np.zeros(len(rf))
    for j in range(0, 7):
        total = total + rf[:, j]
    np.testing.assert_array_equal(total, rf[:, 7])


def test_ppo_time_penalty_quirk(rec):
    """Slot 0 is -1 / (1 + 100 d^2), reported, and not a term of slot 7."""
    d = rec["states"][:, 9]
    np.testing.assert_array_equal(rec["ppo"][:, 0], -1 / (1 + 100 * rp.pow2(d)))
    with_it = rec["ppo"][:, 0] + rec["ppo"][:, 1:7].sum(axis=1)
    assert (np.abs(with_it - rec["ppo"][:, 7]) > 1e-3).any()


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "delivery_drone", "game")),
                    reason="the reference checkout is not present")
def test_fixture_regenerates_from_the_notebooks(tmp_path, rec):
    subprocess.run([sys.executable, "-B", GENERATOR, "--out", str(tmp_path)], check=True, capture_output=True)
    new = np.load(tmp_path / "reward_parts.npz")
    assert sorted(new.files) == sorted(rec)
    for k in new.files:
        np.testing.assert_array_equal(new[k], rec[k], err_msg=k)


def test_struct_layout_and_header():
    assert abi.DD_REWARD_PARTS == 8
    assert ctypes.sizeof(abi.DDRewardParts) == 3 * 8
    assert (abi.DDRewardParts.sum.offset, abi.DDRewardParts.prev_dist.offset, abi.DDRewardParts.per_frame.offset) == \
        (0, 8, 16)
    assert abi.DD_ABI_VERSION == 13 and abi.lib().dd_abi_version() == 13
    header = open(os.path.join(REPO, "include", "dronestep.h")).read()
    assert re.search(r"#define\s+DD_REWARD_PARTS\s+8\b", header)
    for text in ("typedef struct DDRewardParts", "dd_policy_evaluate_parts", "time_penalty", "velocity_alignment",
                 "vertical_position", "-0.5", "NOT a term of slot 7", "rounded to the state's", "ONE frame back",
                 "prev_dist"):
        assert text in header, text
    out = subprocess.run(["nm", "-D", "--defined-only", abi.library_path()], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r"\bT dd_policy_evaluate_parts$", out, flags=re.M)
    assert "dd_policy_evaluate_parts" in abi.EXPORTS
    # the string dd_build_info() returns keeps its three device-code hashes
    info = abi.lib().dd_build_info().decode()
    assert "policy_eval" not in info and "policy_rollout" in info


def _state(precision=abi.DD_F32):
    p = ctypes.c_void_p(8)
    return abi.DDState(p, p, p, p, p, p, p, p, p, p, p, p, p, 0, precision, 0)


BAD_SAMPLINGS = [(3, 1.0), (-1, 1.0), (abi.DD_SAMPLE_TEMPERED, 0.0), (abi.DD_SAMPLE_TEMPERED, -0.5),
                 (abi.DD_SAMPLE_TEMPERED, math.nan), (abi.DD_SAMPLE_TEMPERED, math.inf)]


def test_evaluate_parts_argument_errors_without_gpu():
    lib = abi.lib()
    full = abi.DDEpisodeStats(8, 8, 8, 8)
    ok = abi.DDSampling(abi.DD_SAMPLE_GREEDY, 0.0, None)
    good_parts = abi.DDRewardParts(8, 8, None)

    def io_for(mode="notebook", frames=4):
        io = abi.DDPolicyRolloutIO()
        io.obs0 = 8
        io.frames = frames
        io.shaped_mode = abi.DD_SHAPED_REINFORCE if mode == "reinforce" else abi.DD_SHAPED_PPO
        io.shaped_hist = 8 if mode == "notebook" else None
        return io

    def run(sampling=ok, stats=full, parts=good_parts, packed=16, compute=abi.DD_MLP_F16X3, n=4, io=None, cfg=None):
        cfg = cfg if cfg is not None else EnvConfig().to_abi()
        io = io if io is not None else io_for()
        return lib.dd_policy_evaluate_parts(ctypes.byref(cfg), ctypes.byref(_state()), packed, compute,
                                            ctypes.byref(io), ctypes.byref(sampling) if sampling is not None else None,
                                            ctypes.byref(stats) if stats is not None else None,
                                            ctypes.byref(parts) if parts is not None else None, n, None)

    # the new struct
    assert run(parts=None) == EINVAL
    assert run(parts=abi.DDRewardParts(None, 8, None)) == EINVAL
    assert run(parts=abi.DDRewardParts(8, None, None)) == EINVAL                      # PPO shape without prev_dist
    assert run(parts=abi.DDRewardParts(8, None, None), io=io_for("reinforce"), n=0) == 0  # unused by REINFORCE
    assert run(io=io_for("engine")) == EINVAL                                          # no notebook components
    assert run(io=io_for("engine"), n=0) == EINVAL
    assert run(cfg=EnvConfig(auto_reset=True).to_abi()) == EINVAL
    assert run(cfg=EnvConfig(auto_reset=True).to_abi(), io=io_for("reinforce")) == EINVAL
    # statistics: all four
    assert run(stats=None) == EINVAL
    for k in range(0, 15):
        ptrs = [8 if (k >> j) & 1 else None for j in range(4)]
        assert run(stats=abi.DDEpisodeStats(*ptrs)) == EINVAL, ptrs
    # dd_policy_rollout_sampled's own errors
    for mode, t in BAD_SAMPLINGS:
        assert run(abi.DDSampling(mode, t, None)) == EINVAL, (mode, t)
        assert run(abi.DDSampling(mode, t, None), n=0) == EINVAL, (mode, t)
    assert run(packed=None) == EINVAL
    assert run(packed=8) == EINVAL  # 16-byte fragments
    assert run(compute=7) == EINVAL
    assert run(n=-1) == EINVAL
    assert run(io=io_for(frames=-1)) == EINVAL
    bad_mode = io_for()
    bad_mode.shaped_mode = 5
    assert run(io=bad_mode) == EINVAL
    engine_out = io_for()
    engine_out.engine_reward = engine_out.engine_done = 8
    assert run(io=engine_out) == EINVAL
    # nothing to do: an empty batch; no frames and no final observation wanted
    assert run(n=0) == 0
    assert run(sampling=None, n=0) == 0
    assert run(io=io_for(frames=0)) == 0
    assert run(io=io_for("reinforce", frames=0)) == 0


def synthetic_result(mode, frames=9, n=5):
    """What evaluate_policy(components=True, per_frame=True) returns, on the host."""
    names = abi.REWARD_PART_NAMES[mode]
    g = torch.Generator().manual_seed(3)
    steps = torch.tensor([9, 4, 1, 7, 9], dtype=torch.int32)
    per = torch.randn(frames, 8, n, generator=g, dtype=torch.float32)
    alive = torch.arange(frames)[:, None] < steps[None, :]
    per = per * alive[:, None, :]
    sums = torch.zeros(8, n, dtype=torch.float64)
    for k in range(frames):  # float64, in frame order
        sums = sums + per[k].double()
    return {"total_reward": sums[7].clone(), "steps": steps,
            "components": {name: sums[j] for j, name in enumerate(names)},
            "rewards": {name: per[:, j] for j, name in enumerate(names)}}, per


@pytest.mark.parametrize("mode", ["notebook", "reinforce"])
def test_notebook_rewards_feeds_plot_accumulated_rewards(mode):
    res, per = synthetic_result(mode)
    names = abi.REWARD_PART_NAMES[mode]
    for lane in range(5):
        rewards = notebook_rewards(res, lane)
        assert len(rewards) == int(res["steps"][lane])
        for k, r in enumerate(rewards):
            assert tuple(r) == names and all(type(v) is float for v in r.values())
            assert [r[name] for name in names] == per[k, :, lane].tolist()
        # plot_accumulated_rewards' arithmetic (Actor_Critic_PPO.ipynb:1543-1577), without matplotlib
        reward_dicts = {"rewards": rewards}["rewards"]
        components = [key for key in reward_dicts[0].keys() if key != "total"]
        assert components == list(names[:-1])
        accumulated = {comp: [] for comp in components}
        accumulated["total"] = []
        for comp in components + ["total"]:
            cumsum = 0
            for reward_dict in reward_dicts:
                cumsum += reward_dict[comp]
                accumulated[comp].append(cumsum)
        for name in names:
            assert accumulated[name][-1] == float(res["components"][name][lane]), name
    with pytest.raises(ValueError):
        notebook_rewards({"steps": res["steps"], "components": res["components"]}, 0)
