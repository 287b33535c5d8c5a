"""CPU: the PPO loss surface without a GPU.  The float64 NumPy restatement
(tests/ppo_loss_ref.py) against the notebook's own compute_ppo_losses results
and autograd gradients (tests/golden/ppo_loss/losses.npz), the fixture's
conditions, the restatement's edge cases, and the C ABI of
dd_mlp_evaluate_actions and dd_ppo_losses: exports, struct layouts against the
header as a C compiler lays them out, argument errors (fake pointers
throughout; every error is returned before any HIP call).

The reference's own float32 noise.  The notebook computes in float32: each
row's term carries the rounding of its expf (1 ulp), of one or two products
and of the subtraction, and torch's vectorised mean adds about log2(203) ~ 8
levels of roundings: at most about 16 roundings of 2^-24 relative to the mean
magnitude of the terms.  GAP_ULPS = 16 of those is the bound asserted here for
every scalar, on the scale written next to it; the autograd gradients pass
through about as many float32 operations (Sigmoid, clamp, log, BCE, exp, min,
mean, each once forward and once backward), the same 16 on the magnitude of
the gradient's two terms.  Measured on the fixture (203 rows): total_loss
2.4e-3 of 25,338 (bound 0.024), policy_loss 3.5e-9 (8.1e-7), value_loss 3.6e-3
(0.048), entropy 9.0e-9 (2.4e-7), ratio_mean 4.1e-9 (1.0e-6), ratio_std
1.3e-8 (1.7e-6), ratio_min / ratio_max 0, grad_logits 8.9e-10 at most (of
9.9e-3), grad_values 3.0e-7 (of 4.6).  These gaps are what the GPU parity
bounds add (tests/test_gpu_ppo_loss.py takes them from reference_gap, not from
this text).
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import golden_data as gd
import ppo_loss_ref as ref
import delivery_drone_amd
from delivery_drone_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER_DIR = os.path.join(os.path.dirname(HERE), "include")
EINVAL = 1  # hipErrorInvalidValue
GAP_ULPS = 16
U = 2.0 ** -24


@pytest.fixture(scope="module")
def g():
    return gd.npz(os.path.join("ppo_loss", "losses.npz"))


def test_fixture_rows_are_policy_npz_rows(g):
    d, _ = gd.policy_fixture()
    assert g["states"].shape == (203, 15) and 203 % 32 != 0  # a ragged last tile
    assert np.array_equal(g["states"], d["obs"][g["rows"]])
    assert not any(k.startswith(("actor.", "critic.")) for k in g)  # the weights stay in policy.npz
    assert os.path.getsize(os.path.join(gd.GOLDEN, "ppo_loss", "losses.npz")) < 100 * 1024


def test_fixture_conditions_hold(g):
    """No ratio near 1 +- eps, no near-tie of the two surrogates outside the
    range, every (clip side x advantage sign) cell filled, a block of ratios
    exactly 1 and rows with A == 0 on both sides of the clip: with these,
    clipped_frac and the gradient's selection are matters of fact."""
    r, A = g["ratio"].astype(np.float64), g["advantages"].astype(np.float64)
    eps = float(g["clip_epsilon"])
    lo, hi = 1.0 - eps, 1.0 + eps
    assert np.all(np.abs(r / lo - 1.0) > 1e-3) and np.all(np.abs(r / hi - 1.0) > 1e-3)
    inside = (r >= lo) & (r <= hi)
    gap = np.abs(r * A - np.clip(r, lo, hi) * A)
    assert np.all((gap >= 1e-4 * np.abs(A)) | inside)
    for side in (r < lo, r > hi):
        for sign in (A > 0, A < 0):
            assert int((side & sign).sum()) >= 10
    assert int((r == 1.0).sum()) >= 8
    assert ((A == 0) & inside).any() and ((A == 0) & ~inside).any()
    assert abs(A.mean()) < 0.1 and abs(A.std() - 1.0) < 0.1  # normalised (but for the zeroed rows)
    assert np.abs(g["returns"]).max() > 500.0  # the shaped reward's magnitudes
    off = g["old_log_probs"].astype(np.float64) - g["new_log_probs"]
    assert off.min() < -0.5 and off.max() > 0.5


def test_restatement_matches_the_notebook(g):
    out = ref.fixture_losses(g)
    gap = ref.reference_gap(g)
    m = 203
    r = out["ratio"].astype(np.float64)
    A = g["advantages"].astype(np.float64)
    dv2 = (g["values"].astype(np.float64) - g["returns"]) ** 2
    _, ent = ref.row_log_prob_entropy(g["probs"], g["actions"])
    scale = {"policy_loss": np.abs(r * A).mean(), "value_loss": dv2.mean(), "entropy": ent.mean() / 3.0,
             "ratio_mean": r.mean(), "ratio_std": r.max()}
    scale["total_loss"] = scale["policy_loss"] + float(g["value_coef"]) * scale["value_loss"] \
        + float(g["entropy_coef"]) * scale["entropy"]
    for k, s in scale.items():
        print(k, "gap", gap[k], "bound", GAP_ULPS * U * s)
        assert gap[k] <= GAP_ULPS * U * s, k
    # expf within 1 ulp of the correctly rounded ratio, per row and so for min and max
    assert np.all(np.abs(g["ratio"].astype(np.float64) - r) <= gd.ulp32(r))
    assert gap["ratio_min"] <= gd.ulp32(out["ratio_min"]) and gap["ratio_max"] <= gd.ulp32(out["ratio_max"])
    # clipped_frac exactly: the notebook's float32 mean of 0/1 flags names the same count
    count = int(round(out["clipped_frac"] * m))
    assert count == int(((r < 0.8) | (r > 1.2)).sum()) and round(float(g["clipped_frac"]) * m) == count
    assert abs(float(g["clipped_frac"]) - count / m) <= 2 * U
    # gradients: the magnitude of the two terms each element is made of
    a, p = ref.action_bits(g["actions"]), g["probs"].astype(np.float64)
    mag = np.abs(A * r / m)[:, None] * np.abs(a - p) + float(g["entropy_coef"]) / (3 * m) * np.abs(
        (np.log(p) - np.log1p(-p)) * p * (1 - p))
    print("grad_logits gap", gap["grad_logits"].max(), "grad_values gap", gap["grad_values"].max())
    assert np.all(gap["grad_logits"] <= GAP_ULPS * U * mag)
    assert np.all(gap["grad_values"] <= GAP_ULPS * U * np.abs(out["grad_values"]) + 1e-300)


def test_gradient_selection_matches_autograd_exactly(g):
    """Without the entropy bonus the rows the clip cuts off carry exact zeros
    in autograd's gradient: the restatement's selection is that pattern, and
    its A == 0 rows are zero either way."""
    out = ref.losses(g["new_log_probs"], np.zeros(203, np.float32), g["probs"], g["values"], g["old_log_probs"],
                     g["advantages"], g["returns"], g["actions"], float(g["clip_epsilon"]), 0.0,
                     float(g["value_coef"]))
    nb = g["grad_logits_no_entropy"]
    assert np.array_equal(nb == 0, out["grad_logits"] == 0)
    row_zero = (nb == 0).all(1)
    assert np.array_equal(~row_zero, out["selected"] & (g["advantages"] != 0))
    assert 60 < row_zero.sum() < 140  # both kinds of rows in numbers
    assert np.all(np.abs(nb - out["grad_logits"]) <= GAP_ULPS * U * np.abs(out["grad_logits"]))
    assert abs(float(g["total_loss_no_entropy"]) - out["total_loss"]) <= GAP_ULPS * U * abs(out["total_loss"])


def _rows(n, seed=5):
    rng = np.random.default_rng(seed)
    probs = rng.uniform(0.02, 0.98, (n, 3)).astype(np.float32)
    actions = (rng.random((n, 3)) < probs).astype(np.float32)
    lp, ent = ref.row_log_prob_entropy(probs, actions)
    return dict(log_prob=lp.astype(np.float32), entropy=ent.astype(np.float32), probs=probs,
                values=rng.normal(0, 10, n).astype(np.float32), old_log_prob=None,
                advantages=rng.normal(0, 1, n).astype(np.float32), returns=rng.normal(0, 10, n).astype(np.float32),
                actions=actions)


def test_restatement_edge_cases():
    one = _rows(1)
    one["old_log_prob"] = one["log_prob"] - np.float32(0.1)
    out = ref.losses(**one)
    assert np.isnan(out["ratio_std"]) and out["ratio_min"] == out["ratio_max"] == out["ratio_mean"]
    assert np.isfinite(out["total_loss"]) and np.isfinite(out["grad_logits"]).all()

    same = _rows(77)
    same["old_log_prob"] = same["log_prob"].copy()
    out = ref.losses(**same)
    assert out["clipped_frac"] == 0.0 and out["ratio_min"] == out["ratio_max"] == 1.0 and out["ratio_std"] == 0.0
    assert out["policy_loss"] == -(same["advantages"].astype(np.float64).sum() / 77)
    assert out["selected"].all()

    x = _rows(40)
    x["old_log_prob"] = x["log_prob"] + np.linspace(-0.5, 0.5, 40).astype(np.float32)
    out = ref.losses(**x, entropy_coef=0.0)
    assert out["total_loss"] == out["policy_loss"] + 0.5 * out["value_loss"]
    cut = ~out["selected"]
    assert cut.any() and np.all(out["grad_logits"][cut] == 0) and np.all(out["grad_logits"][~cut] != 0)
    # a probability outside clamp_probs' range contributes nothing; a NaN stays
    x["probs"][3, 1], x["probs"][4, 0], x["probs"][5, 2] = 1e-9, 1.0, np.nan
    out = ref.losses(**x)
    assert out["grad_logits"][3, 1] == 0 and out["grad_logits"][4, 0] == 0 and np.isnan(out["grad_logits"][5, 2])
    # bitmask actions are the same actions
    bits = (x["actions"] @ np.array([1, 2, 4])).astype(np.uint8)
    assert np.array_equal(ref.action_bits(bits), x["actions"])


def test_spread_is_a_first_order_bound():
    """ref.spread against finite differences: moving every input by its bound
    in the worst direction changes each scalar by the spread, to first order."""
    x = _rows(64, seed=9)
    x["old_log_prob"] = x["log_prob"] + np.linspace(-0.5, 0.5, 64).astype(np.float32)
    d_lp, d_v = np.full(64, 1e-3), np.full(64, 1e-2)
    s = ref.spread(**x, d_lp=d_lp, d_p=0.0, d_v=d_v)
    base = ref.losses(**x)
    up = dict(x)
    up["values"] = (x["values"] + np.sign(x["values"].astype(np.float64) - x["returns"]) * d_v).astype(np.float32)
    moved = ref.losses(**up)
    assert 0.9 * s["value_loss"] <= abs(moved["value_loss"] - base["value_loss"]) <= 1.1 * s["value_loss"] + 1e-3
    up = dict(x)
    up["log_prob"] = (x["log_prob"] + 1e-3).astype(np.float32)
    moved = ref.losses(**up)
    assert abs(moved["ratio_mean"] - base["ratio_mean"]) <= 1.05 * s["ratio_mean"]
    assert abs(moved["ratio_mean"] - base["ratio_mean"]) >= 0.9 * s["ratio_mean"]
    assert abs(moved["policy_loss"] - base["policy_loss"]) <= 1.05 * s["policy_loss"]
    assert np.all(np.abs(moved["grad_values"] - base["grad_values"]) == 0)


# ---- the C ABI ---------------------------------------------------------------

NEW = ("dd_mlp_evaluate_actions", "dd_ppo_loss_workspace", "dd_ppo_losses")


def test_new_exports_exist_everywhere():
    out = subprocess.run(["nm", "-D", "--defined-only", abi.library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (dd_[a-z0-9_]+)$", out, flags=re.M))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(HEADER_DIR, "dronestep.h")).read(), flags=re.S)
    for name in NEW:
        assert name in exported and name in abi.EXPORTS and re.search(r"\b%s\s*\(" % name, header), name
    assert abi.DD_ABI_VERSION == 13 and abi.lib().dd_abi_version() == 13  # additions only
    assert {"ppo_losses", "PpoLosses"} <= set(delivery_drone_amd.__all__)
    from delivery_drone_amd import ppo_loss
    assert delivery_drone_amd.ppo_losses is ppo_loss.ppo_losses
    assert hasattr(delivery_drone_amd.MlpNet, "evaluate_actions") and hasattr(delivery_drone_amd.MlpNet,
                                                                              "load_state_dict")


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof and every offsetof as the C compiler lays the header's structs
    out, against the ctypes mirror; and the DD_PPO_* indices."""
    structs = (abi.DDMlpEvalIO, abi.DDPpoLossIO)
    consts = ("DD_PPO_TOTAL_LOSS", "DD_PPO_POLICY_LOSS", "DD_PPO_VALUE_LOSS", "DD_PPO_ENTROPY", "DD_PPO_RATIO_MEAN",
              "DD_PPO_RATIO_MIN", "DD_PPO_RATIO_MAX", "DD_PPO_RATIO_STD", "DD_PPO_CLIPPED_FRAC", "DD_PPO_RESULTS")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dronestep.h"', 'int main(void) {']
    for cls in structs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cls.__name__, cls.__name__))
        for name, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cls.__name__, name, cls.__name__, name))
    for c in consts:
        lines.append('printf("%s %%d\\n", (int)%s);' % (c, c))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", HEADER_DIR, "-o", str(exe), str(src)], check=True, capture_output=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    for cls in structs:
        assert int(got[cls.__name__]) == ctypes.sizeof(cls), cls.__name__
        for name, _ in cls._fields_:
            assert int(got[f"{cls.__name__}.{name}"]) == getattr(cls, name).offset, (cls.__name__, name)
    for c in consts:
        assert int(got[c]) == getattr(abi, c), c
    assert ctypes.sizeof(abi.DDMlpEvalIO) == 56 and ctypes.sizeof(abi.DDPpoLossIO) == 128
    assert abi.DD_PPO_RESULTS == 9


def test_evaluate_actions_argument_errors_without_gpu():
    lib = abi.lib()

    def run(packed=16, compute=abi.DD_MLP_F32, io_none=False, **kw):
        f = dict(obs=8, actions=8, action_format=abi.DD_ACT_BITMASK, _pad=0, probs=8, log_prob=8, entropy=8, n=4)
        f.update(kw)
        io = abi.DDMlpEvalIO(*[f[name] for name, _ in abi.DDMlpEvalIO._fields_])
        return lib.dd_mlp_evaluate_actions(packed, compute, None if io_none else ctypes.byref(io), None)

    assert run(io_none=True) == EINVAL
    assert run(n=-1) == EINVAL
    for fmt in (abi.DD_ACT_U8X3, abi.DD_ACT_PHILOX, -1, 9):
        assert run(action_format=fmt) == EINVAL, fmt
    assert run(compute=2) == EINVAL and run(compute=-1) == EINVAL
    assert run(packed=8) == EINVAL  # 16-byte fragments
    assert run(packed=None) == EINVAL
    assert run(obs=None) == EINVAL
    assert run(actions=None) == EINVAL
    assert run(n=0) == 0
    assert run(n=0, action_format=abi.DD_ACT_F32X3, compute=abi.DD_MLP_F16X3, obs=None, actions=None) == 0
    assert run(n=0, action_format=7) == EINVAL  # checked before the empty batch returns


def test_ppo_losses_argument_errors_without_gpu():
    lib = abi.lib()
    assert lib.dd_ppo_loss_workspace() == 512 * (48 + 8)  # the partial sums of both passes

    def run(m=4, ws=8, io_none=False, **kw):
        f = dict(log_prob=8, entropy=8, probs=8, values=8, old_log_prob=8, advantages=8, returns=8, actions=8,
                 action_format=abi.DD_ACT_F32X3, _pad=0, clip_epsilon=0.2, entropy_coef=0.01, value_coef=0.5,
                 result=8, ratio=8, grad_logits=8, grad_values=8)
        f.update(kw)
        io = abi.DDPpoLossIO(*[f[name] for name, _ in abi.DDPpoLossIO._fields_])
        return lib.dd_ppo_losses(None if io_none else ctypes.byref(io), m, ws, None)

    assert run(io_none=True) == EINVAL
    assert run(m=0) == EINVAL and run(m=-3) == EINVAL  # a mean over no rows has no value
    assert run(ws=None) == EINVAL and run(ws=12) == EINVAL
    for name in ("log_prob", "entropy", "values", "old_log_prob", "advantages", "returns", "result"):
        assert run(**{name: None}) == EINVAL, name
    assert run(probs=None) == EINVAL and run(actions=None) == EINVAL  # grad_logits needs both
    for eps in (-0.1, float("nan"), float("inf"), -float("inf")):
        assert run(clip_epsilon=eps) == EINVAL, eps
    for fmt in (abi.DD_ACT_U8X3, abi.DD_ACT_PHILOX, -1, 9):
        assert run(action_format=fmt) == EINVAL, fmt


def test_python_wrappers_check_before_the_gpu():
    import torch
    from delivery_drone_amd import ppo_losses
    with pytest.raises(ValueError, match="MlpNet actor"):
        ppo_losses(object(), object(), torch.zeros(4, 15), torch.zeros(4, 3), torch.zeros(4), torch.zeros(4),
                   torch.zeros(4))
