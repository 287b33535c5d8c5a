"""CPU: the REINFORCE / actor-critic loss surface without a GPU.  The float64
NumPy restatement (tests/pg_loss_ref.py) against the notebooks' own training
lines (tests/golden/pg_loss/pg.npz), the mask, the empty mask, the fixture's
regeneration, and the C ABI of dd_pg_losses and dd_td_losses: exports, struct
layouts as a C compiler lays the header out, argument errors (fake pointers
throughout; every error is returned before any HIP call).

The reference's own float32 noise.  The notebooks compute in float32, the
restatement in float64 on the same float32 rows, so their distance is the
notebooks' rounding: each term of a loss carries one or two float32 products,
a subtraction or two, and torch's vectorised mean adds about log2(203) ~ 8
levels of roundings; autograd's gradient at the logits passes through Sigmoid,
clamp, log, BCE and mean once forward and once backward.  As
tests/test_ppo_loss_cpu.py argues for the same operations: at most about 16
roundings of 2^-24 relative to the magnitude of the terms, GAP_ULPS = 16, on
the scale written next to each figure.  Measured on the fixture (203 rows), in
those units of 2^-24 x scale: REINFORCE loss 0.33 (of mean|lp A| = 0.448),
its grad_logits 10.7 at most (of |A / m| |a - p|, at most 1.5e-2); td_targets
1.1 and td_errors 1.6 (of |r| + |gamma v'| + |v|, gaps at most 6.1e-5),
critic_loss 0.16 (of 58,239), value_reg 1.04 (of 2,941), grad_values 1.7
(gap at most 9.5e-7), actor_loss 0.83 (of mean|lp delta|), its grad_logits 9.5.
"""
import ctypes
import filecmp
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import golden_data as gd
import pg_loss_ref as ref
import delivery_drone_amd
from delivery_drone_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER_DIR = os.path.join(os.path.dirname(HERE), "include")
GOLDEN = os.path.join(HERE, "golden", "pg_loss")
REF = os.environ.get("RL101_REFERENCE", "/root/reference")
EINVAL = 1  # hipErrorInvalidValue
GAP_ULPS = 16
U = 2.0 ** -24
M = 203


@pytest.fixture(scope="module")
def g():
    return gd.npz(os.path.join("pg_loss", "pg.npz"))


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "Actor_Critic_Basic.ipynb")),
                    reason="reference checkout absent")
def test_fixture_regenerates_byte_identically(tmp_path):
    subprocess.run([sys.executable, "-B", os.path.join(GOLDEN, "make_pg_loss_golden.py"), "--out", str(tmp_path)],
                   check=True, capture_output=True, timeout=300)
    assert os.listdir(tmp_path) == ["pg.npz"]
    assert filecmp.cmp(tmp_path / "pg.npz", os.path.join(GOLDEN, "pg.npz"), shallow=False)


def test_fixture_is_data_of_policy_npz_rows(g):
    d, _ = gd.policy_fixture()
    assert g["states"].shape == (M, 15) and M % 32 != 0  # a ragged last tile
    assert np.array_equal(g["states"], d["obs"][g["rows"]])
    assert np.array_equal(g["next_states"], d["obs"][(g["rows"] + 1) % d["obs"].shape[0]])
    assert os.path.getsize(os.path.join(GOLDEN, "pg.npz")) <= os.path.getsize(
        os.path.join(gd.GOLDEN, "mlp_backward", "grads.npz"))
    assert 10 < g["dones"].sum() < 60 and set(np.unique(g["dones"])) == {0.0, 1.0}
    assert np.abs(g["rewards"]).max() > 400.0 and np.abs(g["returns"]).max() > 400.0
    for tag, k in (("actor", 3), ("critic", 1)):
        idx = g["idx_" + tag]
        assert idx[0] == 0 and idx[-1] == 27456 + 65 * k - 1 and np.all(np.diff(idx) > 0)
    assert g["reinforce.actor_grad"].shape == g["td.actor_after"].shape == g["idx_actor"].shape
    assert g["td.critic_grad"].shape == g["td.critic_after"].shape == g["idx_critic"].shape
    # the cell's two normalisations are reinforce_batch's one: (R - mean) / (std + 1e-8)
    R = g["returns"].astype(np.float64)
    adv = (R - R.mean()) / (R.std(ddof=1) + 1e-8)
    assert np.all(np.abs(g["reinforce.advantages"] - adv) <= 1e-5 * (1.0 + np.abs(adv)))


def test_restatement_matches_the_reinforce_cell(g):
    out = ref.pg_losses(g["reinforce.log_probs"], g["reinforce.probs"], g["actions"], g["reinforce.advantages"])
    lp, A = g["reinforce.log_probs"].astype(np.float64), g["reinforce.advantages"].astype(np.float64)
    gap, scale = abs(out["loss"] - float(g["reinforce.loss"])), np.abs(lp * A).mean()
    print("reinforce loss gap", gap, "bound", GAP_ULPS * U * scale)
    assert gap <= GAP_ULPS * U * scale and out["count"] == M
    mag = np.abs(A / M)[:, None] * np.abs((g["actions"] != 0) - g["reinforce.probs"].astype(np.float64))
    gap = np.abs(out["grad_logits"].astype(np.float64) - g["reinforce.grad_logits"])
    print("reinforce grad_logits gap", (gap / (U * mag)).max(), "units")
    assert np.all(gap <= GAP_ULPS * U * mag)
    assert np.array_equal(out["grad_logits"] == 0, g["reinforce.grad_logits"] == 0)


def test_restatement_matches_the_actor_critic_cell(g):
    t = ref.td_losses(g["td.values"], g["td.next_values"], g["rewards"], g["dones"], float(g["gamma"]), 0.01)
    v, vn, r = (g[k].astype(np.float64) for k in ("td.values", "td.next_values", "rewards"))
    row = np.abs(r) + np.abs(vn) + np.abs(v)
    for k in ("td_targets", "td_errors"):
        gap = np.abs(t[k].astype(np.float64) - g["td." + k])
        print(k, "gap", gap.max(), (gap / (U * row)).max(), "units")
        assert np.all(gap <= GAP_ULPS * U * row), k
    assert np.all(t["td_targets"][g["dones"] == 1.0] == g["rewards"][g["dones"] == 1.0])  # no bootstrap past an end
    for k, scale in (("critic_loss", t["critic_loss"]), ("value_reg", t["value_reg"])):
        gap = abs(t[k] - float(g["td." + k]))
        print(k, "gap", gap, "bound", GAP_ULPS * U * scale)
        assert gap <= GAP_ULPS * U * scale, k
    assert t["critic_loss"] == t["mse"] + t["value_reg"] and t["count"] == M
    mag = (2.0 * row + 0.02 * np.abs(v)) / M
    gap = np.abs(t["grad_values"].astype(np.float64) - g["td.grad_values"])
    print("grad_values gap", gap.max(), (gap / (U * mag)).max(), "units")
    assert np.all(gap <= GAP_ULPS * U * mag)
    assert np.array_equal(t["grad_values"] == 0, g["td.grad_values"] == 0)
    # the actor stage takes the float32 td_errors as its weights
    out = ref.pg_losses(g["td.log_probs"], g["td.probs"], g["actions"], g["td.td_errors"])
    lp, w = g["td.log_probs"].astype(np.float64), g["td.td_errors"].astype(np.float64)
    gap, scale = abs(out["loss"] - float(g["td.actor_loss"])), np.abs(lp * w).mean()
    print("actor_loss gap", gap, "bound", GAP_ULPS * U * scale)
    assert gap <= GAP_ULPS * U * scale
    mag = np.abs(w / M)[:, None] * np.abs((g["actions"] != 0) - g["td.probs"].astype(np.float64))
    gap = np.abs(out["grad_logits"].astype(np.float64) - g["td.grad_logits"])
    assert np.all(gap <= GAP_ULPS * U * mag)
    assert np.array_equal(out["grad_logits"] == 0, g["td.grad_logits"] == 0)


def test_masked_call_equals_the_compacted_call(g):
    rng = np.random.default_rng(4)
    on = rng.random(M) < 0.6
    bits = (g["actions"] @ np.array([1, 2, 4])).astype(np.uint8)
    poison = np.where(on, 0.0, np.nan).astype(np.float32)  # an inactive row's inputs are never read
    full = ref.pg_losses(g["td.log_probs"] + poison, g["td.probs"] + poison[:, None], bits, g["td.td_errors"] + poison,
                         active=on.astype(np.uint8))
    part = ref.pg_losses(g["td.log_probs"][on], g["td.probs"][on], g["actions"][on], g["td.td_errors"][on])
    assert full["count"] == part["count"] == on.sum()
    assert full["loss"] == part["loss"]
    assert np.array_equal(full["grad_logits"][on], part["grad_logits"]) and np.all(full["grad_logits"][~on] == 0)
    full = ref.td_losses(g["td.values"] + poison, g["td.next_values"] + poison, g["rewards"] + poison,
                         g["dones"] + poison, active=on)
    part = ref.td_losses(g["td.values"][on], g["td.next_values"][on], g["rewards"][on], g["dones"][on])
    assert full["count"] == part["count"] and full["critic_loss"] == part["critic_loss"]
    assert full["mse"] == part["mse"] and full["value_reg"] == part["value_reg"]
    for k in ("td_targets", "td_errors", "grad_values"):
        assert np.array_equal(full[k][on], part[k]) and np.all(full[k][~on] == 0), k


def test_no_active_row_gives_nan_scalars_and_zero_gradients(g):
    off = np.zeros(M, dtype=np.uint8)
    out = ref.pg_losses(g["td.log_probs"], g["td.probs"], g["actions"], g["td.td_errors"], active=off)
    assert np.isnan(out["loss"]) and out["count"] == 0 and not out["grad_logits"].any()
    t = ref.td_losses(g["td.values"], g["td.next_values"], g["rewards"], g["dones"], active=off)
    assert all(np.isnan(t[k]) for k in ("critic_loss", "mse", "value_reg")) and t["count"] == 0
    assert not t["grad_values"].any() and not t["td_errors"].any() and not t["td_targets"].any()


def test_saturated_probabilities_in_the_restatement(g):
    p = g["td.probs"].copy()
    p[3, 1], p[4, 0], p[5, 2], p[6, 0] = 1e-9, 1.0, np.nan, 0.0
    out = ref.pg_losses(g["td.log_probs"], p, g["actions"], g["td.td_errors"])["grad_logits"]
    assert out[3, 1] == 0 and out[4, 0] == 0 and out[6, 0] == 0 and np.isnan(out[5, 2])
    assert np.isfinite(np.delete(out.reshape(-1), 5 * 3 + 2)).all() and out[3, 0] != 0


# ---- the C ABI ---------------------------------------------------------------

NEW = ("dd_pg_loss_workspace", "dd_pg_losses", "dd_td_loss_workspace", "dd_td_losses")


def test_new_exports_exist_everywhere():
    out = subprocess.run(["nm", "-D", "--defined-only", abi.library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (dd_[a-z0-9_]+)$", out, flags=re.M))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(HEADER_DIR, "dronestep.h")).read(), flags=re.S)
    for name in NEW:
        assert name in exported and name in abi.EXPORTS and re.search(r"\b%s\s*\(" % name, header), name
    assert abi.DD_ABI_VERSION == 13 and abi.lib().dd_abi_version() == 13  # additions only
    assert re.search(r"#define DD_ABI_VERSION 13\b", header)
    names = {"reinforce_losses", "ReinforceLosses", "reinforce_update", "ReinforceUpdate", "collect_reinforce",
             "td_losses", "TdLosses", "actor_critic_update", "ActorCriticUpdate"}
    assert names <= set(delivery_drone_amd.__all__)
    from delivery_drone_amd import pg_loss
    assert all(getattr(delivery_drone_amd, n) is getattr(pg_loss, n) for n in names)


def test_struct_layouts_match_the_header(tmp_path):
    structs = (abi.DDPgLossIO, abi.DDTdLossIO)
    consts = ("DD_PG_LOSS", "DD_PG_COUNT", "DD_PG_RESULTS", "DD_TD_CRITIC_LOSS", "DD_TD_MSE", "DD_TD_VALUE_REG",
              "DD_TD_COUNT", "DD_TD_RESULTS")
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
    assert ctypes.sizeof(abi.DDPgLossIO) == 64 and ctypes.sizeof(abi.DDTdLossIO) == 88
    assert (abi.DD_PG_RESULTS, abi.DD_TD_RESULTS) == (2, 4)


def test_pg_losses_argument_errors_without_gpu():
    lib = abi.lib()
    assert lib.dd_pg_loss_workspace() == 512 * 16

    def run(m=4, ws=8, io_none=False, **kw):
        f = dict(log_prob=8, probs=8, actions=8, action_format=abi.DD_ACT_F32X3, _pad=0, weights=8, active=8,
                 result=8, grad_logits=8)
        f.update(kw)
        io = abi.DDPgLossIO(*[f[name] for name, _ in abi.DDPgLossIO._fields_])
        return lib.dd_pg_losses(None if io_none else ctypes.byref(io), m, ws, None)

    assert run(io_none=True) == EINVAL
    assert run(m=0) == EINVAL and run(m=-3) == EINVAL
    assert run(ws=None) == EINVAL and run(ws=12) == EINVAL
    for name in ("log_prob", "weights", "result"):
        assert run(**{name: None}) == EINVAL, name
    assert run(probs=None) == EINVAL and run(actions=None) == EINVAL  # grad_logits needs both
    for fmt in (abi.DD_ACT_U8X3, abi.DD_ACT_PHILOX, -1, 9):
        assert run(action_format=fmt) == EINVAL, fmt
        assert run(action_format=fmt, grad_logits=None, probs=None, actions=None) == EINVAL, fmt


def test_td_losses_argument_errors_without_gpu():
    lib = abi.lib()
    assert lib.dd_td_loss_workspace() == 512 * 24

    def run(m=4, ws=8, io_none=False, **kw):
        f = dict(values=8, next_values=8, rewards=8, dones=8, active=8, gamma=0.99, value_reg=0.01, td_targets=8,
                 td_errors=8, result=8, grad_values=8)
        f.update(kw)
        io = abi.DDTdLossIO(*[f[name] for name, _ in abi.DDTdLossIO._fields_])
        return lib.dd_td_losses(None if io_none else ctypes.byref(io), m, ws, None)

    assert run(io_none=True) == EINVAL
    assert run(m=0) == EINVAL and run(m=-3) == EINVAL
    assert run(ws=None) == EINVAL and run(ws=12) == EINVAL
    for name in ("values", "next_values", "rewards", "dones", "td_targets", "td_errors", "result"):
        assert run(**{name: None}) == EINVAL, name
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert run(gamma=bad) == EINVAL and run(value_reg=bad) == EINVAL, bad


def test_python_wrappers_check_before_the_gpu():
    import torch
    from delivery_drone_amd import actor_critic_update, reinforce_losses, reinforce_update, td_losses
    with pytest.raises(ValueError, match="MlpNet actor"):
        reinforce_losses(object(), torch.zeros(4, 15), torch.zeros(4, 3), torch.zeros(4))
    with pytest.raises(ValueError, match="MlpNet critic"):
        td_losses(object(), torch.zeros(4, 15), torch.zeros(4), torch.zeros(4, 15), torch.zeros(4))
    with pytest.raises(ValueError, match="AdamW"):
        reinforce_update(object(), None, object())
    with pytest.raises(ValueError, match="actor_opt"):
        actor_critic_update(object(), object(), *[None] * 5, object(), object())
