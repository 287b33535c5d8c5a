"""CPU: the AdamW step without a GPU.  The NumPy restatement of dd_adamw_step's
contract (tests/adamw_ref.py) against torch.optim.AdamW on the CPU, in float64
and in float32, on a fixed trajectory built from committed data only
(adamw_ref.trajectory: the fixture networks and eight signed, scaled copies of
the notebook's own gradients, with exact-zero, 1e-30 and 1e-20 elements); the
f16x3 refusal rule; torch's optimizer-state layout; the C ABI's exports, struct
layouts and argument errors (fake pointers; every error precedes any launch).

Float64: the restatement without its float32 roundings against float64 torch,
per parameter within s x 2^-47 (|p| + lr) after s steps: a few dozen float64
roundings of an update of size lr or of p, and pow(beta, t) against the
running product (t 2^-53).  Measured: at most 0.12 of that bound.

The reference's own float32 gap G.  torch's float32 step rounds every
intermediate (exp_avg, exp_avg_sq, their quotient, the decayed p), the
restatement rounds p, m, v once; the unit is 2^-24 (|p| + lr A), with A the
update's size had nothing cancelled in exp_avg: the bias-corrected
beta1-average of |g| over sqrt(v_hat) + eps (adamw_ref.update_scale), the
convention of the backward's S.  G(s) = the largest |torch float32 p -
restatement p| / unit after s steps.  Measured, steps 1..8:
    actor  (lr 3e-4, wd 0.01): 2.88 4.81 6.03 8.95 15.8 19.9 23.5 25.3
    actor  (wd 0):             3.06 3.64 3.66 4.44 9.50 8.22 7.77 10.2
    critic (lr 1e-3, wd 0.01): 4.15 4.76 5.96 7.95 10.6 11.9 17.8 27.6
    critic (wd 0):             4.15 4.98 4.64 4.91 8.93 8.13 11.3 11.8
G = 27.6; G_CAP = 64, the next power of two above twice that.  The GPU test's
parity bound is 1 float32 ulp + G_CAP units, from here alone.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import adamw_ref as ref
import golden_data as gd
import delivery_drone_amd
from delivery_drone_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER_DIR = os.path.join(os.path.dirname(HERE), "include")
EINVAL = 1  # hipErrorInvalidValue
G_CAP = 64.0
NETS = (("actor", 3), ("critic", 1))
CASES = [(tag, k, wd) for tag, k in NETS for wd in (0.01, 0.0)]


@pytest.fixture(scope="module")
def fx():
    return gd.npz(os.path.join("mlp_backward", "grads.npz"))


@pytest.fixture(scope="module")
def nets():
    return gd.policy_fixture()[1]


@pytest.fixture(scope="module")
def traj(fx, nets):
    """Per network: the start parameters (flat float32), the eight gradients, the special elements."""
    out = {}
    for tag, k in NETS:
        grads, zero_idx, tiny_idx = ref.trajectory(fx, tag, k)
        out[tag] = dict(p0=ref.flatten(nets[tag]).astype(np.float32), grads=grads, zero=zero_idx, tiny=tiny_idx)
    return out


def test_trajectory_is_what_the_docstring_says(traj):
    for tag, k in NETS:
        t = traj[tag]
        assert t["p0"].shape == (ref.numel(k),) and t["grads"].shape == (ref.STEPS, ref.numel(k))
        assert t["grads"].dtype == np.float32 and len(t["zero"]) == ref.numel(k) // 16
        assert not t["grads"][:, t["zero"]].any()
        assert np.all(np.abs(t["grads"][:, t["tiny"][:8]]) == np.float32(1e-30))
        assert np.all(t["grads"][:, t["tiny"][8:]] == np.float32(1e-20))
        signs = np.sign(t["grads"][:, np.setdiff1d(np.arange(ref.numel(k)), t["zero"])])
        flips = (signs[1:] != signs[:-1]).mean()
        assert 0.3 < flips < 0.7  # exp_avg sees cancellation


@pytest.mark.parametrize("tag,k,wd", CASES)
def test_restatement_matches_float64_torch(traj, tag, k, wd):
    import torch
    t, lr = traj[tag], ref.NOTEBOOK_LR[tag]
    ours = ref.run(t["p0"], t["grads"], lr=lr, out_dim=k, exact=True, weight_decay=wd)
    theirs, _, _ = ref.torch_adamw(t["p0"].astype(np.float64), t["grads"].astype(np.float64), lr=lr, out_dim=k,
                                   dtype=torch.float64, weight_decay=wd)
    for s in range(ref.STEPS):
        p = ours[s][0]
        assert p.dtype == np.float64
        bound = (s + 1) * 2.0 ** -47 * (np.abs(p) + lr)
        err = np.abs(theirs[s] - p)
        print(f"{tag} wd={wd} step {s + 1}: largest error / bound {float((err / bound).max()):.3g}")
        assert np.all(err <= bound), s
    assert ours[-1][3]["step"] == ref.STEPS
    assert abs(ours[-1][3]["b1t"] - 0.9 ** ref.STEPS) <= 8 * 2.0 ** -53 and ours[-1][3]["b2t"] < 1.0


@pytest.mark.parametrize("tag,k,wd", CASES)
def test_reference_gap(traj, tag, k, wd):
    import torch
    t, lr = traj[tag], ref.NOTEBOOK_LR[tag]
    ours = ref.run(t["p0"], t["grads"], lr=lr, out_dim=k, weight_decay=wd)
    theirs, _, _ = ref.torch_adamw(t["p0"], t["grads"], lr=lr, out_dim=k, dtype=torch.float32, weight_decay=wd)
    scale = ref.update_scale(t["grads"])
    gaps = []
    for s in range(ref.STEPS):
        p = ours[s][0]
        assert p.dtype == np.float32 and ours[s][1].dtype == np.float32 and ours[s][2].dtype == np.float32
        unit = ref.gap_unit(p, lr, scale[s])
        gaps.append(float((np.abs(theirs[s].astype(np.float64) - p.astype(np.float64)) / unit).max()))
    print(f"{tag} wd={wd}: G per step count", [round(g, 2) for g in gaps], "G_CAP", G_CAP)
    assert max(gaps) <= G_CAP


@pytest.mark.parametrize("tag,k", NETS)
def test_structure(traj, tag, k):
    t, lr = traj[tag], ref.NOTEBOOK_LR[tag]
    out = ref.run(t["p0"], t["grads"], lr=lr, out_dim=k)
    decay = 1.0 - lr * 0.01
    want = t["p0"][t["zero"]]
    for s in range(ref.STEPS):
        p, m, v, st = out[s]
        # a zero gradient: exp_avg and exp_avg_sq stay zero, the parameter moves by the decay factor only
        want = (want.astype(np.float64) * decay).astype(np.float32)
        assert np.array_equal(p[t["zero"]], want) and not m[t["zero"]].any() and not v[t["zero"]].any()
        assert st == dict(step=s + 1, b1t=st["b1t"], b2t=st["b2t"], status=0)
        # 1e-30: g g underflows float32, exp_avg does not; 1e-20: exp_avg_sq is a float32 denormal, kept
        assert not v[t["tiny"][:8]].any() and np.all(m[t["tiny"][:8]] != 0)
        d = v[t["tiny"][8:]]
        assert np.all(d > 0) and np.all(d < np.finfo(np.float32).tiny)
    # weight_decay = 0 and a zero gradient: nothing moves
    still = ref.run(t["p0"], t["grads"], lr=lr, out_dim=k, weight_decay=0.0)[-1][0]
    assert np.array_equal(still[t["zero"]], t["p0"][t["zero"]])
    # inputs are left alone; the same call gives the same bits
    again = ref.run(t["p0"], t["grads"], lr=lr, out_dim=k)
    assert all(np.array_equal(a[i], b[i]) for a, b in zip(out, again) for i in range(3))
    # running products: one multiplication per step
    b1t = b2t = 1.0
    for s in range(ref.STEPS):
        b1t, b2t = b1t * 0.9, b2t * 0.999
        assert out[s][3]["b1t"] == b1t and out[s][3]["b2t"] == b2t


@pytest.mark.parametrize("tag,k", NETS)
def test_refusal_rule(traj, nets, tag, k):
    t = traj[tag]
    sl = ref.slices(k)
    assert not ref.f16x3_refuses(t["p0"], k)
    # the rule is MlpNet._validated's: the same verdicts on the same vectors
    from delivery_drone_amd.policy import MlpNet
    probe = MlpNet.__new__(MlpNet)
    probe.compute = "f16x3"
    import torch
    probe.device = torch.device("cpu")

    def validated_refuses(flat):
        try:
            MlpNet._validated(probe, {key: torch.from_numpy(v.copy()) for key, v in ref.unflatten(flat, k).items()})
        except ValueError:
            return True
        return False

    gamma_limit = (128.0 - float(np.abs(t["p0"][sl["4.bias"]]).max())) / (128 ** 0.5 * (1 + 2 ** -8))
    crafted = []
    for key, idx, value in (("4.weight", 5, gamma_limit * 1.001), ("4.weight", 5, gamma_limit * 0.999),
                            ("7.bias", 0, 128.0), ("3.weight", 77, 2047.0), ("3.weight", 77, -2046.9),
                            ("6.weight", 3, np.inf), ("0.weight", 9, np.nan), ("1.weight", 2, np.nan),
                            ("9.weight", 1, 1e30), ("3.bias", 1, np.inf)):
        flat = t["p0"].copy()
        flat[sl[key].start + idx] = value
        crafted.append(flat)
        assert ref.f16x3_refuses(flat, k) == validated_refuses(flat), (key, value)
    assert [ref.f16x3_refuses(c, k) for c in crafted] == [True, False, True, True, False, True, True, True, False,
                                                          False]
    # a step whose candidate gamma passes the bound: every array and the counters keep their values
    g = np.zeros_like(t["p0"])
    at = sl["4.weight"].start + 5
    g[at] = -1.0
    lr = 4.0 * gamma_limit  # exp_avg and exp_avg_sq start at zero: the element moves by about 0.58 lr
    m0, v0 = np.zeros_like(t["p0"]), np.zeros_like(t["p0"])
    st0 = dict(ref.new_state(), step=3, b1t=0.9 ** 3, b2t=0.999 ** 3)
    p, m, v, st = ref.step(t["p0"], g, m0, v0, st0, lr=lr, out_dim=k, f16x3=True, weight_decay=0.0)
    assert p is t["p0"] and m is m0 and v is v0
    assert st == dict(st0, status=ref.REFUSED)
    p, m, v, st = ref.step(t["p0"], g, m0, v0, st, lr=lr, out_dim=k, f16x3=False, weight_decay=0.0)  # f32: it commits
    assert st["step"] == 4 and st["status"] == ref.REFUSED and abs(p[at]) > gamma_limit and m[at] != 0


def test_optimizer_state_layout_round_trips_through_torch(traj):
    """adamw_ref -> torch.optim.AdamW.load_state_dict -> one more step ==
    torch all the way; and torch's state_dict back into the restatement's
    arrays.  The layout is what delivery_drone_amd.AdamW.state_dict builds."""
    import torch
    tag, k = "critic", 1
    t, lr = traj[tag], ref.NOTEBOOK_LR[tag]
    sl, sh = ref.slices(k), ref.shapes(k)
    half = 4
    theirs, opt, params = ref.torch_adamw(t["p0"], t["grads"][:half], lr=lr, out_dim=k, dtype=torch.float32)
    sd = opt.state_dict()
    assert sorted(sd["state"]) == list(range(14)) and sd["param_groups"][0]["params"] == list(range(14))
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} and float(s["step"]) == half for s in sd["state"].values())
    # torch's arrays into ours: continue with the restatement, within the gap of the remaining steps
    p = theirs[-1]
    m = np.concatenate([sd["state"][i]["exp_avg"].numpy().reshape(-1) for i in range(14)])
    v = np.concatenate([sd["state"][i]["exp_avg_sq"].numpy().reshape(-1) for i in range(14)])
    b1t = b2t = 1.0
    for _ in range(half):
        b1t, b2t = b1t * 0.9, b2t * 0.999
    st = dict(step=half, b1t=b1t, b2t=b2t, status=0)
    for g in t["grads"][half:]:
        p, m, v, st = ref.step(p, g, m, v, st, lr=lr, out_dim=k)
    rest, _, _ = ref.torch_adamw(t["p0"], t["grads"], lr=lr, out_dim=k, dtype=torch.float32)
    unit = ref.gap_unit(p, lr, ref.update_scale(t["grads"])[-1])
    assert np.all(np.abs(rest[-1].astype(np.float64) - p.astype(np.float64)) <= G_CAP * unit) and st["step"] == 8
    # ours into torch: a fresh optimizer that loads the layout continues exactly as the one that made it
    ours = {"state": {i: {"step": torch.tensor(float(half)),
                          "exp_avg": torch.from_numpy(m0.copy()), "exp_avg_sq": torch.from_numpy(v0.copy())}
                      for i, (m0, v0) in enumerate(
                          (sd["state"][j]["exp_avg"].numpy(), sd["state"][j]["exp_avg_sq"].numpy()) for j in range(14))},
            "param_groups": [dict(sd["param_groups"][0], params=list(range(14)))]}
    fresh_params = [torch.nn.Parameter(q.detach().clone()) for q in params]
    fresh = torch.optim.AdamW(fresh_params, lr=123.0, foreach=False, fused=False)
    fresh.load_state_dict(ours)
    assert fresh.param_groups[0]["lr"] == lr
    for g in t["grads"][half:]:
        for key, q, r in zip(ref.KEYS, params, fresh_params):
            q.grad = torch.from_numpy(g[sl[key]].reshape(sh[key]).copy())
            r.grad = q.grad.clone()
        opt.step()
        fresh.step()
    assert all(torch.equal(q, r) for q, r in zip(params, fresh_params))


# ---- the C ABI and the Python surface --------------------------------------------------

NEW = ("dd_adamw_state_bytes", "dd_adamw_init", "dd_adamw_step")


def test_new_exports_exist_everywhere():
    out = subprocess.run(["nm", "-D", "--defined-only", abi.library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (dd_[a-z0-9_]+)$", out, flags=re.M))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(HEADER_DIR, "dronestep.h")).read(), flags=re.S)
    for name in NEW:
        assert name in exported and name in abi.EXPORTS and re.search(r"\b%s\s*\(" % name, header), name
    assert abi.DD_ABI_VERSION == 13 and abi.lib().dd_abi_version() == 13  # additions only
    assert {"AdamW", "ppo_update", "PpoUpdate"} <= set(delivery_drone_amd.__all__)
    from delivery_drone_amd import adamw
    assert delivery_drone_amd.AdamW is adamw.AdamW and delivery_drone_amd.ppo_update is adamw.ppo_update
    for name in ("flat_parameters", "state_dict", "load_state_dict", "backward"):
        assert hasattr(delivery_drone_amd.MlpNet, name), name
    assert abi.DD_ADAMW_REFUSED == ref.REFUSED == 1


def test_struct_layouts_match_the_header(tmp_path):
    structs = (abi.DDAdamWHyper, abi.DDAdamWState, abi.DDAdamWIO)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dronestep.h"', 'int main(void) {']
    for cls in structs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cls.__name__, cls.__name__))
        for name, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cls.__name__, name, cls.__name__, name))
    lines.append('printf("refused %d\\n", DD_ADAMW_REFUSED);')
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
    assert int(got["refused"]) == abi.DD_ADAMW_REFUSED
    assert ctypes.sizeof(abi.DDAdamWState) == 32 == abi.lib().dd_adamw_state_bytes()
    assert ctypes.sizeof(abi.DDAdamWHyper) == 40 and ctypes.sizeof(abi.DDAdamWIO) == 64


def test_argument_errors_without_gpu():
    lib = abi.lib()

    def run(hyper_none=False, io_none=False, **kw):
        f = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, params=16, grads=16, exp_avg=16,
                 exp_avg_sq=16, state=16, packed=16, out_dim=3, compute=abi.DD_MLP_F16X3, ln_eps=1e-5)
        f.update(kw)
        h = abi.DDAdamWHyper(f["lr"], f["beta1"], f["beta2"], f["eps"], f["weight_decay"])
        io = abi.DDAdamWIO(f["params"], f["grads"], f["exp_avg"], f["exp_avg_sq"], f["state"], f["packed"],
                           f["out_dim"], f["compute"], f["ln_eps"], 0)
        return lib.dd_adamw_step(None if hyper_none else ctypes.byref(h), None if io_none else ctypes.byref(io), None)

    assert run(hyper_none=True) == EINVAL and run(io_none=True) == EINVAL
    for name in ("params", "grads", "exp_avg", "exp_avg_sq", "state"):
        assert run(**{name: None}) == EINVAL, name
    assert run(state=12) == EINVAL and run(packed=8) == EINVAL  # alignment
    assert run(ln_eps=0.0) == EINVAL  # with a packed image to rebuild
    for k in (0, 2, 4, -1):
        assert run(out_dim=k) == EINVAL, k
    assert run(compute=2) == EINVAL and run(compute=-1) == EINVAL
    for name in ("lr", "beta1", "beta2", "eps", "weight_decay"):
        for bad in (-1e-3, float("nan"), float("inf"), -float("inf")):
            assert run(**{name: bad}) == EINVAL, (name, bad)
    assert run(beta1=1.0) == EINVAL and run(beta2=1.0) == EINVAL and run(beta2=1.5) == EINVAL
    assert lib.dd_adamw_init(16, 16, 8, None, None) == EINVAL
    assert lib.dd_adamw_init(None, 16, 8, 16, None) == EINVAL and lib.dd_adamw_init(16, None, 8, 16, None) == EINVAL
    assert lib.dd_adamw_init(16, 16, -1, 16, None) == EINVAL and lib.dd_adamw_init(16, 16, 8, 12, None) == EINVAL


def test_python_wrappers_check_before_the_gpu():
    from delivery_drone_amd import AdamW, ppo_update
    with pytest.raises(ValueError, match="MlpNet"):
        AdamW(object())
    with pytest.raises(ValueError, match="actor_opt"):
        ppo_update(object(), object(), None, type("O", (), {"net": None})(), type("O", (), {"net": None})())
