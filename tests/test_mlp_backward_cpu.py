"""CPU: the networks' backward pass without a GPU.  The float64 NumPy
restatement (tests/mlp_backward_ref.py) against float64 torch autograd and
against the notebook's own float32 gradients
(tests/golden/mlp_backward/grads.npz), and the C ABI of dd_mlp_backward:
exports, struct layouts against the header as a C compiler lays them out,
argument errors (fake pointers throughout; every error is returned before any
HIP call).

The reference's own float32 gap G.  Every gradient element is a sum over rows;
S = sum_rows |the row's contribution| (|dh_i| |a_j| for a weight, |dh_i|,
|dy_i xh_i|, |dy_i| for the vectors) is the scale a float32 summation's
rounding is measured on, and G is the largest |notebook .grad - restatement| /
(2^-24 S) over every element of both networks, the restatement fed the float64
head gradients of tests/ppo_loss_ref.py on the notebook's own rows.  Measured
on the fixture: G = 10,191 (actor 6.weight; the critic's largest is 331, at
6.weight too; every bias and LayerNorm tensor stays below 20, 105 for the
actor's 7.weight).  G is that large because S takes |a_j| as the row's scale,
while a float32 forward's error in a_j = max(gamma xh + beta, 0) is absolute:
about 16 roundings of 2^-24 on |gamma xh| + |beta| (three Linear + LayerNorm
stages deep), whatever is left after the two cancel.  A layer-2 unit that is
almost dead on all 203 rows (a_j ~ 1e-4 of its terms) has a tiny S, and its
column of 6.weight carries that ratio.  G_CAP = 2^14 is the bound asserted
here: 16 roundings x a cancellation of 2^10 between gamma xh and beta in the
worst unit of the fixture's networks.  The GPU test's bound is 4 G 2^-24 S
with G measured here, from the reference alone.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import golden_data as gd
import mlp_backward_ref as ref
import ppo_loss_ref
import delivery_drone_amd
from delivery_drone_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER_DIR = os.path.join(os.path.dirname(HERE), "include")
EINVAL = 1  # hipErrorInvalidValue
G_CAP = 2.0 ** 14
NETS = (("actor", "grad_logits"), ("critic", "grad_values"))


@pytest.fixture(scope="module")
def g():
    return gd.npz(os.path.join("ppo_loss", "losses.npz"))


@pytest.fixture(scope="module")
def fx():
    return gd.npz(os.path.join("mlp_backward", "grads.npz"))


@pytest.fixture(scope="module")
def nets():
    return gd.policy_fixture()[1]


@pytest.fixture(scope="module")
def restated(g, nets):
    """The restatement on the fixture rows, fed ppo_loss_ref's float64 head gradients."""
    heads = ppo_loss_ref.fixture_losses(g)
    return {tag: ref.backward(nets[tag], g["states"], heads[key]) + (heads[key],) for tag, key in NETS}


def reference_gap(fx, restated):
    """G: the notebook's float32 .grad against the restatement in units of 2^-24 S."""
    return {tag: ref.gap_units({k: fx[f"{tag}.{k}"] for k in ref.KEYS}, restated[tag][0], restated[tag][1])
            for tag, _ in NETS}


def test_fixture_is_data_in_the_subdirectory(fx, nets):
    path = os.path.join(gd.GOLDEN, "mlp_backward", "grads.npz")
    assert os.path.getsize(path) < 512 * 1024
    for tag, _ in NETS:
        for k in ref.KEYS:
            assert fx[f"{tag}.{k}"].shape == nets[tag][k].shape and fx[f"{tag}.{k}"].dtype == np.float32
    assert set(fx) == {f"{t}.{k}" for t, _ in NETS for k in ref.KEYS} | {"actor_norm", "critic_norm", "max_grad_norm"}
    assert float(fx["max_grad_norm"]) == 0.5


@pytest.mark.parametrize("tag,key", NETS)
def test_restatement_matches_float64_autograd(g, nets, restated, tag, key):
    import torch
    grads, S, norm, head = restated[tag]
    body = torch.nn.Sequential(*list(gd.torch_mlp(nets[tag]).double().children())[:10])  # up to the last Linear
    z = body(torch.from_numpy(g["states"]).double())
    z.backward(torch.from_numpy(np.asarray(head, dtype=np.float64).reshape(tuple(z.shape))))
    worst = 0.0
    for k, p in body.named_parameters():
        want = p.grad.numpy()
        nz = want != 0
        assert np.array_equal(grads[k] == 0, ~nz), k
        worst = max(worst, float((np.abs(grads[k] - want)[nz] / np.abs(want)[nz]).max()))
    print(tag, "largest relative difference to float64 autograd", worst)
    assert worst <= 1e-10
    total = np.sqrt(sum(float((p.grad.numpy() ** 2).sum()) for p in body.parameters()))
    assert abs(norm - total) <= 1e-12 * total


def test_reference_gap(fx, restated):
    gap = reference_gap(fx, restated)
    for tag, _ in NETS:
        print(tag, {k: round(v, 2) for k, v in gap[tag].items()})
    G = max(max(v.values()) for v in gap.values())
    print("G =", G)
    assert G <= G_CAP
    for tag, _ in NETS:  # clip_grad_norm_'s float32 norm
        assert abs(float(fx[f"{tag}_norm"]) - restated[tag][2]) <= 1e-6 * restated[tag][2]


@pytest.mark.parametrize("variant", ref.VARIANTS)
@pytest.mark.parametrize("tag,key", NETS)
def test_reference_gap_on_the_crafted_networks(g, nets, tag, key, variant):
    """tests/test_gpu_mlp_backward_exact.py holds the kernel to 4 G 2^-24 S on
    mlp_backward_ref.crafted's networks (the ReLU edge y = 0 and +-2^-100 with
    gamma = 0; a layer of zero variance) with the fixture's G: fair only if
    float32 autograd itself stays inside G there.  Measured: actor relu 5,887
    (its 6.weight), var0 31; critic relu 229, var0 84; the fixture's G is
    10,191.  gap_units asserts that where S = 0 autograd gives an exact zero:
    dgamma, dbeta and the next Linear's column of every off unit."""
    import torch
    sd = ref.crafted(nets[tag], variant)
    head = np.asarray(ppo_loss_ref.fixture_losses(g)[key]).astype(np.float32)
    want, S, _ = ref.backward(sd, g["states"], head.astype(np.float64))
    body = torch.nn.Sequential(*list(gd.torch_mlp(sd).children())[:10])  # up to the last Linear, float32
    z = body(torch.from_numpy(g["states"]))
    z.backward(torch.from_numpy(head.reshape(tuple(z.shape))))
    got = {k: p.grad.numpy() for k, p in body.named_parameters()}
    units = ref.gap_units(got, want, S)
    worst = max(units, key=units.get)
    print(f"crafted {tag} {variant}: gap {units[worst]:.0f} x 2^-24 S (its {worst})",
          {k: round(v, 1) for k, v in units.items()})
    assert units[worst] <= G_CAP
    for name, (k, idx) in ref.crafted_zeros(sd, variant).items():
        assert not np.any(S[k][idx]) and not np.any(want[k][idx]) and not np.any(got[k][idx]), name
    if variant == "relu":  # the on units pass their gradient: a next-layer column of about 1e-32, normal
        for ln, nxt in (("1", "3.weight"), ("4", "6.weight"), ("7", "9.weight")):
            assert want[ln + ".bias"][17] != 0 and got[ln + ".bias"][17] != 0, ln
            assert 2.0 ** -126 <= np.abs(got[nxt][:, 17]).max() < 2.0 ** -80, nxt


def test_restatement_edge_cases(g, nets):
    x = g["states"][:40]
    rng = np.random.default_rng(3)
    dz = rng.normal(0, 1, (40, 3))
    a, Sa, na = ref.backward(nets["actor"], x, dz)
    # linear in grad_out; rows with a zero gradient contribute nothing
    b, _, nb = ref.backward(nets["actor"], x, 2.0 * dz)
    assert all(np.allclose(b[k], 2.0 * a[k], rtol=1e-13, atol=0) for k in ref.KEYS) and abs(nb - 2 * na) <= 1e-12 * nb
    more = np.concatenate([x, g["states"][100:117]])
    c, Sc, _ = ref.backward(nets["actor"], more, np.concatenate([dz, np.zeros((17, 3))]))
    assert all(np.array_equal(c[k], a[k]) and np.array_equal(Sc[k], Sa[k]) for k in ref.KEYS)
    # tests/test_gpu_mlp_backward_exact.py's identities 1 and 2, of the oracle itself: one live row gives the
    # m = 1 result wherever it sits among rows with a zero head gradient, and the rows add up.  Within 4 G_CAP
    # 2^-53 S < 1e-11 S, not bit for bit: a BLAS product may add a row's terms in another order at another m,
    # which the forward's cancellation carries into S's units as it does in float32 (the docstring's G).
    tol = 4.0 * G_CAP * 2.0 ** -53
    singles = [ref.backward(nets["actor"], x[j:j + 1], dz[j:j + 1]) for j in range(40)]
    for pos, j in ((0, 5), (16, 0), (39, 39), (17, 23)):
        one = np.zeros((40, 3))
        one[pos] = dz[j]
        rows = x.copy()  # the dead rows keep their own states
        rows[pos] = x[j]
        e, Se, ne = ref.backward(nets["actor"], rows, one)
        for k in ref.KEYS:
            assert np.all(np.abs(e[k] - singles[j][0][k]) <= tol * singles[j][1][k]), (pos, j, k)
            assert np.all(np.abs(Se[k] - singles[j][1][k]) <= tol * singles[j][1][k]), (pos, j, k)
        assert abs(ne - singles[j][2]) <= 1e-9 * ne
    for k in ref.KEYS:
        total = sum(s[0][k] for s in singles)
        assert np.all(np.abs(a[k] - total) <= 40 * tol * Sa[k]), k
        assert np.all(np.abs(Sa[k] - sum(s[1][k] for s in singles)) <= 40 * tol * Sa[k]), k
    # the bias of the last Linear does not enter any gradient; a LayerNorm output is shift invariant
    sd = dict(nets["actor"])
    sd["9.bias"] = sd["9.bias"] + 5.0
    d, _, _ = ref.backward(sd, x, dz)
    assert all(np.array_equal(d[k], a[k]) for k in ref.KEYS)
    assert np.all(np.abs(a["3.bias"].sum()) <= 1e-12 * Sa["3.bias"].sum())  # sum_out dh = 0 after a LayerNorm
    spread = ref.head_spread(nets["actor"], x, np.full((40, 3), 1e-3))
    moved, _, _ = ref.backward(nets["actor"], x, dz + 1e-3)
    assert all(np.all(np.abs(moved[k] - a[k]) <= spread[k] * (1 + 1e-9) + 1e-300) for k in ref.KEYS)


# ---- the C ABI -------------------------------------------------------------------

NEW = ("dd_mlp_backward_workspace", "dd_mlp_backward")


def test_new_exports_exist_everywhere():
    out = subprocess.run(["nm", "-D", "--defined-only", abi.library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (dd_[a-z0-9_]+)$", out, flags=re.M))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(HEADER_DIR, "dronestep.h")).read(), flags=re.S)
    for name in NEW:
        assert name in exported and name in abi.EXPORTS and re.search(r"\b%s\s*\(" % name, header), name
    assert abi.DD_ABI_VERSION == 13 and abi.lib().dd_abi_version() == 13  # additions only
    assert {"ppo_grads", "PpoGrads"} <= set(delivery_drone_amd.__all__)
    from delivery_drone_amd import ppo_grad
    assert delivery_drone_amd.ppo_grads is ppo_grad.ppo_grads and delivery_drone_amd.PpoGrads is ppo_grad.PpoGrads
    assert ppo_grad.PpoGrads._fields == ("losses", "actor", "critic", "actor_grad_norm", "critic_grad_norm")
    assert hasattr(delivery_drone_amd.MlpNet, "backward")


def test_struct_layouts_match_the_header(tmp_path):
    structs = (abi.DDMlpGrads, abi.DDMlpBackwardIO)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dronestep.h"', 'int main(void) {']
    for cls in structs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cls.__name__, cls.__name__))
        for name, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cls.__name__, name, cls.__name__, name))
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
    assert ctypes.sizeof(abi.DDMlpGrads) == 14 * 8 and ctypes.sizeof(abi.DDMlpBackwardIO) == 16 + 14 * 8 + 16
    assert [n for n, _ in abi.DDMlpGrads._fields_] == [n for n, _ in abi.DDMlpParams._fields_][:14]


def test_backward_argument_errors_without_gpu():
    lib = abi.lib()
    ws_bytes = lib.dd_mlp_backward_workspace()
    assert ws_bytes > 0 and ws_bytes % 16 == 0 and ws_bytes < 64 << 20  # fixed: it does not depend on m

    def run(m=4, ws=16, out_dim=3, params_none=False, io_none=False, param=None, grad=None, **kw):
        pf = {name: 8 for name, _ in abi.DDMlpParams._fields_[:14]}
        if param:
            pf[param] = None
        p = abi.DDMlpParams(*[pf[name] for name, _ in abi.DDMlpParams._fields_[:14]], out_dim, 1e-5)
        gf = {name: 8 for name, _ in abi.DDMlpGrads._fields_}
        if grad:
            gf[grad] = None
        f = dict(states=8, grad_out=8, grad_norm=8, max_norm=0.5)
        f.update(kw)
        io = abi.DDMlpBackwardIO(f["states"], f["grad_out"], abi.DDMlpGrads(*[gf[n] for n, _ in abi.DDMlpGrads._fields_]),
                                 f["grad_norm"], f["max_norm"])
        return lib.dd_mlp_backward(None if params_none else ctypes.byref(p), None if io_none else ctypes.byref(io), m,
                                   ws, None)

    assert run(params_none=True) == EINVAL and run(io_none=True) == EINVAL
    assert run(m=-1) == EINVAL
    for k in (0, 2, 4, -1):
        assert run(out_dim=k) == EINVAL, k
    assert run(ws=None) == EINVAL  # with m > 0
    assert run(states=None) == EINVAL and run(grad_out=None) == EINVAL
    for name, _ in abi.DDMlpGrads._fields_:
        assert run(param=name) == EINVAL and run(grad=name) == EINVAL, name
    assert run(m=-1, out_dim=1) == EINVAL


def test_python_wrappers_check_before_the_gpu():
    import torch
    from delivery_drone_amd import ppo_grads
    with pytest.raises(ValueError, match="MlpNet actor"):
        ppo_grads(object(), object(), torch.zeros(4, 15), torch.zeros(4, 3), torch.zeros(4), torch.zeros(4),
                  torch.zeros(4))
