"""GPU: dd_pg_losses, dd_td_losses, reinforce_update and actor_critic_update.

Exactness: the kernels against the float64 restatement (tests/pg_loss_ref.py)
fed the device's OWN log_prob, probs and values.  The per-row outputs
(grad_logits, td_targets, td_errors, grad_values) are IEEE double operations in
the restatement's order and one rounding: bit for bit.  The scalars are sums in
double over a fixed tree against NumPy's pairwise sum: within 1e-9 relative
(tests/test_gpu_ppo_loss.py's bound for at most 2^18 terms); counts exactly.

Parity with the notebooks (tests/golden/pg_loss/pg.npz), every bound computed
on the CPU from the fixture alone, as tests/test_gpu_ppo_loss.py does:
    2 x (first-order spread when each per-row input moves within its accepted
         bound: log_prob 1e-5 (1 + |lp|), probabilities 2e-6, values VALUE_TOL)
    + the notebook's own float32 gap (|restatement on its rows - its result|).
The parameters after the one AdamW step, at the fixture's kept indices: the
gradients first, |ours - notebook| <= GRAD_TOL max|g| per network (dd_mlp_backward's
pinned parity with autograd, tests/test_gpu_mlp_backward.py, accepts about 1e-2
of a tensor's scale and measures 1e-4; 1e-3 here, which also covers the clip
factor's and the head gradient's own spread).  Then the step: in its first
step AdamW moves p by lr u, u = g / (|g| + eps), du/dg = eps / (|g| + eps)^2, so
|du| <= min(2, dg eps / (max(|g| - dg, 0) + eps)^2), and
|ours - notebook| <= 1 ulp + G_CAP 2^-24 (|p| + lr) + lr |du|
(tests/test_gpu_adamw.py's bound against torch, plus the gradient's spread).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_data as gd
import pg_loss_ref as ref
from delivery_drone_amd import (AdamW, MlpNet, VecDroneEnv, abi, actor_critic_update, collect_reinforce,
                                reinforce_losses, reinforce_update, td_losses)
from delivery_drone_amd.config import EnvConfig
from delivery_drone_amd.pg_loss import _score_losses
from delivery_drone_amd.train_batch import ReinforceBatch
from test_adamw_cpu import G_CAP

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
COMPUTE = ("f32", "f16x3")
VALUE_TOL = {"f32": (2e-6, 1e-4), "f16x3": (8e-6, 4e-4)}  # (relative, absolute): tests/test_gpu_policy.py's
PROB_TOL = 2e-6
GRAD_TOL = 1e-3
SUM_TOL = 1e-9
M = 203
LR = 1e-3
U = 2.0 ** -24


def lp_tol(lp):
    return 1e-5 * (1.0 + np.abs(np.asarray(lp, np.float64)))


@pytest.fixture(scope="module")
def g():
    return gd.npz("pg_loss/pg.npz")


@pytest.fixture(scope="module")
def nets():
    return gd.policy_fixture()[1]


@pytest.fixture(scope="module")
def reference(g):
    """Computed once on the CPU, shared and left unchanged: the restatement on
    the notebooks' own rows and its distance from their results."""
    pg = ref.pg_losses(g["reinforce.log_probs"], g["reinforce.probs"], g["actions"], g["reinforce.advantages"])
    td = ref.td_losses(g["td.values"], g["td.next_values"], g["rewards"], g["dones"], float(g["gamma"]), 0.01)
    ac = ref.pg_losses(g["td.log_probs"], g["td.probs"], g["actions"], g["td.td_errors"])
    gap = {"reinforce.loss": abs(pg["loss"] - float(g["reinforce.loss"])),
           "reinforce.grad_logits": np.abs(pg["grad_logits"].astype(np.float64) - g["reinforce.grad_logits"]),
           "td.critic_loss": abs(td["critic_loss"] - float(g["td.critic_loss"])),
           "td.actor_loss": abs(ac["loss"] - float(g["td.actor_loss"])),
           "td.grad_logits": np.abs(ac["grad_logits"].astype(np.float64) - g["td.grad_logits"])}
    for k in ("td_targets", "td_errors", "grad_values"):
        gap["td." + k] = np.abs(td[k].astype(np.float64) - g["td." + k])
    return dict(pg=pg, td=td, ac=ac, gap=gap)


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def same_np(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def close(got, want):
    got, want = float(got), float(want)
    return (np.isnan(got) and np.isnan(want)) or abs(got - want) <= SUM_TOL * abs(want)


def dev_inputs(g, dev, keys, reps=None):
    arrs = [g[k] if reps is None else np.resize(g[k], (reps,) + g[k].shape[1:]) for k in keys]
    return [torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in arrs]


PG_KEYS = ("states", "actions", "reinforce.advantages")
TD_KEYS = ("states", "rewards", "next_states", "dones")


def make(nets, dev, compute):
    actor = MlpNet(nets["actor"], device=dev, compute=compute)
    critic = MlpNet(nets["critic"], device=dev, compute=compute)
    return actor, critic, AdamW(actor, lr=LR), AdamW(critic, lr=LR)


def check_pg_exact(out_loss, out_count, lp, probs, grad, actions, weights, active=None):
    want = ref.pg_losses(host(lp), host(probs), host(actions), host(weights),
                         None if active is None else host(active))
    print(f"exact pg loss: got {float(out_loss)!r} want {want['loss']!r}")
    assert close(out_loss, want["loss"]) and float(out_count) == want["count"]
    if grad is not None:
        assert same_np(host(grad), want["grad_logits"])
    return want


def check_td_exact(td, rewards, dones, gamma=0.99, value_reg=0.01, active=None):
    want = ref.td_losses(host(td.values), host(td.next_values), host(rewards), host(dones), gamma, value_reg,
                         None if active is None else host(active))
    for k in ("critic_loss", "mse", "value_reg"):
        print(f"exact td {k}: got {float(getattr(td, k))!r} want {want[k]!r}")
        assert close(getattr(td, k), want[k]), k
    assert float(td.count) == want["count"]
    assert same_np(host(td.td_targets), want["td_targets"]) and same_np(host(td.td_errors), want["td_errors"])
    if td.grad_values is not None:
        assert same_np(host(td.grad_values), want["grad_values"])
    return want


# ---- the fixture ---------------------------------------------------------------------------

@pytest.mark.parametrize("compute", COMPUTE)
def test_reinforce_losses_on_the_fixture(g, nets, reference, gpu_device, compute):
    actor = MlpNet(nets["actor"], device=gpu_device, compute=compute)
    states, actions, adv = dev_inputs(g, gpu_device, PG_KEYS)
    out = reinforce_losses(actor, states, actions, adv, grads=True)
    assert out.loss.dim() == 0 and out.loss.dtype == torch.float64 and out.loss.device == gpu_device
    none = reinforce_losses(actor, states, actions, adv)
    assert none.grad_logits is None and same(none.loss, out.loss)
    mask = (actions.to(torch.uint8) * torch.tensor([1, 2, 4], dtype=torch.uint8, device=gpu_device)).sum(1)
    masked = reinforce_losses(actor, states, mask.to(torch.uint8), adv, grads=True)  # bitmask actions: the same bits
    assert same(masked.grad_logits, out.grad_logits) and same(masked.loss, out.loss)
    result, lp, probs, grad = _score_losses(actor, states, actions, adv, None, True, "reinforce_losses")
    assert same(result[abi.DD_PG_LOSS], out.loss) and float(result[abi.DD_PG_COUNT]) == M
    check_pg_exact(out.loss, result[abi.DD_PG_COUNT], out.log_probs, out.probs, out.grad_logits, actions, adv)
    # parity with the notebook
    nb_lp, A = g["reinforce.log_probs"].astype(np.float64), g["reinforce.advantages"].astype(np.float64)
    assert np.all(np.abs(host(out.log_probs) - nb_lp) <= lp_tol(nb_lp))
    assert np.all(np.abs(host(out.probs) - g["reinforce.probs"]) <= PROB_TOL)
    bound = 2.0 * (np.abs(A) * lp_tol(nb_lp)).mean() + reference["gap"]["reinforce.loss"]
    err = abs(float(out.loss) - float(g["reinforce.loss"]))
    print(f"parity loss: got {float(out.loss)!r} notebook {float(g['reinforce.loss'])!r} err {err:.3g} bound {bound:.3g}")
    assert err <= bound
    gbound = 2.0 * np.abs(A / M)[:, None] * PROB_TOL + reference["gap"]["reinforce.grad_logits"]
    gerr = np.abs(host(out.grad_logits) - g["reinforce.grad_logits"])
    print(f"parity grad_logits: max err {gerr.max():.3g}, largest bound {gbound.max():.3g}")
    assert np.all(gerr <= gbound)
    assert np.array_equal(host(out.grad_logits) == 0, g["reinforce.grad_logits"] == 0)


@pytest.mark.parametrize("compute", COMPUTE)
def test_td_losses_on_the_fixture(g, nets, reference, gpu_device, compute):
    actor, critic = make(nets, gpu_device, compute)[:2]
    states, rewards, next_states, dones = dev_inputs(g, gpu_device, TD_KEYS)
    actions = torch.as_tensor(g["actions"], device=gpu_device)
    td = td_losses(critic, states, rewards, next_states, dones, gamma=float(g["gamma"]), grads=True)
    for t in (td.critic_loss, td.mse, td.value_reg, td.count):
        assert t.dim() == 0 and t.dtype == torch.float64 and t.device == gpu_device
    none = td_losses(critic, states, rewards, next_states, dones.bool(), gamma=float(g["gamma"]))
    assert none.grad_values is None and same(none.critic_loss, td.critic_loss) and same(none.td_errors, td.td_errors)
    assert same(td.values, critic(states)) and same(td.next_values, critic(next_states))
    check_td_exact(td, rewards, dones)
    # the actor stage on the device's own float32 td_errors
    result, lp, probs, grad = _score_losses(actor, states, actions, td.td_errors, None, True, "actor_critic_update")
    check_pg_exact(result[abi.DD_PG_LOSS], result[abi.DD_PG_COUNT], lp, probs, grad, actions, td.td_errors)
    # parity with the notebook
    rel, abs_ = VALUE_TOL[compute]
    v, vn, d = (g[k].astype(np.float64) for k in ("td.values", "td.next_values", "dones"))
    d_v, d_vn = abs_ + rel * np.abs(v), abs_ + rel * np.abs(vn)
    assert np.all(np.abs(host(td.values) - v) <= d_v) and np.all(np.abs(host(td.next_values) - vn) <= d_vn)
    d_t = float(g["gamma"]) * d_vn * (1.0 - d)
    d_e = d_t + d_v
    delta = reference["td"]["delta"]
    gap = reference["gap"]
    spread = {"td_targets": d_t, "td_errors": d_e, "grad_values": (2.0 * d_e + 0.02 * d_v) / M}
    for k, s in spread.items():
        err = np.abs(host(getattr(td, k)).astype(np.float64) - g["td." + k])
        print(f"parity {k}: max err {err.max():.3g}, largest bound {(2.0 * s + gap['td.' + k]).max():.3g}")
        assert np.all(err <= 2.0 * s + gap["td." + k]), k
    bound = 2.0 * ((2.0 * np.abs(delta) * d_e).mean() + 0.01 * (2.0 * np.abs(v) * d_v).mean()) + gap["td.critic_loss"]
    err = abs(float(td.critic_loss) - float(g["td.critic_loss"]))
    print(f"parity critic_loss: got {float(td.critic_loss)!r} err {err:.3g} bound {bound:.3g}")
    assert err <= bound
    nb_lp, w = g["td.log_probs"].astype(np.float64), g["td.td_errors"].astype(np.float64)
    bound = 2.0 * (np.abs(w) * lp_tol(nb_lp) + np.abs(nb_lp) * d_e).mean() + gap["td.actor_loss"]
    err = abs(float(result[abi.DD_PG_LOSS]) - float(g["td.actor_loss"]))
    print(f"parity actor_loss: got {float(result[abi.DD_PG_LOSS])!r} err {err:.3g} bound {bound:.3g}")
    assert err <= bound
    p = g["td.probs"].astype(np.float64)
    gbound = 2.0 * (np.abs(w / M)[:, None] * PROB_TOL + (d_e / M)[:, None] * np.abs((g["actions"] != 0) - p)) \
        + gap["td.grad_logits"]
    gerr = np.abs(host(grad) - g["td.grad_logits"])
    print(f"parity grad_logits: max err {gerr.max():.3g}, largest bound {gbound.max():.3g}")
    assert np.all(gerr <= gbound)


# ---- sizes -----------------------------------------------------------------------------------

@pytest.mark.parametrize("compute", COMPUTE)
@pytest.mark.parametrize("m", [1, 512 * 256 + 1])
def test_sizes(g, nets, gpu_device, compute, m):
    """One row, and one full trip of the 512 x 256 grid-stride loop with a
    one-row second trip.  Exactness only; two runs give identical bits."""
    actor, critic = make(nets, gpu_device, compute)[:2]
    states, actions, adv = dev_inputs(g, gpu_device, PG_KEYS, reps=m)
    _, rewards, next_states, dones = dev_inputs(g, gpu_device, TD_KEYS, reps=m)
    a = _score_losses(actor, states, actions, adv, None, True, "reinforce_losses")
    b = _score_losses(actor, states, actions, adv, None, True, "reinforce_losses")
    assert all(same(x, y) for x, y in zip(a, b))
    check_pg_exact(a[0][abi.DD_PG_LOSS], a[0][abi.DD_PG_COUNT], a[1], a[2], a[3], actions, adv)
    x = td_losses(critic, states, rewards, next_states, dones, grads=True)
    y = td_losses(critic, states, rewards, next_states, dones, grads=True)
    assert all(same(p, q) for p, q in zip(x, y))
    check_td_exact(x, rewards, dones)


def test_unaligned_input_views(g, nets, gpu_device):
    """Rows 1.. of larger tensors: 4 bytes (60 for the states) past a 16-byte boundary."""
    actor, critic = make(nets, gpu_device, "f32")[:2]
    big = dev_inputs(g, gpu_device, PG_KEYS + TD_KEYS[1:], reps=M + 1)
    views = [t[1:] for t in big]
    assert all(v.is_contiguous() for v in views) and views[2].data_ptr() % 16 == 4
    states, actions, adv, rewards, next_states, dones = views
    got = _score_losses(actor, states, actions, adv, None, True, "reinforce_losses")
    want = _score_losses(actor, *[v.clone() for v in (states, actions, adv)], None, True, "reinforce_losses")
    assert all(same(x, y) for x, y in zip(got, want))
    x = td_losses(critic, states, rewards, next_states, dones, grads=True)
    y = td_losses(critic, *[v.clone() for v in (states, rewards, next_states, dones)], grads=True)
    assert all(same(p, q) for p, q in zip(x, y))
    check_td_exact(x, rewards, dones)


# ---- the mask ----------------------------------------------------------------------------------

@pytest.mark.parametrize("compute", COMPUTE)
def test_mask(g, nets, gpu_device, compute):
    actor, critic = make(nets, gpu_device, compute)[:2]
    states, actions, adv = dev_inputs(g, gpu_device, PG_KEYS)
    _, rewards, next_states, dones = dev_inputs(g, gpu_device, TD_KEYS)
    on = torch.as_tensor(np.random.default_rng(4).random(M) < 0.6, device=gpu_device)
    cnt = int(on.sum())
    assert 0 < cnt < M
    nan = torch.where(on, 0.0, float("nan")).to(torch.float32)  # an inactive row's inputs are never read
    for active in (on, on.to(torch.uint8)):
        full = _score_losses(actor, states, actions, adv + nan, active, True, "reinforce_losses")
        part = _score_losses(actor, states[on], actions[on], adv[on], None, True, "reinforce_losses")
        assert float(full[0][abi.DD_PG_COUNT]) == cnt == float(part[0][abi.DD_PG_COUNT])
        assert close(full[0][abi.DD_PG_LOSS], part[0][abi.DD_PG_LOSS])
        assert same(full[3][on], part[3]) and not bool(full[3][~on].any())
        check_pg_exact(full[0][abi.DD_PG_LOSS], full[0][abi.DD_PG_COUNT], full[1], full[2], full[3], actions,
                       adv + nan, active)
        x = td_losses(critic, states, rewards + nan, next_states, dones + nan, active=active, grads=True)
        y = td_losses(critic, states[on], rewards[on], next_states[on], dones[on], grads=True)
        assert float(x.count) == cnt == float(y.count)
        for k in ("critic_loss", "mse", "value_reg"):
            assert close(getattr(x, k), getattr(y, k)), k
        for k in ("td_targets", "td_errors", "grad_values"):
            assert same(getattr(x, k)[on], getattr(y, k)) and not bool(getattr(x, k)[~on].any()), k
        check_td_exact(x, rewards + nan, dones + nan, active=active)
    # no active row: NaN scalars (torch's mean over nothing), all-zero gradients
    off = torch.zeros(M, dtype=torch.bool, device=gpu_device)
    result, _, _, grad = _score_losses(actor, states, actions, adv, off, True, "reinforce_losses")
    assert bool(torch.isnan(result[abi.DD_PG_LOSS])) and float(result[abi.DD_PG_COUNT]) == 0.0
    assert not bool(grad.any())
    x = td_losses(critic, states, rewards, next_states, dones, active=off, grads=True)
    assert all(bool(torch.isnan(t)) for t in (x.critic_loss, x.mse, x.value_reg)) and float(x.count) == 0.0
    assert not bool(x.grad_values.any()) and not bool(x.td_errors.any()) and not bool(x.td_targets.any())


def test_saturated_probabilities(g, gpu_device):
    """dd_pg_losses on hand-made rows, as tests/test_ppo_loss_cpu.py's edge
    cases make them: a probability outside clamp_probs' range gets a 0
    gradient, a NaN is carried."""
    lib = abi.lib()
    probs = g["td.probs"].copy()
    probs[3, 1], probs[4, 0], probs[5, 2], probs[6, 0], probs[7, 1] = 1e-9, 1.0, np.nan, 0.0, 1.0 - 2.0 ** -25
    t = {k: torch.as_tensor(np.ascontiguousarray(v), device=gpu_device)
         for k, v in dict(lp=g["td.log_probs"], probs=probs, actions=g["actions"], w=g["td.td_errors"]).items()}
    result = torch.empty(abi.DD_PG_RESULTS, dtype=torch.float64, device=gpu_device)
    grad = torch.empty(M, 3, dtype=torch.float32, device=gpu_device)
    ws = torch.empty(int(lib.dd_pg_loss_workspace()) // 8, dtype=torch.int64, device=gpu_device)
    io = abi.DDPgLossIO(t["lp"].data_ptr(), t["probs"].data_ptr(), t["actions"].data_ptr(), abi.DD_ACT_F32X3, 0,
                        t["w"].data_ptr(), None, result.data_ptr(), grad.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)
    abi.check(lib.dd_pg_losses(ctypes.byref(io), M, ws.data_ptr(), stream), "dd_pg_losses")
    out = host(grad)
    assert out[3, 1] == 0 and out[4, 0] == 0 and out[6, 0] == 0 and out[7, 1] == 0 and np.isnan(out[5, 2])
    assert np.isfinite(np.delete(out.reshape(-1), 5 * 3 + 2)).all() and out[3, 0] != 0
    check_pg_exact(result[abi.DD_PG_LOSS], result[abi.DD_PG_COUNT], t["lp"], t["probs"], grad, t["actions"], t["w"])


# ---- the two updates ---------------------------------------------------------------------------

def fixture_batch(g, dev):
    states, actions, adv = dev_inputs(g, dev, PG_KEYS)
    stats = torch.as_tensor(np.array([float(g["reinforce.baseline"]), float(g["reinforce.std"])]), device=dev)
    returns = torch.as_tensor(g["returns"], device=dev)
    return ReinforceBatch(states, actions, returns, adv, stats[0], stats[1], None, None, None, None)


def same_optimizer(o, o2):
    return all(same(p, q) for p, q in ((o.params, o2.params), (o.exp_avg, o2.exp_avg), (o.exp_avg_sq, o2.exp_avg_sq),
                                       (o._state, o2._state), (o.net.packed, o2.net.packed)))


def check_step_parity(tag, grads, opt, nb_grad, nb_after, idx):
    """The docstring's bound on the clipped gradients and the parameters after one step."""
    got_g = host(grads)[idx].astype(np.float64)
    nb_g = nb_grad.astype(np.float64)
    dg = GRAD_TOL * np.abs(nb_g).max()
    print(f"{tag}: gradient max err {np.abs(got_g - nb_g).max():.3g} bound {dg:.3g}")
    assert np.all(np.abs(got_g - nb_g) <= dg)
    eps = 1e-8
    du = np.minimum(2.0, dg * eps / (np.maximum(np.abs(nb_g) - dg, 0.0) + eps) ** 2)
    got, want = host(opt.params)[idx].astype(np.float64), nb_after.astype(np.float64)
    bound = gd.ulp32(want) + G_CAP * U * (np.abs(want) + LR) + LR * du
    err = np.abs(got - want)
    print(f"{tag}: parameters max err {err.max():.3g}, largest err / bound {(err / bound).max():.3g}, "
          f"elements on the sign's edge {(du == 2.0).mean():.3f}")
    assert np.all(err <= bound) and (du < 1e-3).mean() > 0.5


@pytest.mark.parametrize("compute", COMPUTE)
def test_reinforce_update(g, nets, gpu_device, compute):
    batch = fixture_batch(g, gpu_device)
    (actor, _, opt, _), (actor2, _, opt2, _) = make(nets, gpu_device, compute), make(nets, gpu_device, compute)
    out = reinforce_update(actor, batch, opt, max_grad_norm=0.5)
    # its parts, one by one
    parts = reinforce_losses(actor2, batch.states, batch.actions, batch.advantages, grads=True)
    grads, norm = actor2.backward(batch.states, parts.grad_logits, max_norm=0.5)
    opt2.step(grads)
    assert same(out.loss, parts.loss) and same(out.grad_norm, norm) and same_optimizer(opt, opt2)
    assert same(opt._grad_out, torch.as_strided(grads["0.weight"], (actor.grad_numel(),), (1,)))
    assert out.baseline is batch.baseline and out.std is batch.std
    assert all(t.dim() == 0 and t.dtype == torch.float64 and t.device == gpu_device for t in out)
    assert opt.step_count() == 1 and opt.status() == 0
    nb_norm = float(g["reinforce.grad_norm"])
    assert abs(float(out.grad_norm) - nb_norm) <= GRAD_TOL * nb_norm
    check_step_parity(f"{compute} reinforce actor", opt._grad_out, opt, g["reinforce.actor_grad"],
                      g["reinforce.actor_after"], g["idx_actor"])


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("compute", COMPUTE)
def test_actor_critic_update(g, nets, gpu_device, compute, masked):
    states, rewards, next_states, dones = dev_inputs(g, gpu_device, TD_KEYS)
    actions = torch.as_tensor(g["actions"], device=gpu_device)
    active = torch.as_tensor(np.arange(M) % 5 != 0, device=gpu_device) if masked else None
    ours, twin = make(nets, gpu_device, compute), make(nets, gpu_device, compute)
    out = actor_critic_update(*ours[:2], states, actions, rewards, next_states, dones, *ours[2:],
                              gamma=float(g["gamma"]), active=active)
    # its parts, one by one, in the notebook's order
    actor2, critic2, a_opt2, c_opt2 = twin
    td = td_losses(critic2, states, rewards, next_states, dones, gamma=float(g["gamma"]), active=active, grads=True)
    c_grads, c_norm = critic2.backward(states, td.grad_values, max_norm=0.5)
    c_opt2.step(c_grads)
    result, _, _, g_logits = _score_losses(actor2, states, actions, td.td_errors, active, True, "actor_critic_update")
    a_grads, a_norm = actor2.backward(states, g_logits, max_norm=0.5)
    a_opt2.step(a_grads)
    assert same(out.actor_loss, result[abi.DD_PG_LOSS]) and same(out.critic_loss, td.critic_loss)
    assert same(out.td_errors, td.td_errors) and same(out.actor_grad_norm, a_norm)
    assert same(out.critic_grad_norm, c_norm)
    assert same_optimizer(ours[2], a_opt2) and same_optimizer(ours[3], c_opt2)
    assert ours[2].step_count() == 1 and ours[3].step_count() == 1
    if masked:
        assert not bool(out.td_errors[~active].any())
        return
    for k, t in (("td.actor_grad_norm", out.actor_grad_norm), ("td.critic_grad_norm", out.critic_grad_norm)):
        assert abs(float(t) - float(g[k])) <= GRAD_TOL * float(g[k]), k
    check_step_parity(f"{compute} td critic", ours[3]._grad_out, ours[3], g["td.critic_grad"], g["td.critic_after"],
                      g["idx_critic"])
    check_step_parity(f"{compute} td actor", ours[2]._grad_out, ours[2], g["td.actor_grad"], g["td.actor_after"],
                      g["idx_actor"])


def test_no_active_row_still_steps(g, nets, gpu_device):
    states, rewards, next_states, dones = dev_inputs(g, gpu_device, TD_KEYS)
    actions = torch.as_tensor(g["actions"], device=gpu_device)
    actor, critic, a_opt, c_opt = make(nets, gpu_device, "f32")
    off = torch.zeros(M, dtype=torch.bool, device=gpu_device)
    out = actor_critic_update(actor, critic, states, actions, rewards, next_states, dones, a_opt, c_opt, active=off)
    assert bool(torch.isnan(out.actor_loss)) and bool(torch.isnan(out.critic_loss))
    assert float(out.actor_grad_norm) == 0.0 and float(out.critic_grad_norm) == 0.0
    assert a_opt.step_count() == 1 and c_opt.step_count() == 1
    assert bool(torch.isfinite(a_opt.params).all()) and bool(torch.isfinite(c_opt.params).all())
    assert not bool(a_opt._grad_out.any()) and not bool(c_opt._grad_out.any())


def test_graph_replay():
    """tests/pg_graph_check.py in a process of its own, under its own time
    limit: each update captured once and replayed three times, against eager
    calls on twin networks."""
    done = subprocess.run([sys.executable, os.path.join(HERE, "pg_graph_check.py")], capture_output=True, text=True,
                          timeout=120)
    print(done.stdout[-2000:], done.stderr[-2000:])
    assert done.returncode == 0 and "graph replay ok" in done.stdout


# ---- end to end ----------------------------------------------------------------------------------

def test_collect_reinforce_then_update(nets, gpu_device):
    actor, _, opt, _ = make(nets, gpu_device, "f16x3")
    before = opt.params.clone()
    cfg = EnvConfig(randomize_drone=True, randomize_platform=True, seed=3)
    env = VecDroneEnv(64, device=gpu_device, config=cfg, reward_mode="reinforce", max_steps=45)
    batch = collect_reinforce(env, actor, max_steps=40, seed=9, step=2)
    assert isinstance(batch, ReinforceBatch) and batch.states.shape[0] > 64
    a = reinforce_losses(actor, batch, grads=True)
    b = reinforce_losses(actor, batch.states, batch.actions, batch.advantages, grads=True)
    assert all(same(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError, match="not both"):
        reinforce_losses(actor, batch, batch.actions)
    out = reinforce_update(actor, batch, opt)
    assert same(out.loss, a.loss) and out.baseline is batch.baseline and out.std is batch.std
    assert bool(torch.isfinite(out.loss)) and bool(torch.isfinite(out.grad_norm))
    assert bool(torch.isfinite(opt.params).all()) and not torch.equal(opt.params, before)
    assert opt.step_count() == 1 and opt.status() == 0
    with pytest.raises(ValueError, match="at least one row"):
        reinforce_losses(actor, batch.states[:0], batch.actions[:0], batch.advantages[:0])


def test_twenty_frames_of_the_td_loop(nets, gpu_device):
    actor, critic, a_opt, c_opt = make(nets, gpu_device, "f16x3")
    before = a_opt.params.clone(), c_opt.params.clone()
    cfg = EnvConfig(randomize_drone=True, randomize_platform=True, auto_reset=True, seed=5)
    env = VecDroneEnv(64, device=gpu_device, config=cfg, reward_mode="notebook", max_steps=12)
    obs = env.reset()
    done_prev = torch.zeros(64, dtype=torch.bool, device=gpu_device)
    masked = 0
    for t in range(20):
        state = obs.clone()
        actions, _ = actor.act(state, seed=11, step=t)
        obs, reward, done, _ = env.step(actions)
        out = actor_critic_update(actor, critic, state, actions, reward, obs, done, a_opt, c_opt,
                                  active=~done_prev)
        masked += int(done_prev.sum())
        assert not bool(out.td_errors[done_prev].any())
        done_prev = done.clone()
    assert masked > 0  # some re-spawn frames were masked out
    assert a_opt.step_count() == 20 and c_opt.step_count() == 20 and a_opt.status() == 0 and c_opt.status() == 0
    for opt, p0 in zip((a_opt, c_opt), before):
        assert bool(torch.isfinite(opt.params).all()) and not torch.equal(opt.params, p0)
    assert bool(torch.isfinite(out.actor_loss)) and bool(torch.isfinite(out.critic_loss))
