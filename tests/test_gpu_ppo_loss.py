"""GPU: dd_mlp_evaluate_actions, dd_ppo_losses and MlpNet.load_state_dict.

Two layers for the losses.  Exactness: the kernel against the float64
restatement (tests/ppo_loss_ref.py) fed the kernel's OWN per-row log_prob,
entropy, probs and values: scalars within 1e-9 relative (sums in double over at
most 2^18 terms), gradients within 4 float32 ulps, ratio_min / ratio_max
bit-equal, clipped_frac equal.  Parity with the notebook
(tests/golden/ppo_loss/losses.npz: compute_ppo_losses' own scalars and
autograd's gradients): clipped_frac and the gradient's zero pattern exactly (the
fixture keeps every row clear of the clip's edges), every other figure within
a bound computed here on the CPU from the fixture alone:
    2 x (first-order spread of the restatement when each per-row input moves
         within its accepted bound: log_prob 1e-5 (1 + |lp|), probabilities
         2e-6, values VALUE_TOL, as tests/test_gpu_policy.py)   [x 2: curvature]
    + the reference's own float32 gap (ppo_loss_ref.reference_gap).
No kernel output enters a bound.  On the fixture the bounds come to (f32 /
f16x3 where they differ): total_loss 0.206 / 0.818 (of 25,338), policy_loss
1.86e-5, value_loss 0.411 / 1.64 (of 50,675), entropy 1.22e-5, ratio_mean
3.85e-5, ratio_min 1.46e-5, ratio_max 6.51e-5, ratio_std 3.31e-5; grad_logits at
most 6.52e-7 per element (of 9.9e-3), grad_values at most 1.75e-5 / 6.99e-5 (of
4.6).
"""
import ctypes

import numpy as np
import pytest
import torch

import golden_data as gd
import ppo_loss_ref as ref
from delivery_drone_amd import MlpNet, VecDroneEnv, abi, collect_ppo, ppo_losses
from delivery_drone_amd.config import EnvConfig

pytestmark = pytest.mark.gpu

COMPUTE = ("f32", "f16x3")
VALUE_TOL = {"f32": (2e-6, 1e-4), "f16x3": (8e-6, 4e-4)}  # (relative, absolute): tests/test_gpu_policy.py's
PROB_TOL = 2e-6
M = 203


def lp_tol(lp):
    return 1e-5 * (1.0 + np.abs(np.asarray(lp, np.float64)))


@pytest.fixture(scope="module")
def g():
    return gd.npz("ppo_loss/losses.npz")


@pytest.fixture(scope="module")
def nets():
    return gd.policy_fixture()[1]


@pytest.fixture(scope="module")
def reference(g):
    """Computed once on the CPU, shared and left unchanged: the restatement on
    the notebook's rows, the notebook's row log_prob / entropy in float64, the
    reference's float32 gap."""
    lp, ent = ref.row_log_prob_entropy(g["probs"], g["actions"])
    return dict(out=ref.fixture_losses(g), lp=lp, ent=ent, gap=ref.reference_gap(g))


def dev_inputs(g, dev, reps=None):
    """The fixture's five tensors on the device, tiled to `reps` rows."""
    keys = ("states", "actions", "old_log_probs", "advantages", "returns")
    arrs = [g[k] if reps is None else np.resize(g[k], (reps,) + g[k].shape[1:]) for k in keys]
    return [torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in arrs]


def host(t):
    return t.detach().cpu().numpy()


def check_exact(out, old, adv, ret, actions, **coef):
    """The exactness layer: the kernel against the restatement fed its own rows."""
    want = ref.losses(host(out.new_log_probs), host(out.row_entropy), host(out.probs), host(out.values), host(old),
                      host(adv), host(ret), host(actions), **coef)
    got = dict(total_loss=out.total_loss, policy_loss=out.policy_loss, value_loss=out.value_loss,
               entropy=out.entropy, ratio_mean=out.ratio_stats["mean"], ratio_min=out.ratio_stats["min"],
               ratio_max=out.ratio_stats["max"], ratio_std=out.ratio_stats["std"],
               clipped_frac=out.ratio_stats["clipped_frac"])
    got = {k: float(v) for k, v in got.items()}
    for k in ref.SCALARS:
        print(f"exact {k}: got {got[k]!r} want {want[k]!r}")
    for k in ref.SCALARS:
        if np.isnan(want[k]):
            assert np.isnan(got[k]), k
        elif k in ("ratio_min", "ratio_max", "clipped_frac"):
            assert got[k] == want[k], k
        else:
            assert abs(got[k] - want[k]) <= 1e-9 * abs(want[k]), k
    ratio = host(out.ratio)
    assert np.all(np.abs(ratio.astype(np.float64) - want["ratio"]) <= gd.ulp32(want["ratio"]))
    assert float(ratio.min()) == got["ratio_min"] and float(ratio.max()) == got["ratio_max"]
    if out.grad_logits is not None:
        gl, gv = host(out.grad_logits), host(out.grad_values)
        for name, a, b in (("grad_logits", gl, want["grad_logits"]), ("grad_values", gv, want["grad_values"])):
            ulps = np.abs(a.astype(np.float64) - b) / gd.ulp32(b)
            print(f"exact {name}: max {np.nanmax(ulps):.3g} ulps")
            assert np.all(gd.f32_close(a, b, ulps=4.0)), name
        assert np.array_equal(gl == 0, want["grad_logits"] == 0)
    return want, got


# ---- evaluate_actions ----------------------------------------------------------

@pytest.mark.parametrize("compute", COMPUTE)
@pytest.mark.parametrize("n", [1, 31, 32, 33, M])
def test_evaluate_actions(g, nets, reference, gpu_device, compute, n):
    actor = MlpNet(nets["actor"], device=gpu_device, compute=compute)
    obs = torch.as_tensor(g["states"][:n], device=gpu_device)
    # act()'s own actions: the same bits, in both formats
    a, lp_act, p_act = actor.act(obs, seed=7, step=3, probs=True)
    lp, ent, p = actor.evaluate_actions(obs, a, probs=True)
    assert lp.shape == (n,) and ent.shape == (n,) and p.shape == (n, 3)
    assert torch.equal(lp, lp_act) and torch.equal(p, p_act)
    af = torch.stack([(a >> j) & 1 for j in range(3)], dim=1).float()
    lp2, ent2 = actor.evaluate_actions(obs, af)
    assert torch.equal(lp2, lp_act) and torch.equal(ent2, ent)
    lp3, _ = actor.evaluate_actions(obs, af * -2.5)  # any nonzero float is "on", as dd_step reads the format
    assert torch.equal(lp3, lp_act)
    lp_out, ent_out = torch.empty_like(lp), torch.empty_like(ent)
    r = actor.evaluate_actions(obs, a, log_prob_out=lp_out, entropy_out=ent_out)
    assert r[0] is lp_out and r[1] is ent_out and torch.equal(lp_out, lp) and torch.equal(ent_out, ent)
    # the fixture's actions against the notebook's rows
    acts = torch.as_tensor(g["actions"][:n], device=gpu_device)
    lp, ent, p = (host(t).astype(np.float64) for t in actor.evaluate_actions(obs, acts, probs=True))
    nb_lp = g["new_log_probs"][:n].astype(np.float64)
    print("log_prob err", np.abs(lp - nb_lp).max(), "probs err", np.abs(p - g["probs"][:n]).max())
    assert np.all(np.abs(lp - nb_lp) <= lp_tol(nb_lp))
    assert np.all(np.abs(p - g["probs"][:n]) <= PROB_TOL)
    pc = np.clip(g["probs"][:n].astype(np.float64), ref.EPS32, 1 - ref.EPS32)
    ent_tol = (PROB_TOL * np.maximum(1.0, np.abs(np.log(pc) - np.log1p(-pc)))).sum(1)
    print("entropy err", np.abs(ent - reference["ent"][:n]).max(), "bound", ent_tol.min())
    assert np.all(np.abs(ent - reference["ent"][:n]) <= ent_tol)


@pytest.mark.parametrize("compute", COMPUTE)
def test_evaluate_actions_on_an_unaligned_view(nets, gpu_device, compute):
    """515 rows starting at row 1 of a larger tensor (60 bytes in: not 16-byte
    aligned), as the f16x3 prologue's unaligned loads must take them."""
    d, _ = gd.policy_fixture()
    actor = MlpNet(nets["actor"], device=gpu_device, compute=compute)
    big = torch.as_tensor(d["obs"], device=gpu_device)
    view = big[1:516]
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    aligned = view.clone()
    a, lp_act = actor.act(aligned, seed=1, step=2)
    got = actor.evaluate_actions(view, a, probs=True)
    want = actor.evaluate_actions(aligned, a, probs=True)
    assert all(torch.equal(x, y) for x, y in zip(got, want)) and torch.equal(got[0], lp_act)
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())


def test_buffer_packed_for_the_other_compute_gives_nan(g, nets, gpu_device):
    lib = abi.lib()
    obs = torch.as_tensor(g["states"], device=gpu_device)
    acts = torch.as_tensor(g["actions"], device=gpu_device)
    for compute, other in (("f32", abi.DD_MLP_F16X3), ("f16x3", abi.DD_MLP_F32)):
        actor = MlpNet(nets["actor"], device=gpu_device, compute=compute)
        lp, ent = torch.zeros(M, device=gpu_device), torch.zeros(M, device=gpu_device)
        io = abi.DDMlpEvalIO(obs.data_ptr(), acts.data_ptr(), abi.DD_ACT_F32X3, 0, None, lp.data_ptr(),
                             ent.data_ptr(), M)
        abi.check(lib.dd_mlp_evaluate_actions(actor.packed.data_ptr(), other, ctypes.byref(io), None), "eval")
        torch.cuda.synchronize()
        assert bool(torch.isnan(lp).all()) and bool(torch.isnan(ent).all())
        critic = MlpNet(nets["critic"], device=gpu_device, compute=compute)  # a critic's buffer: K = 1
        abi.check(lib.dd_mlp_evaluate_actions(critic.packed.data_ptr(), critic._mode, ctypes.byref(io), None), "eval")
        torch.cuda.synchronize()
        assert bool(torch.isnan(lp).all()) and bool(torch.isnan(ent).all())


# ---- ppo_losses on the fixture ---------------------------------------------------

def parity_bounds(g, reference, compute):
    """2 x the restatement's first-order spread under the accepted per-row
    bounds + the reference's float32 gap.  From the fixture alone."""
    rel, abs_ = VALUE_TOL[compute]
    v = g["values"].astype(np.float64)
    s = ref.spread(g["new_log_probs"], reference["ent"].astype(np.float32), g["probs"], g["values"],
                   g["old_log_probs"], g["advantages"], g["returns"], g["actions"], d_lp=lp_tol(g["new_log_probs"]),
                   d_p=PROB_TOL, d_v=abs_ + rel * np.abs(v), clip_epsilon=float(g["clip_epsilon"]),
                   entropy_coef=float(g["entropy_coef"]), value_coef=float(g["value_coef"]))
    return {k: 2.0 * s[k] + reference["gap"][k] for k in s}


@pytest.mark.parametrize("compute", COMPUTE)
def test_ppo_losses_on_the_fixture(g, nets, reference, gpu_device, compute):
    actor = MlpNet(nets["actor"], device=gpu_device, compute=compute)
    critic = MlpNet(nets["critic"], device=gpu_device, compute=compute)
    states, actions, old, adv, ret = dev_inputs(g, gpu_device)
    coef = dict(clip_epsilon=float(g["clip_epsilon"]), entropy_coef=float(g["entropy_coef"]),
                value_coef=float(g["value_coef"]))
    out = ppo_losses(actor, critic, states, actions, old, adv, ret, grads=True, **coef)
    for t in (out.total_loss, out.policy_loss, out.value_loss, out.entropy, *out.ratio_stats.values()):
        assert t.dim() == 0 and t.dtype == torch.float64 and t.device == gpu_device
    assert set(out.ratio_stats) == {"mean", "min", "max", "std", "clipped_frac"}
    none = ppo_losses(actor, critic, states, actions, old, adv, ret, **coef)
    assert none.grad_logits is None and none.grad_values is None and torch.equal(none.total_loss, out.total_loss)
    # bitmask actions: the same bits
    bits = (actions.to(torch.uint8) * torch.tensor([1, 2, 4], dtype=torch.uint8, device=gpu_device)).sum(1)
    masked = ppo_losses(actor, critic, states, bits.to(torch.uint8), old, adv, ret, grads=True, **coef)
    assert torch.equal(masked.grad_logits, out.grad_logits) and torch.equal(masked.total_loss, out.total_loss)

    want, got = check_exact(out, old, adv, ret, actions, **coef)

    # parity with the notebook
    bound = parity_bounds(g, reference, compute)
    for k in ref.SCALARS:
        print(f"parity {k}: got {got[k]!r} notebook {float(g[k])!r} err {abs(got[k] - float(g[k])):.3g} "
              f"bound {bound[k]:.3g}")
    count = int(round(float(g["clipped_frac"]) * M))
    assert got["clipped_frac"] == count / M
    for k in ref.SCALARS:
        if k != "clipped_frac":
            assert abs(got[k] - float(g[k])) <= bound[k], k
    gl, gv = host(out.grad_logits).astype(np.float64), host(out.grad_values).astype(np.float64)
    err_l, err_v = np.abs(gl - g["grad_logits"]), np.abs(gv - g["grad_values"])
    print(f"parity grad_logits: max err {err_l.max():.3g} (bound there {bound['grad_logits'].flat[err_l.argmax()]:.3g},"
          f" largest bound {bound['grad_logits'].max():.3g}); grad_values: max err {err_v.max():.3g} "
          f"(largest bound {bound['grad_values'].max():.3g})")
    assert np.all(err_l <= bound["grad_logits"]) and np.all(err_v <= bound["grad_values"])
    # the gradient's zero pattern, exactly: without the entropy bonus the rows the clip cuts off are zeros
    bare = ppo_losses(actor, critic, states, actions, old, adv, ret, grads=True, **{**coef, "entropy_coef": 0.0})
    assert np.array_equal(host(bare.grad_logits) == 0, g["grad_logits_no_entropy"] == 0)
    assert float(bare.total_loss) == float(bare.policy_loss) + coef["value_coef"] * float(bare.value_loss)
    check_exact(bare, old, adv, ret, actions, **{**coef, "entropy_coef": 0.0})


# ---- the reduction -----------------------------------------------------------------

@pytest.mark.parametrize("compute", COMPUTE)
def test_reduction_over_more_than_one_grid_trip(g, nets, gpu_device, compute):
    """131,072 + 33 rows: one full trip of the 512 x 256 grid-stride loop and a
    ragged second one.  Exactness only; two runs give identical bits."""
    m = 512 * 256 + 33
    actor = MlpNet(nets["actor"], device=gpu_device, compute=compute)
    critic = MlpNet(nets["critic"], device=gpu_device, compute=compute)
    states, actions, old, adv, ret = dev_inputs(g, gpu_device, reps=m)
    a = ppo_losses(actor, critic, states, actions, old, adv, ret, grads=True)
    b = ppo_losses(actor, critic, states, actions, old, adv, ret, grads=True)
    for x, y in zip(a, b):
        if isinstance(x, dict):
            assert all(torch.equal(x[k], y[k]) for k in x)
        else:
            assert torch.equal(x, y)
    check_exact(a, old, adv, ret, actions)


def test_edge_cases(g, nets, gpu_device):
    actor = MlpNet(nets["actor"], device=gpu_device)
    critic = MlpNet(nets["critic"], device=gpu_device)
    states, actions, old, adv, ret = dev_inputs(g, gpu_device)
    # m == 1: the unbiased std has no value
    one = ppo_losses(actor, critic, states[:1], actions[:1], old[:1], adv[:1], ret[:1], grads=True)
    assert bool(torch.isnan(one.ratio_stats["std"])) and bool(torch.isfinite(one.total_loss))
    assert float(one.ratio_stats["min"]) == float(one.ratio_stats["max"]) == float(one.ratio_stats["mean"])
    check_exact(one, old[:1], adv[:1], ret[:1], actions[:1])
    # every ratio 1: nothing clipped, policy_loss = -mean(A)
    own = ppo_losses(actor, critic, states, actions, old, adv, ret).new_log_probs
    same = ppo_losses(actor, critic, states, actions, own, adv, ret, grads=True)
    assert float(same.ratio_stats["clipped_frac"]) == 0.0 and float(same.ratio_stats["std"]) == 0.0
    assert float(same.ratio_stats["min"]) == float(same.ratio_stats["max"]) == float(same.ratio_stats["mean"]) == 1.0
    mean_a = g["advantages"].astype(np.float64).sum() / M
    assert abs(float(same.policy_loss) + mean_a) <= 1e-9 * abs(mean_a)
    check_exact(same, own, adv, ret, actions)
    # entropy_coef == 0
    bare = ppo_losses(actor, critic, states, actions, old, adv, ret, entropy_coef=0.0, grads=True)
    assert float(bare.total_loss) == float(bare.policy_loss) + 0.5 * float(bare.value_loss)
    cut = host(bare.grad_logits) == 0
    assert cut.any() and np.array_equal(cut, g["grad_logits_no_entropy"] == 0)
    with pytest.raises(ValueError, match="at least one row"):
        ppo_losses(actor, critic, states[:0], actions[:0], old[:0], adv[:0], ret[:0])
    with pytest.raises(ValueError, match="clip_epsilon"):
        ppo_losses(actor, critic, states, actions, old, adv, ret, clip_epsilon=-0.1)


def test_ppo_losses_accepts_a_batch(nets, gpu_device):
    actor = MlpNet(nets["actor"], device=gpu_device, compute="f16x3")
    critic = MlpNet(nets["critic"], device=gpu_device, compute="f16x3")
    cfg = EnvConfig(randomize_drone=True, randomize_platform=True, seed=3)
    env = VecDroneEnv(64, device=gpu_device, config=cfg, reward_mode="notebook", max_steps=45)
    batch = collect_ppo(env, actor, critic, max_steps=40, seed=9, step=2)
    assert batch.states.shape[0] > 64
    a = ppo_losses(actor, critic, batch, grads=True)
    b = ppo_losses(actor, critic, batch.states, batch.actions, batch.old_log_probs, batch.advantages, batch.returns,
                   grads=True)
    for x, y in zip(a, b):
        if isinstance(x, dict):
            assert all(torch.equal(x[k], y[k]) for k in x)
        else:
            assert torch.equal(x, y)
    # the batch's old log-probs are this actor's own: every ratio is 1
    assert float(a.ratio_stats["clipped_frac"]) == 0.0
    assert float(a.ratio_stats["min"]) == float(a.ratio_stats["max"]) == 1.0
    assert torch.equal(a.new_log_probs, batch.old_log_probs) and torch.equal(a.values, batch.values)
    with pytest.raises(ValueError, match="not both"):
        ppo_losses(actor, critic, batch, batch.actions)


# ---- load_state_dict -----------------------------------------------------------------

def _random_sd(k, seed):
    from torch import nn
    torch.manual_seed(seed)
    net = nn.Sequential(nn.Linear(15, 128), nn.LayerNorm(128), nn.ReLU(), nn.Linear(128, 128), nn.LayerNorm(128),
                        nn.ReLU(), nn.Linear(128, 64), nn.LayerNorm(64), nn.ReLU(), nn.Linear(64, k))
    with torch.no_grad():
        for i in (1, 4, 7):
            net[i].weight.uniform_(0.5, 1.5)
            net[i].bias.uniform_(-0.2, 0.2)
    return net.state_dict()


@pytest.mark.parametrize("compute", COMPUTE)
def test_load_state_dict(g, nets, gpu_device, compute):
    obs = torch.as_tensor(g["states"], device=gpu_device)
    actor = MlpNet(nets["actor"], device=gpu_device, compute=compute)
    critic = MlpNet(nets["critic"], device=gpu_device, compute=compute)
    ptr_a, ptr_c = actor.packed.data_ptr(), critic.packed.data_ptr()
    before = actor(obs).clone()
    sd_a, sd_c = _random_sd(3, 1), _random_sd(1, 2)
    assert actor.load_state_dict(sd_a) is actor
    critic.load_state_dict({"network." + k: v for k, v in sd_c.items()})
    fresh_a = MlpNet(sd_a, device=gpu_device, compute=compute)
    fresh_c = MlpNet(sd_c, device=gpu_device, compute=compute)
    assert actor.packed.data_ptr() == ptr_a and critic.packed.data_ptr() == ptr_c
    assert torch.equal(actor(obs), fresh_a(obs)) and torch.equal(critic(obs), fresh_c(obs))
    assert not torch.equal(actor(obs), before)
    x, y = actor.act(obs, seed=4, step=1), fresh_a.act(obs, seed=4, step=1)
    assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    # back to the notebook's weights, and critic-shaped weights into the same buffer
    actor.load_state_dict(nets["actor"])
    assert torch.equal(actor(obs), before)
    actor.load_state_dict(nets["critic"])
    assert actor.out_dim == 1 and actor.packed.data_ptr() == ptr_a
    assert torch.equal(actor(obs), MlpNet(nets["critic"], device=gpu_device, compute=compute)(obs))
    actor.load_state_dict(nets["actor"])
    # a refused state_dict leaves the old parameters in place
    bad = dict(nets["actor"])
    bad["3.weight"] = bad["3.weight"][:, :64]
    with pytest.raises(ValueError):
        actor.load_state_dict(bad)
    missing = {k: v for k, v in nets["actor"].items() if k != "7.bias"}
    with pytest.raises(KeyError):
        actor.load_state_dict(missing)
    if compute == "f16x3":
        big = {k: np.array(v, copy=True) for k, v in nets["actor"].items()}
        big["3.weight"].flat[0] = 3000.0
        with pytest.raises(ValueError, match="f16x3"):
            actor.load_state_dict(big)
    assert actor.out_dim == 3 and actor.packed.data_ptr() == ptr_a and torch.equal(actor(obs), before)
