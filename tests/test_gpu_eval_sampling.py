"""GPU: dd_mlp_forward_sampled, the action selection of the notebooks'
evaluate_policy* cells (temperature == 0: probs > 0.5; else Bernoulli(q) with
q = p^(1/T) / (p^(1/T) + (1-p)^(1/T))) on the actor's MFMA kernels.

Rows N in {1, 31, 32, 33, 257}: the 32-column wave tile, its tails, more than
one block; both computes; the notebook actor of the golden fixture and a
freshly initialised one.

Accuracy of the tempered probabilities (test_tempered_probs_accuracy): the
reference is the notebook's pow formula in float64 on a float64 copy of the
model; the yardstick is the same formula in torch float32 on the float32
model, on the same rows:
    max|q_kernel - q_f64| <= 4 max|q_torch32 - q_f64| + 2^-22.
The factor 4 covers the head's v_exp / v_rcp approximations (a few ulps more
than torch, mlp_core.h actor_probs); 2^-22 is a few float32 ulps of a
probability <= 1.  The maxima measured on an MI355X are in DESIGN.md §3.2.
Log-probabilities: |d| <= 1e-5 (1 + |lp|), as test_gpu_policy.py."""
import numpy as np
import pytest
import torch
from torch import nn
from torch.distributions import Bernoulli

import golden_data as gd
from delivery_drone_amd import MlpNet

pytestmark = pytest.mark.gpu

ROWS = (1, 31, 32, 33, 257)
COMPUTE = ("f32", "f16x3")
KINDS = ("golden", "random")
TEMPERATURES = (0.1, 0.3, 0.5, 2.0)
CASES = [(n, c, k) for k in KINDS for c in COMPUTE for n in ROWS]
case = pytest.mark.parametrize("n,compute,kind", CASES)


def _random_sd(k):
    """A freshly initialised network with non-trivial LayerNorm parameters (as
    test_gpu_policy builds its own)."""
    layers = [nn.Linear(15, 128), nn.LayerNorm(128), nn.ReLU(), nn.Linear(128, 128), nn.LayerNorm(128), nn.ReLU(),
              nn.Linear(128, 64), nn.LayerNorm(64), nn.ReLU(), nn.Linear(64, k)]
    net = nn.Sequential(*layers)
    with torch.no_grad():
        for i in (1, 4, 7):
            net[i].weight.uniform_(0.5, 1.5)
            net[i].bias.uniform_(-0.2, 0.2)
    return net.state_dict()


@pytest.fixture(scope="module")
def world(gpu_device):
    """Per actor kind: the state_dict, 257 observation rows, the torch float32
    and float64 models' probabilities on them (computed once), and the MlpNet
    of each compute."""
    d, nets = gd.policy_fixture()
    torch.manual_seed(1234)
    rnd = {k: v.numpy() for k, v in _random_sd(3).items()}
    out = {}
    for kind, sd, obs in (("golden", nets["actor"], torch.as_tensor(d["obs"][:257])),
                          ("random", rnd, torch.randn(257, 15) * 2.0)):
        obs = obs.to(gpu_device, torch.float32).contiguous()
        m32 = gd.torch_mlp(sd, device=gpu_device)
        m64 = gd.torch_mlp(sd, device=gpu_device).double()
        with torch.no_grad():
            p32, p64 = m32(obs), m64(obs.double())
        out[kind] = dict(sd=sd, obs=obs, p32=p32, p64=p64,
                         nets={c: MlpNet(sd, device=gpu_device, compute=c) for c in COMPUTE})
    return out


def _pow_form(p, t):
    """The notebooks' adjusted_probs, in p's own precision."""
    a = torch.pow(p, 1.0 / t)
    return a / (a + torch.pow(1 - p, 1.0 / t))


def _bits(actions):
    return torch.stack([(actions >> j) & 1 for j in range(3)], dim=1)


def _close_lp(lp, want):
    err = (lp.double() - want.double()).abs()
    bound = 1e-5 * (1 + want.double().abs())
    assert bool((err <= bound).all()), f"max log-prob error {float(err.max()):.3g}"


def _uniforms(seed, env0, n, step):
    """actor_sample's u_k: Philox4x32-10 keyed by (seed; env, step, 0x5A5A5A5A), word k >> 8, times 2^-24."""
    e = np.arange(env0, env0 + n, dtype=np.uint64)
    r = gd.philox4x32_10_np(e & np.uint64(0xFFFFFFFF), e >> np.uint64(32),
                            np.full(n, step & 0xFFFFFFFF, np.uint32),
                            np.full(n, ((step >> 32) ^ 0x5A5A5A5A) & 0xFFFFFFFF, np.uint32),
                            np.full(n, seed & 0xFFFFFFFF, np.uint32), np.full(n, (seed >> 32) & 0xFFFFFFFF, np.uint32))
    return np.stack([(r[k] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24) for k in range(3)], axis=1)


@case
def test_temperature_one_is_the_old_entry_point(world, n, compute, kind):
    w = world[kind]
    net, obs = w["nets"][compute], w["obs"][:n]
    a0, lp0, p0 = net.act(obs, seed=7, step=3, env_id_base=11, probs=True)
    used = torch.full((n, 3), float("nan"), device=obs.device)
    a1, lp1, p1 = net.act(obs, seed=7, step=3, env_id_base=11, probs=True, temperature=1.0, probs_used_out=used)
    assert torch.equal(a0, a1) and torch.equal(lp0, lp1) and torch.equal(p0, p1)
    assert torch.equal(used, p1)


@case
def test_greedy(world, n, compute, kind):
    w = world[kind]
    net, obs = w["nets"][compute], w["obs"][:n]
    used = torch.full((n, 3), float("nan"), device=obs.device)
    a, lp, p = net.act(obs, seed=1, step=5, probs=True, temperature=0, probs_used_out=used)
    on = (p > 0.5).to(torch.uint8)
    assert torch.equal(a, on[:, 0] | (on[:, 1] << 1) | (on[:, 2] << 2))
    assert torch.equal(used, p) and torch.equal(p, net(obs))
    a2, lp2 = net.act(obs, seed=2 ** 40 + 9, step=77, temperature=0)  # nothing is drawn
    assert torch.equal(a, a2) and torch.equal(lp, lp2)
    _close_lp(lp, Bernoulli(probs=p).log_prob(_bits(a).float()).sum(1))


@case
def test_tempered_probs_accuracy(world, n, compute, kind):
    w = world[kind]
    net, obs = w["nets"][compute], w["obs"][:n]
    for t in TEMPERATURES:
        used = torch.full((n, 3), float("nan"), device=obs.device)
        net.act(obs, seed=1, step=0, temperature=t, probs_used_out=used)
        q64 = _pow_form(w["p64"][:n], t)
        q32 = _pow_form(w["p32"][:n], t)
        e_kernel = float((used.double() - q64).abs().max())
        e_torch = float((q32.double() - q64).abs().max())
        print(f"tempered kind={kind} compute={compute} n={n} T={t}: kernel {e_kernel:.3e} torch32 {e_torch:.3e}")
        assert e_kernel <= 4 * e_torch + 2.0 ** -22, (t, e_kernel, e_torch)


@case
def test_tempered_draw_and_log_prob(world, n, compute, kind):
    w = world[kind]
    net, obs = w["nets"][compute], w["obs"][:n]
    seed, step, env0 = 2 ** 33 + 5, 2 ** 32 + 41, 2 ** 32 - 7  # every 64-bit half of the keying in use
    for t in TEMPERATURES:
        used = torch.full((n, 3), float("nan"), device=obs.device)
        a, lp, p = net.act(obs, seed=seed, step=step, env_id_base=env0, probs=True, temperature=t,
                           probs_used_out=used)
        assert torch.equal(p, net(obs))  # probs stays the network's own
        u = _uniforms(seed, env0, n, step)
        want = (u < used.cpu().numpy()).astype(np.uint8)
        assert np.array_equal(_bits(a).cpu().numpy(), want), t
        _close_lp(lp, Bernoulli(probs=used).log_prob(_bits(a).float()).sum(1))


@pytest.mark.parametrize("compute", COMPUTE)
@pytest.mark.parametrize("kind", KINDS)
def test_tempered_action_rates(world, compute, kind, gpu_device):
    """16,384 lanes at T = 0.3: per thruster, the action rate is within 5
    binomial standard deviations of mean(probs_used)."""
    n = 16_384
    w = world[kind]
    net = w["nets"][compute]
    obs = w["obs"].repeat((n + 256) // 257, 1)[:n].contiguous()  # each row draws with its own env id
    used = torch.empty(n, 3, device=gpu_device)
    a, _ = net.act(obs, seed=21, step=4, temperature=0.3, probs_used_out=used)
    q = used.double()
    hits = _bits(a).double().sum(0)
    sd = (q * (1 - q)).sum(0).sqrt()
    dev = (hits - q.sum(0)).abs()
    assert bool((dev <= 5.0 * sd).all()), (hits.tolist(), q.sum(0).tolist(), sd.tolist())


def test_errors(world, gpu_device):
    w = world["golden"]
    net, obs = w["nets"]["f32"], w["obs"][:4]
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            net.act(obs, temperature=bad)
    with pytest.raises(ValueError):
        net.act(obs, temperature=0.3, probs_used_out=torch.empty(4, 2, device=gpu_device))
    _, nets = gd.policy_fixture()
    critic = MlpNet(nets["critic"], device=gpu_device)
    for t in (0, 0.3):
        with pytest.raises(ValueError):
            critic.act(obs, temperature=t)
