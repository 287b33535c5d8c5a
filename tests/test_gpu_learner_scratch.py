"""GPU: who owns the learners' scratch, and that ppo_update's two paths refuse
the same calls.

AdamW owns its flat gradient buffer (``grad_buffer()``, ``_grad_out``) and, on
the actor's optimizer, the fused update's workspace (``_fused_ws``); every
update function that steps an optimizer goes through that one buffer.  Small
random networks, five rows; 130 rows only where two minibatches of 128 (the
row tile and a 2-row tail) are wanted.  Every refusal here is raised on the
host before a launch; the expected words are those of
tests/test_learner_args_cpu.py, literals again.
"""
import pytest
import torch

from delivery_drone_amd import AdamW, MlpNet, actor_critic_update, ppo_update, reinforce_update
from delivery_drone_amd.policy import _SHAPES
from delivery_drone_amd.train_batch import PpoBatch, ReinforceBatch

pytestmark = pytest.mark.gpu

NAN = float("nan")
FIVE = "(states, actions, old_log_probs, advantages, returns)"


def random_net(k, dev, seed, compute="f32"):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in dict(_SHAPES, **{"9.weight": (k, 64), "9.bias": (k,)}).items():
        layer_norm_weight = name in ("1.weight", "4.weight", "7.weight")
        sd[name] = 1.0 + 0.1 * torch.randn(shape, generator=g) if layer_norm_weight else \
            0.1 * torch.randn(shape, generator=g)
    return MlpNet(sd, device=dev, compute=compute)


def learners(dev, compute="f32"):
    actor, critic = random_net(3, dev, 1, compute), random_net(1, dev, 2, compute)
    return actor, critic, AdamW(actor, lr=3e-4), AdamW(critic, lr=1e-3)


def five(m, dev, seed=3):
    g = torch.Generator().manual_seed(seed)
    cols = (torch.randn(m, 15, generator=g), (torch.rand(m, 3, generator=g) < 0.5).float(),
            -2.0 + 0.1 * torch.randn(m, generator=g), torch.randn(m, generator=g), torch.randn(m, generator=g))
    return tuple(t.to(dev) for t in cols)


def reinforce_batch(m, dev):
    states, actions, _, advantages, returns = five(m, dev)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    return ReinforceBatch(states, actions, returns, advantages, zero, zero + 1.0, None, None, None, None)


def test_one_gradient_buffer_per_optimizer(gpu_device):
    actor, critic, a_opt, c_opt = learners(gpu_device)
    assert a_opt._grad_out is None and c_opt._grad_out is None and a_opt._fused_ws is None
    assert actor._backward_ws is None and actor._flat is not None  # AdamW took flat_parameters()
    buf = a_opt.grad_buffer()
    assert buf is a_opt._grad_out and a_opt.grad_buffer() is buf and a_opt.grad_buffer().data_ptr() == buf.data_ptr()
    assert buf.shape == a_opt.params.shape and buf.dtype == torch.float32 and buf.data_ptr() != a_opt.params.data_ptr()
    assert c_opt._grad_out is None
    batch = five(5, gpu_device)
    reinforce_update(actor, reinforce_batch(5, gpu_device), a_opt)
    assert a_opt._grad_out.data_ptr() == buf.data_ptr() and bool(a_opt._grad_out.any())
    ppo_update(actor, critic, batch, a_opt, c_opt, num_epochs=1)
    assert a_opt._grad_out.data_ptr() == buf.data_ptr()
    critic_buf = c_opt._grad_out.data_ptr()
    assert c_opt.grad_buffer().data_ptr() == critic_buf
    states, actions = batch[:2]
    actor_critic_update(actor, critic, states, actions, batch[3], states.flip(0), torch.zeros(5, device=gpu_device),
                        a_opt, c_opt)
    assert a_opt._grad_out.data_ptr() == buf.data_ptr() and c_opt._grad_out.data_ptr() == critic_buf
    assert actor._backward_ws is not None and a_opt._fused_ws is None and c_opt._fused_ws is None


def test_fused_and_looped_updates_share_the_buffers(gpu_device):
    actor, critic, a_opt, c_opt = learners(gpu_device)
    batch = five(130, gpu_device)
    kw = dict(num_epochs=1, minibatch_size=128)
    first = ppo_update(actor, critic, batch, a_opt, c_opt, fused=True, **kw)
    assert tuple(first.logs["total_loss"].shape) == (1, 2)
    grads = a_opt._grad_out.data_ptr(), c_opt._grad_out.data_ptr()
    workspace = a_opt._fused_ws
    assert workspace is not None and c_opt._fused_ws is None
    assert workspace.numel() * 8 == int(actor._lib.dd_ppo_update_fused_workspace())
    ppo_update(actor, critic, batch, a_opt, c_opt, fused=False, shuffle_epoch=1, **kw)
    assert (a_opt._grad_out.data_ptr(), c_opt._grad_out.data_ptr()) == grads and a_opt._fused_ws is workspace
    ppo_update(actor, critic, batch, a_opt, c_opt, fused=True, shuffle_epoch=2, **kw)
    assert (a_opt._grad_out.data_ptr(), c_opt._grad_out.data_ptr()) == grads and a_opt._fused_ws is workspace
    assert a_opt.step_count() == 6 and c_opt.step_count() == 6 and a_opt.status() == 0 and c_opt.status() == 0


# the shared rows of the CPU table, on real networks: (what to change, the message, {who} by path)
REFUSALS = {
    "num_epochs 0": (dict(num_epochs=0), "num_epochs must be at least 1, got 0"),
    "minibatch_size 0": (dict(minibatch_size=0), "minibatch_size must be at least 1, got 0"),
    "no minibatch": (dict(minibatch_size=64, drop_last=True),
                     "no minibatch to step on: 5 rows, minibatch_size 64, drop_last=True"),
    "not a batch": (dict(batch=object()), "batch must be a PpoBatch, a PpoEpisodesBatch or the five tensors"),
    "four tensors": (dict(batch=slice(0, 4)), "{who} all five tensors " + FIVE),
    "batch without log_prob": (dict(batch="without log_prob"), "{who} all five tensors " + FIVE),
    "clip_epsilon NaN": (dict(clip_epsilon=NAN), "clip_epsilon must be finite, got nan"),
    "entropy_coef inf": (dict(entropy_coef=float("inf")), "entropy_coef must be finite, got inf"),
    "value_coef NaN": (dict(value_coef=NAN), "value_coef must be finite, got nan"),
    "clip_epsilon negative": (dict(clip_epsilon=-1e-3), "clip_epsilon must not be negative, got -0.001"),
    "max_grad_norm NaN": (dict(max_grad_norm=NAN), "max_norm must not be NaN"),
    "out_dim swapped": (dict(swap=True), "ppo_losses needs an MlpNet actor (out_dim 3) and an MlpNet critic "
                                         "(out_dim 1)"),
    "bad minibatch_size and coefficient": (dict(minibatch_size=-3, value_coef=NAN),
                                           "minibatch_size must be at least 1, got -3"),
}


@pytest.fixture(scope="module")
def refusing(gpu_device):
    return learners(gpu_device), five(5, gpu_device)


@pytest.mark.parametrize("case", list(REFUSALS))
def test_both_paths_refuse_the_same_calls(refusing, case):
    (actor, critic, a_opt, c_opt), batch = refusing
    change, message = REFUSALS[case]
    kw = dict(dict(num_epochs=1, minibatch_size=4), **change)
    what = kw.pop("batch", batch)
    if isinstance(what, slice):
        what = batch[what]
    elif what == "without log_prob":
        what = PpoBatch(*batch[:2], None, *batch[3:], *[batch[4]] * 7)
    nets = (critic, actor, what, c_opt, a_opt) if kw.pop("swap", False) else (actor, critic, what, a_opt, c_opt)
    before = [t.clone() for t in (actor.flat_parameters(), critic.flat_parameters())]
    for fused in (True, False):
        with pytest.raises(ValueError) as e:
            ppo_update(*nets, fused=fused, **kw)
        assert str(e.value) == message.format(who="fused=True needs" if fused else "minibatches need"), fused
    assert a_opt.step_count() == 0 and c_opt.step_count() == 0
    assert all(torch.equal(a, b) for a, b in zip(before, (actor.flat_parameters(), critic.flat_parameters())))
