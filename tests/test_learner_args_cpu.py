"""No GPU: the learner wrappers' argument layer (delivery_drone_amd/_args.py)
and the plan ppo_update makes of a call (adamw._plan).

Every expected message below is a literal, written out from the wrappers as
they were before the checks were gathered in one module: what is refused, the
exception type and the words must not move.  The helpers take CPU tensors with
``dev = torch.device("cpu")`` (a tensor on the ``meta`` device stands for "on
another device"), and the plan takes stand-in networks, since its checks read
``out_dim``, ``device`` and ``compute`` only.  Nothing here launches.
"""
import ast
import os
import types

import pytest
import torch

import delivery_drone_amd
from delivery_drone_amd import _args, abi, adamw, ppo_losses, ppo_update
from delivery_drone_amd.train_batch import PpoBatch, ReinforceBatch

CPU, META = torch.device("cpu"), torch.device("meta")
NAN, INF = float("nan"), float("inf")
FIVE = "(states, actions, old_log_probs, advantages, returns)"
NEEDS_NETS = "ppo_losses needs an MlpNet actor (out_dim 3) and an MlpNet critic (out_dim 1)"
NO_ROWS = "ppo_losses needs at least one row: a mean over no rows has no value"


def net(out_dim, device=CPU, compute="f32"):
    return types.SimpleNamespace(out_dim=out_dim, device=device, compute=compute)


ACTOR, CRITIC = net(3), net(1)


def five(m, actions="f32x3"):
    acts = torch.zeros(m, dtype=torch.uint8) if actions == "bitmask" else torch.zeros(m, 3)
    return (torch.zeros(m, abi.DD_OBS_DIM), acts, torch.zeros(m), torch.zeros(m), torch.zeros(m))


def ppo_batch(m, **replace):
    cols = dict(zip(PpoBatch._fields, five(m) + (torch.zeros(m),) * 7))
    cols.update(replace)
    return PpoBatch(**cols)


def reinforce_batch(m, **replace):
    s, a = five(m)[:2]
    cols = dict(zip(ReinforceBatch._fields, (s, a) + (torch.zeros(m),) * 8))
    cols.update(replace)
    return ReinforceBatch(**cols)


def plan(batch, actor=ACTOR, critic=CRITIC, *, fused, num_epochs=2, minibatch_size=None, drop_last=False,
         clip_epsilon=0.2, entropy_coef=0.01, value_coef=0.5, max_grad_norm=0.5):
    batch = tuple(batch) if isinstance(batch, (tuple, list)) and not hasattr(batch, "_fields") else (batch,)
    return adamw._plan(actor, critic, batch, fused=fused, num_epochs=num_epochs, minibatch_size=minibatch_size,
                       drop_last=drop_last, clip_epsilon=clip_epsilon, entropy_coef=entropy_coef,
                       value_coef=value_coef, max_grad_norm=max_grad_norm)


def update(batch, actor=ACTOR, critic=CRITIC, **kw):
    """ppo_update itself, with optimizers that are never reached."""
    return ppo_update(actor, critic, batch, types.SimpleNamespace(net=actor), types.SimpleNamespace(net=critic), **kw)


# ---- 1. one fault at a time ----------------------------------------------------------------

HELPER_FAULTS = {
    "rows: wrong count": (lambda: _args.row_tensor(torch.zeros(4), 5, CPU, "advantages"),
                          "advantages must be a tensor of shape (5,), got (4,)"),
    "rows: no tensor": (lambda: _args.row_tensor(None, 5, CPU, "returns"),
                        "returns must be a tensor of shape (5,), got NoneType"),
    "rows: device, 'states on'": (lambda: _args.row_tensor(torch.zeros(5, device=META), 5, CPU, "rewards"),
                                  "rewards is on meta, states on cpu"),
    "column: device, 'the batch on'": (lambda: _args.column("advantages", torch.zeros(5, device=META), 5, CPU),
                                       "advantages is on meta, the batch on cpu"),
    "column: no tensor": (lambda: _args.column("returns", [0.0] * 5, 5, CPU),
                          "returns must be a tensor or None, got list"),
    "column: wrong count": (lambda: _args.column("old_log_probs", torch.zeros(4), 5, CPU),
                            "old_log_probs must have shape (5,), got (4,)"),
    "column: states' width": (lambda: _args.column("states", torch.zeros(5, 14), 5, CPU),
                              "states must have shape (5, 15), got (5, 14)"),
    "column: wrong actions": (lambda: _args.column("actions", torch.zeros(5, dtype=torch.int64), 5, CPU),
                              "actions must be uint8 [5] bitmasks or float32 [5, 3], got torch.int64 (5,)"),
    "column: bitmasks as [M, 3]": (lambda: _args.column("actions", torch.zeros(5, 3, dtype=torch.uint8), 5, CPU),
                                   "actions must be uint8 [5] bitmasks or float32 [5, 3], got torch.uint8 (5, 3)"),
    "states: not 2-d": (lambda: _args.states_rows(torch.zeros(5), "ppo_losses"), "states must be [M, 15]"),
    "states: no tensor": (lambda: _args.states_rows(None, "td_losses"), "states must be [M, 15]"),
    "M == 0: ppo_losses": (lambda: _args.states_rows(torch.zeros(0, 15), "ppo_losses"), NO_ROWS),
    "M == 0: reinforce_losses": (lambda: _args.states_rows(torch.zeros(0, 15), "reinforce_losses"),
                                 "reinforce_losses needs at least one row: a mean over no rows has no value"),
    "M == 0: actor_critic_update": (lambda: _args.states_rows(torch.zeros(0, 15), "actor_critic_update"),
                                    "actor_critic_update needs at least one row: a mean over no rows has no value"),
    "M == 0: td_losses": (lambda: _args.states_rows(torch.zeros(0, 15), "td_losses"),
                          "td_losses needs at least one row: a mean over no rows has no value"),
    "active: shape": (lambda: _args.active_mask(torch.zeros(4, dtype=torch.bool), 5, CPU),
                      "active must be a bool or uint8 tensor of shape (5,)"),
    "active: dtype": (lambda: _args.active_mask(torch.zeros(5), 5, CPU),
                      "active must be a bool or uint8 tensor of shape (5,)"),
    "active: device": (lambda: _args.active_mask(torch.zeros(5, dtype=torch.bool, device=META), 5, CPU),
                       "active is on meta, states on cpu"),
    "clip_epsilon NaN": (lambda: _args.ppo_coefficients(NAN, 0.01, 0.5), "clip_epsilon must be finite, got nan"),
    "entropy_coef inf": (lambda: _args.ppo_coefficients(0.2, INF, 0.5), "entropy_coef must be finite, got inf"),
    "value_coef -inf": (lambda: _args.ppo_coefficients(0.2, 0.01, -INF), "value_coef must be finite, got -inf"),
    "clip_epsilon negative": (lambda: _args.ppo_coefficients(-0.1, 0.01, 0.5),
                              "clip_epsilon must not be negative, got -0.1"),
    "gamma NaN": (lambda: _args.finite("gamma", NAN), "gamma must be finite, got nan"),
    "value_reg inf": (lambda: _args.finite("value_reg", INF), "value_reg must be finite, got inf"),
    "max_norm NaN": (lambda: _args.clip_norm(NAN), "max_norm must not be NaN"),
    "out: shape": (lambda: _args.check_out(torch.zeros(4), (5,), torch.float32, CPU,
                                           "log_prob_out must be a contiguous float32 tensor"),
                   "log_prob_out must be a contiguous float32 tensor of shape (5,) on cpu"),
    "out: dtype": (lambda: _args.check_out(torch.zeros(5, 3, dtype=torch.float64), (5, 3), torch.float32, CPU,
                                           "probs_used_out must be a contiguous float32 tensor"),
                   "probs_used_out must be a contiguous float32 tensor of shape (5, 3) on cpu"),
    "out: strided": (lambda: _args.check_out(torch.zeros(10)[::2], (5,), torch.float32, CPU,
                                             "out must be a contiguous float32 tensor"),
                     "out must be a contiguous float32 tensor of shape (5,) on cpu"),
    "out: device": (lambda: _args.check_out(torch.zeros(5, dtype=torch.int32, device=META), (5,), torch.int32, CPU,
                                            "out.indices must be a contiguous int32 tensor"),
                    "out.indices must be a contiguous int32 tensor of shape (5,) on cpu"),
    "out: no tensor": (lambda: _args.check_out(None, (2, 15), torch.float32, CPU,
                                               "out obs must be a contiguous torch.float32 tensor"),
                       "out obs must be a contiguous torch.float32 tensor of shape (2, 15) on cpu"),
    "batch and tensors": (lambda: _args.ppo_columns(ppo_batch(5), None, None, torch.zeros(5)),
                          "pass a batch or the five tensors, not both"),
    "batch without log_prob": (lambda: _args.ppo_columns(ppo_batch(5, old_log_probs=None)),
                               "the batch was built without obs, actions or log_prob"),
    "reinforce batch and tensors": (lambda: _args.reinforce_columns(reinforce_batch(5), torch.zeros(5, 3)),
                                    "pass a batch or the three tensors, not both"),
    "reinforce batch without obs": (lambda: _args.reinforce_columns(reinforce_batch(5, states=None)),
                                    "the batch was built without obs or actions"),
    "out_dim swapped": (lambda: _args.check_actor_critic(net(1), net(3)), NEEDS_NETS),
    "no networks": (lambda: _args.check_actor_critic(object(), None), NEEDS_NETS),
    "networks' devices": (lambda: _args.check_actor_critic(net(3), net(1, META)),
                          "the actor is on cpu, the critic on meta"),
}


@pytest.mark.parametrize("case", list(HELPER_FAULTS))
def test_helper_refuses_in_these_words(case):
    call, message = HELPER_FAULTS[case]
    with pytest.raises(ValueError) as e:
        call()
    assert str(e.value) == message


def test_helpers_on_good_input():
    bitmask, f32x3 = torch.zeros(5, dtype=torch.uint8), torch.zeros(5, 3)
    assert _args.column("actions", bitmask, 5, CPU).data_ptr() == bitmask.data_ptr()
    assert _args.column("actions", f32x3, 5, CPU).data_ptr() == f32x3.data_ptr()
    assert _args.action_format(bitmask) == abi.DD_ACT_BITMASK and _args.action_format(f32x3) == abi.DD_ACT_F32X3
    assert _args.column("returns", None, 5, CPU) is None and _args.active_mask(None, 5, CPU) is None
    wide = _args.column("returns", torch.ones(5, dtype=torch.float64), 5, CPU)
    assert wide.dtype == torch.float32 and wide.is_contiguous()
    assert _args.row_tensor(torch.ones(10, dtype=torch.int32)[::2], 5, CPU, "dones").dtype == torch.float32
    mask = torch.tensor([True, False, True, True, False])
    assert _args.active_mask(mask, 5, CPU).dtype == torch.uint8
    assert _args.active_mask(mask, 5, CPU).data_ptr() == mask.data_ptr()
    assert _args.states_rows(torch.zeros(7, 15), "td_losses") == 7
    assert _args.ppo_coefficients(0, 1, 2) == (0.0, 1.0, 2.0) and _args.finite("gamma", 1) == 1.0
    assert _args.clip_norm(None) == 0.0 and _args.clip_norm(0.5) == 0.5 and _args.clip_norm(INF) == INF
    assert _args.check_out(torch.zeros(5, 3), (5, 3), torch.float32, CPU, "out") is None
    batch = ppo_batch(5)
    assert all(a is b for a, b in zip(_args.ppo_columns(batch), batch[:5]))
    assert _args.ppo_columns(*five(5)[:2])[2:] == (None, None, None) and _args.batch_five(five(5)) is None
    rb = reinforce_batch(5)
    assert _args.reinforce_columns(rb) == (rb.states, rb.actions, rb.advantages, rb)
    assert _args.reinforce_columns(rb.states, rb.actions, rb.advantages)[3] is None
    assert _args.check_actor_critic(ACTOR, CRITIC) is None


# what both paths of ppo_update refuse before they part: (plan arguments, message with {who})
SHARED_FAULTS = {
    "num_epochs 0": (dict(batch=five(5), num_epochs=0), "num_epochs must be at least 1, got 0"),
    "minibatch_size 0": (dict(batch=five(5), minibatch_size=0), "minibatch_size must be at least 1, got 0"),
    "no minibatch": (dict(batch=five(50), minibatch_size=64, drop_last=True),
                     "no minibatch to step on: 50 rows, minibatch_size 64, drop_last=True"),
    "no rows, no minibatch": (dict(batch=five(0), minibatch_size=64),
                              "no minibatch to step on: 0 rows, minibatch_size 64, drop_last=False"),
    "not a batch": (dict(batch=object(), minibatch_size=4),
                    "batch must be a PpoBatch, a PpoEpisodesBatch or the five tensors"),
    "four tensors": (dict(batch=five(5)[:4], minibatch_size=4), "{who} all five tensors " + FIVE),
    "batch without log_prob": (dict(batch=ppo_batch(5, old_log_probs=None), minibatch_size=4),
                               "{who} all five tensors " + FIVE),
}
# what ppo_losses and MlpNet.backward refuse inside the loop's first step, and the plan for fused=True
FUSED_FAULTS = {
    "clip_epsilon NaN": (dict(clip_epsilon=NAN), "clip_epsilon must be finite, got nan"),
    "entropy_coef inf": (dict(entropy_coef=INF), "entropy_coef must be finite, got inf"),
    "value_coef NaN": (dict(value_coef=NAN), "value_coef must be finite, got nan"),
    "clip_epsilon negative": (dict(clip_epsilon=-1e-3), "clip_epsilon must not be negative, got -0.001"),
    "max_grad_norm NaN": (dict(max_grad_norm=NAN), "max_norm must not be NaN"),
    "out_dim swapped": (dict(actor=net(1), critic=net(3)), NEEDS_NETS),
    "networks' devices": (dict(critic=net(1, META)), "the actor is on cpu, the critic on meta"),
    "no rows": (dict(batch=five(0)), NO_ROWS),
}


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("case", list(SHARED_FAULTS))
def test_both_paths_refuse_in_these_words(case, fused):
    kw, message = SHARED_FAULTS[case]
    message = message.format(who="fused=True needs" if fused else "minibatches need")
    for call in (plan, update):
        with pytest.raises(ValueError) as e:
            call(**kw, fused=fused)
        assert str(e.value) == message


@pytest.mark.parametrize("size", [None, 4])
@pytest.mark.parametrize("case", list(FUSED_FAULTS))
def test_fused_plan_refuses_what_the_first_step_refuses(case, size):
    kw, message = FUSED_FAULTS[case]
    kw = dict(dict(batch=five(5)), **kw)
    if case == "no rows" and size is not None:
        message = "no minibatch to step on: 0 rows, minibatch_size 4, drop_last=False"
    for call in (plan, update):
        with pytest.raises(ValueError) as e:
            call(**kw, fused=True, minibatch_size=size)
        assert str(e.value) == message
    if case == "max_grad_norm NaN":  # MlpNet.backward's, the same helper
        return
    # the loop's first step: ppo_losses, before it touches the networks
    kw.pop("max_grad_norm", None)
    actor, critic, batch = kw.pop("actor", ACTOR), kw.pop("critic", CRITIC), kw.pop("batch")
    with pytest.raises(ValueError) as e:
        ppo_losses(actor, critic, *batch, **kw)
    assert str(e.value) == (NO_ROWS if case == "no rows" else message)


def test_fused_limits_refuse_in_these_words():
    with pytest.raises(ValueError) as e:
        update(five(200), fused=True)
    assert str(e.value) == ("fused=True takes minibatches of at most 128 rows (one row tile of the backward), this "
                            "update has one of 200; pass minibatch_size <= 128 or fused=False")
    with pytest.raises(ValueError) as e:
        update(five(200), fused=True, minibatch_size=129, drop_last=True)
    assert "this update has one of 129;" in str(e.value)
    with pytest.raises(ValueError) as e:
        update(five(5), critic=net(1, compute="f16x3"), fused=True)
    assert str(e.value) == ("fused=True runs compute='f32' networks only, the critic is compute='f16x3'; "
                            "use fused=False")
    with pytest.raises(ValueError) as e:
        update((torch.zeros(5, 14),) + five(5)[1:], fused=True)
    assert str(e.value) == "states must be [M, 15]"
    with pytest.raises(ValueError) as e:
        update(five(5)[:4] + (torch.zeros(4),), fused=True)
    assert str(e.value) == "returns must have shape (5,), got (4,)"


# ---- 2. the first fault wins -------------------------------------------------------------

def test_first_fault_is_the_one_reported_before():
    bad_size = "minibatch_size must be at least 1, got -3"
    for fused in (True, False):  # minibatch_size before a coefficient, on either path
        for call in (plan, update):
            with pytest.raises(ValueError) as e:
                call(five(5), fused=fused, minibatch_size=-3, clip_epsilon=NAN, num_epochs=1)
            assert str(e.value) == bad_size
    # out_dim swapped and M == 0: the fused order is rows, then networks; ppo_losses' (the loop's) is the reverse
    for call in (plan, update):
        with pytest.raises(ValueError) as e:
            call(five(0), net(1), net(3), fused=True)
        assert str(e.value) == NO_ROWS
        with pytest.raises(ValueError) as e:
            call(five(0), net(1), net(3), fused=True, minibatch_size=64)
        assert str(e.value) == "no minibatch to step on: 0 rows, minibatch_size 64, drop_last=False"
    with pytest.raises(ValueError) as e:
        ppo_losses(net(1), net(3), *five(0))
    assert str(e.value) == NEEDS_NETS
    # a network that is not f32 and a step above one row tile: the network first
    with pytest.raises(ValueError) as e:
        update(five(200), net(3, compute="f16x3"), fused=True)
    assert str(e.value) == ("fused=True runs compute='f32' networks only, the actor is compute='f16x3'; "
                            "use fused=False")
    # the rest of the fused order: networks, coefficients, max_grad_norm, then the two limits, then the columns
    order = [(dict(critic=net(1, META)), "the actor is on cpu, the critic on meta"),
             (dict(value_coef=INF), "value_coef must be finite, got inf"),
             (dict(max_grad_norm=NAN), "max_norm must not be NaN"),
             (dict(actor=net(3, compute="f16x3")), "fused=True runs compute='f32' networks only, the actor is "
                                                   "compute='f16x3'; use fused=False"),
             (dict(batch=five(200)[:4] + (torch.zeros(7),)), "fused=True takes minibatches of at most 128 rows (one "
              "row tile of the backward), this update has one of 200; pass minibatch_size <= 128 or fused=False")]
    for first in range(len(order)):
        kw = dict(batch=five(5)[:4] + (torch.zeros(7),))
        for later, _ in reversed(order[first:]):
            kw.update(later)
        with pytest.raises(ValueError) as e:
            update(**kw, fused=True)
        assert str(e.value) == order[first][1], first


# ---- 3. one plan for both paths ------------------------------------------------------------

@pytest.mark.parametrize("m,size,drop_last", [(200, 64, False), (200, 64, True), (37, 1, False)])
def test_one_plan_for_both_paths(m, size, drop_last):
    for batch in (five(m), five(m, "bitmask"), ppo_batch(m)):
        fused = plan(batch, fused=True, minibatch_size=size, drop_last=drop_last)
        loop = plan(batch, fused=False, minibatch_size=size, drop_last=drop_last)
        assert len(fused.five) == 5 and all(a is b for a, b in zip(fused.five, loop.five))
        assert all(a is b for a, b in zip(fused.five, batch[:5]))
        assert fused.ranges == loop.ranges == adamw.minibatch_ranges(m, size, drop_last)
        assert (fused.m, fused.size, fused.num_epochs, fused.drop_last) == (m, size, 2, drop_last) == \
            (loop.m, loop.size, loop.num_epochs, loop.drop_last)
        assert fused.coefficients == loop.coefficients == (0.2, 0.01, 0.5) and fused.max_norm == loop.max_norm == 0.5
    assert [hi - lo for lo, hi in plan(five(200), fused=True, minibatch_size=64).ranges] == [64, 64, 64, 8]
    assert plan(five(96), fused=True).ranges == [(0, 96)] and plan(five(96), fused=True).size is None
    assert plan(five(5), fused=True, max_grad_norm=None).max_norm == 0.0
    # the full batch looped: ppo_losses' arguments as they came, checked in the first step
    batch = ppo_batch(5)
    assert plan(batch, fused=False).five == (batch,) and plan(batch, fused=False).ranges is None


# ---- 4. no private helper crosses a module boundary ------------------------------------------

def test_no_private_helper_is_imported_from_a_sibling():
    package = os.path.dirname(os.path.abspath(delivery_drone_amd.__file__))
    sources = sorted(f for f in os.listdir(package) if f.endswith(".py"))
    assert "_args.py" in sources and len(sources) > 10
    for name in sources:
        tree = ast.parse(open(os.path.join(package, name)).read(), name)
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.level and node.module not in (None, "_args"):
                private = [a.name for a in node.names if a.name.startswith("_")]
                assert not private, f"{name}: from .{node.module} import {private}"
        streams = [n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "_stream"]
        assert not streams, f"{name} defines a module-level _stream"
