"""No GPU: ppo_update_population's argument errors
(delivery_drone_amd/population.py), and the row order
dd_ppo_update_population is specified to read (include/dronestep.h), restated
with tests/shuffle_ref.py.

The wrapper's checks read a network's ``out_dim``, ``device``, ``compute`` and
``_lib`` and an optimizer's ``net`` only, so the members here are MlpNet and
AdamW objects made without their constructors (which need a GPU), with batches
of CPU tensors.  Every refusal comes before anything is allocated or launched.
"""
import functools
import types

import numpy as np
import pytest
import torch

import shuffle_ref
from delivery_drone_amd import AdamW, LearnerPopulation, MlpNet, abi, ppo_update_population
from delivery_drone_amd.adamw import minibatch_ranges

CPU = torch.device("cpu")
LIB = object()


def net(out_dim, compute="f32", device=CPU, lib=LIB):
    n = object.__new__(MlpNet)
    n.out_dim, n.compute, n.device, n._lib = out_dim, compute, device, lib
    return n


def opt(network):
    o = object.__new__(AdamW)
    o.net = network
    return o


def member(compute=("f32", "f32"), **kw):
    actor, critic = net(3, compute[0], **kw), net(1, compute[1], **kw)
    return (actor, critic, opt(actor), opt(critic))


def population(count):
    """A LearnerPopulation of stand-in members, without its device-side parts."""
    pop = object.__new__(LearnerPopulation)
    pop._members = tuple(member() for _ in range(count))
    pop.device, pop._lib = CPU, LIB
    return pop


def five(m):
    return (torch.zeros(m, abi.DD_OBS_DIM), torch.zeros(m, 3), torch.zeros(m), torch.zeros(m), torch.zeros(m))


# ---- LearnerPopulation -------------------------------------------------------------------

def test_member_tuples_are_checked():
    good = member()
    with pytest.raises(ValueError, match="at least one member"):
        LearnerPopulation([])
    with pytest.raises(ValueError, match=r"member 1: expected \(actor, critic, actor_opt, critic_opt\)"):
        LearnerPopulation([good, good[:3]])
    with pytest.raises(ValueError, match="member 0: expected"):
        LearnerPopulation([good[0]])
    with pytest.raises(ValueError, match="member 0: the actor and the critic must be MlpNets"):
        LearnerPopulation([(types.SimpleNamespace(out_dim=3), good[1], good[2], good[3])])
    with pytest.raises(ValueError, match="member 0: actor_opt and critic_opt must be AdamW"):
        LearnerPopulation([(good[0], good[1], good[2], None)])
    other = member()
    with pytest.raises(ValueError, match="member 1: actor_opt must optimize actor and critic_opt critic"):
        LearnerPopulation([good, (other[0], other[1], good[2], other[3])])
    swapped = (good[1], good[0], good[3], good[2])  # critic in the actor's place
    with pytest.raises(ValueError, match=r"member 0: ppo_losses needs an MlpNet actor \(out_dim 3\)"):
        LearnerPopulation([swapped])
    with pytest.raises(ValueError, match="member 1: its actor is in the population already"):
        LearnerPopulation([good, good])


def test_f16x3_members_are_refused():
    for compute, name in ((("f16x3", "f32"), "actor"), (("f32", "f16x3"), "critic")):
        with pytest.raises(ValueError, match=f"member 1: .*f32.* the {name} is compute='f16x3'"):
            LearnerPopulation([member(), member(compute)])


def test_members_share_a_device_and_a_library():
    with pytest.raises(ValueError, match="member 1: on meta, member 0 on cpu"):
        LearnerPopulation([member(), member(device=torch.device("meta"))])
    with pytest.raises(ValueError, match="member 1: uses another build"):
        LearnerPopulation([member(), member(lib=object())])


# ---- ppo_update_population ---------------------------------------------------------------

def test_update_argument_errors_name_the_member():
    pop = population(3)
    batches = [five(200), five(130), five(64)]
    with pytest.raises(ValueError, match="pop must be a LearnerPopulation"):
        ppo_update_population([member()], batches[:1])
    with pytest.raises(ValueError, match="batches: 2 batches for 3 members"):
        ppo_update_population(pop, batches[:2], minibatch_size=64)
    # a per-member sequence of the wrong length
    for name in ("clip_epsilon", "entropy_coef", "value_coef", "max_grad_norm", "shuffle_seed"):
        with pytest.raises(ValueError, match=f"{name}: 2 values for 3 members"):
            ppo_update_population(pop, batches, minibatch_size=64, **{name: [0.1, 0.2]})
    # a minibatch above 128 rows: the launch-wide size, one member's full batch, one member's forced tail
    with pytest.raises(ValueError, match="member 0: .*at most 128 rows.* one of 129"):
        ppo_update_population(pop, batches, minibatch_size=129)
    with pytest.raises(ValueError, match="member 0: .*at most 128 rows.* one of 200"):
        ppo_update_population(pop, batches)
    with pytest.raises(ValueError, match="member 1: .*at most 128 rows.* one of 130"):
        ppo_update_population(pop, [five(100), five(130), five(64)], minibatch_size=150)
    # drop_last leaves member 2 no minibatch
    with pytest.raises(ValueError, match="member 2: no minibatch to step on: 64 rows, minibatch_size 100"):
        ppo_update_population(pop, batches, minibatch_size=100, drop_last=True)
    # the per-member checks of _args, with the member's own value
    with pytest.raises(ValueError, match="member 1: clip_epsilon must not be negative, got -0.5"):
        ppo_update_population(pop, batches, minibatch_size=64, clip_epsilon=[0.1, -0.5, 0.3])
    with pytest.raises(ValueError, match="member 2: max_norm must not be NaN"):
        ppo_update_population(pop, batches, minibatch_size=64, max_grad_norm=[0.5, 0.5, float("nan")])
    with pytest.raises(ValueError, match=r"member 1: advantages must have shape \(130,\), got \(129,\)"):
        bad = list(five(130))
        bad[3] = torch.zeros(129)
        ppo_update_population(pop, [batches[0], tuple(bad), batches[2]], minibatch_size=64)
    with pytest.raises(ValueError, match="member 0: num_epochs must be at least 1"):
        ppo_update_population(pop, batches, minibatch_size=64, num_epochs=0)


# ---- the rows a workgroup reads ----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def perm(m, seed, epoch):
    return shuffle_ref.perm_ref(m, seed, epoch).tolist()


def src(k, i, size, m, seed, epoch, shuffle=True):
    """include/dronestep.h: row k of minibatch i reads source row perm(i size + k; m, seed, epoch)."""
    j = i * size + k
    return perm(m, seed, epoch)[j] if shuffle else j


ROW_CASES = [
    # m, B, seed, first epoch
    (1, 1, 0, 0), (2, 1, 5, 1), (3, 64, 11, 2), (33, 32, 1, 0), (130, 64, 22, 7), (200, 64, 33, 9),
    (200, 128, 0x9E3779B97F4A7C15, (7 << 32) + 3), (100, 32, 4, 0), (64, 32, 2**64 - 1, 2**32 - 1),
]


# with drop_last the call refuses a member with no minibatch (m < B)
@pytest.mark.parametrize("m,size,seed,epoch0,drop_last",
                         [c + (d,) for c in ROW_CASES for d in (False, True) if not (d and c[0] < c[1])])
def test_an_epochs_rows_are_the_shuffled_batch_cut_at_the_ranges(m, size, seed, epoch0, drop_last):
    eff = min(size, m)  # a member's effective size, as the single call passes it
    steps = m // size if drop_last else -(-m // eff)
    ranges = minibatch_ranges(m, size, drop_last)
    assert ranges == shuffle_ref.minibatch_ranges(m, size, drop_last) and len(ranges) == steps
    for e in range(2):
        want = shuffle_ref.perm_ref(m, seed, epoch0 + e)  # the shuffled copy's row j is source row want[j]
        read = []
        for i, (lo, hi) in enumerate(ranges):
            rows = min(eff, m - i * eff)
            assert (lo, hi) == (i * eff, i * eff + rows) and 1 <= rows <= 128
            mine = [src(k, i, eff, m, seed, epoch0 + e) for k in range(rows)]
            assert mine == want[lo:hi].tolist()
            read += mine
        if not drop_last:
            assert sorted(read) == list(range(m))  # a permutation of [0, m)
        else:
            assert len(set(read)) == len(read) == steps * size and set(read) <= set(range(m))
    # without shuffle: the batch in order
    assert [src(k, 1, eff, m, seed, epoch0, shuffle=False) for k in range(2)] == [eff, eff + 1]
    assert any(d and c[0] > c[1] and c[0] % c[1] for c in ROW_CASES for d in (True,))  # a dropped tail occurs
    if m > 8:
        assert not np.array_equal(shuffle_ref.perm_ref(m, seed, epoch0), shuffle_ref.perm_ref(m, seed, epoch0 + 1))
