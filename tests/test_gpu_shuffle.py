"""GPU: shuffle_indices / shuffle_batch (dd_shuffle_*, csrc/shuffle.hip) against
the NumPy restatement of the keyed permutation (tests/shuffle_ref.py), bit for
bit, and ppo_update's shuffled minibatch epochs against the loop they stand
for: shuffle_batch, ppo_grads on row ranges and the two AdamW steps.

Rows are moved, not computed, so every comparison is on bit patterns and the
payloads are arbitrary words: NaNs with payloads, infinities, denormals.
Sources and destinations are `t[1:]` views, aligned to 4 bytes only (1 for the
uint8 actions), between guard words that must keep their bits.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import adamw_ref
import golden_data as gd
import shuffle_ref as ref
from delivery_drone_amd import (AdamW, MlpNet, ShuffledBatch, abi, ppo_grads, ppo_update, shuffle_batch,
                                shuffle_indices)
from delivery_drone_amd.adamw import LOG_KEYS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 0x9E3779B97F4A7C15   # both keys above 2^32: their high halves count
EPOCH = (7 << 32) + 3
SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 131_073]
COLUMNS = ("states", "actions", "old_log_probs", "advantages", "returns")
GUARD = 0x5EED5EED
COEF = dict(clip_epsilon=0.2, entropy_coef=0.01, value_coef=0.5)


@pytest.fixture(scope="module")
def perms():
    """perm_ref under (SEED, EPOCH) for every size, computed once and left unchanged."""
    return {m: ref.perm_ref(m, SEED, EPOCH) for m in SIZES}


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.uint8 if t.dtype == torch.uint8 else torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---- the permutation -----------------------------------------------------------------------

@pytest.mark.parametrize("m", SIZES)
def test_indices_equal_the_restatement(perms, gpu_device, m):
    got = shuffle_indices(m, seed=SEED, epoch=EPOCH, device=gpu_device)
    assert got.dtype == torch.int32 and tuple(got.shape) == (m,) and got.device == gpu_device
    assert np.array_equal(host(got), perms[m])


def test_indices_default_key_and_empty(gpu_device):
    assert np.array_equal(host(shuffle_indices(1000, device=gpu_device)), ref.perm_ref(1000, 0, 0))
    assert np.array_equal(host(shuffle_indices(1000, seed=SEED + (1 << 64), epoch=EPOCH - (1 << 64), device=gpu_device)),
                          ref.perm_ref(1000, SEED, EPOCH))  # keys are taken modulo 2^64
    assert tuple(shuffle_indices(0, device=gpu_device).shape) == (0,)
    for m in (-1, 2**31):
        with pytest.raises(ValueError, match="rows"):
            shuffle_indices(m, device=gpu_device)
    with pytest.raises(ValueError, match="GPU"):
        shuffle_indices(4, device="cpu")


# ---- rows ----------------------------------------------------------------------------------

def words(rng, shape):
    """Arbitrary 32-bit words as float32: about 1 in 256 is a NaN with a payload; the first
    few are the special values by name."""
    w = rng.integers(0, 2**32, size=shape, dtype=np.uint64).astype(np.uint32)
    flat = w.reshape(-1)
    special = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x7F800000, 0xFF800000, 0x00000001, 0x80000000],
                       dtype=np.uint32)
    n = min(flat.size, special.size)
    flat[:n] = special[:n]
    return w.view(np.float32)


def guarded(values, dev):
    """(view, whole): `values` on the device as a `t[1:-1]` view of a buffer with a guard
    word (byte for uint8) at either end: 4-byte (1-byte) aligned only."""
    v = np.ascontiguousarray(values)
    if v.dtype == np.uint8:
        whole = torch.full((v.size + 2,), GUARD & 0xFF, dtype=torch.uint8, device=dev)
    else:
        whole = torch.full((v.size + 2,), GUARD, dtype=torch.int32, device=dev)
        v = v.view(np.int32)
    view = whole[1:-1]
    view.copy_(torch.as_tensor(v.reshape(-1), device=dev))
    if values.dtype == np.float32:
        view = view.view(torch.float32)
    view = view.view(values.shape)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view, whole


def guards_intact(whole):
    want = GUARD & 0xFF if whole.dtype == torch.uint8 else GUARD
    return int(whole[0]) == want and int(whole[-1]) == want


def make_columns(m, fmt, present, seed=0):
    rng = np.random.default_rng(seed + m)
    cols = {"states": words(rng, (m, 15)),
            "actions": (rng.integers(0, 256, size=m, dtype=np.uint8) if fmt == "bitmask" else words(rng, (m, 3))),
            "old_log_probs": words(rng, (m,)), "advantages": words(rng, (m,)), "returns": words(rng, (m,))}
    return {k: (v if k in present else None) for k, v in cols.items()}


def raw(a):
    return a if a.dtype == np.uint8 else a.view(np.uint32)


@pytest.mark.parametrize("fmt", ["bitmask", "f32x3"])
@pytest.mark.parametrize("m", [1, 3, 65, 255, 256, 257, 1000, 131_073])
def test_rows_equal_the_restatement(perms, gpu_device, m, fmt):
    cols = make_columns(m, fmt, COLUMNS)
    assert np.isnan(cols["states"]).any() and (m < 4 or np.isinf(cols["states"]).any())
    src = {k: guarded(v, gpu_device) for k, v in cols.items()}
    dst = {k: guarded(np.zeros_like(v), gpu_device) for k, v in cols.items()}
    idx = guarded(np.zeros(m, dtype=np.int32), gpu_device)
    out = ShuffledBatch(*(dst[k][0] for k in COLUMNS), idx[0])
    got = shuffle_batch(tuple(src[k][0] for k in COLUMNS), seed=SEED, epoch=EPOCH, out=out)
    assert isinstance(got, ShuffledBatch) and all(a is b for a, b in zip(got, out))
    perm = perms[m]
    assert np.array_equal(host(got.indices), perm)
    for k in COLUMNS:
        assert np.array_equal(raw(host(getattr(got, k))), raw(cols[k])[perm]), k
        assert guards_intact(dst[k][1]) and guards_intact(src[k][1]), k
        assert np.array_equal(raw(host(src[k][0])), raw(cols[k])), k  # the source keeps its bits
    assert guards_intact(idx[1])
    # without `out`: fresh tensors, the same bits
    fresh = shuffle_batch([src[k][0] for k in COLUMNS], seed=SEED, epoch=EPOCH)
    assert all(same(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(fresh, got))
    # another epoch is another order
    if m >= 64:
        other = shuffle_batch([src[k][0] for k in COLUMNS], seed=SEED, epoch=EPOCH + 1)
        assert np.array_equal(host(other.indices), ref.perm_ref(m, SEED, EPOCH + 1))
        assert not same(other.indices, got.indices)


@pytest.mark.parametrize("fmt,present", [("bitmask", ("states",)), ("f32x3", ("actions", "returns")),
                                         ("bitmask", ("actions", "old_log_probs", "advantages")),
                                         ("f32x3", ("states", "advantages"))])
def test_rows_with_columns_absent(perms, gpu_device, fmt, present):
    m = 257
    cols = make_columns(m, fmt, present, seed=1)
    src = {k: guarded(v, gpu_device) for k, v in cols.items() if v is not None}
    got = shuffle_batch(tuple(src[k][0] if k in src else None for k in COLUMNS), seed=SEED, epoch=EPOCH)
    assert np.array_equal(host(got.indices), perms[m])
    for k in COLUMNS:
        if k in present:
            assert np.array_equal(raw(host(getattr(got, k))), raw(cols[k])[perms[m]]), k
        else:
            assert getattr(got, k) is None, k


def test_rows_error_paths(gpu_device):
    m = 65
    cols = make_columns(m, "f32x3", COLUMNS)
    five = tuple(torch.as_tensor(cols[k], device=gpu_device) for k in COLUMNS)
    good = shuffle_batch(five)
    # overlap: the shuffle cannot run in place, and the library says so before any launch
    with pytest.raises(abi.NativeLibraryError, match="dd_shuffle_rows"):
        shuffle_batch(five, out=ShuffledBatch(*five, good.indices))
    flat = torch.zeros(2 * m, device=gpu_device)
    with pytest.raises(abi.NativeLibraryError, match="dd_shuffle_rows"):
        shuffle_batch((None, None, None, None, flat[:m]), out=ShuffledBatch(None, None, None, None, flat[m - 1:2 * m - 1],
                                                                            good.indices))
    # pairing and shapes of `out`
    with pytest.raises(ValueError, match="out.states"):
        shuffle_batch(five, out=good._replace(states=None))
    with pytest.raises(ValueError, match="out.returns"):
        shuffle_batch((five[0], None, None, None, None), out=good._replace(actions=None, old_log_probs=None,
                                                                          advantages=None))
    with pytest.raises(ValueError, match="out.actions"):
        shuffle_batch(five, out=good._replace(actions=torch.zeros(m, dtype=torch.uint8, device=gpu_device)))
    with pytest.raises(ValueError, match="out.advantages"):
        shuffle_batch(five, out=good._replace(advantages=torch.zeros(m + 1, device=gpu_device)))
    with pytest.raises(ValueError, match="out.indices"):
        shuffle_batch(five, out=good._replace(indices=torch.zeros(m, dtype=torch.int64, device=gpu_device)))
    with pytest.raises(ValueError, match="ShuffledBatch"):
        shuffle_batch(five, out=five)
    # the batch itself
    with pytest.raises(ValueError, match="no column"):
        shuffle_batch((None,) * 5)
    with pytest.raises(ValueError, match="five tensors"):
        shuffle_batch(five[:4])
    with pytest.raises(ValueError, match="returns"):
        shuffle_batch(five[:4] + (five[4][:-1],))
    with pytest.raises(ValueError, match="actions"):
        shuffle_batch((five[0], five[1].to(torch.float64)) + five[2:])
    with pytest.raises(ValueError, match="GPU"):
        shuffle_batch(tuple(t.cpu() for t in five))
    # the library's own size check (the wrapper's bypassed): before any launch
    assert abi.lib().dd_shuffle_indices(2**31, 0, 0, good.indices.data_ptr(), None) == 1
    empty = shuffle_batch(tuple(t[:0] for t in five))
    assert all(t.shape[0] == 0 for t in empty)


# ---- ppo_update in minibatches -------------------------------------------------------------

M = 1000


@pytest.fixture(scope="module")
def nets():
    return gd.policy_fixture()[1]


@pytest.fixture(scope="module")
def batch(gpu_device):
    """The ppo_loss fixture's 203 rows, repeated to M = 1000."""
    g = gd.npz("ppo_loss/losses.npz")
    return tuple(torch.as_tensor(np.ascontiguousarray(np.resize(g[k], (M,) + g[k].shape[1:])), device=gpu_device)
                 for k in COLUMNS)


def make(nets, dev, compute):
    actor = MlpNet(nets["actor"], device=dev, compute=compute)
    critic = MlpNet(nets["critic"], device=dev, compute=compute)
    return (actor, critic, AdamW(actor, lr=adamw_ref.NOTEBOOK_LR["actor"]),
            AdamW(critic, lr=adamw_ref.NOTEBOOK_LR["critic"]))


def by_hand(actor, critic, a_opt, c_opt, batch, size, drop_last, epochs, seed, epoch0):
    """The loop ppo_update(minibatch_size=size) stands for, from its parts: [11, epochs, steps]."""
    logs = []
    for e in range(epochs):
        shuffled = shuffle_batch(batch, seed=seed, epoch=epoch0 + e)
        row = []
        for lo, hi in ref.minibatch_ranges(batch[0].shape[0], size, drop_last):
            out = ppo_grads(actor, critic, *(t[lo:hi] for t in shuffled[:5]), **COEF, max_grad_norm=0.5)
            a_opt.step(out.actor)
            c_opt.step(out.critic)
            s = out.losses.ratio_stats
            row.append(torch.stack([out.losses.total_loss, out.losses.policy_loss, out.losses.value_loss,
                                    out.losses.entropy, s["mean"], s["min"], s["max"], s["std"], s["clipped_frac"],
                                    out.actor_grad_norm, out.critic_grad_norm]))
        logs.append(torch.stack(row, dim=1))
    return torch.stack(logs, dim=1)


def same_training_state(x, y):
    (a, c, ao, co), (a2, c2, ao2, co2) = x, y
    return all(same(p, q) for o, o2 in ((ao, ao2), (co, co2))
               for p, q in ((o.params, o2.params), (o.exp_avg, o2.exp_avg), (o.exp_avg_sq, o2.exp_avg_sq),
                            (o._state, o2._state))) and same(a.packed, a2.packed) and same(c.packed, c2.packed)


@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("size", [67, 256])
@pytest.mark.parametrize("compute", ["f32", "f16x3"])
def test_minibatch_update_equals_its_parts(nets, batch, gpu_device, compute, size, drop_last):
    epochs = 2
    steps = M // size if drop_last else -(-M // size)
    assert (size, steps) in ((67, 15), (67, 14), (256, 4), (256, 3))  # 67: a tail of 62 rows, ranges 4-byte aligned only
    ours, twin = make(nets, gpu_device, compute), make(nets, gpu_device, compute)
    out = ppo_update(*ours[:2], batch, *ours[2:], num_epochs=epochs, **COEF, max_grad_norm=0.5, minibatch_size=size,
                     shuffle_seed=SEED, shuffle_epoch=EPOCH, drop_last=drop_last)
    want = by_hand(*twin, batch, size, drop_last, epochs, SEED, EPOCH)
    assert same_training_state(ours, twin)
    assert ours[2].step_count() == epochs * steps and ours[3].step_count() == epochs * steps
    assert ours[2].status() == 0 and ours[3].status() == 0
    assert tuple(out.logs) == LOG_KEYS
    for i, key in enumerate(LOG_KEYS):
        assert out.logs[key].shape == (epochs, steps) and out.logs[key].dtype == torch.float64
        assert out.logs[key].device == gpu_device and same(out.logs[key], want[i]), key
        derived = {"ratio_min": want[i].min(), "ratio_max": want[i].max()}.get(key, want[i].mean())
        assert same(out.summary[key], derived), key
    # the second epoch saw another order: its first minibatch's loss is not the first epoch's
    assert not same(out.logs["policy_grad_norm"][0], out.logs["policy_grad_norm"][1])


@pytest.mark.parametrize("compute", ["f32", "f16x3"])
def test_one_minibatch_of_all_rows_is_the_full_batch_epoch_on_permuted_rows(nets, batch, gpu_device, compute):
    perm = torch.as_tensor(ref.perm_ref(M, SEED, EPOCH).astype(np.int64), device=gpu_device)
    ours, twin = make(nets, gpu_device, compute), make(nets, gpu_device, compute)
    out = ppo_update(*ours[:2], batch, *ours[2:], num_epochs=1, **COEF, minibatch_size=M, shuffle_seed=SEED,
                     shuffle_epoch=EPOCH)
    want = ppo_update(*twin[:2], tuple(t[perm].contiguous() for t in batch), *twin[2:], num_epochs=1, **COEF)
    assert same_training_state(ours, twin)
    for key in LOG_KEYS:
        assert out.logs[key].shape == (1, 1) and same(out.logs[key].reshape(1), want.logs[key]), key
        assert same(out.summary[key], want.summary[key]), key


def test_minibatch_error_paths(nets, batch, gpu_device):
    nets4 = make(nets, gpu_device, "f32")
    for bad in (0, -3):
        with pytest.raises(ValueError, match="minibatch_size"):
            ppo_update(*nets4[:2], batch, *nets4[2:], minibatch_size=bad)
    with pytest.raises(ValueError, match="no minibatch"):
        ppo_update(*nets4[:2], batch, *nets4[2:], minibatch_size=M + 1, drop_last=True)
    with pytest.raises(ValueError, match="five tensors"):
        ppo_update(*nets4[:2], batch[:4] + (None,), *nets4[2:], minibatch_size=64)
    assert nets4[2].step_count() == 0 and nets4[3].step_count() == 0
    out = ppo_update(*nets4[:2], batch, *nets4[2:], num_epochs=1, minibatch_size=M + 1)  # the tail is the whole batch
    assert out.logs["total_loss"].shape == (1, 1) and nets4[2].step_count() == 1


def test_graph_replay():
    """tests/shuffle_graph_check.py in a process of its own, under its own time
    limit: one captured ppo_update(minibatch_size=256, num_epochs=1), replayed,
    against the same eager calls with the same shuffle_epoch."""
    done = subprocess.run([sys.executable, os.path.join(HERE, "shuffle_graph_check.py")], capture_output=True,
                          text=True, timeout=120)
    print(done.stdout[-2000:], done.stderr[-2000:])
    assert done.returncode == 0 and "graph replay ok" in done.stdout
