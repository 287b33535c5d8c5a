"""GPU: the every-episode training batch (csrc/train_batch_episodes.hip behind
``ppo_episodes_batch`` / ``reinforce_episodes_batch`` / ``collect_ppo_steps``)
against the NumPy restatement tests/episodes_ref.py, which
test_train_batch_episodes_cpu.py pins to the notebooks' own results.

Base shape T = 37, N = 515 (more than two 256-lane scan tiles and eight
64-lane gather tiles, N % 4 != 0, T no multiple of the 8- or 16-frame tile),
done density 0.08 with the re-spawn frame's flag forced to zero in auto-reset
lanes, the special lanes of the CPU fixture, 64 consecutive lanes without a
row and 64 consecutive lanes with a done on every other kept frame.  Layout,
gathers, values, GAE, returns and episode_return are compared bit for bit; the
normalised values within test_gpu_train_batch.py's bound,
1 ulp_f32(|ref|) + 64 * 2^-53 * max|a| / std  (the rounding to float32 plus
the two double reductions' different summation orders: trees of depth <= 16
over M < 2^16 rows, relative error <= 16 * 2^-53 per side on values <= max|a|,
scaled by 1 / std as the output is), computed from the test's own data.
"""
import ctypes
import dataclasses
import os

import numpy as np
import pytest
import torch

import episodes_ref as eref
from delivery_drone_amd import EnvConfig, MlpNet, VecDroneEnv, abi
from delivery_drone_amd import collect_ppo_steps, ppo_batch, ppo_episodes_batch, reinforce_batch
from delivery_drone_amd import reinforce_episodes_batch
from delivery_drone_amd import train_batch as tb

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
T0, N0 = 37, 515


def _dev():
    return torch.device("cuda", 0)


def respawn_frames_not_done(done, before, lanes):
    """An auto-reset env never reports done on the re-spawn frame."""
    for i in lanes:
        prev = before[i]
        for t in range(done.shape[0]):
            if prev:
                done[t, i] = False
            prev = done[t, i]


def make_rollout(T, n, seed=0, density=0.08, before_p=0.1, special=False, sticky=False):
    rng = np.random.default_rng(seed)
    done = rng.random((T, n)) < density
    before = rng.random(n) < before_p
    auto = set(range(n))
    if special:  # T0 x N0: the lanes of tests/golden/train_batch_episodes, then the two runs of 64 lanes
        done[:, :10] = False
        before[:10] = False
        done[0, 0] = True
        done[T - 1, 1] = True
        done[T - 2, 2] = True
        done[20, 3], before[3] = True, True
        done[:, 4], before[4] = True, True
        done[[9, 11], 6] = True
        done[13:, 7] = True
        done[[4, 12, 13, 25, 31], 8] = True
        done[17, 9] = True
        done[:, 100:164], before[100:164] = True, True          # no row in 64 lanes, across two gather tiles
        done[:, 300:364], before[300:364] = False, False
        done[1::3, 300:364] = True                              # kept, kept + done, re-spawn, ...
        auto -= {4, 7, 8} | set(range(100, 164))
    if sticky:
        first = done.argmax(axis=0)
        for i in range(n):
            if done[:, i].any():
                done[first[i]:, i] = True
        before[:] = False
    else:
        respawn_frames_not_done(done, before, sorted(auto))
    # distinct per (t, lane, column): a misplaced row or element is visible
    obs = (np.arange(T * n * 15, dtype=np.float64).reshape(T, n, 15) * 0.25 - 1000.0).astype(np.float32)
    reward = rng.normal(0.0, 3.0, (T, n))
    reward[done] = rng.choice([-500.0, 500.0, 557.3], size=int(done.sum()))
    bootstrap = rng.normal(0.0, 40.0, n).astype(np.float32)
    bootstrap[bootstrap == 0] = 1.0
    return dict(done=done.astype(np.uint8), before=before.astype(np.uint8), obs=obs,
                actions=rng.integers(0, 8, (T, n)).astype(np.uint8),
                log_prob=rng.normal(-2.0, 1.0, (T, n)).astype(np.float32), reward=reward,
                values=rng.normal(0.0, 40.0, (T, n)).astype(np.float32), bootstrap=bootstrap)


class TableCritic:
    """A critic whose values the test chooses: row -> value by the row's
    first column (distinct per (t, lane) in make_rollout)."""

    def __init__(self, r, dev):
        keys = np.concatenate([r["obs"][:, :, 0].reshape(-1), boot_obs_of(r)[:, 0]])
        vals = np.concatenate([r["values"].reshape(-1), r["bootstrap"]])
        order = np.argsort(keys)
        self.keys = torch.from_numpy(keys[order]).to(dev)
        self.vals = torch.from_numpy(vals[order]).to(dev)

    def __call__(self, rows):
        idx = torch.searchsorted(self.keys, rows[:, 0].contiguous())
        assert bool((self.keys[idx] == rows[:, 0]).all())
        return self.vals[idx]


def boot_obs_of(r):
    n = r["done"].shape[1]
    return (np.arange(n * 15, dtype=np.float64).reshape(n, 15) * 0.25 + 1.0e6).astype(np.float32)


def to_dev(r, reward_dtype=torch.float64):
    dev = _dev()
    d = {k: torch.from_numpy(v).to(dev) for k, v in r.items()}
    d["reward"] = d["reward"].to(reward_dtype)
    d["boot_obs"] = torch.from_numpy(boot_obs_of(r)).to(dev)
    return d


def expected(r, reward=None, bootstrap=True, before=True, drop_open=False, gamma=0.99, lam=0.95):
    reward = r["reward"] if reward is None else reward
    lay = eref.layout(r["done"], r["before"] if before else None, drop_open=drop_open)
    values = eref.gather(r["values"], lay)
    adv, ret = eref.gae_flat(reward, values, lay, r["bootstrap"] if bootstrap else None, gamma, lam)
    return dict(lay=lay, states=eref.gather(r["obs"], lay), actions=eref.actions_f32(eref.gather(r["actions"], lay)),
                log_prob=eref.gather(r["log_prob"], lay), values=values, adv=adv, ret=ret,
                G=eref.returns_flat(reward, lay, gamma), ep=eref.episode_return(reward, lay))


def norm_bound(raw, want):
    raw = raw.astype(np.float64)
    return np.spacing(np.abs(want)).astype(np.float64) + 64 * 2.0 ** -53 * np.abs(raw).max() / raw.std(ddof=1)


def check_normalised(got, mean, std, raw):
    m, s, want = eref.normalize(raw)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bound = norm_bound(raw, want)
    print(f"normalised: max err {err.max():.3e}, min bound {bound.min():.3e}, mean {mean!r} vs {m!r}, std {std!r} vs {s!r}")
    assert (err <= bound).all()
    slack = 64 * 2.0 ** -53 * np.abs(raw).max()
    assert abs(mean - m) <= slack and abs(std - s) <= slack


def cpu(t):
    return None if t is None else t.cpu().numpy()


def check_layout(b, lay):
    got = dict(lane_episode=b.lane_episode_offsets, lane_row=b.lane_row_offsets, ep_lane=b.ep_lane,
               ep_start=b.ep_start, ep_length=b.ep_lengths, ep_ended=b.ep_ended, ep_offset=b.ep_offsets)
    for name in eref.LAYOUT_ARRAYS:
        g = cpu(got[name])
        want = lay[name].astype(bool) if name == "ep_ended" else lay[name]
        assert g.dtype == want.dtype and np.array_equal(g, want), name


def check_rows(b, x, lp=True):
    M = int(x["lay"]["ep_offset"][-1])
    assert b.states.shape == (M, 15) and b.actions.shape == (M, 3)
    assert np.array_equal(cpu(b.states), x["states"]) and np.array_equal(cpu(b.actions), x["actions"])
    if lp:
        assert b.old_log_probs.shape == (M,) and np.array_equal(cpu(b.old_log_probs), x["log_prob"])


def run_ppo(r, d, before=True, **kw):
    return ppo_episodes_batch(d["obs"], d["actions"], d["log_prob"], d["reward"], d["done"], TableCritic(r, _dev()),
                              bootstrap_obs=d["boot_obs"], done_before=d["before"] if before else None, **kw)


@pytest.fixture(scope="module")
def base():
    r = make_rollout(T0, N0, seed=1, special=True)
    return r, expected(r)


def test_base_shape_covers_the_cases(base):
    r, x = base
    lay = x["lay"]
    cases = eref.covered_cases(r["done"], r["before"], lay, r["reward"], r["bootstrap"])
    assert all(cases.values()), [k for k, v in cases.items() if not v]
    assert (np.diff(lay["lane_row"])[100:164] == 0).all()
    e = slice(lay["lane_episode"][300], lay["lane_episode"][364])
    # dones at frames 1, 4, ..., 34: twelve episodes of two frames, then frame 36 alone, open
    assert (np.diff(lay["lane_episode"])[300:364] == 13).all()
    assert (lay["ep_length"][e][lay["ep_ended"][e] != 0] == 2).all() and (lay["ep_ended"][e] != 0).sum() == 64 * 12
    density = r["done"][:, 10:100].mean()
    assert 0.05 < density < 0.09
    assert lay["lane_episode"][-1] > N0 and lay["lane_row"][-1] < 2 ** 16


@pytest.mark.parametrize("reward_dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_ppo_episodes_batch_base_shape(base, reward_dtype):
    r, x = base
    if reward_dtype == torch.float32:
        x = expected(r, reward=r["reward"].astype(np.float32))
    d = to_dev(r, reward_dtype)
    b = run_ppo(r, d)
    check_layout(b, x["lay"])
    check_rows(b, x)
    assert np.array_equal(cpu(b.values), x["values"])
    assert np.array_equal(cpu(b.returns), x["ret"])
    assert np.array_equal(cpu(b.episode_return), x["ep"]) and b.episode_return.dtype == torch.float64
    check_normalised(cpu(b.advantages), float(b.adv_mean), float(b.adv_std), x["adv"])
    raw = run_ppo(r, d, normalize=False)
    assert np.array_equal(cpu(raw.advantages), x["adv"])
    assert float(raw.adv_mean) == float(b.adv_mean) and float(raw.adv_std) == float(b.adv_std)
    again = run_ppo(r, d)  # repeated calls: identical bits
    for got, first in zip(again, b):
        assert torch.equal(got, first)


@pytest.mark.parametrize("drop_open", [True, False], ids=["closed", "all"])
def test_reinforce_episodes_batch_base_shape(base, drop_open):
    r, x = base
    if drop_open:
        x = expected(r, drop_open=True)
        assert x["lay"]["ep_ended"].all() and len(x["lay"]["ep_lane"]) < len(base[1]["lay"]["ep_lane"])
    d = to_dev(r)
    b = reinforce_episodes_batch(d["obs"], d["actions"], d["reward"], d["done"], done_before=d["before"],
                                 drop_open=drop_open)
    check_layout(b, x["lay"])
    check_rows(b, x, lp=False)
    assert np.array_equal(cpu(b.returns), x["G"]) and np.array_equal(cpu(b.episode_return), x["ep"])
    check_normalised(cpu(b.advantages), float(b.baseline), float(b.std), x["G"])
    raw = reinforce_episodes_batch(d["obs"], d["actions"], d["reward"], d["done"], done_before=d["before"],
                                   drop_open=drop_open, normalize=False)
    assert np.array_equal(cpu(raw.advantages), x["G"]) and float(raw.baseline) == float(b.baseline)
    # float32 rewards, another gamma
    x32 = expected(r, reward=r["reward"].astype(np.float32), drop_open=drop_open, gamma=0.9)
    b32 = reinforce_episodes_batch(None, None, d["reward"].float(), d["done"], done_before=d["before"], gamma=0.9,
                                   normalize=False, drop_open=drop_open)
    assert np.array_equal(cpu(b32.returns), x32["G"]) and np.array_equal(cpu(b32.episode_return), x32["ep"])
    if drop_open:  # the default
        dflt = reinforce_episodes_batch(None, None, d["reward"], d["done"], done_before=d["before"])
        assert torch.equal(dflt.returns, b.returns) and torch.equal(dflt.ep_offsets, b.ep_offsets)


def test_gather_tiles_of_8_and_16_frames(base):
    r, x = base
    d = to_dev(r)
    for drop_open in (False, True):
        want = expected(r, drop_open=True) if drop_open else x
        plan = tb._EpisodePlan(d["done"], d["before"], drop_open=drop_open)
        for frames in (8, 16):
            s, a, lp = plan.gather(d["obs"], d["actions"], d["log_prob"], tile_frames=frames)
            assert np.array_equal(cpu(s), want["states"]) and np.array_equal(cpu(a), want["actions"])
            assert np.array_equal(cpu(lp), want["log_prob"])


def test_no_row_past_m_and_no_dropped_frame_is_written(base):
    """The gather and the advantages into larger, pre-filled buffers through
    the C ABI, at every 16-byte phase of obs and states: rows >= M keep their
    fill (and every row < M is a kept frame's, by the comparison)."""
    r, _ = base
    d = to_dev(r)
    dev = _dev()
    x = expected(r, drop_open=True)
    plan = tb._EpisodePlan(d["done"], d["before"], drop_open=True)
    M, pad = plan.M, 300
    assert M == x["lay"]["ep_offset"][-1]
    for shift in (0, 1, 2, 3):
        src = torch.empty(T0 * N0 * 15 + 4, device=dev)
        src[shift:shift + T0 * N0 * 15] = d["obs"].reshape(-1)
        o = (4 - shift) % 4
        states = torch.full(((M + pad) * 15 + 8,), -7.0, device=dev)
        acts = torch.full((M + pad, 3), -7.0, device=dev)
        lps = torch.full((M + pad,), -7.0, device=dev)
        io = abi.DDBatchGatherIO(src.data_ptr() + 4 * shift, d["actions"].data_ptr(), d["log_prob"].data_ptr(),
                                 states.data_ptr() + 4 * o, acts.data_ptr(), lps.data_ptr(), 16 if shift % 2 else 8, 0)
        abi.check(abi.lib().dd_episodes_gather(ctypes.byref(plan.layout), d["done"].data_ptr(),
                                               d["before"].data_ptr(), ctypes.byref(io), T0, N0, None), "gather")
        torch.cuda.synchronize()
        assert np.array_equal(cpu(states[o:o + M * 15]).reshape(-1, 15), x["states"])
        assert bool((states[:o] == -7.0).all()) and bool((states[o + M * 15:] == -7.0).all())
        assert np.array_equal(cpu(acts[:M]), x["actions"]) and bool((acts[M:] == -7.0).all())
        assert np.array_equal(cpu(lps[:M]), x["log_prob"]) and bool((lps[M:] == -7.0).all())
    ret = torch.full((M + pad,), -7.0, device=dev)
    ep = torch.full((plan.E + pad,), -7.0, device=dev, dtype=torch.float64)
    io = abi.DDBatchAdvIO(d["reward"].data_ptr(), abi.DD_F64, abi.DD_BATCH_RETURNS, None, None, None, ret.data_ptr(),
                          ep.data_ptr(), 0.99, 0.0)
    abi.check(abi.lib().dd_episodes_advantages(ctypes.byref(plan.layout), ctypes.byref(io), T0, N0, None), "adv")
    torch.cuda.synchronize()
    assert np.array_equal(cpu(ret[:M]), x["G"]) and bool((ret[M:] == -7.0).all())
    assert np.array_equal(cpu(ep[:plan.E]), x["ep"]) and bool((ep[plan.E:] == -7.0).all())


def test_optional_inputs_absent_in_turn(base):
    r, x = base
    d = to_dev(r)
    critic = TableCritic(r, _dev())
    kw = dict(bootstrap_obs=d["boot_obs"], done_before=d["before"], normalize=False)
    b = ppo_episodes_batch(d["obs"], None, d["log_prob"], d["reward"], d["done"], critic, **kw)
    assert b.actions is None and np.array_equal(cpu(b.old_log_probs), x["log_prob"])
    assert np.array_equal(cpu(b.states), x["states"]) and np.array_equal(cpu(b.advantages), x["adv"])
    b = ppo_episodes_batch(d["obs"], d["actions"], None, d["reward"], d["done"], critic, **kw)
    assert b.old_log_probs is None and np.array_equal(cpu(b.actions), x["actions"])
    assert np.array_equal(cpu(b.advantages), x["adv"])
    # no bootstrap state: 0, as compute_gae appends
    b = ppo_episodes_batch(d["obs"], None, None, d["reward"], d["done"], critic, done_before=d["before"],
                           normalize=False)
    x0 = expected(r, bootstrap=False)
    assert np.array_equal(cpu(b.advantages), x0["adv"]) and np.array_equal(cpu(b.returns), x0["ret"])
    assert not np.array_equal(x0["adv"], x["adv"])
    # no done_before: all zero, and bool flags as the env hands them out
    xb = expected(r, before=False)
    assert not np.array_equal(xb["lay"]["lane_row"], x["lay"]["lane_row"])
    b = ppo_episodes_batch(d["obs"], d["actions"], d["log_prob"], d["reward"], d["done"].bool(), critic,
                           bootstrap_obs=d["boot_obs"], normalize=False)
    check_layout(b, xb["lay"])
    check_rows(b, xb)
    assert np.array_equal(cpu(b.advantages), xb["adv"]) and np.array_equal(cpu(b.episode_return), xb["ep"])
    b = ppo_episodes_batch(d["obs"], None, None, d["reward"], d["done"], critic, bootstrap_obs=d["boot_obs"],
                           done_before=d["before"].bool(), normalize=False)
    assert np.array_equal(cpu(b.advantages), x["adv"])
    rb = reinforce_episodes_batch(None, d["actions"], d["reward"], d["done"], d["before"], normalize=False,
                                  drop_open=False)
    assert rb.states is None and np.array_equal(cpu(rb.actions), x["actions"])
    rb = reinforce_episodes_batch(d["obs"], None, d["reward"], d["done"], d["before"], normalize=False,
                                  drop_open=False)
    assert rb.actions is None and np.array_equal(cpu(rb.states), x["states"])
    with pytest.raises(ValueError):
        ppo_episodes_batch(None, None, None, d["reward"], d["done"], critic)
    with pytest.raises(ValueError, match="contiguous"):
        reinforce_episodes_batch(d["obs"].transpose(0, 1).contiguous().transpose(0, 1), None, d["reward"], d["done"])
    with pytest.raises(ValueError, match="shape"):
        reinforce_episodes_batch(None, None, d["reward"], d["done"], done_before=d["before"][:-1])
    with pytest.raises(ValueError, match="uint8"):
        reinforce_episodes_batch(None, None, d["reward"], d["done"], done_before=d["before"].int())


def test_reduces_to_the_first_episode_batch_on_sticky_buffers():
    """Every lane sticky after its first done, done_before null: the two
    builders give the same bits."""
    r = make_rollout(T0, N0, seed=4, sticky=True)
    assert r["done"].any(axis=0).sum() > N0 // 2 and not r["done"].all(axis=0).all()
    d = to_dev(r)
    critic = TableCritic(r, _dev())
    a = ppo_episodes_batch(d["obs"], d["actions"], d["log_prob"], d["reward"], d["done"], critic,
                           bootstrap_obs=d["boot_obs"])
    b = ppo_batch(d["obs"], d["actions"], d["log_prob"], d["reward"], d["done"], critic, bootstrap_obs=d["boot_obs"])
    for name in ("states", "actions", "old_log_probs", "values", "advantages", "returns", "episode_return",
                 "adv_mean", "adv_std"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.ep_lengths, b.lengths) and torch.equal(a.ep_offsets, b.offsets)
    assert torch.equal(a.ep_ended, b.ended) and torch.equal(a.lane_row_offsets, b.offsets)
    assert torch.equal(a.ep_lane, torch.arange(N0, device=_dev(), dtype=torch.int32)) and not bool(a.ep_start.any())
    ra = reinforce_episodes_batch(d["obs"], d["actions"], d["reward"], d["done"], drop_open=False)
    rb = reinforce_batch(d["obs"], d["actions"], d["reward"], d["done"])
    for name in ("states", "actions", "returns", "advantages", "baseline", "std", "episode_return"):
        assert torch.equal(getattr(ra, name), getattr(rb, name)), name
    assert torch.equal(ra.ep_lengths, rb.lengths) and torch.equal(ra.ep_offsets, rb.offsets)
    assert torch.equal(ra.ep_ended, rb.ended)


@pytest.mark.parametrize("T,n,density,before_p", [
    (1, 70, 0.3, 0.3),
    (37, 1, 0.15, 0.0),
    (37, 1, 0.15, 1.0),
    (9, 256, 0.2, 0.2),
    (9, 257, 0.2, 0.2),
], ids=["T1", "N1", "N1-done-before", "N256", "N257"])
def test_edge_shapes(T, n, density, before_p):
    r = make_rollout(T, n, seed=7, density=density, before_p=before_p)
    d = to_dev(r)
    for drop_open in (False, True):
        x = expected(r, drop_open=drop_open)
        rb = reinforce_episodes_batch(d["obs"], d["actions"], d["reward"], d["done"], d["before"], normalize=False,
                                      drop_open=drop_open)
        check_layout(rb, x["lay"])
        check_rows(rb, x, lp=False)
        assert np.array_equal(cpu(rb.returns), x["G"]) and np.array_equal(cpu(rb.episode_return), x["ep"])
    x = expected(r)
    assert x["lay"]["ep_offset"][-1] >= 2
    b = run_ppo(r, d)
    check_layout(b, x["lay"])
    check_rows(b, x)
    assert np.array_equal(cpu(b.returns), x["ret"]) and np.array_equal(cpu(b.episode_return), x["ep"])
    check_normalised(cpu(b.advantages), float(b.adv_mean), float(b.adv_std), x["adv"])


def test_batch_without_a_row():
    """Every lane done before and sticky: E == M == 0, empty tensors, NaN
    statistics as M < 2 gives, nothing launched on empty buffers."""
    T, n = 5, 70
    r = make_rollout(T, n, seed=2)
    r["done"][:] = 1
    r["before"][:] = 1
    d = to_dev(r)
    b = run_ppo(r, d)
    assert b.states.shape == (0, 15) and b.actions.shape == (0, 3) and b.old_log_probs.shape == (0,)
    assert b.advantages.shape == b.returns.shape == b.values.shape == (0,)
    assert b.ep_lane.shape == b.ep_start.shape == b.ep_lengths.shape == b.ep_ended.shape == (0,)
    assert b.episode_return.shape == (0,) and cpu(b.ep_offsets).tolist() == [0]
    assert not cpu(b.lane_episode_offsets).any() and not cpu(b.lane_row_offsets).any()
    assert np.isnan(float(b.adv_mean)) and np.isnan(float(b.adv_std))
    rb = reinforce_episodes_batch(d["obs"], d["actions"], d["reward"], d["done"], d["before"])
    assert rb.returns.shape == (0,) and np.isnan(float(rb.std))
    # T == 0 and N == 0 through the wrapper: the count's empty batch
    dev = _dev()
    e = reinforce_episodes_batch(None, None, torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.bool,
                                                                                        device=dev))
    assert cpu(e.lane_row_offsets).tolist() == [0, 0, 0, 0] and e.returns.shape == (0,)
    e = reinforce_episodes_batch(None, None, torch.zeros(4, 0, device=dev), torch.zeros(4, 0, dtype=torch.bool,
                                                                                        device=dev))
    assert cpu(e.lane_episode_offsets).tolist() == [0] and cpu(e.ep_offsets).tolist() == [0]


def test_batch_of_one_row():
    """M == 1: one lane with one kept frame, the rest without a row."""
    T, n = 5, 70
    r = make_rollout(T, n, seed=2)
    r["done"][:] = 1
    r["before"][:] = 1
    r["before"][33] = 0
    d = to_dev(r)
    x = expected(r)
    assert x["lay"]["ep_offset"].tolist() == [0, 1] and x["lay"]["ep_lane"].tolist() == [33]
    b = run_ppo(r, d)
    check_layout(b, x["lay"])
    check_rows(b, x)
    assert np.array_equal(cpu(b.returns), x["ret"]) and np.array_equal(cpu(b.episode_return), x["ep"])
    assert float(b.adv_mean) == float(x["adv"][0]) and np.isnan(float(b.adv_std))
    assert np.isnan(cpu(b.advantages)).all()
    rb = reinforce_episodes_batch(d["obs"], d["actions"], d["reward"], d["done"], d["before"])
    assert np.array_equal(cpu(rb.returns), x["G"]) and np.isnan(float(rb.std)) and np.isnan(cpu(rb.advantages)).all()


def test_collect_ppo_steps_end_to_end():
    dev = _dev()
    w = np.load(os.path.join(HERE, "golden", "policy.npz"))
    sd = lambda p: {k[len(p):]: torch.from_numpy(w[k]) for k in w.files if k.startswith(p)}  # noqa: E731
    actor, critic = MlpNet(sd("actor."), device=dev), MlpNet(sd("critic."), device=dev)
    cfg = EnvConfig(randomize_drone=True, randomize_platform=True, auto_reset=True, seed=3)
    n, T = 520, 40
    env = VecDroneEnv(n, device=dev, config=cfg, reward_mode="notebook", max_steps=12)
    twin = VecDroneEnv(n, device=dev, config=cfg, reward_mode="notebook", max_steps=12)
    env.reset()
    twin.reset()
    last_done = np.zeros(n, dtype=np.uint8)
    for call in range(2):
        b = collect_ppo_steps(env, actor, critic, T, seed=9, step=call * T)
        before = cpu((twin.status & abi.DD_ST_DONE) != 0).astype(np.uint8)
        # the lanes that re-spawn in frame 0 are those whose last frame was done
        assert np.array_equal(before, last_done)
        obs, acts, lp, reward, done = twin.policy_rollout(actor, T, seed=9, step=call * T)
        values_rect = critic(obs.reshape(T * n, 15)).reshape(T, n)
        boot = critic(twin.obs)
        torch.cuda.synchronize()
        r = dict(done=cpu(done).astype(np.uint8), before=before, obs=cpu(obs), actions=cpu(acts), log_prob=cpu(lp),
                 reward=cpu(reward), values=cpu(values_rect), bootstrap=cpu(boot))
        last_done = r["done"][T - 1]
        x = expected(r)
        lay = x["lay"]
        E, M = len(lay["ep_lane"]), int(lay["ep_offset"][-1])
        print(f"call {call}: E = {E}, M = {M} of {T * n}, done before {int(before.sum())}")
        assert E > n and M > 0.8 * T * n
        if call == 1:
            assert before.any() and (lay["ep_start"][lay["lane_episode"][:-1][before != 0]] == 1).all()
            assert not np.array_equal(expected(r, before=False)["lay"]["lane_row"], lay["lane_row"])
        check_layout(b, lay)
        check_rows(b, x)
        assert np.array_equal(cpu(b.values), x["values"])
        assert np.array_equal(cpu(b.returns), x["ret"]) and np.array_equal(cpu(b.episode_return), x["ep"])
        check_normalised(cpu(b.advantages), float(b.adv_mean), float(b.adv_std), x["adv"])
    sticky = VecDroneEnv(8, device=dev, config=dataclasses.replace(cfg, auto_reset=False), reward_mode="notebook",
                         max_steps=12)
    with pytest.raises(ValueError, match="collect_ppo"):
        collect_ppo_steps(sticky, actor, critic, T)
