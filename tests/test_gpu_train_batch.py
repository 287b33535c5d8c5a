"""GPU: delivery_drone_amd.train_batch (csrc/train_batch.hip) against the NumPy
restatement tests/train_batch_ref.py, which test_train_batch_cpu.py pins to
the notebooks' own results.

Base shape T = 37, N = 515: more than two 256-lane blocks and eight 64-lane
gather tiles, N % 4 != 0 (so a frame's rows start on every 16-byte phase), T
no multiple of the 8- or 16-frame tile.  The plan, the gathers, GAE, returns
and episode_return are compared bit for bit.  The normalised values are
compared within  1 ulp_f32(|ref|) + 64 * 2^-53 * max|a| / std : the rounding
to float32, plus the effect of the two double reductions' (mean, squared
deviations) different summation orders, each a tree of depth <= 16 over M <
2^16 rows here with relative error <= 16 * 2^-53 per side on values <=
max|a|, scaled by 1 / std as the output is; computed from the test's own data.

The 2^31-byte boundary is not run at full size: the kernels index rows and
elements in int64 (checked by reading).
"""
import os

import numpy as np
import pytest
import torch

import train_batch_ref as ref
from delivery_drone_amd import EnvConfig, MlpNet, VecDroneEnv, abi, gae
from delivery_drone_amd import collect_ppo, ppo_batch, reinforce_batch
from delivery_drone_amd import train_batch as tb

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
T0, N0 = 37, 515


def _dev():
    return torch.device("cuda", 0)


def make_rollout(T, n, seed=0, lengths=None, ended=None):
    """Rectangular buffers with every frame filled, also past the episodes'
    ends (with further dones there, as an auto-reset env leaves them)."""
    rng = np.random.default_rng(seed)
    if lengths is None:
        lengths = rng.integers(1, T + 1, n)
        ended = np.ones(n, dtype=bool)
        ended[lengths == T] = rng.random(int((lengths == T).sum())) < 0.5
    done = rng.random((T, n)) < 0.08
    for i in range(n):
        done[:lengths[i], i] = False
        if ended[i]:
            done[lengths[i] - 1, i] = True
        else:
            done[:, i] = False
    # distinct per (t, lane, column): a misplaced row or element is visible
    obs = (np.arange(T * n * 15, dtype=np.float64).reshape(T, n, 15) * 0.25 - 1000.0).astype(np.float32)
    reward = rng.normal(0.0, 3.0, (T, n))
    reward[done] = rng.choice([-500.0, 500.0, 557.3], size=int(done.sum()))
    return dict(done=done.astype(np.uint8), obs=obs, actions=rng.integers(0, 8, (T, n)).astype(np.uint8),
                log_prob=rng.normal(-2.0, 1.0, (T, n)).astype(np.float32), reward=reward,
                values=rng.normal(0.0, 40.0, (T, n)).astype(np.float32),
                bootstrap=rng.normal(0.0, 40.0, n).astype(np.float32))


def base_lengths():
    rng = np.random.default_rng(3)
    lengths = rng.integers(1, T0 + 1, N0)
    ended = np.ones(N0, dtype=bool)
    lengths[0], lengths[1], lengths[2] = 1, T0, T0  # done at frame 0, done at frame T-1, never done
    ended[2] = False
    lengths[100:164] = 1    # 64 consecutive lanes of length 1 (across two gather tiles)
    lengths[300:364] = T0   # 64 consecutive lanes of full length
    ended[300:364] = rng.random(64) < 0.5
    ended[(lengths == T0) & (np.arange(N0) > 364)] = False
    return lengths, ended


class TableCritic:
    """A critic whose values the test chooses: row -> value by the row's
    first column (distinct per (t, lane) in make_rollout)."""

    def __init__(self, obs, values, boot_obs, bootstrap, dev):
        keys = np.concatenate([obs[:, :, 0].reshape(-1), boot_obs[:, 0]])
        vals = np.concatenate([values.reshape(-1), bootstrap])
        order = np.argsort(keys)
        self.keys = torch.from_numpy(keys[order]).to(dev)
        self.vals = torch.from_numpy(vals[order]).to(dev)

    def __call__(self, rows):
        idx = torch.searchsorted(self.keys, rows[:, 0].contiguous())
        assert bool((self.keys[idx] == rows[:, 0]).all())
        return self.vals[idx]


def to_dev(r, reward_dtype=torch.float64):
    dev = _dev()
    d = {k: torch.from_numpy(v).to(dev) for k, v in r.items()}
    d["reward"] = d["reward"].to(reward_dtype)
    d["boot_obs"] = torch.from_numpy(boot_obs_of(r)).to(dev)
    return d


def boot_obs_of(r):
    n = r["done"].shape[1]
    return (np.arange(n * 15, dtype=np.float64).reshape(n, 15) * 0.25 + 1.0e6).astype(np.float32)


def expected(r, reward=None, bootstrap=True, gamma=0.99, lam=0.95):
    reward = r["reward"] if reward is None else reward
    ln, off, e = ref.plan(r["done"])
    values = ref.gather(r["values"], ln)
    adv, ret = ref.gae_flat(reward, values, ln, off, e, r["bootstrap"] if bootstrap else None, gamma, lam)
    return dict(length=ln, offset=off, ended=e, states=ref.gather(r["obs"], ln),
                actions=ref.actions_f32(ref.gather(r["actions"], ln)), log_prob=ref.gather(r["log_prob"], ln),
                values=values, adv=adv, ret=ret, G=ref.returns_flat(reward, ln, off, gamma),
                ep=ref.episode_return(reward, ln))


def norm_bound(raw, want):
    raw = raw.astype(np.float64)
    return np.spacing(np.abs(want)).astype(np.float64) + 64 * 2.0 ** -53 * np.abs(raw).max() / raw.std(ddof=1)


def check_normalised(got, mean, std, raw):
    m, s, want = ref.normalize(raw)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bound = norm_bound(raw, want)
    print(f"normalised: max err {err.max():.3e}, min bound {bound.min():.3e}, mean {mean!r} vs {m!r}, std {std!r} vs {s!r}")
    assert (err <= bound).all()
    slack = 64 * 2.0 ** -53 * np.abs(raw).max()
    assert abs(mean - m) <= slack and abs(std - s) <= slack


def cpu(t):
    return None if t is None else t.cpu().numpy()


@pytest.fixture(scope="module")
def base():
    lengths, ended = base_lengths()
    r = make_rollout(T0, N0, seed=1, lengths=lengths, ended=ended)
    return r, expected(r)


def run_ppo(r, d, **kw):
    critic = TableCritic(r["obs"], r["values"], boot_obs_of(r), r["bootstrap"], _dev())
    return ppo_batch(d["obs"], d["actions"], d["log_prob"], d["reward"], d["done"], critic,
                     bootstrap_obs=d["boot_obs"], **kw)


def test_base_shape_covers_the_cases(base):
    r, x = base
    ln, e = x["length"], x["ended"]
    assert ln[0] == 1 and e[0] and ln[1] == T0 and e[1] and ln[2] == T0 and not e[2]
    assert (ln[100:164] == 1).all() and (ln[300:364] == T0).all()
    assert ((ln == T0) & (e == 0)).sum() > 1 and ((ln == T0) & (e == 1)).sum() > 1


@pytest.mark.parametrize("reward_dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_ppo_batch_base_shape(base, reward_dtype):
    r, x = base
    if reward_dtype == torch.float32:
        x = expected(r, reward=r["reward"].astype(np.float32))
    d = to_dev(r, reward_dtype)
    b = run_ppo(r, d)
    assert np.array_equal(cpu(b.lengths), x["length"]) and b.lengths.dtype == torch.int32
    assert np.array_equal(cpu(b.offsets), x["offset"]) and b.offsets.dtype == torch.int64
    assert np.array_equal(cpu(b.ended), x["ended"].astype(bool))
    M = int(x["offset"][-1])
    assert b.states.shape == (M, 15) and b.actions.shape == (M, 3) and b.old_log_probs.shape == (M,)
    assert np.array_equal(cpu(b.states), x["states"])
    assert np.array_equal(cpu(b.actions), x["actions"])
    assert np.array_equal(cpu(b.old_log_probs), x["log_prob"])
    assert np.array_equal(cpu(b.values), x["values"])
    assert np.array_equal(cpu(b.returns), x["ret"])
    assert np.array_equal(cpu(b.episode_return), x["ep"]) and b.episode_return.dtype == torch.float64
    check_normalised(cpu(b.advantages), float(b.adv_mean), float(b.adv_std), x["adv"])
    raw = run_ppo(r, d, normalize=False)
    assert np.array_equal(cpu(raw.advantages), x["adv"])
    assert float(raw.adv_mean) == float(b.adv_mean) and float(raw.adv_std) == float(b.adv_std)
    # two runs of the normalisation: identical bits
    again = run_ppo(r, d)
    assert torch.equal(again.advantages, b.advantages)
    assert torch.equal(again.adv_mean, b.adv_mean) and torch.equal(again.adv_std, b.adv_std)


def test_gather_tile_of_16_frames(base):
    r, x = base
    d = to_dev(r)
    plan = tb._Plan(d["done"])
    for frames in (8, 16):
        s, a, lp = plan.gather(d["obs"], d["actions"], d["log_prob"], tile_frames=frames)
        assert np.array_equal(cpu(s), x["states"]) and np.array_equal(cpu(a), x["actions"])
        assert np.array_equal(cpu(lp), x["log_prob"])


def test_no_row_past_m_is_written(base):
    """The gather and the advantages into larger, pre-filled buffers through
    the C ABI: rows >= M keep their fill."""
    r, x = base
    d = to_dev(r)
    dev = _dev()
    plan = tb._Plan(d["done"])
    M, pad = plan.M, 300
    states = torch.full((M + pad, 15), -7.0, device=dev)
    acts = torch.full((M + pad, 3), -7.0, device=dev)
    lps = torch.full((M + pad,), -7.0, device=dev)
    io = abi.DDBatchGatherIO(d["obs"].data_ptr(), d["actions"].data_ptr(), d["log_prob"].data_ptr(),
                             states.data_ptr(), acts.data_ptr(), lps.data_ptr(), 0, 0)
    import ctypes
    abi.check(abi.lib().dd_batch_gather(ctypes.byref(plan.layout), ctypes.byref(io), T0, N0, None), "gather")
    torch.cuda.synchronize()
    assert np.array_equal(cpu(states[:M]), x["states"]) and bool((states[M:] == -7.0).all())
    assert np.array_equal(cpu(acts[:M]), x["actions"]) and bool((acts[M:] == -7.0).all())
    assert np.array_equal(cpu(lps[:M]), x["log_prob"]) and bool((lps[M:] == -7.0).all())


def test_misaligned_states_and_obs(base):
    """obs and states that start 4, 8 and 12 bytes past a 16-byte boundary."""
    r, x = base
    d = to_dev(r)
    dev = _dev()
    plan = tb._Plan(d["done"])
    import ctypes
    for shift in (1, 2, 3):
        src = torch.empty(T0 * N0 * 15 + 4, device=dev)
        src[shift:shift + T0 * N0 * 15] = d["obs"].reshape(-1)
        dst = torch.full((plan.M * 15 + 8,), -7.0, device=dev)
        o = 4 - shift
        io = abi.DDBatchGatherIO(src.data_ptr() + 4 * shift, None, None, dst.data_ptr() + 4 * o, None, None, 16, 0)
        abi.check(abi.lib().dd_batch_gather(ctypes.byref(plan.layout), ctypes.byref(io), T0, N0, None), "gather")
        torch.cuda.synchronize()
        assert np.array_equal(cpu(dst[o:o + plan.M * 15]).reshape(-1, 15), x["states"])
        assert bool((dst[:o] == -7.0).all()) and bool((dst[o + plan.M * 15:] == -7.0).all())


def test_reinforce_batch_base_shape(base):
    r, x = base
    d = to_dev(r)
    b = reinforce_batch(d["obs"], d["actions"], d["reward"], d["done"])
    assert np.array_equal(cpu(b.lengths), x["length"]) and np.array_equal(cpu(b.offsets), x["offset"])
    assert np.array_equal(cpu(b.states), x["states"]) and np.array_equal(cpu(b.actions), x["actions"])
    assert np.array_equal(cpu(b.returns), x["G"])
    assert np.array_equal(cpu(b.episode_return), x["ep"])
    check_normalised(cpu(b.advantages), float(b.baseline), float(b.std), x["G"])
    raw = reinforce_batch(d["obs"], d["actions"], d["reward"], d["done"], normalize=False)
    assert np.array_equal(cpu(raw.advantages), x["G"]) and float(raw.baseline) == float(b.baseline)
    # float32 rewards, another gamma
    x32 = expected(r, reward=r["reward"].astype(np.float32), gamma=0.9)
    b32 = reinforce_batch(None, None, d["reward"].float(), d["done"], gamma=0.9, normalize=False)
    assert np.array_equal(cpu(b32.returns), x32["G"]) and np.array_equal(cpu(b32.episode_return), x32["ep"])


def test_optional_inputs_absent_in_turn(base):
    r, x = base
    d = to_dev(r)
    critic = TableCritic(r["obs"], r["values"], boot_obs_of(r), r["bootstrap"], _dev())
    b = ppo_batch(d["obs"], None, d["log_prob"], d["reward"], d["done"], critic, bootstrap_obs=d["boot_obs"],
                  normalize=False)
    assert b.actions is None and np.array_equal(cpu(b.old_log_probs), x["log_prob"])
    assert np.array_equal(cpu(b.states), x["states"]) and np.array_equal(cpu(b.advantages), x["adv"])
    b = ppo_batch(d["obs"], d["actions"], None, d["reward"], d["done"], critic, bootstrap_obs=d["boot_obs"],
                  normalize=False)
    assert b.old_log_probs is None and np.array_equal(cpu(b.actions), x["actions"])
    assert np.array_equal(cpu(b.advantages), x["adv"])
    # no bootstrap state: 0, as compute_gae appends
    b = ppo_batch(d["obs"], None, None, d["reward"], d["done"], critic, normalize=False)
    x0 = expected(r, bootstrap=False)
    assert np.array_equal(cpu(b.advantages), x0["adv"]) and np.array_equal(cpu(b.returns), x0["ret"])
    assert not np.array_equal(x0["adv"], x["adv"])
    rb = reinforce_batch(None, d["actions"], d["reward"], d["done"], normalize=False)
    assert rb.states is None and np.array_equal(cpu(rb.actions), x["actions"])
    rb = reinforce_batch(d["obs"], None, d["reward"], d["done"], normalize=False)
    assert rb.actions is None and np.array_equal(cpu(rb.states), x["states"])
    with pytest.raises(ValueError):
        ppo_batch(None, None, None, d["reward"], d["done"], critic)
    with pytest.raises(ValueError, match="contiguous"):
        reinforce_batch(d["obs"].transpose(0, 1).contiguous().transpose(0, 1), None, d["reward"], d["done"])
    with pytest.raises(ValueError, match="shape"):
        reinforce_batch(d["obs"][:, :-1].contiguous(), None, d["reward"], d["done"])
    with pytest.raises(ValueError, match="float32"):
        reinforce_batch(d["obs"].double(), None, d["reward"], d["done"])


def test_gae_equals_the_rectangular_gae_on_valid_rows(base):
    r, x = base
    d = to_dev(r)
    b = run_ppo(r, d, normalize=False, gamma=0.97, lambda_=0.9)
    ln = x["length"]
    values = np.concatenate([ref.scatter(cpu(b.values), ln, T0), r["bootstrap"][None]], axis=0)
    adv, ret = gae(d["reward"].float(), torch.from_numpy(values).to(_dev()), d["done"], gamma=0.97, lambda_=0.9)
    torch.cuda.synchronize()
    assert np.array_equal(ref.gather(cpu(adv), ln), cpu(b.advantages))
    assert np.array_equal(ref.gather(cpu(ret), ln), cpu(b.returns))


@pytest.mark.parametrize("T,n,lengths,ended", [
    (1, 1, [1], [True]),      # M = 1
    (1, 1, [1], [False]),
    (37, 1, [37], [False]),
    (37, 1, [20], [True]),
], ids=["1x1-done", "1x1-open", "37x1-open", "37x1-done"])
def test_single_lane_shapes(T, n, lengths, ended):
    r = make_rollout(T, n, seed=7, lengths=np.asarray(lengths), ended=np.asarray(ended))
    x = expected(r)
    d = to_dev(r)
    b = run_ppo(r, d)
    assert np.array_equal(cpu(b.offsets), x["offset"]) and np.array_equal(cpu(b.ended), x["ended"].astype(bool))
    assert np.array_equal(cpu(b.states), x["states"]) and np.array_equal(cpu(b.actions), x["actions"])
    assert np.array_equal(cpu(b.returns), x["ret"]) and np.array_equal(cpu(b.episode_return), x["ep"])
    rb = reinforce_batch(d["obs"], d["actions"], d["reward"], d["done"])
    assert np.array_equal(cpu(rb.returns), x["G"])
    if x["offset"][-1] == 1:  # M < 2: NaN, as torch.std of one element
        assert np.isnan(float(b.adv_std)) and np.isnan(cpu(b.advantages)).all()
        assert float(b.adv_mean) == float(x["adv"][0])
        assert np.isnan(float(rb.std)) and np.isnan(cpu(rb.advantages)).all()
    else:
        check_normalised(cpu(b.advantages), float(b.adv_mean), float(b.adv_std), x["adv"])
        check_normalised(cpu(rb.advantages), float(rb.baseline), float(rb.std), x["G"])


def test_many_lanes_plan_and_gather():
    """70,001 lanes x 3 frames: more than 65,536 lanes, 274 tile sums to scan
    and 1,094 gather tiles per frame tile, the last one of 49 lanes."""
    T, n = 3, 70001
    rng = np.random.default_rng(5)
    done = (rng.random((T, n)) < 0.4).astype(np.uint8)
    obs = rng.integers(-2 ** 20, 2 ** 20, (T, n, 15)).astype(np.float32)
    actions = rng.integers(0, 8, (T, n)).astype(np.uint8)
    reward = rng.normal(0, 3, (T, n)).astype(np.float32)
    ln, off, e = ref.plan(done)
    dev = _dev()
    b = reinforce_batch(torch.from_numpy(obs).to(dev), torch.from_numpy(actions).to(dev),
                        torch.from_numpy(reward).to(dev), torch.from_numpy(done).to(dev), normalize=False)
    assert np.array_equal(cpu(b.lengths), ln) and np.array_equal(cpu(b.offsets), off)
    assert np.array_equal(cpu(b.ended), e.astype(bool))
    valid = (np.arange(T)[:, None] < ln[None, :])
    assert np.array_equal(cpu(b.states), obs.transpose(1, 0, 2)[valid.T])
    assert np.array_equal(cpu(b.actions), ref.actions_f32(actions.T[valid.T]))
    G = np.zeros((T + 1, n))
    for t in range(T - 1, -1, -1):
        G[t] = np.where(valid[t], reward[t].astype(np.float64) + 0.99 * G[t + 1], 0.0)
    assert np.array_equal(cpu(b.returns), G[:T].T[valid.T].astype(np.float32))


def test_scan_carry_across_scan_tiles():
    """The plan alone at 262,145 lanes x 1 frame: 1,025 tile sums, one more
    than a scan pass holds."""
    n = 256 * 1024 + 1
    done = torch.ones(1, n, dtype=torch.uint8, device=_dev())
    plan = tb._Plan(done)
    assert plan.M == n
    assert torch.equal(plan.offsets, torch.arange(n + 1, device=_dev()))


def test_collect_ppo_end_to_end():
    dev = _dev()
    w = np.load(os.path.join(HERE, "golden", "policy.npz"))
    sd = lambda p: {k[len(p):]: torch.from_numpy(w[k]) for k in w.files if k.startswith(p)}  # noqa: E731
    actor_sd, critic_sd = sd("actor."), sd("critic.")
    if not actor_sd:
        pytest.fail(f"policy.npz keys: {w.files[:8]}")
    actor, critic = MlpNet(actor_sd, device=dev), MlpNet(critic_sd, device=dev)
    cfg = EnvConfig(randomize_drone=True, randomize_platform=True, seed=3)
    n, T = 520, 60
    env = VecDroneEnv(n, device=dev, config=cfg, reward_mode="notebook", max_steps=45)
    b = collect_ppo(env, actor, critic, max_steps=T, seed=9, step=2)
    env2 = VecDroneEnv(n, device=dev, config=cfg, reward_mode="notebook", max_steps=45)
    env2.reset()
    obs, acts, lp, reward, done = env2.policy_rollout(actor, T, seed=9, step=2)
    values_rect = critic(obs.reshape(T * n, 15)).reshape(T, n)
    boot = critic(env2.obs)
    torch.cuda.synchronize()
    r = dict(done=cpu(done).astype(np.uint8), obs=cpu(obs), actions=cpu(acts), log_prob=cpu(lp),
             reward=cpu(reward), values=cpu(values_rect), bootstrap=cpu(boot))
    x = expected(r)
    assert np.array_equal(cpu(b.lengths), x["length"]) and np.array_equal(cpu(b.ended), x["ended"].astype(bool))
    assert 0 < x["ended"].sum()  # some episodes end within the rollout
    assert np.array_equal(cpu(b.states), x["states"]) and np.array_equal(cpu(b.actions), x["actions"])
    assert np.array_equal(cpu(b.old_log_probs), x["log_prob"])
    assert np.array_equal(cpu(b.values), x["values"])
    assert np.array_equal(cpu(b.returns), x["ret"]) and np.array_equal(cpu(b.episode_return), x["ep"])
    check_normalised(cpu(b.advantages), float(b.adv_mean), float(b.adv_std), x["adv"])
