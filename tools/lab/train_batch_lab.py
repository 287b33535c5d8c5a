#!/usr/bin/env python
"""Time the training-batch stages next to the same batch built with torch (lab).

65,536 lanes x 256 frames of a reward_mode="notebook" rollout, once with a
randomly initialised actor and once with the fixture actor
(tests/golden/policy.npz); the critic is the fixture's.  Per rollout:

    ppo_batch      the whole of delivery_drone_amd.ppo_batch: plan, the read of
                   M, gather, the critic on M rows (+ N bootstrap rows), GAE,
                   normalisation (wall clock around a synchronised call)
    plan / gather_f8 / gather_f16 / critic_M / advantages / normalize
                   the stages alone (GPU events)
    torch_batch    the yardstick, from what the package offered before: the
                   critic over T*N rows, gae() on the rectangle, a cumsum
                   validity mask, a transpose to lane-major, boolean indexing
                   into episode-major order, torch's mean / std

Medians and spreads over `--reps` runs after `--warmup` runs, one JSON line per
variant.  The gather line also reports its algorithmic bytes (valid obs rows
read and written once, done, and the valid actions / log-probs in and out)
and the fraction of 8 TB/s they were moved at.

    python tools/lab/train_batch_lab.py [--envs 65536] [--frames 256] [--reps 9] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "reinforcement-learning-101_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch import nn  # noqa: E402
from delivery_drone_amd import EnvConfig, MlpNet, VecDroneEnv, abi, gae, ppo_batch  # noqa: E402
from delivery_drone_amd import train_batch as tb  # noqa: E402

PEAK = 8.0e12  # bytes per second


def nets(dev):
    w = np.load(os.path.join(REPO, "tests", "golden", "policy.npz"))
    sd = lambda p: {k[len(p):]: torch.from_numpy(w[k]) for k in w.files if k.startswith(p)}  # noqa: E731
    torch.manual_seed(0)
    rand = nn.Sequential(nn.Linear(15, 128), nn.LayerNorm(128), nn.ReLU(), nn.Linear(128, 128), nn.LayerNorm(128),
                         nn.ReLU(), nn.Linear(128, 64), nn.LayerNorm(64), nn.ReLU(), nn.Linear(64, 3))
    return {"random": MlpNet(rand.state_dict(), device=dev), "fixture": MlpNet(sd("actor."), device=dev)}, \
        MlpNet(sd("critic."), device=dev)


def timed(fn, warmup, reps, events=True):
    """Median and spread of fn's time in microseconds."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        if events:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b) * 1e3)
        else:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e6)
    return {"us_median": round(statistics.median(out), 1), "us_min": round(min(out), 1), "us_max": round(max(out), 1)}


def torch_batch(obs, acts, lp, reward, done, critic, boot_obs, gamma=0.99, lam=0.95):
    T, n = done.shape
    values = critic(obs.reshape(T * n, 15)).reshape(T, n)
    boot = critic(boot_obs)
    adv, ret = gae(reward, torch.cat([values, boot[None]], dim=0), done, gamma, lam)
    d = done.to(torch.int32)
    valid = (torch.cumsum(d, dim=0) - d) == 0          # frames up to and including the first done
    mask = valid.t()                                    # [N, T]: boolean indexing walks it lane by lane
    states = obs.transpose(0, 1)[mask]
    actions = torch.stack([(acts >> k) & 1 for k in range(3)], dim=-1).to(torch.float32).transpose(0, 1)[mask]
    old_lp = lp.t()[mask]
    a = adv.t()[mask]
    r = ret.t()[mask]
    a = (a - a.mean()) / (a.std() + 1e-8)
    return states, actions, old_lp, a, r


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--envs", type=int, default=65_536)
    p.add_argument("--frames", type=int, default=256)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=9)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    n, T = a.envs, a.frames
    actors, critic = nets(dev)
    lines = []

    def emit(**kw):
        kw.update(envs=n, frames=T, device=torch.cuda.get_device_name(dev))
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    for name, actor in actors.items():
        env = VecDroneEnv(n, device=dev, reward_mode="notebook", max_steps=T,
                          config=EnvConfig(randomize_drone=True, randomize_platform=True, seed=1))
        env.reset()
        obs, acts, lp, reward, done = env.policy_rollout(actor, T, seed=0)
        boot_obs = env.obs.clone()
        plan = tb._Plan(done)
        M = plan.M
        common = dict(policy=name, rows=M, valid_fraction=round(M / (T * n), 4),
                      ended_fraction=round(float(plan.ended.float().mean()), 4))
        w, r = a.warmup, a.reps
        emit(variant="ppo_batch", **common,
             **timed(lambda: ppo_batch(obs, acts, lp, reward, done, critic, bootstrap_obs=boot_obs), w, r, events=False))
        emit(variant="torch_batch", **common,
             **timed(lambda: torch_batch(obs, acts, lp, reward, done, critic, boot_obs), w, r, events=False))
        emit(variant="plan", **common, **timed(lambda: tb._Plan(done), w, r, events=False))
        gather_bytes = M * (60 + 60) + T * n + M * (1 + 12) + M * (4 + 4)
        for frames in (8, 16):
            t = timed(lambda: plan.gather(obs, acts, lp, tile_frames=frames), w, r)
            emit(variant=f"gather_f{frames}", **common, **t, algorithmic_bytes=gather_bytes,
                 fraction_of_8TBps=round(gather_bytes / (t["us_median"] * 1e-6) / PEAK, 4))
        t = timed(lambda: plan.gather(obs, None, None), w, r)
        emit(variant="gather_obs_only_f8", **common, **t, algorithmic_bytes=M * 120,
             fraction_of_8TBps=round(M * 120 / (t["us_median"] * 1e-6) / PEAK, 4))
        states, _, _ = plan.gather(obs, None, None)
        emit(variant="critic_M_rows", **common, **timed(lambda: critic(states), w, r))
        emit(variant="critic_TN_rows", **common, **timed(lambda: critic(obs.reshape(T * n, 15)), w, r))
        values = critic(states)
        boot = critic(boot_obs)
        emit(variant="advantages_gae", **common,
             **timed(lambda: plan.advantages(reward, abi.DD_BATCH_GAE, 0.99, 0.95, values=values, bootstrap=boot), w, r))
        emit(variant="advantages_returns", **common,
             **timed(lambda: plan.advantages(reward, abi.DD_BATCH_RETURNS, 0.99), w, r))
        raw, _, _ = plan.advantages(reward, abi.DD_BATCH_GAE, 0.99, 0.95, values=values, bootstrap=boot)
        emit(variant="normalize", **common, **timed(lambda: plan.normalize(raw, True), w, r))
        vt = torch.cat([critic(obs.reshape(T * n, 15)).reshape(T, n), boot[None]], dim=0)
        emit(variant="gae_rectangle", **common, **timed(lambda: gae(reward, vt, done, 0.99, 0.95), w, r))
        del env, obs, acts, lp, reward, done, plan, states, values, raw, vt
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
