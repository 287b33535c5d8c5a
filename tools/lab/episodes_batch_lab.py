#!/usr/bin/env python
"""Time the every-episode training batch next to the first-episode one (lab).

65,536 lanes x 256 frames of a reward_mode="notebook", auto_reset=True rollout,
once with a randomly initialised actor and once with the fixture actor
(tests/golden/policy.npz); the critic is the fixture's.  On the same buffers,
in the same session:

    ppo_episodes_batch   the whole call: count, the read of E and M, fill,
                         gather, the critic on M rows (+ N bootstrap rows),
                         GAE, normalisation (wall clock, synchronised)
    ppo_batch            the first-episode builder, the same way
    count / fill / gather_f8 / gather_f16 / critic_M_rows / advantages_gae /
    advantages_returns / normalize, and first_* for ppo_batch's stages
                         the stages alone (GPU events; count and plan include
                         their host read: wall clock)

Every line carries its rows M, M / (T * N) and microseconds per million rows.
Medians and spreads over `--reps` runs after `--warmup` runs, one JSON line per
variant.

    python tools/lab/episodes_batch_lab.py [--envs 65536] [--frames 256] [--reps 9] [--out FILE]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "reinforcement-learning-101_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from delivery_drone_amd import EnvConfig, VecDroneEnv, abi, ppo_batch, ppo_episodes_batch  # noqa: E402
from delivery_drone_amd import train_batch as tb  # noqa: E402
from train_batch_lab import nets, timed  # noqa: E402


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

    def emit(rows, **kw):
        kw.update(rows=rows, valid_fraction=round(rows / (T * n), 4), envs=n, frames=T,
                  device=torch.cuda.get_device_name(dev))
        if "us_median" in kw and rows:
            kw["us_per_million_rows"] = round(kw["us_median"] / (rows / 1e6), 1)
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    for name, actor in actors.items():
        env = VecDroneEnv(n, device=dev, reward_mode="notebook", max_steps=T,
                          config=EnvConfig(randomize_drone=True, randomize_platform=True, auto_reset=True, seed=1))
        env.reset()
        before = (env.status & abi.DD_ST_DONE).ne(0).to(torch.uint8)
        obs, acts, lp, reward, done = env.policy_rollout(actor, T, seed=0)
        boot_obs = env.obs.clone()
        w, r = a.warmup, a.reps
        plan = tb._EpisodePlan(done, before)
        first = tb._Plan(done)
        M, M1 = plan.M, first.M
        common = dict(policy=name, episodes=plan.E)
        emit(M, variant="ppo_episodes_batch", **common, **timed(
            lambda: ppo_episodes_batch(obs, acts, lp, reward, done, critic, bootstrap_obs=boot_obs,
                                       done_before=before), w, r, events=False))
        emit(M1, variant="ppo_batch", **common, **timed(
            lambda: ppo_batch(obs, acts, lp, reward, done, critic, bootstrap_obs=boot_obs), w, r, events=False))
        emit(M, variant="count_fill", **common, **timed(lambda: tb._EpisodePlan(done, before), w, r, events=False))
        emit(M1, variant="first_plan", **common, **timed(lambda: tb._Plan(done), w, r, events=False))
        lib, lay = plan.lib, plan.layout
        ws, tot = plan.workspace, torch.empty(2, dtype=torch.int64, device=dev)
        emit(M, variant="count", **common, **timed(lambda: abi.check(lib.dd_episodes_count(
            plan.done.data_ptr(), before.data_ptr(), T, n, 0, lay, tot.data_ptr(), ws.data_ptr(), tb._args.stream_ptr(dev)),
            "count"), w, r))
        emit(M, variant="fill", **common, **timed(lambda: abi.check(lib.dd_episodes_fill(
            plan.done.data_ptr(), before.data_ptr(), T, n, 0, lay, tb._args.stream_ptr(dev)), "fill"), w, r))
        for frames in (8, 16):
            emit(M, variant=f"gather_f{frames}", **common,
                 **timed(lambda: plan.gather(obs, acts, lp, tile_frames=frames), w, r))
            emit(M1, variant=f"first_gather_f{frames}", **common,
                 **timed(lambda: first.gather(obs, acts, lp, tile_frames=frames), w, r))
        states, _, _ = plan.gather(obs, None, None)
        states1, _, _ = first.gather(obs, None, None)
        emit(M, variant="critic_M_rows", **common, **timed(lambda: critic(states), w, r))
        emit(M1, variant="first_critic_M_rows", **common, **timed(lambda: critic(states1), w, r))
        values, values1, boot = critic(states), critic(states1), critic(boot_obs)
        del states, states1
        emit(M, variant="advantages_gae", **common, **timed(
            lambda: plan.advantages(reward, abi.DD_BATCH_GAE, 0.99, 0.95, values=values, bootstrap=boot), w, r))
        emit(M1, variant="first_advantages_gae", **common, **timed(
            lambda: first.advantages(reward, abi.DD_BATCH_GAE, 0.99, 0.95, values=values1, bootstrap=boot), w, r))
        emit(M, variant="advantages_returns", **common,
             **timed(lambda: plan.advantages(reward, abi.DD_BATCH_RETURNS, 0.99), w, r))
        emit(M1, variant="first_advantages_returns", **common,
             **timed(lambda: first.advantages(reward, abi.DD_BATCH_RETURNS, 0.99), w, r))
        raw, _, _ = plan.advantages(reward, abi.DD_BATCH_GAE, 0.99, 0.95, values=values, bootstrap=boot)
        raw1, _, _ = first.advantages(reward, abi.DD_BATCH_GAE, 0.99, 0.95, values=values1, bootstrap=boot)
        emit(M, variant="normalize", **common, **timed(lambda: plan.normalize(raw, True), w, r))
        emit(M1, variant="first_normalize", **common, **timed(lambda: first.normalize(raw1, True), w, r))
        del env, obs, acts, lp, reward, done, plan, first, values, values1, raw, raw1
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
