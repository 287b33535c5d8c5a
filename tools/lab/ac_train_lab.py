#!/usr/bin/env python
"""Time actor_critic_train_population against the loop of launches it replaces (lab).

Same session, the notebook's shape: --frames 300 frames an episode on a
reward_mode="notebook" env (max_steps = frames, auto_reset on), --lanes lanes
per learner, --members learners, f32 networks:

    loop    per learner and frame: MlpNet.act, env.step, actor_critic_update on
            the learner's own env (about 25 launches), the learners one after
            the other on one stream
    fused   actor_critic_train_population: one persistent launch for all
            learners and frames

The two are interleaved, loop then fused, each on its own learners and envs,
which keep training from call to call (a new step offset each time).  Wall
clock per call between stream synchronisations; medians of --reps calls after
--warmup, with the min-max spread, and the time per frame.  The loop's cost per
frame does not depend on the frame, and at 128 learners an episode of it takes
minutes: --loop-frames runs it for fewer frames (its per-frame figure is what is
compared; the line says how many it ran).  One JSON line per variant, then the
ratio of the per-frame medians.

    python tools/lab/ac_train_lab.py [--members 16] [--lanes 64] [--frames 300] [--loop-frames N] [--out FILE]
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
from delivery_drone_amd import (AdamW, EnvConfig, LearnerPopulation, MlpNet, VecDroneEnv,  # noqa: E402
                                actor_critic_train_population, actor_critic_update)

LR = {"actor": 3e-4, "critic": 1e-3}  # the training cell's two optimizers


def state_dicts():
    w = np.load(os.path.join(REPO, "tests", "golden", "policy.npz"))
    sd = lambda p: {k[len(p):]: torch.from_numpy(w[k]) for k in w.files if k.startswith(p)}  # noqa: E731
    return sd("actor.network."), sd("critic.network.")


def loop_episode(envs, learners, frames, seed, step):
    """The loop of launches: every learner on its own env, one after the other."""
    for env, (actor, critic, a_opt, c_opt) in zip(envs, learners):
        obs = env.obs
        done_prev = torch.zeros(env.num_envs, dtype=torch.bool, device=env.device)
        for t in range(frames):
            state = obs.clone()
            actions, _ = actor.act(state, seed=seed, step=step + t, env_id_base=env.env_id_base)
            obs, reward, done, _ = env.step(actions)
            actor_critic_update(actor, critic, state, actions, reward, obs, done, a_opt, c_opt, active=~done_prev)
            done_prev = done.clone()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--members", type=int, default=16)
    p.add_argument("--lanes", type=int, default=64)
    p.add_argument("--frames", type=int, default=300)
    p.add_argument("--loop-frames", type=int, default=None)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    loop_frames = a.loop_frames or a.frames
    dev = torch.device("cuda", 0)
    actor_sd, critic_sd = state_dicts()
    cfg = EnvConfig(randomize_drone=True, randomize_platform=True, auto_reset=True, seed=3)
    kw = dict(device=dev, config=cfg, reward_mode="notebook", max_steps=a.frames)

    def learner():
        actor, critic = MlpNet(actor_sd, device=dev), MlpNet(critic_sd, device=dev)
        return actor, critic, AdamW(actor, lr=LR["actor"]), AdamW(critic, lr=LR["critic"])

    loop_learners = [learner() for _ in range(a.members)]
    loop_envs = [VecDroneEnv(a.lanes, env_id_base=g * a.lanes, **kw) for g in range(a.members)]
    pop = LearnerPopulation([learner() for _ in range(a.members)])
    env = VecDroneEnv(a.members * a.lanes, **kw)
    times = {"loop": [], "fused": []}
    for call in range(a.warmup + a.reps):
        for variant in ("loop", "fused"):
            for e in (loop_envs if variant == "loop" else [env]):
                e.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if variant == "loop":
                loop_episode(loop_envs, loop_learners, loop_frames, 7, call * a.frames)
            else:
                actor_critic_train_population(env, pop, a.frames, seed=7, step=call * a.frames)
            torch.cuda.synchronize()
            if call >= a.warmup:
                times[variant].append((time.perf_counter() - t0) * 1e6)
    lines = []
    for variant, us in times.items():
        ran = loop_frames if variant == "loop" else a.frames
        lines.append(dict(variant=variant, members=a.members, lanes=a.lanes, frames_run=ran,
                          us_median=round(statistics.median(us), 1), us_min=round(min(us), 1),
                          us_max=round(max(us), 1), us_per_frame=round(statistics.median(us) / ran, 2),
                          us_per_frame_min=round(min(us) / ran, 2), us_per_frame_max=round(max(us) / ran, 2),
                          reps=a.reps, device=torch.cuda.get_device_name(dev)))
    same = None
    if loop_frames == a.frames:  # the same work on both sides: the same parameters after it
        same = all(torch.equal(x[k].params.view(torch.int32), y[k].params.view(torch.int32))
                   for x, y in zip(loop_learners, pop) for k in (2, 3))
    lines.append(dict(ratio="loop / fused, per frame",
                      value=round(lines[0]["us_per_frame"] / lines[1]["us_per_frame"], 2),
                      fused_is_faster=lines[1]["us_per_frame_max"] < lines[0]["us_per_frame_min"],
                      same_parameters_after=same))
    for line in lines:
        print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(line) + "\n" for line in lines)


if __name__ == "__main__":
    main()
