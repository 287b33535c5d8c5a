#!/usr/bin/env python
"""Time ppo_train_population against the launches it replaces.

Same session, the PPO notebook's shape: --frames 300 frames at most on a
reward_mode="notebook" env (max_steps = frames, auto_reset off), --lanes games
per learner, --members learners, f32 networks, --epochs epochs, --minibatch B
rows a step (0: the full batch):

    loop    collect_ppo_population (one population rollout, then ppo_batch per
            member in a host loop), then the update: ppo_update_population (one
            launch) with --minibatch; per member ppo_update(fused=fits_fused(M))
            for the full batch, which the population update cannot run
    fused   ppo_train_population: the env's reset and one persistent launch for
            all learners

The two are interleaved, loop then fused, each on its own learners and env,
which keep training from call to call (a new step offset each time).  Wall
clock per iteration between stream synchronisations (the host loop is what the
fused launch removes), and for the fused side the device time of the launch
itself between two events around the call (which includes the env's reset
launch); medians of --reps iterations after --warmup, with the min-max spread.
One JSON line per variant, then the ratio of the medians and whether both sides
hold the same parameters.

    python tools/ppo_train_point.py [--members 16] [--lanes 6] [--frames 300] [--minibatch 64] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "reinforcement-learning-101_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from delivery_drone_amd import (AdamW, EnvConfig, LearnerPopulation, MlpNet, VecDroneEnv,  # noqa: E402
                                collect_ppo_population, ppo_train_population, ppo_update, ppo_update_population)
from delivery_drone_amd.adamw import fits_fused  # noqa: E402

LR = {"actor": 3e-4, "critic": 1e-3}  # the training cell's two optimizers


def state_dict(name):
    w = np.load(os.path.join(REPO, "tests", "golden", "policy.npz"))
    prefix = name + ".network."
    return {k[len(prefix):]: torch.from_numpy(w[k]) for k in w.files if k.startswith(prefix)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--members", type=int, default=16)
    p.add_argument("--lanes", type=int, default=6)
    p.add_argument("--frames", type=int, default=300)
    p.add_argument("--epochs", type=int, default=4)
    p.add_argument("--minibatch", type=int, default=0)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    sds = {name: state_dict(name) for name in ("actor", "critic")}
    cfg = EnvConfig(randomize_drone=True, randomize_platform=True, seed=3)
    kw = dict(device=dev, config=cfg, reward_mode="notebook", max_steps=a.frames)
    size = a.minibatch or None

    def learner():
        actor, critic = MlpNet(sds["actor"], device=dev), MlpNet(sds["critic"], device=dev)
        return actor, critic, AdamW(actor, lr=LR["actor"]), AdamW(critic, lr=LR["critic"])

    loop_pop = LearnerPopulation([learner() for _ in range(a.members)])
    loop_env = VecDroneEnv(a.members * a.lanes, **kw)
    pop = LearnerPopulation([learner() for _ in range(a.members)])
    env = VecDroneEnv(a.members * a.lanes, **kw)
    times = {"loop": [], "fused": []}
    device_us = []
    rows = 0.0
    for call in range(a.warmup + a.reps):
        step, epoch = call * a.frames, call * a.epochs
        for variant in ("loop", "fused"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if variant == "loop":
                batches = collect_ppo_population(loop_env, loop_pop, a.frames, seed=7, step=step)
                if size is not None:
                    ppo_update_population(loop_pop, batches, num_epochs=a.epochs, minibatch_size=size,
                                          shuffle_epoch=epoch)
                else:
                    for (actor, critic, ao, co), batch in zip(loop_pop, batches):
                        ppo_update(actor, critic, batch, ao, co, num_epochs=a.epochs,
                                   fused=fits_fused(batch.returns.numel()))
            else:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run = ppo_train_population(env, pop, a.frames, seed=7, step=step, num_epochs=a.epochs,
                                           minibatch_size=size, shuffle_epoch=epoch)
                e1.record()
            torch.cuda.synchronize()
            if call >= a.warmup:
                times[variant].append((time.perf_counter() - t0) * 1e6)
                if variant == "fused":
                    device_us.append(e0.elapsed_time(e1) * 1e3)
        rows = float(run.batch_log("rows").mean().item())
    lines = []
    for variant, us in times.items():
        lines.append(dict(variant=variant, members=a.members, lanes=a.lanes, frames=a.frames,
                          epochs=a.epochs, minibatch=a.minibatch, us_median=round(statistics.median(us), 1), us_min=round(min(us), 1),
                          us_max=round(max(us), 1), rows_per_member_last=round(rows, 1), reps=a.reps,
                          device=torch.cuda.get_device_name(dev)))
    lines[1]["device_us_median"] = round(statistics.median(device_us), 1)
    lines[1]["device_us_min"], lines[1]["device_us_max"] = round(min(device_us), 1), round(max(device_us), 1)
    same = all(torch.equal(x[k].params.view(torch.int32), y[k].params.view(torch.int32))
               for x, y in zip(loop_pop, pop) for k in (2, 3))
    lines.append(dict(ratio="loop / fused, per iteration", value=round(lines[0]["us_median"] / lines[1]["us_median"], 2),
                      fused_is_faster=lines[1]["us_max"] < lines[0]["us_min"], same_parameters_after=same))
    for line in lines:
        print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(line) + "\n" for line in lines)


if __name__ == "__main__":
    main()
