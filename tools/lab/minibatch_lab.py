#!/usr/bin/env python
"""Time the device-side shuffle and a minibatch epoch of ppo_update (lab).

Same session, same batch, at --rows rows (default 2,048, the notebook's scale)
and on the whole every-episode batch of an --envs x --frames auto-reset
rollout:

    shuffle_batch   one epoch's shuffle of the five tensors (dd_shuffle_rows,
                    one launch, into buffers allocated once): algorithmic
                    bytes per second (every column read and written once, the
                    indices written: 172 bytes per row)
    torch_shuffle   the path it replaces: torch.randperm on the device and
                    index_select of the five tensors
    epoch_full      ppo_update(num_epochs=1), the full-batch epoch
    epoch_minibatch ppo_update(num_epochs=1, minibatch_size=--minibatch)
                    (default 65,536), shuffle included

Wall clock around each call with a final synchronize; medians of --reps runs
after --warmup runs, with the min-max spread.  One JSON line per variant and
size, then the ratios: torch_shuffle / shuffle_batch with the condition
"shuffle_batch is not slower" (its fastest run no slower than torch's slowest
counts as a tie: both variants' own min-max spread), shuffle_batch as a share
of epoch_full, epoch_minibatch / epoch_full.

    python tools/lab/minibatch_lab.py [--envs 65536] [--frames 256] [--rows 2048] [--reps 7] [--out FILE]
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
from delivery_drone_amd import (AdamW, EnvConfig, MlpNet, VecDroneEnv, collect_ppo_steps, ppo_update,  # noqa: E402
                                shuffle_batch)

LR = {"actor": 3e-4, "critic": 1e-3}  # the training cell's two optimizers
ROW_BYTES = 2 * (60 + 12 + 4 + 4 + 4) + 4


def state_dicts():
    w = np.load(os.path.join(REPO, "tests", "golden", "policy.npz"))
    sd = lambda p: {k[len(p):]: torch.from_numpy(w[k]) for k in w.files if k.startswith(p)}  # noqa: E731
    return sd("actor.network."), sd("critic.network.")


def timed(fn, reset, warmup, reps):
    """Median and spread of fn's wall time in microseconds, each run from `reset`'s state."""
    out = []
    for i in range(warmup + reps):
        reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e6)
    return {"us_median": round(statistics.median(out), 1), "us_min": round(min(out), 1), "us_max": round(max(out), 1)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--envs", type=int, default=65_536)
    p.add_argument("--frames", type=int, default=256)
    p.add_argument("--rows", type=int, default=2048)
    p.add_argument("--minibatch", type=int, default=65_536)
    p.add_argument("--compute", default="f32", choices=["f32", "f16x3"])
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    actor_sd, critic_sd = state_dicts()
    lines = []

    def emit(**kw):
        kw.update(device=torch.cuda.get_device_name(dev))
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    actor = MlpNet(actor_sd, device=dev, compute=a.compute)
    critic = MlpNet(critic_sd, device=dev, compute=a.compute)
    env = VecDroneEnv(a.envs, device=dev, reward_mode="notebook", max_steps=a.frames,
                      config=EnvConfig(randomize_drone=True, randomize_platform=True, auto_reset=True, seed=1))
    env.reset()
    batch = collect_ppo_steps(env, actor, critic, a.frames, seed=0)
    whole = [t.clone() for t in batch[:5]]
    del env, batch
    for rows in (a.rows, int(whole[0].shape[0])):
        five = tuple(t[:rows].contiguous() for t in whole)
        epoch = {"e": 0}

        def next_epoch():
            epoch["e"] += 1

        # the shuffle alone, into buffers allocated once, a new key every run
        buffers = {"out": shuffle_batch(five, seed=7, epoch=0)}

        def ours_shuffle():
            buffers["out"] = shuffle_batch(five, seed=7, epoch=epoch["e"], out=buffers["out"])

        ours = timed(ours_shuffle, next_epoch, a.warmup, a.reps)
        emit(variant="shuffle_batch", rows=rows, bytes_per_row=ROW_BYTES,
             tb_per_s=round(rows * ROW_BYTES / ours["us_median"] / 1e6, 4), **ours)
        del buffers

        def torch_shuffle():
            perm = torch.randperm(rows, device=dev)
            return [t.index_select(0, perm) for t in five]

        theirs = timed(torch_shuffle, next_epoch, a.warmup, a.reps)
        emit(variant="torch_shuffle", rows=rows, **theirs)

        # one epoch of ppo_update, full batch and in minibatches
        actor_opt, critic_opt = AdamW(actor, lr=LR["actor"]), AdamW(critic, lr=LR["critic"])
        fresh = AdamW(actor, lr=LR["actor"]).state_dict()  # an empty optimizer state

        def reset_nets():
            next_epoch()
            actor.load_state_dict(actor_sd)
            critic.load_state_dict(critic_sd)
            actor_opt.load_state_dict(fresh)
            critic_opt.load_state_dict(dict(fresh, param_groups=[dict(fresh["param_groups"][0], lr=LR["critic"])]))

        full = timed(lambda: ppo_update(actor, critic, five, actor_opt, critic_opt, num_epochs=1, max_grad_norm=0.5),
                     reset_nets, a.warmup, a.reps)
        emit(variant="epoch_full", compute=a.compute, rows=rows, **full)
        size = min(a.minibatch, rows)
        mini = timed(lambda: ppo_update(actor, critic, five, actor_opt, critic_opt, num_epochs=1, max_grad_norm=0.5,
                                        minibatch_size=size, shuffle_seed=7, shuffle_epoch=epoch["e"]),
                     reset_nets, a.warmup, a.reps)
        emit(variant="epoch_minibatch", compute=a.compute, rows=rows, minibatch_size=size, steps=-(-rows // size),
             refused=actor_opt.status() | critic_opt.status(), **mini)
        emit(variant="ratio", compute=a.compute, rows=rows,
             torch_over_shuffle_batch=round(theirs["us_median"] / ours["us_median"], 3),
             shuffle_not_slower=bool(ours["us_median"] <= theirs["us_median"]),
             shuffle_tie_within_spread=bool(ours["us_median"] > theirs["us_median"]
                                            and ours["us_min"] <= theirs["us_max"]),
             shuffle_share_of_epoch_full=round(ours["us_median"] / full["us_median"], 5),
             minibatch_over_full_epoch=round(mini["us_median"] / full["us_median"], 3))
        del five, actor_opt, critic_opt
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
