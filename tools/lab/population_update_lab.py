#!/usr/bin/env python
"""Time ppo_update_population against the sequential fused updates it replaces (lab).

For every P of --members (default 1 2 16 64 128), in one session, on the same
batch per member (the ppo_loss fixture's rows repeated to --rows, default 2,048,
rolled by the member's index), --minibatch 64, --epochs 4, f32 networks:

    sequential  P calls of ppo_update(minibatch_size=B, fused=True), one per
                learner: each lays out its epochs' shuffled copies (one
                shuffle_batch launch per epoch, inside the timing) and runs
                its two-workgroup launch
    population  one ppo_update_population of the P learners: the table's
                upload, one launch of 2 P workgroups that read the batches in
                place, the total_loss kernel

The two are interleaved, sequential then population, each on its own learners,
which keep training from call to call (a new shuffle_epoch each time) as a
sweep's do.  Wall clock per call between stream synchronisations; medians of
--reps calls after --warmup, with the min-max spread.  One JSON line per
variant and P, then the ratio sequential / population and whether the two sets
of learners hold the same parameters afterwards (they must: the same updates).

    python tools/lab/population_update_lab.py [--members 1 2 16 64 128] [--rows 2048] [--minibatch 64]
                                              [--epochs 4] [--reps 5] [--out FILE]
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
from delivery_drone_amd import AdamW, LearnerPopulation, MlpNet, ppo_update, ppo_update_population  # noqa: E402

LR = {"actor": 3e-4, "critic": 1e-3}  # the training cell's two optimizers
COLUMNS = ("states", "actions", "old_log_probs", "advantages", "returns")


def state_dicts():
    w = np.load(os.path.join(REPO, "tests", "golden", "policy.npz"))
    sd = lambda p: {k[len(p):]: torch.from_numpy(w[k]) for k in w.files if k.startswith(p)}  # noqa: E731
    return sd("actor.network."), sd("critic.network.")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--members", type=int, nargs="+", default=[1, 2, 16, 64, 128])
    p.add_argument("--rows", type=int, default=2048)
    p.add_argument("--minibatch", type=int, default=64)
    p.add_argument("--epochs", type=int, default=4)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    g = np.load(os.path.join(REPO, "tests", "golden", "ppo_loss", "losses.npz"))
    actor_sd, critic_sd = state_dicts()

    def batch(member):
        return tuple(torch.as_tensor(np.ascontiguousarray(np.resize(np.roll(g[k], -member, axis=0),
                                                                    (a.rows,) + g[k].shape[1:])), device=dev)
                     for k in COLUMNS)

    def learner():
        actor, critic = MlpNet(actor_sd, device=dev), MlpNet(critic_sd, device=dev)
        return actor, critic, AdamW(actor, lr=LR["actor"]), AdamW(critic, lr=LR["critic"])

    steps = a.epochs * -(-a.rows // a.minibatch)
    lines = []
    for members in a.members:
        batches = [batch(m) for m in range(members)]
        seeds = list(range(7, 7 + members))
        sequential = [learner() for _ in range(members)]
        pop = LearnerPopulation([learner() for _ in range(members)])
        times = {"sequential": [], "population": []}
        for call in range(a.warmup + a.reps):
            kw = dict(num_epochs=a.epochs, minibatch_size=a.minibatch, shuffle_epoch=call * a.epochs)
            for variant in times:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if variant == "sequential":
                    for n, b, seed in zip(sequential, batches, seeds):
                        ppo_update(*n[:2], b, *n[2:], shuffle_seed=seed, fused=True, **kw)
                else:
                    ppo_update_population(pop, batches, shuffle_seed=seeds, **kw)
                torch.cuda.synchronize()
                if call >= a.warmup:
                    times[variant].append((time.perf_counter() - t0) * 1e6)
        mine = []
        for variant, us in times.items():
            mine.append(dict(variant=variant, members=members, rows=a.rows, minibatch=a.minibatch, epochs=a.epochs,
                             optimizer_steps_per_member=steps, us_median=round(statistics.median(us), 1),
                             us_min=round(min(us), 1), us_max=round(max(us), 1), reps=a.reps,
                             device=torch.cuda.get_device_name(dev)))
        same = all(torch.equal(x.params.view(torch.int32), y.params.view(torch.int32))
                   for n, m in zip(sequential, pop) for x, y in zip(n[2:], m[2:]))
        mine.append(dict(ratio="sequential / population", members=members,
                         value=round(mine[0]["us_median"] / mine[1]["us_median"], 2),
                         population_is_faster=mine[1]["us_max"] < mine[0]["us_min"], same_parameters_after=same))
        for line in mine:
            print(json.dumps(line), flush=True)
        lines += mine
        del sequential, pop, batches
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(line) + "\n" for line in lines)


if __name__ == "__main__":
    main()
