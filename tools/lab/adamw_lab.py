#!/usr/bin/env python
"""Time one PHASE 3 (4 epochs) by ppo_update next to the loop it replaces (lab).

Two variants, same session, same batch, same start weights:

    ppo_update     delivery_drone_amd.ppo_update(num_epochs=4): per epoch
                   ppo_losses, the two MlpNet.backward calls, the two
                   dd_adamw_step launches (with their repack), logs on device
    parent_loop    the loop INTEGRATION.md §3 had before AdamW moved onto the
                   device: per epoch ppo_grads, the 28 `.grad` assignments on
                   torch modules on the same device, two torch.optim.AdamW
                   steps, two state_dict() + MlpNet.load_state_dict (which
                   re-validates on the host: nine blocking reads per network
                   with compute="f16x3")

for compute f32 and f16x3, at --rows rows of the batch (default 2,048, the
notebook's scale) and on the whole every-episode batch of an --envs x --frames
auto-reset rollout.  Wall clock around the 4 epochs with a final synchronize;
medians of --reps runs after --warmup runs.  One JSON line per variant and
size; reported numbers and the ratio parent_loop / ppo_update.

    python tools/lab/adamw_lab.py [--envs 65536] [--frames 256] [--rows 2048] [--reps 7] [--out FILE]
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
from delivery_drone_amd import (AdamW, EnvConfig, MlpNet, VecDroneEnv, collect_ppo_steps, ppo_grads,  # noqa: E402
                                ppo_update)

EPOCHS = 4
LR = {"actor": 3e-4, "critic": 1e-3}  # the training cell's two optimizers


def state_dicts():
    w = np.load(os.path.join(REPO, "tests", "golden", "policy.npz"))
    sd = lambda p: {k[len(p):]: torch.from_numpy(w[k]) for k in w.files if k.startswith(p)}  # noqa: E731
    return sd("actor.network."), sd("critic.network.")


class Module(nn.Module):
    """The notebooks' DroneGamerBoi / DroneTeacherBoi: an nn.Sequential under `.network`."""

    def __init__(self, sd, dev):
        super().__init__()
        k = sd["9.weight"].shape[0]
        layers = [nn.Linear(15, 128), nn.LayerNorm(128), nn.ReLU(), nn.Linear(128, 128), nn.LayerNorm(128), nn.ReLU(),
                  nn.Linear(128, 64), nn.LayerNorm(64), nn.ReLU(), nn.Linear(64, k)]
        if k == 3:
            layers.append(nn.Sigmoid())
        self.network = nn.Sequential(*layers)
        self.network.load_state_dict(sd)
        self.to(dev)


def parent_phase3(actor, critic, policy, critic_module, policy_optimizer, critic_optimizer, five):
    for _ in range(EPOCHS):
        out = ppo_grads(actor, critic, *five, clip_epsilon=0.2, entropy_coef=0.01, value_coef=0.5, max_grad_norm=0.5)
        for module, grads in ((policy, out.actor), (critic_module, out.critic)):
            for k, p in module.network.named_parameters():
                p.grad = grads[k]
        policy_optimizer.step()
        critic_optimizer.step()
        actor.load_state_dict(policy.state_dict())
        critic.load_state_dict(critic_module.state_dict())


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
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    actor_sd, critic_sd = state_dicts()
    lines = []

    def emit(**kw):
        kw.update(epochs=EPOCHS, device=torch.cuda.get_device_name(dev))
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    for compute in ("f32", "f16x3"):
        actor = MlpNet(actor_sd, device=dev, compute=compute)
        critic = MlpNet(critic_sd, device=dev, compute=compute)
        env = VecDroneEnv(a.envs, device=dev, reward_mode="notebook", max_steps=a.frames,
                          config=EnvConfig(randomize_drone=True, randomize_platform=True, auto_reset=True, seed=1))
        env.reset()
        batch = collect_ppo_steps(env, actor, critic, a.frames, seed=0)
        whole = [t.clone() for t in batch[:5]]
        del env, batch
        for rows in (a.rows, int(whole[0].shape[0])):
            five = tuple(t[:rows].contiguous() for t in whole)
            # ours
            actor_opt, critic_opt = AdamW(actor, lr=LR["actor"]), AdamW(critic, lr=LR["critic"])
            fresh = AdamW(actor, lr=LR["actor"]).state_dict()  # an empty optimizer state

            def reset_ours():
                actor.load_state_dict(actor_sd)
                critic.load_state_dict(critic_sd)
                actor_opt.load_state_dict(fresh)
                critic_opt.load_state_dict(dict(fresh, param_groups=[dict(fresh["param_groups"][0], lr=LR["critic"])]))

            ours = timed(lambda: ppo_update(actor, critic, five, actor_opt, critic_opt, num_epochs=EPOCHS,
                                            max_grad_norm=0.5), reset_ours, a.warmup, a.reps)
            refused = actor_opt.status() | critic_opt.status()
            emit(variant="ppo_update", compute=compute, rows=rows, refused=refused, **ours)
            # the parent commit's loop, on networks of its own (no flat buffer)
            p_actor = MlpNet(actor_sd, device=dev, compute=compute)
            p_critic = MlpNet(critic_sd, device=dev, compute=compute)
            policy, critic_module = Module(actor_sd, dev), Module(critic_sd, dev)
            state = {}

            def reset_parent():
                policy.network.load_state_dict(actor_sd)
                critic_module.network.load_state_dict(critic_sd)
                p_actor.load_state_dict(actor_sd)
                p_critic.load_state_dict(critic_sd)
                state["po"] = torch.optim.AdamW(policy.parameters(), lr=LR["actor"])
                state["co"] = torch.optim.AdamW(critic_module.parameters(), lr=LR["critic"])

            theirs = timed(lambda: parent_phase3(p_actor, p_critic, policy, critic_module, state["po"], state["co"],
                                                 five), reset_parent, a.warmup, a.reps)
            emit(variant="parent_loop", compute=compute, rows=rows, **theirs)
            emit(variant="ratio", compute=compute, rows=rows,
                 parent_over_ppo_update=round(theirs["us_median"] / ours["us_median"], 3),
                 ppo_update_not_slower=bool(ours["us_median"] <= theirs["us_median"]))
            del five, p_actor, p_critic, policy, critic_module, state
        del whole
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
