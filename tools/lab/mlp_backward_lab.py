#!/usr/bin/env python
"""Time the networks' backward pass next to torch autograd and our own forward (lab).

The ``ppo_episodes_batch`` of a 65,536-lane x 256-frame auto-reset rollout with
the fixture actor and critic (tests/golden/policy.npz).  GPU events around:

    ppo_grads          delivery_drone_amd.ppo_grads end to end (ppo_losses with
                       grads=True and the two MlpNet.backward calls), f32 and f16x3
    mlp_backward       dd_mlp_backward alone, actor and critic (float32 whatever
                       the forward's compute)
    evaluate_actions   MlpNet.evaluate_actions on the same rows, f32 and f16x3:
                       the MFMA yardstick (the backward with its recomputed
                       forward is about three forwards' worth of FLOPs)
    torch_step         the path ppo_grads replaces: compute_ppo_losses' lines on
                       torch modules with the same weights on the same device,
                       total_loss.backward() and the two clip_grad_norm_ calls.
                       Autograd keeps every activation, so the M rows go through
                       in chunks of --torch-chunk rows whose gradients accumulate
                       (each chunk's loss scaled by its share of the rows); the
                       figure is the sum over the chunks.

Medians and spreads over ``--reps`` runs after ``--warmup`` runs, one JSON line
per variant, each with its time per million rows.  Reported numbers, not pass
criteria.

    python tools/lab/mlp_backward_lab.py [--envs 65536] [--frames 256] [--reps 7] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "reinforcement-learning-101_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch import nn  # noqa: E402
from torch.distributions import Bernoulli  # noqa: E402
from delivery_drone_amd import EnvConfig, MlpNet, VecDroneEnv, collect_ppo_steps, ppo_grads, ppo_losses  # noqa: E402


def state_dicts():
    w = np.load(os.path.join(REPO, "tests", "golden", "policy.npz"))
    sd = lambda p: {k[len(p):]: torch.from_numpy(w[k]) for k in w.files if k.startswith(p)}  # noqa: E731
    return sd("actor.network."), sd("critic.network.")


def torch_net(sd, dev):
    k = sd["9.weight"].shape[0]
    layers = [nn.Linear(15, 128), nn.LayerNorm(128), nn.ReLU(), nn.Linear(128, 128), nn.LayerNorm(128), nn.ReLU(),
              nn.Linear(128, 64), nn.LayerNorm(64), nn.ReLU(), nn.Linear(64, k)]
    if k == 3:
        layers.append(nn.Sigmoid())
    net = nn.Sequential(*layers)
    net.load_state_dict(sd)
    return net.to(dev).train()


def torch_total_loss(policy, critic, states, actions, old_log_probs, advantages, returns, clip_epsilon=0.2,
                     entropy_coef=0.01, value_coef=0.5):
    """compute_ppo_losses' lines up to total_loss."""
    action_probs = torch.clamp(policy(states), 1e-8, 1 - 1e-8)
    dist = Bernoulli(probs=action_probs)
    new_log_probs = dist.log_prob(actions).sum(dim=1)
    entropy = dist.entropy().mean()
    ratio = torch.exp(new_log_probs - old_log_probs)
    surr1 = ratio * advantages
    surr2 = torch.clamp(ratio, 1 - clip_epsilon, 1 + clip_epsilon) * advantages
    policy_loss = -torch.min(surr1, surr2).mean()
    values = critic(states).squeeze(-1)
    value_loss = ((values - returns) ** 2).mean()
    return policy_loss + value_coef * value_loss - entropy_coef * entropy


def torch_step(policy, critic, five, chunk, max_grad_norm=0.5):
    m = five[0].shape[0]
    policy.zero_grad(set_to_none=True)
    critic.zero_grad(set_to_none=True)
    for first in range(0, m, chunk):
        part = [t[first:first + chunk] for t in five]
        (torch_total_loss(policy, critic, *part) * (part[0].shape[0] / m)).backward()
    torch.nn.utils.clip_grad_norm_(policy.parameters(), max_norm=max_grad_norm)
    torch.nn.utils.clip_grad_norm_(critic.parameters(), max_norm=max_grad_norm)


def timed(fn, warmup, reps):
    """Median and spread of fn's GPU time in microseconds."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return {"us_median": round(statistics.median(out), 1), "us_min": round(min(out), 1), "us_max": round(max(out), 1)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--envs", type=int, default=65_536)
    p.add_argument("--frames", type=int, default=256)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--torch-chunk", type=int, default=1 << 21)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    n, T = a.envs, a.frames
    actor_sd, critic_sd = state_dicts()
    lines = []

    def emit(**kw):
        kw["us_per_million_rows"] = round(kw["us_median"] / (kw["rows"] / 1e6), 2)
        kw.update(envs=n, frames=T, device=torch.cuda.get_device_name(dev))
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    w, r = a.warmup, a.reps
    for compute in ("f32", "f16x3"):
        actor = MlpNet(actor_sd, device=dev, compute=compute)
        critic = MlpNet(critic_sd, device=dev, compute=compute)
        env = VecDroneEnv(n, device=dev, reward_mode="notebook", max_steps=T,
                          config=EnvConfig(randomize_drone=True, randomize_platform=True, auto_reset=True, seed=1))
        env.reset()
        batch = collect_ppo_steps(env, actor, critic, T, seed=0)
        states, actions, old, adv, ret = batch[:5]
        M = int(states.shape[0])
        # a learner some epochs on: the old log-probs a little off the current policy's
        old = old + 0.3 * torch.randn(M, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
        common = dict(compute=compute, rows=M)
        lp, ent, probs = actor.evaluate_actions(states, actions, probs=True)
        emit(variant="evaluate_actions", **common,
             **timed(lambda: actor.evaluate_actions(states, actions, probs=True, log_prob_out=lp, entropy_out=ent), w, r))
        emit(variant="ppo_losses_grads", **common,
             **timed(lambda: ppo_losses(actor, critic, states, actions, old, adv, ret, grads=True), w, r))
        emit(variant="ppo_grads", **common,
             **timed(lambda: ppo_grads(actor, critic, states, actions, old, adv, ret, max_grad_norm=0.5), w, r))
        if compute == "f32":  # the backward is float32 either way, torch too: once
            heads = ppo_losses(actor, critic, states, actions, old, adv, ret, grads=True)
            for tag, net, head in (("actor", actor, heads.grad_logits), ("critic", critic, heads.grad_values)):
                flat = torch.empty(net.grad_numel(), device=dev)
                emit(variant="mlp_backward_" + tag, compute="f32", rows=M,
                     **timed(lambda: net.backward(states, head, max_norm=0.5, out=flat), w, r))
            del heads
            t_actor, t_critic = torch_net(actor_sd, dev), torch_net(critic_sd, dev)
            five = [states, actions, old, adv, ret]
            emit(variant="torch_step", compute="torch_f32", rows=M, torch_chunk=a.torch_chunk,
                 **timed(lambda: torch_step(t_actor, t_critic, five, a.torch_chunk), 1, max(3, r // 2)))
            del t_actor, t_critic, five
        del env, batch, states, actions, old, adv, ret, lp, ent, probs
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
