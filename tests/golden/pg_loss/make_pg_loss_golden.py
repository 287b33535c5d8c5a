#!/usr/bin/env python
"""Generate tests/golden/pg_loss/pg.npz by running the REFERENCE notebooks' own
training lines over 203 rows of policy.npz.

Runs only where the reference checkout exists (/root/reference, or
$RL101_REFERENCE).  The lines sit inside the training cells, not in functions,
so each cell's source is sliced between two marker lines at run time, dedented
and exec'd in a prepared namespace (no notebook text is kept here):

* Policy_Gradients.ipynb, from ``returns_tensor = torch.tensor(`` through
  ``optimizer.step()``: the baseline, the two normalisations, the loss,
  backward, clip_grad_norm_ and the AdamW step;
* Actor_Critic_Basic.ipynb, from ``values = critic(batch_data['states'])``
  through ``policy_optimizer.step()``: the critic update, then the actor's.

The networks are golden_data.torch_mlp modules built from policy.npz's own
weights (not copied here), the optimizers torch.optim.AdamW(lr=1e-3) as the
notebooks build them.  A forward hook on each network's last Linear retains
that output's gradient, and clip_grad_norm_ is wrapped to keep the norm it
returns.  The file holds data only: the inputs, the losses, the gradients at
the networks' outputs, and, at the element indices ``idx.*`` (every eighth
element of the flat parameter vector and the whole last layer; the full
vectors would not fit the size kept for a fixture), the clipped parameter
gradients and the parameters after the one step.

    python -B tests/golden/pg_loss/make_pg_loss_golden.py [--out DIR]
"""
from __future__ import annotations

import io
import json
import os
import sys
import textwrap
import zipfile

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # tests/
REF = os.environ.get("RL101_REFERENCE", "/root/reference")
ROWS = 203  # six 32-row tiles and a ragged seventh
GAMMA, LR = 0.99, 1e-3


def notebook_lines(notebook: str, first: str, last: str) -> str:
    """The training cell's lines from the one that starts with `first` through
    the one that is `last`, dedented."""
    path = os.path.join(REF, notebook)
    if not os.path.isfile(path):
        raise SystemExit(f"reference not found at {REF}; the fixture is committed, nothing to do")
    for cell in json.load(open(path))["cells"]:
        lines = "".join(cell["source"]).splitlines()
        starts = [i for i, s in enumerate(lines) if s.strip().startswith(first)]
        if cell["cell_type"] != "code" or not starts:
            continue
        ends = [i for i, s in enumerate(lines) if s.strip() == last and i > starts[0]]
        return textwrap.dedent("\n".join(lines[starts[0]:ends[0] + 1]))
    raise SystemExit(f"{notebook}: no line starts with {first!r}")


def save_npz(path: str, **arrays) -> None:
    """A deflated .npz with fixed member dates: regenerates byte for byte."""
    with zipfile.ZipFile(path, "w") as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy")
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def kept_indices(out_dim: int) -> np.ndarray:
    total = 27456 + 65 * out_dim
    return np.union1d(np.arange(0, total, 8), np.arange(27456, total)).astype(np.int64)


def pg_set(seed=31) -> dict:
    import torch
    from torch.distributions import Bernoulli
    import golden_data as gd
    torch.set_num_threads(1)
    reinforce_src = notebook_lines("Policy_Gradients.ipynb", "returns_tensor = torch.tensor(", "optimizer.step()")
    td_src = notebook_lines("Actor_Critic_Basic.ipynb", "values = critic(batch_data['states'])",
                            "policy_optimizer.step()")
    d, nets = gd.policy_fixture()
    rng = np.random.default_rng(seed)
    n_obs = d["obs"].shape[0]
    rows = np.sort(rng.choice(n_obs, ROWS, replace=False)).astype(np.int64)
    states = torch.from_numpy(d["obs"][rows].copy())
    next_states = torch.from_numpy(d["obs"][(rows + 1) % n_obs].copy())
    with torch.no_grad():
        probs0 = gd.torch_mlp(nets["actor"])(states)
    actions = torch.from_numpy((rng.random((ROWS, 3)) < probs0.numpy()).astype(np.float32))
    # discounted returns at the REINFORCE reward's magnitudes, a few terminal -500 / +500 episodes among them
    returns = rng.normal(-40.0, 60.0, ROWS)
    returns[rng.choice(ROWS, 20, replace=False)] += rng.choice([-500.0, 500.0], 20)
    returns = returns.astype(np.float32)
    # one frame's transitions: per-step rewards, one lane in seven ends (timeout penalty or landing)
    dones = (rng.random(ROWS) < 1.0 / 7.0).astype(np.float32)
    rewards = rng.normal(0.0, 3.0, ROWS)
    rewards[dones == 1.0] += rng.choice([-500.0, 500.0, -150.0], int(dones.sum()))
    rewards = rewards.astype(np.float32)

    norms = []
    clip = torch.nn.utils.clip_grad_norm_

    def keeping_clip(*a, **kw):
        norms.append(float(clip(*a, **kw).item()))
        return norms[-1]

    def network(tag, kept):
        net = gd.torch_mlp(nets[tag])

        def hook(module, args, output):  # the critic's second forward runs under no_grad
            if output.requires_grad:
                output.retain_grad()
                kept.append(output)

        net[9].register_forward_hook(hook)
        return net

    def flat(net, what, idx):
        return np.concatenate([(p.grad if what == "grad" else p).detach().numpy().reshape(-1)
                               for p in net.parameters()])[idx]

    idx_a, idx_c = kept_indices(3), kept_indices(1)
    out = dict(rows=rows, states=states.numpy(), next_states=next_states.numpy(), actions=actions.numpy(),
               returns=returns, rewards=rewards, dones=dones, gamma=np.float64(GAMMA), lr=np.float64(LR),
               idx_actor=idx_a, idx_critic=idx_c)
    torch.nn.utils.clip_grad_norm_ = keeping_clip
    try:
        # ---- REINFORCE ----
        kept = []
        policy = network("actor", kept)
        log_probs = Bernoulli(probs=policy(states)).log_prob(actions).sum(dim=1)
        ns = dict(torch=torch, device="cpu", policy=policy, batch_returns=[float(x) for x in returns],
                  batch_log_probs=list(log_probs.unbind(0)),
                  optimizer=torch.optim.AdamW(policy.parameters(), lr=LR, foreach=False, fused=False))
        exec(compile(reinforce_src, "Policy_Gradients.ipynb", "exec"), ns)
        out.update({"reinforce.probs": torch.sigmoid(kept[0]).detach().numpy(),
                    "reinforce.log_probs": log_probs.detach().numpy(),
                    "reinforce.advantages": ns["advantages"].detach().numpy(),
                    "reinforce.baseline": np.float64(ns["baseline"].item()),
                    "reinforce.std": np.float64(ns["returns_tensor"].std().item()),
                    "reinforce.loss": np.float64(ns["loss"].item()),
                    "reinforce.grad_logits": kept[0].grad.numpy(),
                    "reinforce.grad_norm": np.float64(norms.pop()),
                    "reinforce.actor_grad": flat(policy, "grad", idx_a),
                    "reinforce.actor_after": flat(policy, "param", idx_a)})
        # ---- one-step TD actor-critic ----
        kept_a, kept_c = [], []
        policy, critic_net = network("actor", kept_a), network("critic", kept_c)

        def critic(x):  # DroneTeacherBoi.forward: [B, 1] -> [B]
            return critic_net(x).squeeze(-1)

        log_probs = Bernoulli(probs=policy(states)).log_prob(actions).sum(dim=1)
        batch_data = {"states": states, "next_states": next_states, "rewards": torch.from_numpy(rewards),
                      "dones": torch.from_numpy(dones), "log_probs": log_probs}
        critic.parameters = critic_net.parameters
        ns = dict(torch=torch, policy=policy, critic=critic, batch_data=batch_data, bellman_gamma=GAMMA,
                  critic_optimizer=torch.optim.AdamW(critic_net.parameters(), lr=LR, foreach=False, fused=False),
                  policy_optimizer=torch.optim.AdamW(policy.parameters(), lr=LR, foreach=False, fused=False))
        exec(compile(td_src, "Actor_Critic_Basic.ipynb", "exec"), ns)
        critic_norm, actor_norm = norms
        out.update({"td.values": ns["values"].detach().numpy(), "td.next_values": ns["next_values"].numpy(),
                    "td.td_targets": ns["td_targets"].detach().numpy(),
                    "td.td_errors": ns["td_errors"].detach().numpy(),
                    "td.critic_loss": np.float64(ns["critic_loss"].item()),
                    "td.value_reg": np.float64(ns["value_reg"].item()),
                    "td.grad_values": kept_c[0].grad.squeeze(-1).numpy(),
                    "td.critic_grad_norm": np.float64(critic_norm),
                    "td.critic_grad": flat(critic_net, "grad", idx_c),
                    "td.critic_after": flat(critic_net, "param", idx_c),
                    "td.probs": torch.sigmoid(kept_a[0]).detach().numpy(),
                    "td.log_probs": log_probs.detach().numpy(),
                    "td.actor_loss": np.float64(ns["actor_loss"].item()),
                    "td.grad_logits": kept_a[0].grad.numpy(),
                    "td.actor_grad_norm": np.float64(actor_norm),
                    "td.actor_grad": flat(policy, "grad", idx_a),
                    "td.actor_after": flat(policy, "param", idx_a)})
    finally:
        torch.nn.utils.clip_grad_norm_ = clip
    return out


def main():
    out = HERE
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(out, exist_ok=True)
    save_npz(os.path.join(out, "pg.npz"), **pg_set())


if __name__ == "__main__":
    main()
