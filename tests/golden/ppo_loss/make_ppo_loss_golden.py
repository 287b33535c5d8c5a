#!/usr/bin/env python
"""Generate tests/golden/ppo_loss/losses.npz by running the REFERENCE
notebook's own compute_ppo_losses over 203 rows of policy.npz.

Runs only where the reference checkout exists (/root/reference, or
$RL101_REFERENCE).  ``compute_ppo_losses`` is executed from
Actor_Critic_PPO.ipynb's cell at run time, as make_train_batch_golden.py runs
``compute_gae``.  The actor and critic are golden_data.torch_mlp modules built
from policy.npz's own weights (not copied here); a forward hook on each
network's last Linear retains that output's gradient, so after
``total_loss.backward()`` the file records what autograd leaves at the actor's
pre-Sigmoid logits and at the critic's value.  The file holds data only: the
inputs, the notebook's scalars and ratio statistics, its per-row
probabilities, values and new_log_probs, and the two gradients.

    python -B tests/golden/ppo_loss/make_ppo_loss_golden.py [--out DIR]
"""
from __future__ import annotations

import io
import json
import os
import sys
import zipfile

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # tests/
REF = os.environ.get("RL101_REFERENCE", "/root/reference")
ROWS = 203  # six 32-row tiles and a ragged seventh
CLIP, ENT_COEF, VAL_COEF = 0.2, 0.01, 0.5


def notebook_function(notebook: str, name: str, ns: dict):
    path = os.path.join(REF, notebook)
    if not os.path.isfile(path):
        raise SystemExit(f"reference not found at {REF}; the fixture is committed, nothing to do")
    for cell in json.load(open(path))["cells"]:
        src = "".join(cell["source"])
        if cell["cell_type"] == "code" and f"def {name}" in src:
            exec(compile(src, notebook, "exec"), ns)
    return ns[name]


def save_npz(path: str, **arrays) -> None:
    """A deflated .npz with fixed member dates: regenerates byte for byte."""
    with zipfile.ZipFile(path, "w") as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy")
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def check_conditions(ratio, adv, clip=CLIP) -> None:
    """What makes clipped_frac and the gradient's selection exact matters of
    fact, not of rounding (tests/test_ppo_loss_cpu.py re-checks them)."""
    r, A = ratio.astype(np.float64), adv.astype(np.float64)
    lo, hi = 1.0 - clip, 1.0 + clip
    assert np.all(np.abs(r / lo - 1.0) > 1e-3) and np.all(np.abs(r / hi - 1.0) > 1e-3)
    inside = (r >= lo) & (r <= hi)
    gap = np.abs(r * A - np.clip(r, lo, hi) * A)
    assert np.all((gap >= 1e-4 * np.abs(A)) | inside)
    for side in (r < lo, r > hi):
        for sign in (A > 0, A < 0):
            assert int((side & sign).sum()) >= 10
    assert int((r == 1.0).sum()) >= 8 and int((A == 0).sum()) >= 3
    assert ((A == 0) & ~inside).any() and ((A == 0) & inside).any()


def loss_set(seed=23) -> dict:
    import torch
    from torch.distributions import Bernoulli
    import golden_data as gd
    torch.set_num_threads(1)
    compute_ppo_losses = notebook_function("Actor_Critic_PPO.ipynb", "compute_ppo_losses",
                                           {"torch": torch, "Bernoulli": Bernoulli})
    d, nets = gd.policy_fixture()
    actor, critic_net = gd.torch_mlp(nets["actor"]), gd.torch_mlp(nets["critic"])
    rng = np.random.default_rng(seed)
    rows = np.sort(rng.choice(d["obs"].shape[0], ROWS, replace=False)).astype(np.int64)
    states = torch.from_numpy(d["obs"][rows].copy())

    kept = {}

    def keep(tag):
        def hook(module, args, output):
            output.retain_grad()
            kept[tag] = output
        return hook

    def critic(x):  # DroneTeacherBoi.forward: [B, 1] -> [B]
        return critic_net(x).squeeze(-1)

    with torch.no_grad():
        probs0 = actor(states)
        values0 = critic(states)
        actions = torch.from_numpy((rng.random((ROWS, 3)) < probs0.numpy()).astype(np.float32))
        lp0 = Bernoulli(probs=torch.clamp(probs0, 1e-8, 1 - 1e-8)).log_prob(actions).sum(dim=1)

    # old_log_probs = the notebook actor's log_prob + offsets over about +-0.6 (ratio 0.55 .. 1.82): both
    # clip sides with both advantage signs; rows 0-15 offset exactly 0 (ratio == 1)
    raw = rng.normal(0.0, 1.0, ROWS).astype(np.float32)
    adv = torch.from_numpy(raw)
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    adv[16:22] = 0.0  # A == 0: min's tie, inside the range and outside it
    lo, hi = 1.0 - CLIP, 1.0 + CLIP
    offset = np.zeros(ROWS, dtype=np.float32)
    for i in range(16, ROWS):
        while True:
            off = np.float32(rng.uniform(-0.6, 0.6))
            r = float(np.exp(np.float64(lp0[i].item() - np.float32(lp0[i].item() + off))))
            if abs(r / lo - 1.0) > 2e-3 and abs(r / hi - 1.0) > 2e-3:
                break
        offset[i] = off
    offset[16:22] = (0.05, -0.11, 0.02, 0.45, -0.4, 0.3)  # the A == 0 rows: three inside the range, three outside
    old_lp = (lp0 + torch.from_numpy(offset)).to(torch.float32)
    # returns at the shaped reward's magnitudes: around the critic's values (|v| up to ~850), terminal
    # rewards of -500 / +500 and more on some rows
    ret = values0.numpy().astype(np.float64) + rng.normal(0.0, 30.0, ROWS)
    ret[rng.choice(ROWS, 24, replace=False)] += rng.choice([-500.0, 500.0, 873.21], 24)
    returns = torch.from_numpy(ret.astype(np.float32))

    actor[9].register_forward_hook(keep("logits"))
    critic_net[9].register_forward_hook(keep("value"))
    actor.register_forward_hook(lambda module, args, output: kept.__setitem__("probs", output))
    out = compute_ppo_losses(actor, critic, states, actions, old_lp, adv.detach(), returns.detach(),
                             clip_epsilon=CLIP, entropy_coef=ENT_COEF, value_coef=VAL_COEF)
    out["total_loss"].backward()
    with torch.no_grad():
        probs = kept["probs"].detach()
        dist = Bernoulli(probs=torch.clamp(probs, 1e-8, 1 - 1e-8))  # the cell's own lines
        new_lp = dist.log_prob(actions).sum(dim=1)
        ratio = torch.exp(new_lp - old_lp)
    check_conditions(ratio.numpy(), adv.numpy())
    stats = out["ratio_stats"]
    grad_logits, grad_values = kept["logits"].grad.numpy(), kept["value"].grad.squeeze(-1).numpy()
    values = kept["value"].detach().squeeze(-1).numpy()
    # once more without the entropy bonus: the rows the clip cuts off then carry exact zeros
    bare = compute_ppo_losses(actor, critic, states, actions, old_lp, adv.detach(), returns.detach(),
                              clip_epsilon=CLIP, entropy_coef=0.0, value_coef=VAL_COEF)
    bare["total_loss"].backward()
    return dict(rows=rows, states=states.numpy(), actions=actions.numpy(), old_log_probs=old_lp.numpy(),
                advantages=adv.numpy(), returns=returns.numpy(),
                clip_epsilon=np.float64(CLIP), entropy_coef=np.float64(ENT_COEF), value_coef=np.float64(VAL_COEF),
                probs=probs.numpy(), values=values,
                new_log_probs=new_lp.numpy(), ratio=ratio.numpy(),
                total_loss=np.float64(out["total_loss"].item()), policy_loss=np.float64(out["policy_loss"].item()),
                value_loss=np.float64(out["value_loss"].item()), entropy=np.float64(out["entropy"].item()),
                ratio_mean=np.float64(stats["mean"]), ratio_min=np.float64(stats["min"]),
                ratio_max=np.float64(stats["max"]), ratio_std=np.float64(stats["std"]),
                clipped_frac=np.float64(stats["clipped_frac"]),
                grad_logits=grad_logits, grad_values=grad_values,
                total_loss_no_entropy=np.float64(bare["total_loss"].item()),
                grad_logits_no_entropy=kept["logits"].grad.numpy())


def main():
    out = HERE
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(out, exist_ok=True)
    save_npz(os.path.join(out, "losses.npz"), **loss_set())


if __name__ == "__main__":
    main()
