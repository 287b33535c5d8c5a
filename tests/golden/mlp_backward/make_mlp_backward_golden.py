#!/usr/bin/env python
"""Generate tests/golden/mlp_backward/grads.npz: the parameter gradients the
REFERENCE notebook's own training step leaves in the two networks on
ppo_loss/losses.npz's 203 rows.

Runs only where the reference checkout exists (/root/reference, or
$RL101_REFERENCE).  ``compute_ppo_losses`` is executed from
Actor_Critic_PPO.ipynb's cell at run time, as make_ppo_loss_golden.py does, on
golden_data.torch_mlp modules built from policy.npz's own weights, with
losses.npz's states, actions, old_log_probs, advantages, returns and
coefficients; then ``total_loss.backward()`` and the training cell's
``clip_grad_norm_(network.parameters(), max_norm=max_grad_norm)`` per network
(max_grad_norm = 0.5, the notebook's).  The file holds data only: every
parameter's .grad before clipping for both networks (``actor.<key>``,
``critic.<key>``), clip_grad_norm_'s returned norms, and max_grad_norm.

    python -B tests/golden/mlp_backward/make_mlp_backward_golden.py [--out DIR]
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
MAX_GRAD_NORM = 0.5


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


def grad_set() -> dict:
    import torch
    from torch.distributions import Bernoulli
    import golden_data as gd
    torch.set_num_threads(1)
    compute_ppo_losses = notebook_function("Actor_Critic_PPO.ipynb", "compute_ppo_losses",
                                           {"torch": torch, "Bernoulli": Bernoulli})
    g = gd.npz(os.path.join("ppo_loss", "losses.npz"))
    _, nets = gd.policy_fixture()
    actor, critic_net = gd.torch_mlp(nets["actor"]), gd.torch_mlp(nets["critic"])

    def critic(x):  # DroneTeacherBoi.forward: [B, 1] -> [B]
        return critic_net(x).squeeze(-1)

    t = {k: torch.from_numpy(g[k].copy()) for k in ("states", "actions", "old_log_probs", "advantages", "returns")}
    out = compute_ppo_losses(actor, critic, t["states"], t["actions"], t["old_log_probs"], t["advantages"],
                             t["returns"], clip_epsilon=float(g["clip_epsilon"]),
                             entropy_coef=float(g["entropy_coef"]), value_coef=float(g["value_coef"]))
    assert float(out["total_loss"].item()) == float(g["total_loss"])  # the same run as losses.npz records
    out["total_loss"].backward()
    arrays = {}
    for tag, net in (("actor", actor), ("critic", critic_net)):
        for k, p in net.named_parameters():
            arrays[f"{tag}.{k}"] = p.grad.detach().numpy().copy()
    # the training cell's two calls; they return the norm before clipping
    arrays["actor_norm"] = np.float64(torch.nn.utils.clip_grad_norm_(actor.parameters(), max_norm=MAX_GRAD_NORM).item())
    arrays["critic_norm"] = np.float64(
        torch.nn.utils.clip_grad_norm_(critic_net.parameters(), max_norm=MAX_GRAD_NORM).item())
    arrays["max_grad_norm"] = np.float64(MAX_GRAD_NORM)
    return arrays


def main():
    out = HERE
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(out, exist_ok=True)
    save_npz(os.path.join(out, "grads.npz"), **grad_set())


if __name__ == "__main__":
    main()
