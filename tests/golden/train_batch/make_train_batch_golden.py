#!/usr/bin/env python
"""Generate tests/golden/train_batch/ragged.npz by running the REFERENCE
notebooks' own functions over a ragged batch of episodes.

Runs only where the reference checkout exists (/root/reference, or
$RL101_REFERENCE).  ``compute_gae`` (Actor_Critic_PPO.ipynb) and
``compute_returns`` (Policy_Gradients.ipynb) are executed from the notebooks'
cells at run time, as make_golden.py's gae_set does; the batch lines of the two
training cells (returns = advantages + values, torch.cat, the normalisation,
the baseline) are applied to their outputs with torch float32 CPU tensors.
The file holds data only: the rectangular inputs and the notebooks' results in
episode order.

    python -B tests/golden/train_batch/make_train_batch_golden.py [--out DIR]
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
REF = os.environ.get("RL101_REFERENCE", "/root/reference")
T, N = 37, 40
GAMMA, LAM = 0.99, 0.95


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


def ragged_set(seed=11) -> dict:
    import torch
    compute_gae = notebook_function("Actor_Critic_PPO.ipynb", "compute_gae", {"torch": torch})
    compute_returns = notebook_function("Policy_Gradients.ipynb", "compute_returns", {})
    rng = np.random.default_rng(seed)
    # lengths: 1, 2, T with a done at the last frame, T without a done, random ones
    length = rng.integers(1, T + 1, N)
    ended = np.ones(N, dtype=bool)
    length[:6] = (1, 2, T, T, 1, T)
    ended[3] = ended[5] = False
    for i in range(6, N):
        if length[i] == T:
            ended[i] = bool(rng.random() < 0.5)
    # every frame filled, also past an episode's end (later episodes of an auto-reset lane)
    reward = rng.normal(0.0, 3.0, (T, N))
    values = rng.normal(0.0, 40.0, (T, N)).astype(np.float32)
    bootstrap = rng.normal(0.0, 40.0, N).astype(np.float32)
    bootstrap[3] = np.float32(17.25)
    done = rng.random((T, N)) < 0.1
    for i in range(N):
        done[:length[i], i] = False
        if ended[i]:
            done[length[i] - 1, i] = True
        else:
            done[:, i] = False
        # terminal rewards of the shaped reward's magnitudes: crash, landing, landing + fuel * 100
        if ended[i]:
            reward[length[i] - 1, i] = (-500.0, 500.0, 500.0 + rng.random() * 100.0)[i % 3]
    reward[0, 4] = 500.0 + 0.7321 * 100.0

    adv, ret, rets64, ep_ret = [], [], [], []
    for i in range(N):
        ln = int(length[i])
        rewards = [float(r) for r in reward[:ln, i]]
        v = torch.from_numpy(values[:ln, i].copy())
        boot = 0.0 if ended[i] else float(bootstrap[i])
        with_boot = torch.cat([v, torch.tensor([boot])])
        dones = [False] * ln
        if ended[i]:
            dones[-1] = True
        a = compute_gae(rewards, with_boot.cpu().numpy(), dones, gamma=GAMMA, lambda_=LAM,
                        device=torch.device("cpu"))
        adv.append(a)
        ret.append(a + v)
        rets64.extend(compute_returns(rewards, gamma=GAMMA))
        ep_ret.append(sum(rewards))
    all_adv = torch.cat(adv)
    all_ret = torch.cat(ret)
    norm_adv = (all_adv - all_adv.mean()) / (all_adv.std() + 1e-8)
    returns_tensor = torch.tensor(rets64, dtype=torch.float32)
    baseline = returns_tensor.mean()
    r_adv = returns_tensor - baseline
    r_adv = (r_adv - r_adv.mean()) / (r_adv.std() + 1e-8)
    return dict(done=done.astype(np.uint8), reward=reward, values=values, bootstrap=bootstrap,
                length=length.astype(np.int32), ended=ended.astype(np.uint8),
                gae_advantages=all_adv.numpy(), gae_returns=all_ret.numpy(), gae_normalized=norm_adv.numpy(),
                reinforce_returns=returns_tensor.numpy(), reinforce_baseline=baseline.numpy(),
                reinforce_std=returns_tensor.std().numpy(), reinforce_normalized=r_adv.numpy(),
                episode_return=np.asarray(ep_ret, dtype=np.float64),
                gamma=np.float64(GAMMA), lam=np.float64(LAM))


def main():
    out = HERE
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(out, exist_ok=True)
    save_npz(os.path.join(out, "ragged.npz"), **ragged_set())


if __name__ == "__main__":
    main()
