#!/usr/bin/env python
"""Generate tests/golden/train_batch_episodes/multi.npz by running the
REFERENCE notebooks' own functions over every episode of a rollout in which
lanes re-spawn (several episodes per lane).

Runs only where the reference checkout exists (/root/reference, or
$RL101_REFERENCE).  ``compute_gae`` (Actor_Critic_PPO.ipynb) and
``compute_returns`` (Policy_Gradients.ipynb) are executed from the notebooks'
cells at run time, as make_train_batch_golden.py does, once per episode exactly
as the PPO training cell calls them: ``dones = [False] * len(rewards)``,
``dones[-1] = True`` when the episode ended, the bootstrap value of the final
state appended when it did not; then ``returns = advantages + values``,
``torch.cat`` and the normalisation, on torch float32 CPU tensors.  The
episodes are cut here by a plain loop of its own (a frame that follows a done
is the re-spawn frame and belongs to no episode), not by the code under test.
The file holds data only: the rectangular inputs, the episodes, and the
notebooks' results in lane-major, time-ordered episode order.

    python -B tests/golden/train_batch_episodes/make_episodes_golden.py [--out DIR]
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


def rollout(seed=23):
    rng = np.random.default_rng(seed)
    done = rng.random((T, N)) < 0.08
    before = rng.random(N) < 0.15
    done[:, 0] = False; done[0, 0] = True; before[0] = False     # done at frame 0
    done[:, 1] = False; done[T - 1, 1] = True; before[1] = False  # done at frame T-1: ended, nothing open
    done[:, 2] = False; done[T - 2, 2] = True                     # done at T-2: frame T-1 dropped, nothing open
    done[:, 3] = False; done[20, 3] = True; before[3] = True      # done before: frame 0 dropped
    done[:, 4] = True; before[4] = True                           # done before and at every frame: no row
    done[:, 5] = False; before[5] = False                         # never done: one open episode of T rows
    done[:, 6] = False; done[9, 6] = done[11, 6] = True           # dones at t and t + 2: an episode of length 1
    done[:, 7] = False; done[13:, 7] = True; before[7] = False    # sticky: the first episode only
    done[:, 8] = False; done[[4, 12, 13, 25, 31], 8] = True       # four ended episodes (13 is a re-spawn frame
    #                                                               whose flag is set: still dropped) and an open one
    done[:, 9] = False; done[17, 9] = True; before[9] = False     # ended, then an open episode with a bootstrap
    for i in list(range(10, N)) + [0, 3, 6, 9]:                   # auto-reset lanes: never done on the re-spawn frame
        prev = before[i]
        for t in range(T):
            if prev:
                done[t, i] = False
            prev = done[t, i]
    reward = rng.normal(0.0, 3.0, (T, N))
    terminal = (-500.0, 500.0, 557.3, 500.0 + 0.7321 * 100.0)
    for k, (t, i) in enumerate(zip(*np.nonzero(done))):
        reward[t, i] = terminal[k % 4]
    values = rng.normal(0.0, 40.0, (T, N)).astype(np.float32)
    bootstrap = rng.normal(0.0, 40.0, N).astype(np.float32)
    bootstrap[5], bootstrap[9] = np.float32(17.25), np.float32(-3.5)
    return done, before, reward, values, bootstrap


def episodes_of(done, before):
    """[(lane, start, length, ended)], lanes ascending, in time order."""
    out = []
    for i in range(N):
        prev, start = bool(before[i]), None
        for t in range(T):
            if not prev and start is None:
                start = t
            if not prev and done[t, i]:
                out.append((i, start, t - start + 1, True))
                start = None
            prev = bool(done[t, i])
        if start is not None:
            out.append((i, start, T - start, False))
    return out


def multi_set() -> dict:
    import torch
    compute_gae = notebook_function("Actor_Critic_PPO.ipynb", "compute_gae", {"torch": torch})
    compute_returns = notebook_function("Policy_Gradients.ipynb", "compute_returns", {})
    done, before, reward, values, bootstrap = rollout()
    eps = episodes_of(done, before)
    adv, ret, rets64, closed64, ep_ret = [], [], [], [], []
    for lane, start, ln, ended in eps:
        rewards = [float(r) for r in reward[start:start + ln, lane]]
        v = torch.from_numpy(values[start:start + ln, lane].copy())
        boot = 0.0 if ended else float(bootstrap[lane])
        with_boot = torch.cat([v, torch.tensor([boot])])
        dones = [False] * ln
        if ended:
            dones[-1] = True
        a = compute_gae(rewards, with_boot.cpu().numpy(), dones, gamma=GAMMA, lambda_=LAM, device=torch.device("cpu"))
        adv.append(a)
        ret.append(a + v)
        G = compute_returns(rewards, gamma=GAMMA)
        rets64.extend(G)
        if ended:
            closed64.extend(G)
        ep_ret.append(sum(rewards))
    all_adv = torch.cat(adv)
    all_ret = torch.cat(ret)
    norm_adv = (all_adv - all_adv.mean()) / (all_adv.std() + 1e-8)

    def reinforce(rets):
        returns_tensor = torch.tensor(rets, dtype=torch.float32)
        baseline = returns_tensor.mean()
        r_adv = returns_tensor - baseline
        r_adv = (r_adv - r_adv.mean()) / (r_adv.std() + 1e-8)
        return returns_tensor.numpy(), baseline.numpy(), returns_tensor.std().numpy(), r_adv.numpy()

    r_all, base_all, std_all, norm_all = reinforce(rets64)
    r_closed, base_closed, std_closed, norm_closed = reinforce(closed64)
    e = np.asarray(eps, dtype=np.int64).reshape(-1, 4)
    return dict(done=done.astype(np.uint8), done_before=before.astype(np.uint8), reward=reward, values=values,
                bootstrap=bootstrap, ep_lane=e[:, 0].astype(np.int32), ep_start=e[:, 1].astype(np.int32),
                ep_length=e[:, 2].astype(np.int32), ep_ended=e[:, 3].astype(np.uint8),
                gae_advantages=all_adv.numpy(), gae_returns=all_ret.numpy(), gae_normalized=norm_adv.numpy(),
                reinforce_returns=r_all, reinforce_baseline=base_all, reinforce_std=std_all,
                reinforce_normalized=norm_all, closed_returns=r_closed, closed_baseline=base_closed,
                closed_std=std_closed, closed_normalized=norm_closed,
                episode_return=np.asarray(ep_ret, dtype=np.float64), gamma=np.float64(GAMMA), lam=np.float64(LAM))


def main():
    out = HERE
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(out, exist_ok=True)
    save_npz(os.path.join(out, "multi.npz"), **multi_set())


if __name__ == "__main__":
    main()
