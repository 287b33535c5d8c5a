#!/usr/bin/env python
"""Time evaluate_policy's kernel next to the collection rollout (lab).

65,536 lanes, 64 frames per launch, the same random actor and the same
auto-reset env config for both, alternated over `--rounds` rounds in one
process:

    collection   dd_policy_rollout: Bernoulli draw, the PPO buffers obs
                 [T, N, 15], actions, log-probs, rewards, dones
    eval_T0.3    dd_policy_rollout_sampled: tempered draw, DDEpisodeStats, no
                 per-frame buffer
    eval_greedy  the same with DD_SAMPLE_GREEDY
    eval_sticky  eval_T0.3 on an auto_reset=False env (evaluate_policy's own
                 shape: lanes that are done stay done)

One JSON line per variant: the median and the spread of us per frame.

    python tools/lab/eval_lab.py [--envs 65536] [--frames 64] [--rounds 7]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "reinforcement-learning-101_amd"))
import torch  # noqa: E402
from torch import nn  # noqa: E402
from delivery_drone_amd import EnvConfig, MlpNet, VecDroneEnv, abi  # noqa: E402


def actor(dev, compute):
    torch.manual_seed(0)
    net = nn.Sequential(nn.Linear(15, 128), nn.LayerNorm(128), nn.ReLU(), nn.Linear(128, 128), nn.LayerNorm(128),
                        nn.ReLU(), nn.Linear(128, 64), nn.LayerNorm(64), nn.ReLU(), nn.Linear(64, 3))
    return MlpNet(net.state_dict(), device=dev, compute=compute)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--envs", type=int, default=65_536)
    p.add_argument("--frames", type=int, default=64)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--compute", default="f16x3", choices=("f32", "f16x3"))
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    n, frames = a.envs, a.frames
    net = actor(dev, a.compute)
    mode = {"f32": abi.DD_MLP_F32, "f16x3": abi.DD_MLP_F16X3}[a.compute]
    lib = abi.lib()

    def env(auto):
        e = VecDroneEnv(n, device=dev, config=EnvConfig(randomize_drone=True, randomize_platform=True,
                                                        auto_reset=auto, seed=1))
        e.reset()
        return e

    bufs = dict(obs_out=torch.empty(frames, n, 15, device=dev),
                actions_out=torch.empty(frames, n, dtype=torch.uint8, device=dev),
                log_prob_out=torch.empty(frames, n, device=dev), reward_out=torch.empty(frames, n, device=dev),
                done_out=torch.empty(frames, n, dtype=torch.bool, device=dev))
    e_col, e_eval, e_sticky = env(True), env(True), env(False)
    stats_t = [torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
               torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, device=dev)]
    stats = abi.DDEpisodeStats(*[t.data_ptr() for t in stats_t])
    stream = torch.cuda.Stream(dev)

    def eval_launch(e, sample_mode, temperature, step):
        io = abi.DDPolicyRolloutIO()
        io.obs0 = io.obs_final = e.obs.data_ptr()
        io.seed, io.step, io.frames = 1, step, frames
        io.shaped_mode = abi.DD_SHAPED_PPO
        sm = abi.DDSampling(sample_mode, temperature, None)
        abi.check(lib.dd_policy_rollout_sampled(ctypes.byref(e._cfg), ctypes.byref(e._state), net.packed.data_ptr(),
                                                mode, ctypes.byref(io), ctypes.byref(sm), ctypes.byref(stats), n,
                                                ctypes.c_void_p(stream.cuda_stream)), "dd_policy_rollout_sampled")

    variants = {
        "collection": lambda step: e_col.policy_rollout(net, frames, seed=1, step=step, **bufs),
        "eval_T0.3": lambda step: eval_launch(e_eval, abi.DD_SAMPLE_TEMPERED, 0.3, step),
        "eval_greedy": lambda step: eval_launch(e_eval, abi.DD_SAMPLE_GREEDY, 0.0, step),
        "eval_sticky": lambda step: eval_launch(e_sticky, abi.DD_SAMPLE_TEMPERED, 0.3, step),
    }
    times = {k: [] for k in variants}
    with torch.cuda.stream(stream):
        for run in variants.values():  # warm-up: code objects, the LDS attribute
            run(0)
        torch.cuda.synchronize(dev)
        step = frames
        for _ in range(a.rounds):
            for name, run in variants.items():
                for t in stats_t[:3]:
                    t.zero_()  # every lane counts again
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.reps):
                    run(step)
                    step += frames
                e1.record(stream)
                torch.cuda.synchronize(dev)
                times[name].append(e0.elapsed_time(e1) * 1e3 / (a.reps * frames))
    for name, ts in times.items():
        print(json.dumps({"variant": name, "envs": n, "frames": frames, "compute": a.compute,
                          "us_per_frame_median": round(statistics.median(ts), 3),
                          "us_per_frame_min": round(min(ts), 3), "us_per_frame_max": round(max(ts), 3),
                          "rounds": a.rounds, "reps": a.reps}), flush=True)


if __name__ == "__main__":
    main()
