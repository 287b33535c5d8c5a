#!/usr/bin/env python
"""Time a checkpoint tournament both ways: one population launch against one
single-actor launch per member.

Workload: `members` actors x `lanes` lanes each, env.evaluate_policy for
`frames` frames, f32 storage, reference world, sticky done, for both actor
arithmetics (compute f32 and f16x3).

  population   one env of members * lanes lanes, evaluate_policy(ActorPopulation):
               a grid of members * ceil(lanes / 256) blocks
  sequential   `members` envs of `lanes` lanes (env_id_base g * lanes),
               evaluate_policy(actors[g]) one after the other on one stream:
               what the library offered before dd_policy_rollout_population.
               Each launch's grid is ceil(lanes / 256) blocks.

Both sides are whole evaluate_policy calls (reset, the statistics' buffers,
the launch), timed with device events on the current stream around the calls
and a synchronise after the closing event; the two sides alternate, after
`warmup` untimed rounds, and the medians over `repeats` rounds are reported
with the spread (min, max).  Before timing, the two results are compared bit
for bit, so the times are times of the same answer.

Prints one JSON line per compute; --out appends them to a file.

    python tools/population_point.py --out profiles/r16/population_point.jsonl
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "reinforcement-learning-101_amd"))
import torch  # noqa: E402
from torch import nn  # noqa: E402
from delivery_drone_amd import ActorPopulation, EnvConfig, MlpNet, VecDroneEnv, abi  # noqa: E402


def actor_state_dict(seed):
    """A seeded torch-default actor; the thrusters' biases differ by member so the episodes do."""
    torch.manual_seed(seed)
    net = nn.Sequential(nn.Linear(15, 128), nn.LayerNorm(128), nn.ReLU(), nn.Linear(128, 128), nn.LayerNorm(128),
                        nn.ReLU(), nn.Linear(128, 64), nn.LayerNorm(64), nn.ReLU(), nn.Linear(64, 3))
    with torch.no_grad():
        net[9].bias.copy_(torch.tensor([-1.0, 0.0, 0.0]) + 0.05 * seed * torch.tensor([1.0, -1.0, 0.5]))
    return net.state_dict()


def timed(fn):
    """Milliseconds of fn() by device events on the current stream."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), out


def point(dev, compute, members, lanes, frames, temperature, warmup, repeats):
    cfg = EnvConfig(randomize_drone=True, seed=5)
    actors = [MlpNet(actor_state_dict(g), device=dev, compute=compute) for g in range(members)]
    pop = ActorPopulation(actors)
    big = VecDroneEnv(members * lanes, device=dev, config=cfg)
    small = [VecDroneEnv(lanes, device=dev, config=cfg, env_id_base=g * lanes) for g in range(members)]

    def population():
        return big.evaluate_policy(pop, max_steps=frames, temperature=temperature, seed=3)

    def sequential():
        return [e.evaluate_policy(a, max_steps=frames, temperature=temperature, seed=3) for e, a in zip(small, actors)]

    got, want = population(), sequential()
    equal = all(torch.equal(got[k], torch.cat([w[k] for w in want])) for k in got)
    t_pop, t_seq = [], []
    for r in range(warmup + repeats):
        a, _ = timed(population)
        b, _ = timed(sequential)
        if r >= warmup:
            t_pop.append(a)
            t_seq.append(b)
    med_pop, med_seq = statistics.median(t_pop), statistics.median(t_seq)
    return {"tool": "population_point", "device": torch.cuda.get_device_name(dev),
            "build_info": abi.lib().dd_build_info().decode(), "compute": compute, "storage": "f32",
            "members": members, "lanes_per_member": lanes, "frames": frames, "temperature": temperature,
            "blocks_population": members * -(-lanes // 256), "blocks_per_sequential_launch": -(-lanes // 256),
            "warmup": warmup, "repeats": repeats, "results_bit_equal": equal,
            "population_ms": {"median": med_pop, "min": min(t_pop), "max": max(t_pop)},
            "sequential_ms": {"median": med_seq, "min": min(t_seq), "max": max(t_seq)},
            "sequential_over_population": med_seq / med_pop,
            "landed_fraction": float(got["landed"].double().mean())}


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--members", type=int, default=16)
    p.add_argument("--lanes", type=int, default=4096)
    p.add_argument("--frames", type=int, default=300)
    p.add_argument("--temperature", type=float, default=0.5)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=15)
    p.add_argument("--out")
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("population_point measures on the GPU: torch.cuda.is_available() is False")
    dev = torch.device("cuda", 0)
    bad = 0
    for compute in ("f32", "f16x3"):
        row = point(dev, compute, a.members, a.lanes, a.frames, a.temperature, a.warmup, a.repeats)
        bad += not row["results_bit_equal"]
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
