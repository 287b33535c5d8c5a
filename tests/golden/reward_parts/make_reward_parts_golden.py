#!/usr/bin/env python
"""Generate tests/golden/reward_parts/reward_parts.npz by running the REFERENCE
notebooks' own ``calc_reward`` cells and keeping the whole dict they return.

Runs only where the reference checkout exists (/root/reference, or
$RL101_REFERENCE).  ``calc_reward`` (with ``calc_velocity_alignment`` and
rl_helpers/scalers.py) is exec'd from the cells of Actor_Critic_PPO.ipynb,
Actor_Critic_Basic.ipynb and Policy_Gradients.ipynb at generation time; no
notebook text is kept here.  The states are ``DroneGame.get_state()`` dicts of
reference episodes flown by a keyed random pilot (prev_state = the state one
frame back, the reset state at frame 0: the notebooks' evaluate_policy), plus
hand-made states for the branches an episode rarely meets.

The file holds data only: ``states [M, 15]`` (state_to_array order),
``prev_dist [M]`` and the eight values of the PPO and the REINFORCE function,
``ppo [M, 8]`` / ``reinforce [M, 8]``, in the notebooks' key order (``names_*``).

Actor_Critic_Basic.ipynb's calc_reward is checked here against the PPO
notebook's on every recorded state: all eight values are equal (the two cells
are the same function), recorded as ``basic_equals_ppo``; the generator stops if
they ever differ, so the kernel's PPO shape serves both notebooks.

The generator asserts its own coverage (tests/reward_parts_ref.coverage): every
branch of both functions is taken at least once.

    python -B tests/golden/reward_parts/make_reward_parts_golden.py [--out DIR]
"""
from __future__ import annotations

import io
import json
import math
import os
import sys
import types
import zipfile
from types import SimpleNamespace

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # tests/
REF = os.environ.get("RL101_REFERENCE", "/root/reference")

import reward_parts_ref as rp  # noqa: E402

OBS_KEYS = ("drone_x", "drone_y", "drone_vx", "drone_vy", "drone_angle", "drone_angular_vel",
            "drone_fuel", "platform_x", "platform_y", "distance_to_platform", "dx_to_platform",
            "dy_to_platform", "speed", "landed", "crashed")
ACTION_KEYS = ("main_thrust", "left_thrust", "right_thrust")


def import_reference():
    if not os.path.isdir(os.path.join(REF, "delivery_drone", "game")):
        raise SystemExit(f"reference not found at {REF}; the fixture is committed, nothing to do")
    sys.modules.setdefault("pygame", types.ModuleType("pygame"))
    sys.path.insert(0, REF)
    from delivery_drone.game.game_engine import DroneGame
    return DroneGame


def calc_reward_of(notebook: str):
    """calc_reward of `notebook`, executed from its own cells."""
    from delivery_drone.game.socket_client import DroneState
    import rl_helpers.scalers as scalers
    ns = {"np": np, "math": math, "DroneState": DroneState}
    ns.update({k: getattr(scalers, k) for k in dir(scalers) if not k.startswith("_")})
    for cell in json.load(open(os.path.join(REF, notebook)))["cells"]:
        src = "".join(cell["source"])
        if cell["cell_type"] == "code" and ("def calc_velocity_alignment" in src or "def calc_reward" in src):
            exec(compile(src, notebook, "exec"), ns)
    return ns["calc_reward"]


def save_npz(path: str, **arrays) -> None:
    """A deflated .npz with fixed member dates: regenerates byte for byte."""
    with zipfile.ZipFile(path, "w") as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy")
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def episodes(DroneGame, rng, games=12, frames=120):
    """(state, prev_dist) pairs of reference episodes: a pilot that mostly
    burns against the fall, idles or tumbles, by game."""
    out = []
    for g_i in range(games):
        g = DroneGame(render_mode=None, randomize_drone=True, randomize_platform=True)
        np.random.seed(1000 + g_i)
        import random
        random.seed(1000 + g_i)
        state = g.reset()
        style = g_i % 4
        for _ in range(frames):
            if style == 0:    # brake the fall, steer little
                bits = (1 if state["drone_vy"] > 0.05 else 0) | (int(rng.integers(0, 8)) & 6 if rng.random() < 0.1 else 0)
            elif style == 1:  # idle: free fall
                bits = 0
            elif style == 2:  # random
                bits = int(rng.integers(0, 8))
            else:             # hover in place
                bits = 1 if state["drone_vy"] > 0.0 else 0
            prev = state
            state, _, done, _ = g.step({k: (bits >> i) & 1 for i, k in enumerate(ACTION_KEYS)})
            out.append(([float(state[k]) for k in OBS_KEYS], float(prev["distance_to_platform"])))
            if done:
                break
    return out


def hand_made():
    """States for the rare branches, as plain observation vectors."""
    def st(vx=0.0, vy=0.0, angle=0.0, fuel=0.9, dist=0.4, dx=0.3, dy=0.2, speed=None, landed=0.0, crashed=0.0):
        speed = math.hypot(vx, vy) if speed is None else speed
        return [0.5, 0.3, vx, vy, angle, 0.0, fuel, 0.5, 0.6, dist, dx, dy, speed, landed, crashed]
    rows = [
        (st(vx=0.3, vy=0.2), 0.41),                          # fast toward: 0.01 * 1000 * (1 + 2 speed) > 5, clipped at 5
        (st(vx=0.3, vy=0.2), 0.4005),                        # fast toward, unclipped
        (st(vx=0.3, vy=0.2), 0.39),                          # fast toward, clipped at -2
        (st(vx=-0.3, vy=-0.2), 0.39),                        # moving away
        (st(vx=0.01, vy=0.0), 0.4),                          # hover -1.0
        (st(vx=0.1, vy=0.0), 0.4),                           # hover -0.3
        (st(vx=-0.3, vy=-0.2), 0.4),                         # none of the branches
        (st(vx=0.3, vy=0.2, dist=1.2, dx=0.9, dy=0.8), 1.21),  # dist >= 1, under the far speed limit
        (st(vx=0.9, vy=0.2, dist=1.2, dx=0.9, dy=0.8), 1.21),  # dist >= 1, speed > 0.6
        (st(vx=0.9, vy=0.2), 0.42),                          # dist < 1, speed > 0.6
        (st(vx=0.1, vy=-0.1, dy=-0.2, dx=0.35), 0.4),        # below the pad
        (st(angle=0.5), 0.4),                                # excess angle
        (st(vx=0.01, vy=0.02, dist=0.01, dx=0.005, dy=0.008, landed=1.0, fuel=0.73), 0.012),  # landed
        (st(vx=0.2, vy=0.5, dist=0.1, dx=0.06, dy=0.08, crashed=1.0), 0.12),   # crashed near
        (st(vx=0.2, vy=0.5, dist=0.6, dx=0.5, dy=-0.33, crashed=1.0), 0.62),   # crashed far
        (st(vx=0.2, vy=0.1, dist=0.0, dx=0.0, dy=0.0), 0.01),                  # onorm < 1e-6 (at the platform)
        (st(vx=0.0, vy=0.0, speed=0.0), 0.4),                                  # speed < 1e-6
        (st(vx=0.3, vy=0.2), float("nan")),                                    # prev_state None (the collection loop's frame 0)
    ]
    return rows


def main():
    out_dir = HERE
    if "--out" in sys.argv:
        out_dir = sys.argv[sys.argv.index("--out") + 1]
    DroneGame = import_reference()
    ppo, basic, reinforce = (calc_reward_of(nb) for nb in
                             ("Actor_Critic_PPO.ipynb", "Actor_Critic_Basic.ipynb", "Policy_Gradients.ipynb"))
    rows = episodes(DroneGame, np.random.default_rng(20)) + hand_made()
    states = np.array([r[0] for r in rows], np.float64)
    prev = np.array([r[1] for r in rows], np.float64)
    out_ppo, out_rf, basic_equal = [], [], True
    for s, pd in zip(states, prev):
        ns = SimpleNamespace(**{k: (bool(v) if k in ("landed", "crashed") else float(v)) for k, v in zip(OBS_KEYS, s)},
                             steps=0)
        p = None if math.isnan(pd) else SimpleNamespace(distance_to_platform=float(pd))
        a, b, c = ppo(ns, prev_state=p), basic(ns, prev_state=p), reinforce(ns)
        assert tuple(a) == rp.PPO_NAMES and tuple(b) == rp.PPO_NAMES and tuple(c) == rp.REINFORCE_NAMES
        basic_equal &= all(float(a[k]) == float(b[k]) for k in a)
        out_ppo.append([float(a[k]) for k in rp.PPO_NAMES])
        out_rf.append([float(c[k]) for k in rp.REINFORCE_NAMES])
    assert basic_equal, "Actor_Critic_Basic.ipynb's calc_reward differs from the PPO notebook's"
    cov = rp.coverage(states, prev)
    missing = [k for k, v in cov.items() if v == 0]
    assert not missing, f"branches never taken: {missing}"
    assert np.isnan(prev).any()
    os.makedirs(out_dir, exist_ok=True)
    save_npz(os.path.join(out_dir, "reward_parts.npz"), states=states, prev_dist=prev, ppo=np.array(out_ppo),
             reinforce=np.array(out_rf), names_ppo=np.array(rp.PPO_NAMES), names_reinforce=np.array(rp.REINFORCE_NAMES),
             basic_equals_ppo=np.bool_(basic_equal))
    print(f"{len(rows)} states; coverage {cov}")


if __name__ == "__main__":
    main()
