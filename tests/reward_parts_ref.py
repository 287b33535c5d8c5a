"""NumPy float64 restatement of the notebooks' two ``calc_reward`` functions,
returning the whole dict as eight slots instead of ``total`` alone:

    0 time_penalty  1 distance  2 hovering (PPO) / velocity_alignment (REINFORCE)
    3 angle  4 speed  5 vertical_position  6 terminal  7 total

``states`` is ``[..., 15]`` doubles in ``state_to_array`` order (the oracle's
``obs64``), ``prev_dist`` the ``distance_to_platform`` of ``prev_state`` (NaN =
``prev_state is None``).  Every term is formed as the notebook's Python forms
it: ``x ** 2`` is the C library's ``pow(x, 2)`` (CPython's float power),
``math.exp`` its ``exp``, the sums run in the notebook's order.  The PPO
notebook's quirk is kept: ``time_penalty`` is
``-inverse_quadratic(dist, decay=100, scaler=1)`` while ``total`` adds the
literal ``-0.5`` in its place.

Actor_Critic_PPO.ipynb:164-263 (Actor_Critic_Basic.ipynb's cell is the same
function), Policy_Gradients.ipynb:128-238, rl_helpers/scalers.py.
"""
import math

import numpy as np

PPO_NAMES = ("time_penalty", "distance", "hovering", "angle", "speed", "vertical_position", "terminal", "total")
REINFORCE_NAMES = ("time_penalty", "distance", "velocity_alignment", "angle", "speed", "vertical_position",
                   "terminal", "total")

_pow2 = np.frompyfunc(lambda x: float(x) ** 2, 1, 1)
_exp = np.frompyfunc(lambda x: math.exp(float(x)), 1, 1)


def pow2(a):
    return _pow2(np.asarray(a, np.float64)).astype(np.float64)


def _columns(states):
    s = np.asarray(states, np.float64)
    assert s.shape[-1] == 15
    return (s[..., 2], s[..., 3], s[..., 4], s[..., 6], s[..., 9], s[..., 10], s[..., 11], s[..., 12],
            s[..., 13] != 0.0, s[..., 14] != 0.0)


def _shared_terms(angle, fuel, dist, dy, speed, landed, crashed, max_speed, landing_bonus):
    excess = np.abs(angle) - (((0.20 - 0.111) * dist) + 0.111)
    r_angle = -np.maximum(excess, 0)
    r_speed = np.where(dist < 1, -2 * np.maximum(speed - 0.1, 0), -1 * np.maximum(speed - max_speed, 0))
    r_vertical = np.where(dy > 0, 0.0, dy * 4.0)
    r_terminal = np.where(landed, landing_bonus + fuel * 100.0,
                          np.where(crashed, np.where(dist > 0.3, -200.0 - 100.0, -200.0), 0.0))
    return r_angle, r_speed, r_vertical, r_terminal


def ppo_parts(states, prev_dist):
    """calc_reward(state, prev_state) of the PPO / Actor-Critic notebooks."""
    vx, vy, angle, fuel, dist, dx, dy, speed, landed, crashed = _columns(states)
    prev = np.broadcast_to(np.asarray(prev_dist, np.float64), dist.shape)
    time_penalty = -(1 * (1 / (1 + (100 * pow2(dist))))) - 0
    have_prev = ~np.isnan(prev)
    with np.errstate(invalid="ignore", divide="ignore"):
        delta = prev - dist
        vtp = np.where(dist > 1e-6, (vx * dx + vy * dy) / np.where(dist > 1e-6, dist, 1.0), 0.0)
        fast_toward = (speed >= 0.15) & (vtp > 0.1) & (dist > 0.065)
        clipped = np.clip(delta * 1000 * (1.0 + speed * 2.0), -2, 5)
        away = ~fast_toward & (delta < -0.001)
        distance = np.where(fast_toward, clipped, np.where(away, -2.0 * np.abs(delta) * 1000, 0.0))
    hovering = np.where(fast_toward | away, 0.0, np.where(speed < 0.05, -1.0, np.where(speed < 0.15, -0.3, 0.0)))
    distance = np.where(have_prev, distance, 0.0)
    hovering = np.where(have_prev, hovering, 0.0)
    r_angle, r_speed, r_vertical, r_terminal = _shared_terms(angle, fuel, dist, dy, speed, landed, crashed, 0.6, 800.0)
    total = np.zeros_like(dist)
    total = total + -0.5
    for term in (distance, hovering, r_angle, r_speed, r_vertical, r_terminal):
        total = total + term
    return np.stack([time_penalty, distance, hovering, r_angle, r_speed, r_vertical, r_terminal, total], axis=-1)


def reinforce_parts(states):
    """calc_reward(state) of the REINFORCE notebook."""
    vx, vy, angle, fuel, dist, dx, dy, speed, landed, crashed = _columns(states)
    time_penalty = -((1 - 0.3) * (1 / (1 + (50 * pow2(dist))))) - 0.3
    odx, ody = -dx, -dy
    onorm = np.sqrt(pow2(odx) + pow2(ody))
    with np.errstate(invalid="ignore", divide="ignore"):
        ux, uy = odx / onorm, ody / onorm
        align = np.where(onorm < 1e-6, 1.0, np.where(speed < 1e-6, 0.0, (vx / speed) * ux + (vy / speed) * uy))
    above = (dist > 0.065) & (dy > 0)
    sig = 4.5 * (1 / (1 + _exp(10 * (dist - 0.5)).astype(np.float64)))
    distance = np.where(above, (align > 0).astype(np.float64) * speed * sig, 0.0)
    valign = np.where(above & (align > 0), 0.5, 0.0)
    r_angle, r_speed, r_vertical, r_terminal = _shared_terms(angle, fuel, dist, dy, speed, landed, crashed, 0.4, 500.0)
    total = np.zeros_like(dist)
    for term in (time_penalty, distance, valign, r_angle, r_speed, r_vertical, r_terminal):
        total = total + term
    return np.stack([time_penalty, distance, valign, r_angle, r_speed, r_vertical, r_terminal, total], axis=-1)


def parts(mode, states, prev_dist=None):
    """By the env's reward_mode: "notebook" (PPO) or "reinforce"."""
    if mode == "notebook":
        return ppo_parts(states, prev_dist)
    if mode == "reinforce":
        return reinforce_parts(states)
    raise ValueError(mode)


def coverage(states, prev_dist):
    """How many of the recorded (state, prev_dist) pairs take each branch of
    the two calc_reward functions: the fixture's generator and its test assert
    that none is zero."""
    vx, vy, angle, fuel, dist, dx, dy, speed, landed, crashed = _columns(states)
    prev = np.asarray(prev_dist, np.float64)
    delta = prev - dist
    vtp = np.where(dist > 1e-6, (vx * dx + vy * dy) / np.where(dist > 1e-6, dist, 1.0), 0.0)
    fast = (speed >= 0.15) & (vtp > 0.1) & (dist > 0.065)
    raw = delta * 1000 * (1.0 + speed * 2.0)
    away = ~fast & (delta < -0.001)
    rest = ~fast & ~away
    excess = np.abs(angle) - (((0.20 - 0.111) * dist) + 0.111)
    onorm = np.sqrt(pow2(-dx) + pow2(-dy))
    with np.errstate(invalid="ignore", divide="ignore"):
        align = np.where(onorm < 1e-6, 1.0, np.where(speed < 1e-6, 0.0, (vx / speed) * (-dx / onorm) +
                                                     (vy / speed) * (-dy / onorm)))
    above = (dist > 0.065) & (dy > 0)
    cases = {
        "prev_state present": ~np.isnan(prev),
        "fast toward, clipped at -2": fast & (raw < -2), "fast toward, clipped at 5": fast & (raw > 5),
        "fast toward, unclipped": fast & (raw >= -2) & (raw <= 5) & (raw != 0),
        "moving away": away, "hover -1.0": rest & (speed < 0.05), "hover -0.3": rest & (speed >= 0.05) & (speed < 0.15),
        "no distance / hover branch": rest & (speed >= 0.15),
        "dist < 1": dist < 1, "dist >= 1": dist >= 1, "above the pad": dy > 0, "below the pad": ~(dy > 0),
        "excess angle": excess > 0, "no excess angle": ~(excess > 0),
        "over the speed limit near": (dist < 1) & (speed > 0.6), "over the speed limit far": (dist >= 1) & (speed > 0.6),
        "landed": landed, "crashed near": ~landed & crashed & ~(dist > 0.3), "crashed far": ~landed & crashed & (dist > 0.3),
        "flying": ~landed & ~crashed,
        "reinforce above, aligned": above & (align > 0), "reinforce above, not aligned": above & ~(align > 0),
        "reinforce not above": ~above, "reinforce onorm < 1e-6": onorm < 1e-6,
        "reinforce speed < 1e-6": (onorm >= 1e-6) & (speed < 1e-6),
    }
    return {k: int(np.count_nonzero(v)) for k, v in cases.items()}
