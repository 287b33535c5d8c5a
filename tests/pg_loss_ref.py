"""Float64 NumPy restatement of dd_pg_losses and dd_td_losses as
include/dronestep.h states them: the score-function loss of the REINFORCE and
actor-critic notebooks and the actor-critic notebook's critic stage, from
per-row network outputs, mask included.  What the GPU tests compare the kernels
with, and what tests/test_pg_loss_cpu.py pins to the notebooks' own results
(tests/golden/pg_loss/pg.npz).

Inputs are float32 arrays; every product and sum is float64, in the kernels'
order of operations, and each per-row output is rounded to float32 once.
"""
from __future__ import annotations

import numpy as np

from ppo_loss_ref import EPS32, action_bits


def _active(active, m) -> np.ndarray:
    return np.ones(m, dtype=bool) if active is None else np.asarray(active).astype(bool)


def _f64(x) -> np.ndarray:
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def pg_losses(log_prob, probs, actions, weights, active=None) -> dict:
    """loss = -sum_active(lp w) / cnt, count, grad_logits [m, 3] float32."""
    m = len(log_prob)
    on = _active(active, m)
    cnt = float(on.sum())
    lp, w = _f64(log_prob), _f64(weights)
    with np.errstate(divide="ignore", invalid="ignore"):
        loss = -(np.float64((lp * w)[on].sum()) / np.float64(cnt))
        g = -(w / np.float64(cnt))
        pf = np.asarray(probs, dtype=np.float32)
        p = pf.astype(np.float64)
        inside = (pf >= np.float32(EPS32)) & (pf <= np.float32(1.0) - np.float32(EPS32))
        full = g[:, None] * (action_bits(actions) - p)
        grad = np.where(inside, full, np.where(np.isnan(p), p, 0.0))
    grad = np.where(on[:, None], grad, 0.0)
    return dict(loss=float(loss), count=cnt, grad_logits=grad.astype(np.float32))


def td_losses(values, next_values, rewards, dones, gamma=0.99, value_reg=0.01, active=None) -> dict:
    """td_targets, td_errors, grad_values [m] float32 (0 on inactive rows) and
    critic_loss, mse, value_reg, count."""
    m = len(values)
    on = _active(active, m)
    cnt = float(on.sum())
    v, vn, r, d = _f64(values), _f64(next_values), _f64(rewards), _f64(dones)
    g = float(np.float32(gamma))
    with np.errstate(divide="ignore", invalid="ignore"):
        target = np.where(on, r + (g * vn) * (1.0 - d), 0.0)
        delta = np.where(on, target - v, 0.0)
        mse = np.float64((delta * delta)[on].sum()) / np.float64(cnt)
        reg = value_reg * (np.float64((v * v)[on].sum()) / np.float64(cnt))
        grad = np.where(on, (-2.0 * delta + 2.0 * value_reg * v) / np.float64(cnt), 0.0)
    return dict(critic_loss=float(mse + reg), mse=float(mse), value_reg=float(reg), count=cnt,
                td_targets=target.astype(np.float32), td_errors=delta.astype(np.float32),
                grad_values=grad.astype(np.float32), delta=delta)
