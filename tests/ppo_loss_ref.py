"""Float64 NumPy restatement of the PPO notebook's compute_ppo_losses
(Actor_Critic_PPO.ipynb, the cell after collect_episodes_ppo) from per-row
network outputs, as include/dronestep.h states dd_ppo_losses: what the GPU
tests compare the kernels with, and what tests/test_ppo_loss_cpu.py pins to
the notebook's own results (tests/golden/ppo_loss/losses.npz).

Inputs are float32 arrays (the networks' outputs and the batch); every product
and sum is float64.  The ratio is exp of the float32 difference, rounded to
float32 once; the clip bounds are float32(1 -+ eps).
"""
from __future__ import annotations

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)  # torch's clamp_probs bound for float32


def action_bits(actions) -> np.ndarray:
    """[m, 3] 0/1 float64 from uint8 bitmasks [m] or a float [m, 3] array (nonzero = on)."""
    a = np.asarray(actions)
    if a.ndim == 1:
        return np.stack([(a >> k) & 1 for k in range(3)], axis=1).astype(np.float64)
    return (a != 0).astype(np.float64)


def row_log_prob_entropy(probs, actions):
    """Bernoulli(probs=p).log_prob(a).sum(1) and .entropy().sum(1) in float64
    on the float32 clamp of p (clamp_probs)."""
    p = np.asarray(probs, dtype=np.float32)
    pc = np.clip(p, np.float32(EPS32), np.float32(1.0) - np.float32(EPS32)).astype(np.float64)
    a = action_bits(actions)
    lp = (a * np.log(pc) + (1.0 - a) * np.log1p(-pc)).sum(1)
    ent = -(pc * np.log(pc) + (1.0 - pc) * np.log1p(-pc)).sum(1)
    return lp, ent


def ratio_of(log_prob, old_log_prob) -> np.ndarray:
    d = np.asarray(log_prob, dtype=np.float32) - np.asarray(old_log_prob, dtype=np.float32)
    with np.errstate(over="ignore"):
        return np.exp(d.astype(np.float64)).astype(np.float32)


def losses(log_prob, entropy, probs, values, old_log_prob, advantages, returns, actions,
           clip_epsilon=0.2, entropy_coef=0.01, value_coef=0.5) -> dict:
    """The scalars, ratio statistics, per-row ratio and both head gradients.

    log_prob, entropy (row sums), values, old_log_prob, advantages, returns:
    [m]; probs [m, 3]; actions: bitmasks [m] or [m, 3]."""
    m = len(log_prob)
    md = float(m)
    lo, hi = np.float32(1.0 - clip_epsilon), np.float32(1.0 + clip_epsilon)
    rf = ratio_of(log_prob, old_log_prob)
    r = rf.astype(np.float64)
    A = np.asarray(advantages, dtype=np.float32).astype(np.float64)
    cf = np.where(rf < lo, lo, np.where(rf > hi, hi, rf)).astype(np.float64)
    outside = (rf < lo) | (rf > hi)
    s1, s2 = r * A, cf * A
    surr = np.where(s2 < s1, s2, s1)
    dv = np.asarray(values, dtype=np.float32).astype(np.float64) - np.asarray(returns, np.float32).astype(np.float64)
    policy = -(surr.sum() / md)
    value = (dv * dv).sum() / md
    ent = np.asarray(entropy, dtype=np.float32).astype(np.float64).sum() / (3.0 * md)
    mean = r.sum() / md
    std = float("nan") if m < 2 else float(np.sqrt(((r - mean) ** 2).sum() / (m - 1)))
    g = np.where(~(s1 < s2) & outside, 0.0, -A * r / md)
    pf = np.asarray(probs, dtype=np.float32)
    p = pf.astype(np.float64)
    inside = (pf >= np.float32(EPS32)) & (pf <= np.float32(1.0) - np.float32(EPS32))
    a = action_bits(actions)
    with np.errstate(divide="ignore", invalid="ignore"):
        full = g[:, None] * (a - p) + entropy_coef / (3.0 * md) * (np.log(p) - np.log1p(-p)) * (p * (1.0 - p))
    grad_logits = np.where(inside, full, np.where(np.isnan(p), p, 0.0))
    return dict(total_loss=policy + value_coef * value - entropy_coef * ent, policy_loss=policy, value_loss=value,
                entropy=ent, ratio_mean=mean, ratio_min=float(rf.min()), ratio_max=float(rf.max()), ratio_std=std,
                clipped_frac=outside.sum() / md, ratio=rf, selected=~(~(s1 < s2) & outside),
                grad_logits=grad_logits, grad_values=value_coef * 2.0 * dv / md)


SCALARS = ("total_loss", "policy_loss", "value_loss", "entropy", "ratio_mean", "ratio_min", "ratio_max", "ratio_std",
           "clipped_frac")


def spread(log_prob, entropy, probs, values, old_log_prob, advantages, returns, actions, d_lp, d_p, d_v,
           clip_epsilon=0.2, entropy_coef=0.01, value_coef=0.5) -> dict:
    """First-order spread of :func:`losses`' outputs when every per-row input
    moves within its own bound: log_prob by d_lp [m], each probability by d_p
    (scalar), each value by d_v [m]; the row entropy then moves by the sum of
    d_p |logit(p)| over its factors (dH/dp = -logit(p)).  The clip selection is
    held (the fixture keeps every row clear of its edges).  Returns the bound
    of each scalar and arrays for the two gradients: sums of |partial
    derivative| x bound, no cancellation assumed."""
    base = losses(log_prob, entropy, probs, values, old_log_prob, advantages, returns, actions, clip_epsilon,
                  entropy_coef, value_coef)
    m = len(log_prob)
    md = float(m)
    r = base["ratio"].astype(np.float64)
    A = np.asarray(advantages, dtype=np.float64)
    sel = base["selected"]
    d_lp = np.asarray(d_lp, dtype=np.float64)
    d_v = np.asarray(d_v, dtype=np.float64)
    p = np.asarray(probs, dtype=np.float64)
    logit = np.log(p) - np.log1p(-p)
    dv = np.asarray(values, dtype=np.float64) - np.asarray(returns, dtype=np.float64)
    d_r = r * d_lp                                      # dr = r dlp
    # policy: rows on the unclipped branch move with r, clipped rows not at all
    d_policy = (np.where(sel, np.abs(A), 0.0) * d_r).sum() / md
    d_value = (2.0 * np.abs(dv) * d_v).sum() / md
    d_rowent = (d_p * np.abs(logit)).sum(1)
    d_ent = d_rowent.sum() / (3.0 * md)
    d_mean = d_r.sum() / md
    mean, std = base["ratio_mean"], base["ratio_std"]
    # d std = sum (r_i - mean) dr_i / ((m - 1) std)
    d_std = (np.abs(r - mean) * d_r).sum() / ((m - 1) * std) if m > 1 else 0.0
    out = dict(total_loss=d_policy + abs(value_coef) * d_value + abs(entropy_coef) * d_ent, policy_loss=d_policy,
               value_loss=d_value, entropy=d_ent, ratio_mean=d_mean, ratio_min=float(d_r[np.argmin(r)]),
               ratio_max=float(d_r[np.argmax(r)]), ratio_std=d_std, clipped_frac=0.0)
    # grad_logits = g (a - p) + c logit(p) p (1 - p), g = -A r / m on the selected rows
    g = np.where(sel, -A * r / md, 0.0)
    d_g = np.where(sel, np.abs(A) * d_r / md, 0.0)
    a = action_bits(actions)
    c = abs(entropy_coef) / (3.0 * md)
    # d/dp [logit p (1 - p)] = 1 + logit (1 - 2 p)
    out["grad_logits"] = (d_g[:, None] * np.abs(a - p) + np.abs(g)[:, None] * d_p
                          + c * np.abs(1.0 + logit * (1.0 - 2.0 * p)) * d_p)
    out["grad_values"] = abs(value_coef) * 2.0 * d_v / md
    return out


def fixture_losses(g) -> dict:
    """:func:`losses` fed the notebook's own per-row outputs recorded in the
    fixture g (losses.npz): its new_log_probs, probabilities and values, and
    the row entropy of those probabilities rounded to float32."""
    _, ent = row_log_prob_entropy(g["probs"], g["actions"])
    return losses(g["new_log_probs"], ent.astype(np.float32), g["probs"], g["values"], g["old_log_probs"],
                  g["advantages"], g["returns"], g["actions"], float(g["clip_epsilon"]), float(g["entropy_coef"]),
                  float(g["value_coef"]))


def reference_gap(g) -> dict:
    """|the notebook's float32 result - the float64 restatement fed the
    notebook's own rows|: each scalar's, and per element for the two
    gradients.  This is the reference's own float32 noise (its float32
    products, expf and reductions); no kernel output enters it."""
    out = fixture_losses(g)
    gap = {k: abs(float(g[k]) - out[k]) for k in SCALARS}
    gap["grad_logits"] = np.abs(g["grad_logits"].astype(np.float64) - out["grad_logits"])
    gap["grad_values"] = np.abs(g["grad_values"].astype(np.float64) - out["grad_values"])
    return gap
