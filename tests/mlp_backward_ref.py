"""Float64 NumPy restatement of the notebooks' network (DroneGamerBoi /
DroneTeacherBoi: Linear LayerNorm ReLU x 3, Linear) forward and backward, as
csrc/mlp_backward.hip's header states it: what the GPU tests compare
dd_mlp_backward with, and what tests/test_mlp_backward_cpu.py pins to float64
torch autograd and to the notebook's own float32 gradients
(tests/golden/mlp_backward/grads.npz).

Per layer (a = its input):  h = W a + b;  xh = (h - mean h) rstd, rstd = 1 /
sqrt(var_biased + eps);  y = gamma xh + beta;  a' = max(y, 0).  Backward:  dy =
da' [y > 0];  dgamma = sum_rows dy xh;  dbeta = sum_rows dy;  g = dy gamma;  dh =
rstd (g - mean(g) - xh mean(g xh));  dW = sum_rows dh (x) a;  db = sum_rows dh;
da = W^T dh.  Next to every gradient its condition sum S = sum_rows |the row's
contribution|: the scale a float32 evaluation's rounding is measured on.
"""
from __future__ import annotations

import numpy as np

KEYS = ("0.weight", "0.bias", "1.weight", "1.bias", "3.weight", "3.bias", "4.weight", "4.bias",
        "6.weight", "6.bias", "7.weight", "7.bias", "9.weight", "9.bias")
LAYERS = (("0", "1"), ("3", "4"), ("6", "7"))
U = 2.0 ** -24


TINY = np.float32(2.0 ** -100)
# "relu": (unit, gamma, beta) of every LayerNorm, n its width.  gamma = 0 makes
# y = beta exactly in float32 and float64 alike, so [y > 0] is unambiguous.
RELU_UNITS = ((3, 0.0, 0.0), (17, 0.0, TINY), (40, 0.0, -TINY), (-1, 0.0, 0.0), (0, 0.0, TINY))
RELU_OFF, RELU_ON = (3, 40, -1), (17, 0)
VARIANTS = ("relu", "var0")


def crafted(sd, variant):
    """A fixture network with the edges the fixture rows never reach, as a new
    float32 state_dict (sd is left alone).
    "relu": units 3, 40 and n - 1 of every LayerNorm have y = 0, -2^-100, 0 on
    every row (no gradient passes), units 17 and 0 have y = 2^-100 (it passes
    on every row).
    "var0": 0.weight = 0 and 0.bias = 0.25: layer 1 has zero variance, xh = 0
    exactly and rstd = 1 / sqrt(eps)."""
    out = {k: np.array(sd[k], dtype=np.float32) for k in KEYS}
    if variant == "relu":
        for _, ln in LAYERS:
            for j, gamma, beta in RELU_UNITS:
                out[ln + ".weight"][j] = gamma
                out[ln + ".bias"][j] = beta
    elif variant == "var0":
        out["0.weight"][:] = 0.0
        out["0.bias"][:] = 0.25
    else:
        raise ValueError(variant)
    return out


def crafted_zeros(sd, variant):
    """{name: (key, index)} of the gradient elements that are exact zeros on
    the crafted network by construction, whatever the rows: dgamma and dbeta
    of a unit that passes no gradient, and the next Linear's dW column of a
    unit whose activation is 0 (and dgamma of a unit whose xh is 0)."""
    nxt = {"1": "3.weight", "4": "6.weight", "7": "9.weight"}
    zeros = {}
    if variant == "relu":
        for _, ln in LAYERS:
            for j in RELU_OFF:
                zeros[f"dgamma {ln}.weight[{j}]"] = (ln + ".weight", j)
                zeros[f"dbeta {ln}.bias[{j}]"] = (ln + ".bias", j)
                zeros[f"{nxt[ln]}[:, {j}]"] = (nxt[ln], (slice(None), j))
    else:
        zeros["dgamma 1.weight (xh = 0)"] = ("1.weight", slice(None))
        for j in np.flatnonzero(np.asarray(sd["1.bias"]) <= 0):  # y = beta exactly
            zeros[f"dbeta 1.bias[{j}]"] = ("1.bias", j)
            zeros[f"3.weight[:, {j}]"] = ("3.weight", (slice(None), j))
    return zeros


def _f64(sd):
    return {k: np.asarray(sd[k], dtype=np.float64) for k in KEYS}


def forward(sd, states, eps=1e-5):
    """The last Linear's output z [m, K] (pre-Sigmoid for the actor) and what
    the backward needs: each layer's input, xh, rstd and y."""
    p = _f64(sd)
    a = np.asarray(states, dtype=np.float64)
    cache = []
    for lin, ln in LAYERS:
        h = a @ p[lin + ".weight"].T + p[lin + ".bias"]
        mean = h.mean(1, keepdims=True)
        rstd = 1.0 / np.sqrt(((h - mean) ** 2).mean(1, keepdims=True) + eps)
        xh = (h - mean) * rstd
        y = xh * p[ln + ".weight"] + p[ln + ".bias"]
        cache.append((a, xh, rstd, y))
        a = np.maximum(y, 0.0)
    z = a @ p["9.weight"].T + p["9.bias"]
    return z, cache, a


def backward(sd, states, grad_out, eps=1e-5):
    """(grads, S, norm): per-parameter float64 gradients in torch's shapes for
    grad_out [m, K] (or [m] for K = 1) at the last Linear's output, the
    condition sums, and the L2 norm over all fourteen."""
    p = _f64(sd)
    m = len(states)
    dz = np.asarray(grad_out, dtype=np.float64).reshape(m, -1)
    _, cache, a3 = forward(sd, states, eps)
    grads, S = {}, {}
    grads["9.weight"], S["9.weight"] = dz.T @ a3, np.abs(dz).T @ np.abs(a3)
    grads["9.bias"], S["9.bias"] = dz.sum(0), np.abs(dz).sum(0)
    da = dz @ p["9.weight"]
    for (lin, ln), (a, xh, rstd, y) in reversed(list(zip(LAYERS, cache))):
        dy = da * (y > 0.0)
        grads[ln + ".weight"], S[ln + ".weight"] = (dy * xh).sum(0), np.abs(dy * xh).sum(0)
        grads[ln + ".bias"], S[ln + ".bias"] = dy.sum(0), np.abs(dy).sum(0)
        g = dy * p[ln + ".weight"]
        dh = rstd * (g - g.mean(1, keepdims=True) - xh * (g * xh).mean(1, keepdims=True))
        grads[lin + ".weight"], S[lin + ".weight"] = dh.T @ a, np.abs(dh).T @ np.abs(a)
        grads[lin + ".bias"], S[lin + ".bias"] = dh.sum(0), np.abs(dh).sum(0)
        da = dh @ p[lin + ".weight"]
    norm = float(np.sqrt(sum(float((grads[k] ** 2).sum()) for k in KEYS)))
    return grads, S, norm


def head_spread(sd, states, d_out, eps=1e-5):
    """First-order spread of every gradient when each element of grad_out moves
    within d_out [m, K] (or [m]): the backward is linear in grad_out once the
    forward is fixed, so element (i, k) contributes |d grads / d grad_out[i, k]|
    d_out[i, k], summed with no cancellation assumed.  |d/d grad_out| is taken
    row by row: the backward of the row's unit gradient."""
    m = len(states)
    d_out = np.asarray(d_out, dtype=np.float64).reshape(m, -1)
    K = d_out.shape[1]
    out = None
    for k in range(K):
        unit = np.zeros((m, K))
        unit[:, k] = d_out[:, k]
        # per-row contributions in absolute value: S of the backward fed d_out in column k alone
        # bounds sum_rows |row's gradient| x its bound (S takes the absolute value per row and factor)
        _, S, _ = backward(sd, states, unit, eps)
        out = S if out is None else {key: out[key] + S[key] for key in out}
    return out


def gap_units(got, want, S):
    """max over elements of |got - want| / (2^-24 S), per tensor; elements with
    S == 0 must match exactly (they are exact zeros)."""
    units = {}
    for k in KEYS:
        err = np.abs(np.asarray(got[k], dtype=np.float64) - want[k])
        zero = S[k] == 0
        assert np.all(err[zero] == 0), k
        units[k] = float((err[~zero] / (U * S[k][~zero])).max()) if (~zero).any() else 0.0
    return units


def reference_gap(g, fx, nets):
    """The reference's own float32 gap: the notebook's .grad (fx:
    mlp_backward/grads.npz) against :func:`backward` fed ppo_loss_ref's
    float64 head gradients on the notebook's own rows (g: ppo_loss/losses.npz),
    per tensor in units of 2^-24 S, and G, the largest of them.  No kernel
    output enters it."""
    import ppo_loss_ref
    heads = ppo_loss_ref.fixture_losses(g)
    units = {}
    for tag, key in (("actor", "grad_logits"), ("critic", "grad_values")):
        grads, S, _ = backward(nets[tag], g["states"], heads[key])
        units[tag] = gap_units({k: fx[f"{tag}.{k}"] for k in KEYS}, grads, S)
    return units, max(max(v.values()) for v in units.values())
