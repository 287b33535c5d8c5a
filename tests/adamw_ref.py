"""NumPy float64 restatement of dd_adamw_step's contract (include/dronestep.h,
csrc/adamw.hip): torch.optim.AdamW (decoupled weight decay, amsgrad=False,
maximize=False) on a network's flat parameter vector.

    decay = 1 - lr wd,  omb1 = 1 - beta1,  omb2 = 1 - beta2
    pd = p decay;  md = beta1 m + omb1 g;  vd = beta2 v + omb2 (g g)
    b1t' = b1t beta1;  b2t' = b2t beta2          (running products, not pow)
    pn = pd - (lr / (1 - b1t')) (md / (sqrt(vd) / sqrt(1 - b2t') + eps))

from the float32 p, g, m, v in double, in that order of operations, each of
pn, md, vd rounded to float32 once (``exact=True``: no rounding, everything
stays float64, for the comparison with float64 torch).  IEEE double +, *, /
and sqrt are correctly rounded on the host and on the device, so the kernel is
expected to give these bits.  With ``f16x3=True`` the candidate parameters
must pass :func:`f16x3_refuses`, MlpNet._validated's operand-range rules; a
refused step returns its inputs unchanged and sets the status bit.
"""
from __future__ import annotations

import numpy as np

KEYS = ("0.weight", "0.bias", "1.weight", "1.bias", "3.weight", "3.bias", "4.weight", "4.bias",
        "6.weight", "6.bias", "7.weight", "7.bias", "9.weight", "9.bias")
REFUSED = 1
NOTEBOOK_LR = {"actor": 3e-4, "critic": 1e-3}  # the training cell's two optimizers; everything else torch's default
DEFAULTS = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)


def shapes(out_dim: int) -> dict:
    return {"0.weight": (128, 15), "0.bias": (128,), "1.weight": (128,), "1.bias": (128,),
            "3.weight": (128, 128), "3.bias": (128,), "4.weight": (128,), "4.bias": (128,),
            "6.weight": (64, 128), "6.bias": (64,), "7.weight": (64,), "7.bias": (64,),
            "9.weight": (out_dim, 64), "9.bias": (out_dim,)}


def slices(out_dim: int) -> dict:
    """Each tensor's slice of the flat vector (KEYS order)."""
    out, first = {}, 0
    for k, shape in shapes(out_dim).items():
        n = int(np.prod(shape))
        out[k] = slice(first, first + n)
        first += n
    return out


def numel(out_dim: int) -> int:
    return 27456 + 65 * out_dim


def flatten(sd: dict, prefix: str = "") -> np.ndarray:
    return np.concatenate([np.asarray(sd[prefix + k]).reshape(-1) for k in KEYS])


def unflatten(flat: np.ndarray, out_dim: int) -> dict:
    sh = shapes(out_dim)
    return {k: flat[s].reshape(sh[k]) for k, s in slices(out_dim).items()}


def new_state() -> dict:
    return dict(step=0, b1t=1.0, b2t=1.0, status=0)


def f16x3_refuses(p: np.ndarray, out_dim: int) -> bool:
    """MlpNet._validated's f16x3 rules on a flat float32 parameter vector."""
    s = slices(out_dim)
    for k in ("0.weight", "3.weight", "6.weight"):
        w = p[s[k]]
        if not np.isfinite(w).all() or float(np.abs(w).max()) >= 65504.0 / 32:
            return True
    for g, b, rows in (("1.weight", "1.bias", 128), ("4.weight", "4.bias", 128), ("7.weight", "7.bias", 64)):
        bound = float(np.abs(p[s[g]]).max()) * rows ** 0.5 * (1 + 2 ** -8) + float(np.abs(p[s[b]]).max())
        if not bound < 128.0:
            return True
    return False


def step(p, g, m, v, st, *, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, out_dim=3, f16x3=False, exact=False):
    """One step: ``(p, m, v, state)`` after it.  Inputs are not modified."""
    beta1, beta2 = float(betas[0]), float(betas[1])
    lr, eps, wd = float(lr), float(eps), float(weight_decay)
    decay, omb1, omb2 = 1.0 - lr * wd, 1.0 - beta1, 1.0 - beta2
    p64, g64, m64, v64 = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    b1t, b2t = st["b1t"] * beta1, st["b2t"] * beta2
    step_size = lr / (1.0 - b1t)
    root = np.sqrt(np.float64(1.0 - b2t))
    with np.errstate(all="ignore"):
        pd = p64 * decay
        md = beta1 * m64 + omb1 * g64
        vd = beta2 * v64 + omb2 * (g64 * g64)
        pn = pd - step_size * (md / (np.sqrt(vd) / root + eps))
        if exact:
            out = pn, md, vd
        else:
            out = pn.astype(np.float32), md.astype(np.float32), vd.astype(np.float32)
    if f16x3 and f16x3_refuses(out[0].astype(np.float32), out_dim):
        return p, m, v, dict(st, status=st["status"] | REFUSED)
    return out + (dict(step=st["step"] + 1, b1t=b1t, b2t=b2t, status=st["status"]),)


# ---- the tests' fixed trajectory ---------------------------------------------------

STEPS = 8
SCALES = (1.0, -0.75, 2.5, -1.0, 0.3125, 1.5, -2.0, 0.625)  # step s's gradient is the notebook's times this ...


def trajectory(fx: dict, tag: str, out_dim: int, seed: int = 12):
    """Eight gradients for one network from the notebook's own
    (tests/golden/mlp_backward/grads.npz): step s is the fixture times
    SCALES[s] times a seeded per-element sign (so exp_avg sees cancellation);
    one element in 16 has an exactly zero gradient in every step; a few are
    1e-30 (g g underflows float32) or 1e-20 (exp_avg_sq is a float32
    denormal) throughout.  Returns ``(grads float32 [8][n], zero_idx, tiny_idx)``."""
    base = flatten({k: fx[f"{tag}.{k}"] for k in KEYS}).astype(np.float32)
    n = numel(out_dim)
    assert base.shape == (n,)
    rng = np.random.default_rng(seed + out_dim)
    zero_idx = np.sort(rng.choice(n, n // 16, replace=False))
    rest = np.setdiff1d(np.arange(n), zero_idx)
    tiny_idx = np.sort(rng.choice(rest, 12, replace=False))
    grads = np.empty((STEPS, n), dtype=np.float32)
    for s in range(STEPS):
        sign = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), n, p=[0.35, 0.65])
        grads[s] = base * np.float32(SCALES[s]) * sign
        grads[s, zero_idx] = 0.0
        grads[s, tiny_idx[:8]] = np.float32(1e-30) * sign[tiny_idx[:8]]
        grads[s, tiny_idx[8:]] = np.float32(1e-20)
    return grads, zero_idx, tiny_idx


def run(p0, grads, *, lr, out_dim, f16x3=False, exact=False, **hyper):
    """The restatement over ``grads``: per step ``(p, m, v, state)``."""
    p = np.asarray(p0, dtype=np.float64 if exact else np.float32)
    m, v, st = np.zeros_like(p), np.zeros_like(p), new_state()
    out = []
    for g in grads:
        p, m, v, st = step(p, g, m, v, st, lr=lr, out_dim=out_dim, f16x3=f16x3, exact=exact, **hyper)
        out.append((p, m, v, st))
    return out


def update_scale(grads, *, betas=(0.9, 0.999), eps=1e-8):
    """A per step: the update's size had nothing cancelled, the bias-corrected
    beta1-average of |g| over sqrt(v_hat) + eps, in float64.  [steps][n]."""
    beta1, beta2 = betas
    a = np.zeros(grads.shape[1])
    v = np.zeros(grads.shape[1])
    b1t = b2t = 1.0
    out = []
    for g in np.asarray(grads, dtype=np.float64):
        a = beta1 * a + (1.0 - beta1) * np.abs(g)
        v = beta2 * v + (1.0 - beta2) * g * g
        b1t *= beta1
        b2t *= beta2
        out.append((a / (1.0 - b1t)) / (np.sqrt(v / (1.0 - b2t)) + eps))
    return np.stack(out)


def gap_unit(p, lr, a):
    """2^-24 (|p| + lr A): the scale one float32 rounding of an AdamW step is measured on."""
    return 2.0 ** -24 * (np.abs(np.asarray(p, dtype=np.float64)) + lr * a)


def torch_adamw(p0_flat, grads, *, lr, out_dim, dtype, **hyper):
    """torch.optim.AdamW (foreach=False, fused=False) on CPU tensors of
    ``dtype`` over the fourteen parameters: per step the flat parameters, and
    the optimizer itself at the end."""
    import torch
    sl, sh = slices(out_dim), shapes(out_dim)
    params = [torch.nn.Parameter(torch.tensor(np.asarray(p0_flat)[sl[k]].reshape(sh[k]), dtype=dtype)) for k in KEYS]
    opt = torch.optim.AdamW(params, lr=lr, foreach=False, fused=False, **hyper)
    out = []
    for g in grads:
        for k, q in zip(KEYS, params):
            q.grad = torch.tensor(np.asarray(g)[sl[k]].reshape(sh[k]), dtype=dtype)
        opt.step()
        out.append(np.concatenate([q.detach().numpy().reshape(-1) for q in params]))
    return out, opt, params
