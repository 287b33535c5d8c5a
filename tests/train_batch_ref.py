"""NumPy restatement of the four stages of ``delivery_drone_amd.train_batch``
(plan, gather, advantages, normalise): float32 GAE in compute_gae's operation
order, double returns, float64 statistics.  ``test_train_batch_cpu.py`` pins it
to the notebooks' own results (tests/golden/train_batch/); the GPU tests
compare the kernels with it."""
import numpy as np

F32 = np.float32


def plan(done):
    """(length int32 [N], offset int64 [N+1], ended uint8 [N]) of done [T][N]."""
    done = np.asarray(done) != 0
    T, n = done.shape
    ended = done.any(axis=0)
    first = done.argmax(axis=0)
    length = np.where(ended, first + 1, T).astype(np.int32)
    offset = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(length, out=offset[1:])
    return length, offset, ended.astype(np.uint8)


def gather(x, length):
    """Episode-major rows of x [T][N](...)."""
    x = np.asarray(x)
    parts = [x[:length[i], i] for i in range(len(length))]
    return np.concatenate(parts, axis=0) if parts else x[:0, 0]


def actions_f32(bits):
    """uint8 bitmasks [M] -> float32 [M][3] in (main, left, right) order."""
    bits = np.asarray(bits, dtype=np.uint8)
    return np.stack([(bits >> k) & 1 for k in range(3)], axis=-1).astype(F32)


def scatter(flat, length, T, fill=0):
    """The inverse of gather for a [M] array: [T][N], `fill` past each episode."""
    out = np.full((T, len(length)), fill, dtype=np.asarray(flat).dtype)
    o = 0
    for i, ln in enumerate(length):
        out[:ln, i] = flat[o:o + ln]
        o += ln
    return out


def episode_return(reward, length):
    """sum(rewards) per lane: doubles added in frame order."""
    reward = np.asarray(reward)
    out = np.zeros(len(length), dtype=np.float64)
    for i, ln in enumerate(length):
        s = 0.0
        for t in range(ln):
            s = s + float(reward[t, i])
        out[i] = s
    return out


def gae_flat(reward, values, length, offset, ended, bootstrap=None, gamma=0.99, lam=0.95):
    """(advantages, returns) float32 [M]: compute_gae per episode, dones all
    false but the last frame of an ended episode."""
    reward = np.asarray(reward)
    values = np.asarray(values, dtype=F32)
    g, gl, one = F32(gamma), F32(gamma * lam), F32(1.0)
    adv = np.zeros(int(offset[-1]), dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for i, ln in enumerate(length):
            o = int(offset[i])
            e = bool(ended[i])
            v_next = F32(0.0) if e or bootstrap is None else F32(bootstrap[i])
            mask = F32(0.0) if e else one
            gae = F32(0.0)
            for t in range(ln - 1, -1, -1):
                v = values[o + t]
                delta = F32(F32(F32(reward[t, i]) + F32(F32(g * v_next) * mask)) - v)
                gae = F32(delta + F32(F32(gl * mask) * gae))
                adv[o + t] = gae
                v_next, mask = v, one
    return adv, (adv + values).astype(F32)


def returns_flat(reward, length, offset, gamma=0.99):
    """compute_returns per episode in double, rounded to float32 once."""
    reward = np.asarray(reward)
    out = np.zeros(int(offset[-1]), dtype=np.float64)
    gamma = float(gamma)
    for i, ln in enumerate(length):
        o = int(offset[i])
        G = 0.0
        for t in range(ln - 1, -1, -1):
            G = float(reward[t, i]) + gamma * G
            out[o + t] = G
    return out.astype(F32)


def normalize(a):
    """(mean, unbiased std, (a - mean) / (std + 1e-8) as float32) in float64."""
    a64 = np.asarray(a, dtype=F32).astype(np.float64)
    with np.errstate(all="ignore"):
        mean = a64.mean() if a64.size else np.float64("nan")
        std = a64.std(ddof=1) if a64.size > 1 else np.float64("nan")
        out = ((a64 - mean) / (std + 1e-8)).astype(F32)
    return np.float64(mean), np.float64(std), out
