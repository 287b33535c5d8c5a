"""NumPy restatement of the keyed permutation behind shuffle_indices /
shuffle_batch (include/dronestep.h, csrc/shuffle.hip) and of ppo_update's
minibatch slicing.  The definition is the contract; the device is held to it
bit for bit (tests/test_gpu_shuffle.py).

    b = bit_length(m - 1) (0 for m == 1);  h = max(1, ceil(b / 2));  mask = 2^h - 1
    cipher(x) on [0, 2^(2h)): (L, R) = (x >> h, x & mask); 8 rounds r = 0..7 of
        F = philox4x32_10((R, r, epoch_lo, epoch_hi ^ 0xC3C3C3C3), (seed_lo, seed_hi))[0] & mask
        (L, R) = (R, L ^ F)
      then x = (L << h) | R
    perm(j): x = j; apply the cipher until x < m  (cycle walking)
"""
import numpy as np

import golden_data as gd

ROUNDS = 8
EPOCH_TAG = 0xC3C3C3C3


def half_bits(m: int) -> int:
    b = (m - 1).bit_length()
    return max(1, (b + 1) // 2)


def cipher(x, h, seed, epoch, rounds=ROUNDS):
    """The Feistel network on a uint32 array x of domain values; epoch is one
    integer or an array of them, one per element of x."""
    mask = np.uint32((1 << h) - 1)
    seed = int(seed) & (2**64 - 1)
    epoch = np.asarray(epoch, dtype=object) & (2**64 - 1)
    n = x.shape[0]
    full = lambda v: np.broadcast_to(np.asarray(v, dtype=np.uint32), (n,))  # noqa: E731
    k0, k1 = full(seed & 0xFFFFFFFF), full(seed >> 32)
    e0 = full((epoch & 0xFFFFFFFF).astype(np.uint32))
    e1 = full(((epoch >> 32) ^ EPOCH_TAG).astype(np.uint32))
    left, right = x >> np.uint32(h), x & mask
    for r in range(rounds):
        f = gd.philox4x32_10_np(right, full(r), e0, e1, k0, k1)[0] & mask
        left, right = right, left ^ f
    return (left << np.uint32(h)) | right


def perms_ref(m: int, seed, epochs, rounds=ROUNDS, applications=None) -> np.ndarray:
    """perm(j) for j in [0, m) under each of epochs: int32 [len(epochs), m].
    applications (a list): receives the number of cipher applications made."""
    assert 1 <= m < 2**31
    h = half_bits(m)
    epochs = np.asarray([int(e) for e in epochs], dtype=object)
    x = np.tile(np.arange(m, dtype=np.uint32), len(epochs))
    key = np.repeat(epochs, m)
    todo = np.arange(x.shape[0])
    count = 0
    while todo.size:
        x[todo] = cipher(x[todo], h, seed, key[todo], rounds)
        count += todo.size
        todo = todo[x[todo] >= m]
    if applications is not None:
        applications.append(count)
    return x.astype(np.int32).reshape(len(epochs), m)


def perm_ref(m: int, seed: int = 0, epoch: int = 0, rounds=ROUNDS, applications=None) -> np.ndarray:
    """perm(j) for j in [0, m): int32 [m]."""
    return perms_ref(m, seed, [epoch], rounds, applications)[0]


def minibatch_ranges(m: int, size: int, drop_last: bool = False):
    """ppo_update's minibatches of m shuffled rows: [i size, min((i + 1) size, m)),
    without the tail shorter than size when drop_last."""
    out, lo = [], 0
    while lo < m:
        hi = min(lo + size, m)
        if hi - lo == size or not drop_last:
            out.append((lo, hi))
        lo = hi
    return out
