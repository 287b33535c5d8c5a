"""A reproducible shuffle of a training batch's rows, on device.

``perm = shuffle_indices(M, seed=s, epoch=e)`` is a stateless keyed permutation
of ``[0, M)`` (``dd_shuffle_indices``, ``csrc/shuffle.hip``; the definition is
in ``include/dronestep.h``): every thread computes ``perm[j]`` for its own
``j`` from ``(M, seed, epoch)`` alone, so there is no sort and no random state,
and the same key gives the same permutation on every run, device and
sharding.  :func:`shuffle_batch` moves a PPO batch's five tensors by it,
``out[j] = in[perm[j]]``, in one launch (``dd_shuffle_rows``); consecutive row
ranges of the result are the minibatches of :func:`ppo_update`.  Both run on
the current stream and read nothing back.  The columns are checked by
``_args.column``, as ``ppo_update(fused=True)`` checks the ones it stacks.

``seed`` and ``epoch`` are host integers (taken modulo 2^64): a captured
launch replays the permutation of the key it was captured with.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import torch

from . import _args, abi

__all__ = ["ShuffledBatch", "shuffle_batch", "shuffle_indices"]

_U64 = (1 << 64) - 1
_MAX_ROWS = 1 << 31


class ShuffledBatch(NamedTuple):
    """Row ``j`` of every column is row ``indices[j]`` of the batch it was
    shuffled from.  A column the batch did not have is ``None``."""
    states: Optional[torch.Tensor]         # [M, 15] float32
    actions: Optional[torch.Tensor]        # uint8 [M] bitmasks or float32 [M, 3], as given
    old_log_probs: Optional[torch.Tensor]  # [M] float32
    advantages: Optional[torch.Tensor]     # [M] float32
    returns: Optional[torch.Tensor]        # [M] float32
    indices: torch.Tensor                  # [M] int32: the permutation


_COLUMNS = ShuffledBatch._fields[:5]


def _rows(m) -> int:
    m = int(m)
    if not 0 <= m < _MAX_ROWS:
        raise ValueError(f"the number of rows must be in [0, 2^31), got {m}")
    return m


def shuffle_indices(m: int, *, seed: int = 0, epoch: int = 0, device) -> torch.Tensor:
    """The permutation of ``[0, m)`` keyed by ``(seed, epoch)``: int32 ``[m]``
    on ``device`` (a GPU)."""
    m = _rows(m)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"shuffle_indices runs on a GPU, got device {dev}")
    out = torch.empty(m, dtype=torch.int32, device=dev)
    if m:
        abi.check(abi.lib().dd_shuffle_indices(m, int(seed) & _U64, int(epoch) & _U64, out.data_ptr(),
                                               _args.stream_ptr(dev)), "dd_shuffle_indices")
    return out


def shuffle_batch(batch, *, seed: int = 0, epoch: int = 0, out: Optional[ShuffledBatch] = None) -> ShuffledBatch:
    """``batch`` with its rows in the order ``shuffle_indices(M, seed=seed,
    epoch=epoch)``: a :class:`PpoBatch`, a :class:`PpoEpisodesBatch`, or the
    five tensors ``(states, actions, old_log_probs, advantages, returns)``, of
    which any may be ``None`` (not all).  Rows are moved, not computed: every
    bit of a row arrives, NaN payloads included.

    ``out``: a previous :class:`ShuffledBatch` of the same shapes to write
    into (``ValueError`` if it does not fit); it must not share memory with
    the batch, the shuffle does not run in place."""
    five = _args.batch_five(batch)
    if five is None and isinstance(batch, (tuple, list)) and len(batch) == 5:
        five = tuple(batch)
    if five is None:
        raise ValueError("batch must be a PpoBatch, a PpoEpisodesBatch or the five tensors "
                         "(states, actions, old_log_probs, advantages, returns)")
    first = next((t for t in five if isinstance(t, torch.Tensor)), None)
    if first is None:
        raise ValueError("the batch has no column to shuffle")
    if first.dim() < 1:
        raise ValueError("the batch's columns must have a row dimension")
    m, dev = _rows(first.shape[0]), first.device
    if dev.type != "cuda":
        raise ValueError(f"shuffle_batch runs on a GPU, the batch is on {dev}")
    src = [_args.column(name, t, m, dev) for name, t in zip(_COLUMNS, five)]
    if out is None:
        dst = [None if s is None else torch.empty_like(s) for s in src]
        indices = torch.empty(m, dtype=torch.int32, device=dev)
    else:
        if not isinstance(out, ShuffledBatch):
            raise ValueError("out must be a ShuffledBatch")
        dst, indices = list(out[:5]), out.indices
        for name, s, d in zip(_COLUMNS, src, dst):
            if (s is None) != (d is None):
                raise ValueError(f"out.{name} is {'missing' if d is None else 'present'}, the batch's is not")
            if s is not None:
                _args.check_out(d, s.shape, s.dtype, dev, f"out.{name} must be a contiguous {s.dtype} tensor")
        _args.check_out(indices, (m,), torch.int32, dev, "out.indices must be a contiguous int32 tensor")
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    fmt = abi.DD_ACT_BITMASK if src[1] is None else _args.action_format(src[1])
    io = abi.DDShuffleIO(ptr(src[0]), ptr(src[1]), ptr(src[2]), ptr(src[3]), ptr(src[4]), fmt, 0,
                         ptr(dst[0]), ptr(dst[1]), ptr(dst[2]), ptr(dst[3]), ptr(dst[4]), indices.data_ptr())
    if m:
        abi.check(abi.lib().dd_shuffle_rows(ctypes.byref(io), m, int(seed) & _U64, int(epoch) & _U64,
                                            _args.stream_ptr(dev)), "dd_shuffle_rows")
    return ShuffledBatch(*dst, indices)
