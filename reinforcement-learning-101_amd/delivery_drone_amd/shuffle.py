"""A reproducible shuffle of a training batch's rows, on device.

``perm = shuffle_indices(M, seed=s, epoch=e)`` is a stateless keyed permutation
of ``[0, M)`` (``dd_shuffle_indices``, ``csrc/shuffle.hip``; the definition is
in ``include/dronestep.h``): every thread computes ``perm[j]`` for its own
``j`` from ``(M, seed, epoch)`` alone, so there is no sort and no random state,
and the same key gives the same permutation on every run, device and
sharding.  :func:`shuffle_batch` moves a PPO batch's five tensors by it,
``out[j] = in[perm[j]]``, in one launch (``dd_shuffle_rows``); consecutive row
ranges of the result are the minibatches of :func:`ppo_update`.  Both run on
the current stream and read nothing back.

``seed`` and ``epoch`` are host integers (taken modulo 2^64): a captured
launch replays the permutation of the key it was captured with.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import torch

from . import abi
from .train_batch import PpoBatch, PpoEpisodesBatch

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


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


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
        abi.check(abi.lib().dd_shuffle_indices(m, int(seed) & _U64, int(epoch) & _U64, out.data_ptr(), _stream(dev)),
                  "dd_shuffle_indices")
    return out


def _column(name, t, m, dev):
    """A source column as the kernel reads it, or None."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a tensor or None, got {type(t).__name__}")
    if t.device != dev:
        raise ValueError(f"{name} is on {t.device}, the batch on {dev}")
    shape = tuple(t.shape)
    if name == "actions":
        if t.dtype == torch.uint8 and shape == (m,):
            return t.detach().contiguous()
        if t.dtype == torch.float32 and shape == (m, 3):
            return t.detach().contiguous()
        raise ValueError(f"actions must be uint8 [{m}] bitmasks or float32 [{m}, 3], got {t.dtype} {shape}")
    want = (m, abi.DD_OBS_DIM) if name == "states" else (m,)
    if shape != want:
        raise ValueError(f"{name} must have shape {want}, got {shape}")
    return t.detach().to(torch.float32).contiguous()


def shuffle_batch(batch, *, seed: int = 0, epoch: int = 0, out: Optional[ShuffledBatch] = None) -> ShuffledBatch:
    """``batch`` with its rows in the order ``shuffle_indices(M, seed=seed,
    epoch=epoch)``: a :class:`PpoBatch`, a :class:`PpoEpisodesBatch`, or the
    five tensors ``(states, actions, old_log_probs, advantages, returns)``, of
    which any may be ``None`` (not all).  Rows are moved, not computed: every
    bit of a row arrives, NaN payloads included.

    ``out``: a previous :class:`ShuffledBatch` of the same shapes to write
    into (``ValueError`` if it does not fit); it must not share memory with
    the batch, the shuffle does not run in place."""
    if isinstance(batch, (PpoBatch, PpoEpisodesBatch)):
        five = tuple(batch[:5])
    elif isinstance(batch, (tuple, list)) and len(batch) == 5:
        five = tuple(batch)
    else:
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
    src = [_column(name, t, m, dev) for name, t in zip(_COLUMNS, five)]
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
            if s is not None and (not isinstance(d, torch.Tensor) or d.shape != s.shape or d.dtype != s.dtype
                                  or d.device != dev or not d.is_contiguous()):
                raise ValueError(f"out.{name} must be a contiguous {s.dtype} tensor of shape {tuple(s.shape)} on {dev}")
        if (not isinstance(indices, torch.Tensor) or tuple(indices.shape) != (m,) or indices.dtype != torch.int32
                or indices.device != dev or not indices.is_contiguous()):
            raise ValueError(f"out.indices must be a contiguous int32 tensor of shape ({m},) on {dev}")
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    actions = src[1]
    fmt = abi.DD_ACT_BITMASK if actions is None or actions.dtype == torch.uint8 else abi.DD_ACT_F32X3
    io = abi.DDShuffleIO(ptr(src[0]), ptr(src[1]), ptr(src[2]), ptr(src[3]), ptr(src[4]), fmt, 0,
                         ptr(dst[0]), ptr(dst[1]), ptr(dst[2]), ptr(dst[3]), ptr(dst[4]), indices.data_ptr())
    if m:
        abi.check(abi.lib().dd_shuffle_rows(ctypes.byref(io), m, int(seed) & _U64, int(epoch) & _U64, _stream(dev)),
                  "dd_shuffle_rows")
    return ShuffledBatch(*dst, indices)
