"""The PPO notebook's optimizer steps and its whole PHASE 3, on device.

:class:`AdamW` is ``torch.optim.AdamW`` on an :class:`MlpNet`'s flat parameter
buffer (``dd_adamw_step``, ``csrc/adamw.hip``): one launch per step that also
keeps the step count and the bias corrections on the device, so the host
passes no ``t`` and a captured step can be replayed.  Where the network runs
``compute="f16x3"`` the kernel applies the operand-range rules of
``MlpNet.load_state_dict`` to the parameters it is about to write and, if they
fail, writes nothing but a status bit.  :func:`ppo_update` is the training
cell's ``for epoch in range(num_epochs)`` loop: :func:`ppo_losses`,
:meth:`MlpNet.backward` and the two optimizer steps per epoch, with the
per-epoch logs left on the device.  Nothing here reads back to the host
unless asked (:meth:`AdamW.status`).  What an update accepts is stated once,
by :func:`_plan` from the checks of ``_args``, for the loop and for
``fused=True``; an :class:`AdamW` owns the gradient buffer every update
function steps it from (:meth:`AdamW.grad_buffer`).
"""
from __future__ import annotations

import copy
import ctypes
import math
import struct
from typing import Dict, Mapping, NamedTuple, Optional, Union

import torch

from . import _args, abi
from .policy import STATE_DICT_KEYS, MlpNet
from .ppo_loss import ppo_losses
from .shuffle import ShuffledBatch, shuffle_batch

__all__ = ["AdamW", "PpoUpdate", "ppo_update", "fused_rows", "fits_fused", "FUSED_MAX_ROWS"]

_STATE = struct.Struct("<qddii")  # DDAdamWState


class AdamW:
    """``torch.optim.AdamW(net.parameters(), lr, betas, eps, weight_decay)``
    for an :class:`MlpNet` (``amsgrad=False``, ``maximize=False``; the
    defaults are torch's).  It takes :meth:`MlpNet.flat_parameters` and updates
    that buffer in place; ``exp_avg`` and ``exp_avg_sq`` are float32 buffers of
    the same length, as torch keeps them.  Each element is evaluated in double
    and rounded to float32 once (include/dronestep.h)."""

    def __init__(self, net: MlpNet, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.01):
        if not isinstance(net, MlpNet):
            raise ValueError("AdamW optimizes an MlpNet")
        beta1, beta2 = (float(b) for b in betas)
        for name, x in (("lr", lr), ("eps", eps), ("weight_decay", weight_decay)):
            self._rate(name, x)
        for name, b in (("betas[0]", beta1), ("betas[1]", beta2)):
            if not 0.0 <= b < 1.0:
                raise ValueError(f"{name} must be in [0, 1), got {b!r}")
        self.net = net
        self._lr = float(lr)
        self.betas, self.eps, self.weight_decay = (beta1, beta2), float(eps), float(weight_decay)
        self._lib = net._lib
        if int(self._lib.dd_adamw_state_bytes()) != _STATE.size:
            raise abi.NativeLibraryError("DDAdamWState: the library's layout is not this module's; rebuild it")
        self.params = net.flat_parameters()
        self.exp_avg = torch.empty_like(self.params)
        self.exp_avg_sq = torch.empty_like(self.params)
        self._state = torch.empty(_STATE.size // 8, dtype=torch.int64, device=net.device)
        self._grad_out = None  # grad_buffer(): the flat gradient the update functions fill and step from
        # ppo_update(fused=True), on the actor's optimizer only: both networks' weight images and head
        # gradients; dd_ppo_update_fused_workspace() bytes
        self._fused_ws = None
        abi.check(self._lib.dd_adamw_init(self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.params.numel(),
                                          self._state.data_ptr(), net._stream()), "dd_adamw_init")

    @staticmethod
    def _rate(name, x) -> float:
        x = float(x)
        if not (math.isfinite(x) and x >= 0.0):
            raise ValueError(f"{name} must be finite and not negative, got {x!r}")
        return x

    @property
    def lr(self) -> float:
        return self._lr

    @lr.setter
    def lr(self, value) -> None:
        self._lr = self._rate("lr", value)

    def grad_buffer(self) -> torch.Tensor:
        """The optimizer's flat gradient buffer (``params``' shape), allocated
        on first use and the same tensor from then on: ``backward``'s ``out``."""
        if self._grad_out is None:
            self._grad_out = torch.empty_like(self.params)
        return self._grad_out

    def _hyper(self) -> abi.DDAdamWHyper:
        return abi.DDAdamWHyper(self._lr, self.betas[0], self.betas[1], self.eps, self.weight_decay)

    def step(self, grads: Union[torch.Tensor, Mapping[str, torch.Tensor]]) -> None:
        """One optimizer step from ``grads``: the flat gradient buffer, or the
        dict of views into it that :meth:`MlpNet.backward` returns.  Then
        ``dd_mlp_pack`` into the network's ``packed`` (same address).  Runs on
        the current stream and reads nothing back."""
        net = self.net
        flat = grads
        if isinstance(grads, Mapping):  # backward's dict: fourteen views of one flat buffer, in order
            first = None
            for k in STATE_DICT_KEYS:
                t = grads[k]
                if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous()
                        or t.shape != net._src[k].shape or (first is not None and t.data_ptr() != first)):
                    raise ValueError("grads must be the flat buffer MlpNet.backward fills, or its dict of views")
                first = t.data_ptr() + 4 * t.numel()
            flat = torch.as_strided(grads[STATE_DICT_KEYS[0]], (self.params.numel(),), (1,))
        if not isinstance(flat, torch.Tensor) or flat.device != net.device:
            raise ValueError(f"grads must be a tensor on {net.device}")
        if (tuple(flat.shape) != (self.params.numel(),) or flat.dtype != torch.float32 or not flat.is_contiguous()):
            raise ValueError(f"grads must be a contiguous float32 tensor of shape ({self.params.numel()},), got "
                             f"{flat.dtype} {tuple(flat.shape)}")
        hyper = self._hyper()
        io = abi.DDAdamWIO(self.params.data_ptr(), flat.data_ptr(), self.exp_avg.data_ptr(),
                           self.exp_avg_sq.data_ptr(), self._state.data_ptr(), net.packed.data_ptr(), net.out_dim,
                           net._mode, net.ln_eps, 0)
        abi.check(self._lib.dd_adamw_step(ctypes.byref(hyper), ctypes.byref(io), net._stream()), "dd_adamw_step")

    # ---- the device state block; each of these is a host read --------------------------
    def _read_state(self):
        return _STATE.unpack(self._state.cpu().numpy().tobytes())

    def status(self) -> int:
        """The sticky status word (``abi.DD_ADAMW_REFUSED``: a step's
        parameters were not ones ``compute="f16x3"`` can hold, and the step
        was dropped).  A host read, the only one, and only on request."""
        return int(self._read_state()[3])

    def step_count(self) -> int:
        """Steps committed so far (a host read)."""
        return int(self._read_state()[0])

    def raise_if_refused(self) -> None:
        """The ``ValueError`` :meth:`MlpNet.load_state_dict` would have raised
        for the parameters of a refused step."""
        if self.status() & abi.DD_ADAMW_REFUSED:
            raise ValueError("AdamW: a step led to parameters that compute='f16x3' cannot hold (it needs finite "
                             "hidden weights below 2047 in magnitude and LayerNorm outputs below 128) and was "
                             "dropped; the parameters of the last good step are in place; use compute='f32'")

    # ---- torch's optimizer-state layout ------------------------------------------------
    def state_dict(self) -> dict:
        """``torch.optim.AdamW(...).state_dict()`` for the fourteen parameters
        in ``STATE_DICT_KEYS`` order (``network.parameters()``' order): per
        parameter ``step``, ``exp_avg``, ``exp_avg_sq`` (clones), and one
        param_group, so a torch optimizer over the notebook's module loads it
        and carries on.  Before the first step the state is empty, as torch's."""
        group = copy.deepcopy(torch.optim.AdamW([torch.zeros(1)], lr=self._lr, betas=self.betas, eps=self.eps,
                                                weight_decay=self.weight_decay).state_dict()["param_groups"][0])
        group["params"] = list(range(len(STATE_DICT_KEYS)))
        step = self.step_count()
        state = {}
        if step > 0:
            m, v = self.net._views(self.exp_avg), self.net._views(self.exp_avg_sq)
            state = {i: {"step": torch.tensor(float(step)), "exp_avg": m[k].clone(), "exp_avg_sq": v[k].clone()}
                     for i, k in enumerate(STATE_DICT_KEYS)}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, state_dict: Mapping) -> "AdamW":
        """Take over from a ``torch.optim.AdamW`` (or an :class:`AdamW`):
        ``step``, ``exp_avg`` and ``exp_avg_sq`` of the fourteen parameters,
        and the group's ``lr``, ``betas``, ``eps``, ``weight_decay``.  The
        running products are rebuilt by ``step`` multiplications, as the
        kernel forms them; the status word is cleared."""
        groups = state_dict["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(STATE_DICT_KEYS):
            raise ValueError("expected one param_group over the network's fourteen parameters")
        group = groups[0]
        if group.get("amsgrad") or group.get("maximize"):
            raise ValueError("amsgrad and maximize are not supported")
        beta1, beta2 = (float(b) for b in group["betas"])
        for b in (beta1, beta2):
            if not 0.0 <= b < 1.0:
                raise ValueError(f"betas must be in [0, 1), got {group['betas']!r}")
        lr, eps, wd = (self._rate(k, group[k]) for k in ("lr", "eps", "weight_decay"))
        state = state_dict["state"]
        ids = list(group["params"])
        steps = set()
        m_new, v_new = torch.zeros_like(self.exp_avg), torch.zeros_like(self.exp_avg_sq)
        if state:
            m, v = self.net._views(m_new), self.net._views(v_new)
            for i, k in zip(ids, STATE_DICT_KEYS):
                s = state[i]
                if tuple(s["exp_avg"].shape) != tuple(m[k].shape) or tuple(s["exp_avg_sq"].shape) != tuple(m[k].shape):
                    raise ValueError(f"parameter {i} ({k}): expected shape {tuple(m[k].shape)}")
                steps.add(int(s["step"]))
                m[k].copy_(torch.as_tensor(s["exp_avg"]).detach().to(torch.float32))
                v[k].copy_(torch.as_tensor(s["exp_avg_sq"]).detach().to(torch.float32))
        if len(steps) > 1:
            raise ValueError(f"the parameters disagree on the step count: {sorted(steps)}")
        step = steps.pop() if steps else 0
        if step < 0:
            raise ValueError(f"negative step count {step}")
        b1t = b2t = 1.0
        for _ in range(step):
            b1t *= beta1
            b2t *= beta2
        self._lr, self.betas, self.eps, self.weight_decay = lr, (beta1, beta2), eps, wd
        self.exp_avg.copy_(m_new)
        self.exp_avg_sq.copy_(v_new)
        block = torch.frombuffer(bytearray(_STATE.pack(step, b1t, b2t, 0, 0)), dtype=torch.int64)
        self._state.copy_(block)
        return self


class PpoUpdate(NamedTuple):
    """What the training cell logs after PHASE 3.  ``logs`` maps
    ``total_loss``, ``policy_loss``, ``value_loss``, ``entropy``,
    ``ratio_mean``, ``ratio_min``, ``ratio_max``, ``ratio_std``,
    ``clipped_frac``, ``policy_grad_norm``, ``critic_grad_norm`` to
    ``[num_epochs]`` float64 device tensors (``[num_epochs, n_minibatches]``
    with ``minibatch_size``); ``summary`` holds what the cell derives from
    them, 0-d float64 device tensors."""
    logs: Dict[str, torch.Tensor]
    summary: Dict[str, torch.Tensor]


LOG_KEYS = ("total_loss", "policy_loss", "value_loss", "entropy", "ratio_mean", "ratio_min", "ratio_max", "ratio_std",
            "clipped_frac", "policy_grad_norm", "critic_grad_norm")


def minibatch_ranges(m: int, size: int, drop_last: bool = False):
    """The row ranges ``[lo, hi)`` of an epoch's minibatches over ``m``
    shuffled rows: ``[i size, min((i + 1) size, m))``, without the tail shorter
    than ``size`` when ``drop_last``."""
    stop = m - m % size if drop_last else m
    return [(lo, min(lo + size, m)) for lo in range(0, stop, size)]


#: the largest minibatch ``ppo_update(fused=True)`` takes: ``dd_mlp_backward``'s row tile
FUSED_MAX_ROWS = abi.DD_PPO_FUSED_ROWS


def fused_rows(m: int, minibatch_size: Optional[int] = None, drop_last: bool = False) -> int:
    """The rows of the largest step ``ppo_update(minibatch_size=...,
    drop_last=...)`` takes on a batch of ``m`` rows: ``m`` itself for the full
    batch, else the longest of :func:`minibatch_ranges` (0 when there is none)."""
    if minibatch_size is None:
        return int(m)
    return max((hi - lo for lo, hi in minibatch_ranges(int(m), int(minibatch_size), drop_last)), default=0)


def fits_fused(m: int, minibatch_size: Optional[int] = None, drop_last: bool = False) -> bool:
    """Whether every step of such an update is at most one row tile
    (``FUSED_MAX_ROWS`` rows), which is what ``fused=True`` needs."""
    return 1 <= fused_rows(m, minibatch_size, drop_last) <= FUSED_MAX_ROWS


class _Plan(NamedTuple):
    """One :func:`ppo_update` call, normalised by :func:`_plan`.  The full
    batch looped keeps ``five`` as given and has None for the next three."""
    five: tuple
    m: Optional[int]
    size: Optional[int]
    ranges: Optional[list]
    num_epochs: int
    drop_last: bool
    coefficients: tuple           # clip_epsilon, entropy_coef, value_coef
    max_norm: Optional[float]


def _plan(actor, critic, five, *, fused, num_epochs, minibatch_size, drop_last, clip_epsilon, entropy_coef,
          value_coef, max_grad_norm) -> _Plan:
    """What an update accepts, stated once for ``fused=True`` and the loop, in
    the order each has always reported faults in.  ``five`` is ``(batch,)`` or
    the five tensors.  The loop's first step checks the networks, the
    coefficients and ``max_grad_norm`` in :func:`ppo_losses` and
    :meth:`MlpNet.backward`, after the shuffle has checked the columns (the
    full batch is checked there alone); ``fused=True`` calls neither, so the
    same ``_args`` checks are made here and the scalars come back as floats."""
    num_epochs = int(num_epochs)
    if num_epochs < 1:
        raise ValueError(f"num_epochs must be at least 1, got {num_epochs}")
    size = None if minibatch_size is None else int(minibatch_size)
    if size is not None and size < 1:
        raise ValueError(f"minibatch_size must be at least 1, got {minibatch_size!r}")
    coefficients, max_norm, drop_last = (clip_epsilon, entropy_coef, value_coef), max_grad_norm, bool(drop_last)
    if size is None and not fused:
        return _Plan(five, None, None, None, num_epochs, drop_last, coefficients, max_norm)
    if len(five) == 1:  # a batch: its five tensors
        five = _args.batch_five(five[0])
        if five is None:
            raise ValueError("batch must be a PpoBatch, a PpoEpisodesBatch or the five tensors")
    if len(five) != 5 or not all(isinstance(t, torch.Tensor) for t in five):
        raise ValueError(f"{'fused=True needs' if fused else 'minibatches need'} all five tensors "
                         "(states, actions, old_log_probs, advantages, returns)")
    m = int(five[0].shape[0])
    ranges = [(0, m)] if size is None else minibatch_ranges(m, size, drop_last)
    if not ranges:
        raise ValueError(f"no minibatch to step on: {m} rows, minibatch_size {size}, drop_last={drop_last}")
    if fused:
        _args.some_rows(m, "ppo_losses")
        _args.check_actor_critic(actor, critic)
        coefficients = _args.ppo_coefficients(*coefficients)
        max_norm = _args.clip_norm(max_norm)
    return _Plan(five, m, size, ranges, num_epochs, drop_last, coefficients, max_norm)


def _fused_net(net: MlpNet, opt: "AdamW") -> abi.DDPpoFusedNet:
    return abi.DDPpoFusedNet(opt.params.data_ptr(), opt.grad_buffer().data_ptr(), opt.exp_avg.data_ptr(),
                             opt.exp_avg_sq.data_ptr(), opt._state.data_ptr(), net.packed.data_ptr(), opt._hyper(),
                             net.ln_eps, 0)


def _fused_columns(actor, critic, plan: _Plan) -> list:
    """What a fused update (``dd_ppo_update_fused``, ``dd_ppo_update_population``)
    asks beyond :func:`_plan`: its own two limits, then the batch's five
    columns as the kernels read them."""
    for name, net in (("actor", actor), ("critic", critic)):
        if net.compute != "f32":
            raise ValueError(f"fused=True runs compute='f32' networks only, the {name} is compute={net.compute!r}; "
                             "use fused=False")
    rows = max(hi - lo for lo, hi in plan.ranges)
    if rows > FUSED_MAX_ROWS:
        raise ValueError(f"fused=True takes minibatches of at most {FUSED_MAX_ROWS} rows (one row tile of the "
                         f"backward), this update has one of {rows}; pass minibatch_size <= {FUSED_MAX_ROWS} or "
                         "fused=False")
    five = plan.five
    if five[0].dim() != 2 or five[0].shape[1] != abi.DD_OBS_DIM:
        raise ValueError(f"states must be [M, {abi.DD_OBS_DIM}]")
    return [_args.column(name, t, plan.m, actor.device) for name, t in zip(ShuffledBatch._fields[:5], five)]


def _ppo_update_fused(actor, critic, plan: _Plan, actor_opt, critic_opt, shuffle_seed, shuffle_epoch) -> torch.Tensor:
    """The steps of ``plan`` as ``dd_ppo_update_fused``: the ``[11, num_epochs,
    steps]`` log tensor.  Its own two limits, then the columns, stacked per
    epoch where they are shuffled, and the launch."""
    cols = _fused_columns(actor, critic, plan)
    m, size, num_epochs = plan.m, plan.size, plan.num_epochs
    dev = actor.device
    stride = 0
    if size is not None:  # the epochs' shuffled batches, one after the other: num_epochs launches, whatever M / B is
        stacked = [torch.empty((num_epochs * m,) + tuple(c.shape[1:]), dtype=c.dtype, device=dev) for c in cols]
        indices = torch.empty(m, dtype=torch.int32, device=dev)
        for epoch in range(num_epochs):
            out = ShuffledBatch(*(t[epoch * m:(epoch + 1) * m] for t in stacked), indices)
            shuffle_batch(cols, seed=shuffle_seed, epoch=int(shuffle_epoch) + epoch, out=out)
        cols, stride = stacked, m
    lib = actor._lib
    if actor_opt._fused_ws is None:
        actor_opt._fused_ws = torch.empty(int(lib.dd_ppo_update_fused_workspace()) // 8, dtype=torch.int64, device=dev)
    logs = torch.empty(abi.DD_PPO_FUSED_LOGS, num_epochs, len(plan.ranges), dtype=torch.float64, device=dev)
    io = abi.DDPpoFusedIO(_fused_net(actor, actor_opt), _fused_net(critic, critic_opt), cols[0].data_ptr(),
                          cols[1].data_ptr(), cols[2].data_ptr(), cols[3].data_ptr(), cols[4].data_ptr(),
                          _args.action_format(cols[1]), 1 if plan.drop_last else 0, m, stride, num_epochs,
                          min(size, m) if size is not None else m, *plan.coefficients, plan.max_norm,
                          logs.data_ptr())
    abi.check(lib.dd_ppo_update_fused(ctypes.byref(io), actor_opt._fused_ws.data_ptr(), actor._stream()),
              "dd_ppo_update_fused")
    return logs


def _ppo_step(actor, critic, five, actor_opt, critic_opt, plan: _Plan) -> torch.Tensor:
    """One optimizer step of each network on the rows of ``five`` (a batch or
    five tensors); its log entries."""
    rows = five[0] if isinstance(five[0], torch.Tensor) else five[0].states
    clip_epsilon, entropy_coef, value_coef = plan.coefficients
    losses = ppo_losses(actor, critic, *five, clip_epsilon=clip_epsilon, entropy_coef=entropy_coef,
                        value_coef=value_coef, grads=True)
    g_actor, g_critic = actor_opt.grad_buffer(), critic_opt.grad_buffer()
    _, n_actor = actor.backward(rows, losses.grad_logits, max_norm=plan.max_norm, out=g_actor)
    _, n_critic = critic.backward(rows, losses.grad_values, max_norm=plan.max_norm, out=g_critic)
    actor_opt.step(g_actor)
    critic_opt.step(g_critic)
    s = losses.ratio_stats
    return torch.stack([losses.total_loss, losses.policy_loss, losses.value_loss, losses.entropy,
                        s["mean"], s["min"], s["max"], s["std"], s["clipped_frac"], n_actor, n_critic])


def ppo_update(actor: MlpNet, critic: MlpNet, batch, actor_opt: AdamW, critic_opt: AdamW, *, num_epochs: int = 4,
               clip_epsilon: float = 0.2, entropy_coef: float = 0.01, value_coef: float = 0.5,
               max_grad_norm: float = 0.5, minibatch_size: Optional[int] = None, shuffle_seed: int = 0,
               shuffle_epoch: int = 0, drop_last: bool = False, fused: bool = False) -> PpoUpdate:
    """PHASE 3 of the notebook's training cell: ``num_epochs`` times
    ``compute_ppo_losses``, ``total_loss.backward()``, the two
    ``clip_grad_norm_`` and the two optimizer steps, on the full batch (a
    :class:`PpoBatch`, a :class:`PpoEpisodesBatch`, or the five tensors
    ``(states, actions, old_log_probs, advantages, returns)``).  Epoch ``e``
    is exactly ``ppo_grads(...)`` followed by ``actor_opt.step`` and
    ``critic_opt.step``; one flat gradient buffer per network is reused.

    ``minibatch_size=B`` (default ``None``: the full batch, as above) runs the
    notebook's "shuffle collected data into minibatches / for each minibatch":
    at epoch ``e`` the batch is shuffled on device with the key
    ``(shuffle_seed, shuffle_epoch + e)`` (:func:`shuffle_batch`, into buffers
    allocated once per call), and each row range ``[i B, min((i + 1) B, M))``
    of the shuffled batch is one minibatch: ``ppo_grads`` on that range, then
    the two optimizer steps.  The tail shorter than ``B`` is a minibatch of its
    own unless ``drop_last``.  Advantages stay as the batch has them
    (normalised over the whole batch by the batch builders), not re-normalised
    per minibatch.  ``logs[k]`` is then ``[num_epochs, n_minibatches]``.
    ``shuffle_epoch`` is a host integer: pass a different one on every call
    (for instance ``update * num_epochs``) or every call repeats the same
    permutations, and a captured graph replays the permutations it was
    captured with.

    ``fused=True`` runs the same steps as one persistent launch
    (``dd_ppo_update_fused``, ``csrc/ppo_fused.hip``: one workgroup per network
    walks the epochs' minibatches in order) instead of about twenty launches
    per step: the same logs, parameters, moments, state blocks and packed
    images, bit for bit.  It needs ``compute="f32"`` networks and steps of at
    most ``FUSED_MAX_ROWS`` = 128 rows (:func:`fits_fused`:
    ``minibatch_size <= 128``, or a full batch of at most 128 rows) and raises
    ``ValueError`` otherwise; the epochs' shuffled batches are laid out first,
    one ``shuffle_batch`` launch per epoch.

    ``summary``: the steps' mean of every log under its own name (the cell's
    ``avg_*``: ``total_loss``, ..., ``ratio_mean``, ``ratio_std``,
    ``clipped_frac``, the two norms), and ``ratio_min`` = min over all steps,
    ``ratio_max`` = max over all steps.  Runs on the current stream and reads
    nothing back for either ``compute``; a refused ``f16x3`` step shows in
    ``actor_opt.status()`` / ``critic_opt.status()``."""
    if actor_opt.net is not actor or critic_opt.net is not critic:
        raise ValueError("actor_opt must optimize actor and critic_opt critic")
    five = tuple(batch) if isinstance(batch, (tuple, list)) and not hasattr(batch, "_fields") else (batch,)
    plan = _plan(actor, critic, five, fused=fused, num_epochs=num_epochs, minibatch_size=minibatch_size,
                 drop_last=drop_last, clip_epsilon=clip_epsilon, entropy_coef=entropy_coef, value_coef=value_coef,
                 max_grad_norm=max_grad_norm)
    num_epochs, dev = plan.num_epochs, actor.device
    if fused:
        logs = _ppo_update_fused(actor, critic, plan, actor_opt, critic_opt, shuffle_seed, shuffle_epoch)
        if plan.size is None:
            logs = logs.view(len(LOG_KEYS), num_epochs)
    elif plan.size is None:
        logs = torch.empty(len(LOG_KEYS), num_epochs, dtype=torch.float64, device=dev)
        for epoch in range(num_epochs):
            logs[:, epoch] = _ppo_step(actor, critic, plan.five, actor_opt, critic_opt, plan)
    else:
        logs = torch.empty(len(LOG_KEYS), num_epochs, len(plan.ranges), dtype=torch.float64, device=dev)
        shuffled = None
        for epoch in range(num_epochs):
            shuffled = shuffle_batch(plan.five, seed=shuffle_seed, epoch=int(shuffle_epoch) + epoch, out=shuffled)
            for i, (lo, hi) in enumerate(plan.ranges):
                logs[:, epoch, i] = _ppo_step(actor, critic, tuple(t[lo:hi] for t in shuffled[:5]), actor_opt,
                                              critic_opt, plan)
    return _update_of(logs)


def _update_of(logs: torch.Tensor) -> PpoUpdate:
    """The ``[11, ...]`` log tensor of an update as its :class:`PpoUpdate`."""
    by_key = {k: logs[i] for i, k in enumerate(LOG_KEYS)}
    summary = {k: v.mean() for k, v in by_key.items()}
    summary["ratio_min"] = by_key["ratio_min"].min()
    summary["ratio_max"] = by_key["ratio_max"].max()
    return PpoUpdate(by_key, summary)
