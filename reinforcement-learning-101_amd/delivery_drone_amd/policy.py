"""The notebooks' policy and value networks on the GPU (``dd_mlp_forward``).

``DroneGamerBoi`` (actor) and ``DroneTeacherBoi`` (critic) of
Actor_Critic_PPO.ipynb:376-424 share one body,

    Linear(15,128) LayerNorm ReLU  Linear(128,128) LayerNorm ReLU
    Linear(128,64) LayerNorm ReLU  Linear(64,K)

with K = 3 + Sigmoid for the actor and K = 1 for the critic.  A
:class:`MlpNet` takes that state_dict (the notebooks' ``.pth`` files load with
``torch.load(path, weights_only=True)``), packs it once into the kernel's
MFMA operand order, and evaluates N observation rows per call in float32
(``compute="f32"``, the default) or with the hidden GEMMs on the f16 MFMA as
split hi/lo operand pairs (``compute="f16x3"``: about 2x faster — 65,536 rows
35.8 -> 15-18 us on MI355X — about the same end-to-end error;
include/dronestep.h ``DD_MLP_F16X3``).
The actor also does the collection loop's ``Bernoulli(probs).sample()`` and
``.log_prob(actions).sum(dim=1)`` (:857-859) in the same launch, returning the
actions as the ``dd_step`` bitmask, so a policy-driven rollout never leaves
the device.  :meth:`MlpNet.backward` is the training side: the parameter
gradients from the gradient at the network's output (``dd_mlp_backward``,
float32 MFMA with the forward recomputed tile by tile) and the notebook's
``clip_grad_norm_``.
"""
from __future__ import annotations

import ctypes
import math
from collections.abc import Sequence
from typing import Dict, Mapping, Optional, Tuple

import torch

from . import _args, abi

__all__ = ["MlpNet", "STATE_DICT_KEYS", "ActorPopulation", "population_summary"]

#: state_dict keys of the notebooks' nn.Sequential (``network.<i>.<param>``)
STATE_DICT_KEYS = ("0.weight", "0.bias", "1.weight", "1.bias", "3.weight", "3.bias", "4.weight", "4.bias",
                   "6.weight", "6.bias", "7.weight", "7.bias", "9.weight", "9.bias")
_SHAPES = {"0.weight": (128, 15), "0.bias": (128,), "1.weight": (128,), "1.bias": (128,),
           "3.weight": (128, 128), "3.bias": (128,), "4.weight": (128,), "4.bias": (128,),
           "6.weight": (64, 128), "6.bias": (64,), "7.weight": (64,), "7.bias": (64,)}
_COMPUTE = {"f32": abi.DD_MLP_F32, "f16x3": abi.DD_MLP_F16X3}


class MlpNet:
    """Actor (``out_dim == 3``) or critic (``out_dim == 1``) on one GPU.

    ``state_dict`` keys may carry the notebooks' ``network.`` prefix or not.
    ``ln_eps`` is nn.LayerNorm's default.  ``compute`` is ``"f32"`` or
    ``"f16x3"`` (see the module docstring).  The packed parameters stay on
    ``device``; ``library`` selects a build of libdronestep.so (tests, A/B).
    """

    def __init__(self, state_dict: Mapping[str, torch.Tensor], *, device="cuda", ln_eps: float = 1e-5,
                 compute: str = "f32", library=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("MlpNet runs on the GPU (HIP); there is no CPU path")
        if self.device.index is None:  # "cuda" -> the current device, as VecDroneEnv does
            self.device = torch.device("cuda", torch.cuda.current_device())
        if compute not in _COMPUTE:
            raise ValueError(f"compute must be one of {sorted(_COMPUTE)}, got {compute!r}")
        self.compute = compute
        self._mode = _COMPUTE[compute]
        self._lib = library if library is not None else abi.lib()
        self.ln_eps = float(ln_eps)
        self._src, self.out_dim = self._validated(state_dict)
        self.packed = torch.empty(int(self._lib.dd_mlp_packed_floats()), dtype=torch.float32, device=self.device)
        self._flat = None         # flat_parameters(), once handed out
        self._backward_ws = None  # backward()'s packed weight images and block sums: a fixed size, kept
        self._pack()

    def _validated(self, state_dict: Mapping[str, torch.Tensor]):
        """The constructor's checks of a state_dict (keys, shapes, the f16x3
        operand ranges): its float32 device tensors and K, or an exception."""
        compute = self.compute
        sd = {k[len("network."):] if k.startswith("network.") else k: v for k, v in state_dict.items()}
        missing = [k for k in STATE_DICT_KEYS if k not in sd]
        if missing:
            raise KeyError(f"state_dict lacks {missing}")
        for k, shape in _SHAPES.items():
            if tuple(sd[k].shape) != shape:
                raise ValueError(f"{k}: expected shape {shape}, got {tuple(sd[k].shape)}")
        k_out = sd["9.weight"].shape[0]
        if k_out not in (1, 3) or tuple(sd["9.weight"].shape) != (k_out, 64) or tuple(sd["9.bias"].shape) != (k_out,):
            raise ValueError("last layer must be Linear(64, 3) (actor) or Linear(64, 1) (critic)")
        src = {k: torch.as_tensor(sd[k]).detach().to(device=self.device, dtype=torch.float32).contiguous()
               for k in STATE_DICT_KEYS}
        if compute == "f16x3":
            # the hidden Linears' weights go into f16 halves x16 (kWScale) after
            # centring over their outputs (|w - mean| <= 2 max|w|): beyond the f16
            # range the hi half is inf and every probability NaN, so refuse such
            # weights here (observations must stay below 1023 as well)
            for k in ("0.weight", "3.weight", "6.weight"):
                w = src[k]
                if not bool(torch.isfinite(w).all()) or float(w.abs().max()) >= 65504.0 / 32:
                    raise ValueError(f"{k}: compute='f16x3' needs finite weights below 2047 in magnitude "
                                     "(the f16 range after centring and x16); use compute='f32'")
            # each LayerNorm's output x16 is split with its ReLU (mlp_core.h
            # split_pair_relu), which needs it below 2048: |gamma| sqrt(rows) +
            # |beta| bounds a LayerNorm's output
            for g, b, rows in (("1.weight", "1.bias", 128), ("4.weight", "4.bias", 128), ("7.weight", "7.bias", 64)):
                bound = float(src[g].abs().max()) * rows ** 0.5 * (1 + 2 ** -8) + float(src[b].abs().max())
                if not bound < 128.0:
                    raise ValueError(f"{g}/{b}: compute='f16x3' needs LayerNorm outputs below 128 "
                                     f"(max|weight| sqrt({rows}) + max|bias| = {bound:.4g}); use compute='f32'")
        return src, int(k_out)

    def _pack(self):
        """dd_mlp_pack of ``_src`` into ``packed`` on the current stream."""
        p = abi.DDMlpParams(*[self._src[k].data_ptr() for k in STATE_DICT_KEYS], self.out_dim, self.ln_eps)
        abi.check(self._lib.dd_mlp_pack(ctypes.byref(p), self._mode, self.packed.data_ptr(), self._stream()),
                  "dd_mlp_pack")

    def load_state_dict(self, state_dict: Mapping[str, torch.Tensor]) -> "MlpNet":
        """New weights into the same ``packed`` buffer, on the current stream.

        The state_dict is checked exactly as the constructor checks one (keys,
        shapes, the ``f16x3`` operand ranges); a refused one raises and leaves
        the old parameters in place.  ``packed`` keeps its address, so a
        captured graph or a ``policy_rollout`` that holds the pointer sees the
        new weights at its next launch after this one on the stream.  The last
        layer may change between ``Linear(64, 3)`` and ``Linear(64, 1)`` (the
        buffer's size is the same); ``out_dim`` follows, and a launch that
        still asks for the other K gets NaN by the layout tag."""
        src, out_dim = self._validated(state_dict)
        if self._flat is not None:
            # flat_parameters() was handed out: the values go into that buffer, which keeps its address
            if out_dim != self.out_dim:
                raise ValueError(f"flat_parameters() fixed the last layer at Linear(64, {self.out_dim}); "
                                 f"the state_dict has Linear(64, {out_dim})")
            for k in STATE_DICT_KEYS:
                self._src[k].copy_(src[k])
        else:
            self._src, self.out_dim = src, out_dim  # kept alive until the pack kernel has read them
        self._pack()
        return self

    def flat_parameters(self) -> torch.Tensor:
        """The fourteen parameter tensors as one flat float32 device buffer in
        ``STATE_DICT_KEYS`` order (:meth:`grad_numel` elements, the layout of
        :meth:`backward`'s flat gradient), which an optimizer updates in place
        (:class:`AdamW`).  The first call copies the parameters into it and
        re-points the network at views of it, so :meth:`backward` and the next
        pack read what was written there with no copy; from then on
        :meth:`load_state_dict` copies into the buffer, so its address stays
        fixed, and the last layer's width is fixed with it.  After writing the
        buffer directly, the forward sees the new values once ``packed`` is
        rebuilt (:class:`AdamW` does that in its step)."""
        if self._flat is None:
            flat = torch.empty(self.grad_numel(), dtype=torch.float32, device=self.device)
            views = self._views(flat)
            for k in STATE_DICT_KEYS:
                views[k].copy_(self._src[k])
            self._src, self._flat = views, flat
        return self._flat

    def _views(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        """``STATE_DICT_KEYS`` -> the parameters' shapes as views into ``flat``
        (:meth:`grad_numel` elements), one after the other."""
        views, first = {}, 0
        for k in STATE_DICT_KEYS:
            shape = self._src[k].shape
            views[k] = flat[first:first + shape.numel()].view(shape)
            first += shape.numel()
        return views

    def state_dict(self, prefix: str = "network.") -> Dict[str, torch.Tensor]:
        """Clones of the current float32 parameters under the notebooks' keys
        (``network.0.weight`` ...), for the training cell's
        ``torch.save(policy.state_dict(), path)``; :class:`MlpNet`,
        :meth:`load_state_dict` and the notebooks' ``nn.Module`` load it."""
        return {prefix + k: self._src[k].clone() for k in STATE_DICT_KEYS}

    @classmethod
    def from_file(cls, path: str, **kw) -> "MlpNet":
        """Load a notebook checkpoint (a state_dict) without unpickling code."""
        return cls(torch.load(path, map_location="cpu", weights_only=True), **kw)

    def _stream(self):
        return _args.stream_ptr(self.device)

    def _obs(self, obs: torch.Tensor) -> torch.Tensor:
        if obs.dim() != 2 or obs.shape[1] != abi.DD_OBS_DIM:
            raise ValueError(f"obs must be [N, {abi.DD_OBS_DIM}], got {tuple(obs.shape)}")
        if obs.device != self.device:
            raise ValueError(f"obs is on {obs.device}, the network on {self.device}")
        return obs.to(torch.float32).contiguous()

    def _run(self, obs, out=None, actions=None, log_prob=None, seed=0, step=0, env_id_base=0, sampling=None):
        io = abi.DDMlpIO(obs.data_ptr(), out.data_ptr() if out is not None else None,
                         actions.data_ptr() if actions is not None else None,
                         log_prob.data_ptr() if log_prob is not None else None,
                         int(seed) & (2 ** 64 - 1), int(step), int(env_id_base))
        if sampling is not None:
            abi.check(self._lib.dd_mlp_forward_sampled(self.packed.data_ptr(), self._mode, self.out_dim,
                                                       ctypes.byref(io), ctypes.byref(sampling), obs.shape[0],
                                                       self._stream()), "dd_mlp_forward_sampled")
            return
        abi.check(self._lib.dd_mlp_forward(self.packed.data_ptr(), self._mode, self.out_dim, ctypes.byref(io),
                                           obs.shape[0], self._stream()), "dd_mlp_forward")

    def __call__(self, obs: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``network(obs)``: probabilities ``[N, 3]`` (actor) or values ``[N]`` (critic)."""
        obs = self._obs(obs)
        n = obs.shape[0]
        if out is None:
            out = torch.empty((n, 3) if self.out_dim == 3 else (n,), dtype=torch.float32, device=self.device)
        self._run(obs, out=out)
        return out

    def act(self, obs: torch.Tensor, *, seed: int = 0, step: int = 0, env_id_base: int = 0,
            probs: bool = False, actions_out: Optional[torch.Tensor] = None,
            log_prob_out: Optional[torch.Tensor] = None, temperature: float = 1.0,
            probs_used_out: Optional[torch.Tensor] = None):
        """Sample actions as the collection loop does (actor only).

        Returns ``(actions, log_prob)`` or ``(actions, log_prob, probs)``:
        actions is the uint8 ``[N]`` bitmask ``dd_step`` consumes (bit 0 main,
        1 left, 2 right), log_prob the float32 ``[N]`` sum over the three
        Bernoulli factors.  Draws are Philox4x32-10 keyed by (seed; env id,
        step), so a lane's sample does not depend on sharding.

        ``temperature`` is the notebooks' ``evaluate_policy`` argument
        (``dd_mlp_forward_sampled``): 1 (default) the plain
        ``Bernoulli(probs).sample()``; 0 greedy, ``probs > 0.5``, with no
        draw; any other positive finite value draws from ``q = p**(1/T) /
        (p**(1/T) + (1-p)**(1/T))``, evaluated as ``sigmoid(z / T)`` on the
        network's pre-Sigmoid outputs, and ``log_prob`` is then that of
        ``Bernoulli(q)``.  ``probs_used_out`` (float32 ``[N, 3]``) receives the
        probabilities the draw was compared with (``p``, ``q``, or ``p`` when
        greedy); ``probs=True`` returns the network's own ``p`` in every mode.
        """
        if self.out_dim != 3:
            raise ValueError("act() needs the actor (out_dim 3)")
        mode = abi.sampling_mode(temperature)
        obs = self._obs(obs)
        n = obs.shape[0]
        sampling = None
        if mode != abi.DD_SAMPLE_BERNOULLI or probs_used_out is not None:
            if probs_used_out is not None:
                _args.check_out(probs_used_out, (n, 3), torch.float32, self.device,
                                "probs_used_out must be a contiguous float32 tensor")
            sampling = abi.DDSampling(mode, float(temperature),
                                      probs_used_out.data_ptr() if probs_used_out is not None else None)
        actions = actions_out if actions_out is not None else torch.empty(n, dtype=torch.uint8, device=self.device)
        log_prob = log_prob_out if log_prob_out is not None else torch.empty(n, dtype=torch.float32,
                                                                             device=self.device)
        p = torch.empty(n, 3, dtype=torch.float32, device=self.device) if probs else None
        self._run(obs, out=p, actions=actions, log_prob=log_prob, seed=seed, step=step, env_id_base=env_id_base,
                  sampling=sampling)
        return (actions, log_prob, p) if probs else (actions, log_prob)

    def evaluate_actions(self, obs: torch.Tensor, actions: torch.Tensor, *, probs: bool = False,
                         log_prob_out: Optional[torch.Tensor] = None, entropy_out: Optional[torch.Tensor] = None):
        """Score given actions as ``compute_ppo_losses`` does (actor only):
        ``dist = Bernoulli(probs=policy(obs))``, ``dist.log_prob(actions).sum(1)``
        and ``dist.entropy().sum(1)`` (``dd_mlp_evaluate_actions``).

        ``actions`` is the uint8 ``[N]`` bitmask :meth:`act` returns, or the
        float32 ``[N, 3]`` tensor of a training batch (nonzero = on).  Returns
        ``(log_prob, entropy)`` or ``(log_prob, entropy, probs)``, float32
        ``[N]`` and ``[N, 3]``.  For the actions :meth:`act` drew on the same
        rows, ``log_prob`` has the bits of :meth:`act`'s own."""
        if self.out_dim != 3:
            raise ValueError("evaluate_actions() needs the actor (out_dim 3)")
        obs = self._obs(obs)
        n = obs.shape[0]
        if not isinstance(actions, torch.Tensor) or actions.device != self.device:
            raise ValueError(f"actions must be a tensor on {self.device}")
        if actions.dtype == torch.uint8 and tuple(actions.shape) == (n,):
            fmt = abi.DD_ACT_BITMASK
        elif actions.dtype == torch.float32 and tuple(actions.shape) == (n, 3):
            fmt = abi.DD_ACT_F32X3
        else:
            raise ValueError(f"actions must be uint8 ({n},) bitmasks or float32 ({n}, 3), got {actions.dtype} "
                             f"{tuple(actions.shape)}")
        actions = actions.contiguous()
        for name, t in (("log_prob_out", log_prob_out), ("entropy_out", entropy_out)):
            if t is not None:
                _args.check_out(t, (n,), torch.float32, self.device, f"{name} must be a contiguous float32 tensor")
        lp = log_prob_out if log_prob_out is not None else torch.empty(n, dtype=torch.float32, device=self.device)
        ent = entropy_out if entropy_out is not None else torch.empty(n, dtype=torch.float32, device=self.device)
        p = torch.empty(n, 3, dtype=torch.float32, device=self.device) if probs else None
        io = abi.DDMlpEvalIO(obs.data_ptr(), actions.data_ptr(), fmt, 0, p.data_ptr() if probs else None,
                             lp.data_ptr(), ent.data_ptr(), n)
        abi.check(self._lib.dd_mlp_evaluate_actions(self.packed.data_ptr(), self._mode, ctypes.byref(io),
                                                    self._stream()), "dd_mlp_evaluate_actions")
        return (lp, ent, p) if probs else (lp, ent)

    def grad_numel(self) -> int:
        """Elements of the flat gradient vector :meth:`backward` fills (the
        fourteen tensors of ``STATE_DICT_KEYS``, concatenated)."""
        return sum(math.prod(_SHAPES[k]) for k in _SHAPES) + 65 * self.out_dim

    def backward(self, states: torch.Tensor, grad_out: torch.Tensor, *, max_norm: Optional[float] = None,
                 out: Optional[torch.Tensor] = None) -> Tuple[Dict[str, torch.Tensor], torch.Tensor]:
        """The parameter gradients autograd leaves when it starts from
        ``grad_out`` at the last Linear's output on ``states``
        (``dd_mlp_backward``): for the actor ``grad_out [M, 3]`` is the
        gradient at the pre-Sigmoid logits, for the critic ``[M]`` (or ``[M,
        1]``) the gradient at the value, i.e. ``ppo_losses(...,
        grads=True)``'s ``grad_logits`` / ``grad_values``.

        Returns ``(grads, grad_norm)``.  ``grads`` maps ``STATE_DICT_KEYS`` to
        float32 tensors in ``nn.Linear`` / ``nn.LayerNorm`` shapes, views into
        one flat buffer in that order (``out``, a contiguous float32 tensor of
        :meth:`grad_numel` elements, or a new one), so ``grads["0.weight"]``'s
        storage is also the flat gradient vector.  ``grad_norm`` is the L2
        norm over all fourteen before clipping, a 0-d float64 device tensor.
        ``max_norm`` (finite, positive) applies the notebook's
        ``clip_grad_norm_(parameters, max_norm)``: every gradient times
        ``min(1, max_norm / (norm + 1e-6))``.  Float32 arithmetic from the
        float32 parameters whatever ``compute`` is; the same bits on every run
        and every device.  ``M == 0`` gives zeros.  Runs on the current stream
        and reads nothing back."""
        states = self._obs(states)
        m = states.shape[0]
        want = (m, 3) if self.out_dim == 3 else (m,)
        if not isinstance(grad_out, torch.Tensor) or grad_out.device != self.device:
            raise ValueError(f"grad_out must be a tensor on {self.device}")
        if self.out_dim == 1 and tuple(grad_out.shape) == (m, 1):
            grad_out = grad_out.reshape(m)
        if tuple(grad_out.shape) != want:
            raise ValueError(f"grad_out must be {want} for out_dim {self.out_dim}, got {tuple(grad_out.shape)}")
        grad_out = grad_out.detach().to(torch.float32).contiguous()
        max_norm = _args.clip_norm(max_norm)
        total = self.grad_numel()
        if out is None:
            out = torch.empty(total, dtype=torch.float32, device=self.device)
        else:
            _args.check_out(out, (total,), torch.float32, self.device, "out must be a contiguous float32 tensor")
        grads = self._views(out)
        norm = torch.empty((), dtype=torch.float64, device=self.device)
        if self._backward_ws is None:
            self._backward_ws = torch.empty(int(self._lib.dd_mlp_backward_workspace()) // 8, dtype=torch.int64,
                                            device=self.device)
        p = abi.DDMlpParams(*[self._src[k].data_ptr() for k in STATE_DICT_KEYS], self.out_dim, self.ln_eps)
        io = abi.DDMlpBackwardIO(states.data_ptr(), grad_out.data_ptr(),
                                 abi.DDMlpGrads(*[grads[k].data_ptr() for k in STATE_DICT_KEYS]), norm.data_ptr(),
                                 max_norm)
        abi.check(self._lib.dd_mlp_backward(ctypes.byref(p), ctypes.byref(io), m, self._backward_ws.data_ptr(),
                                            self._stream()), "dd_mlp_backward")
        return grads, norm


class ActorPopulation(Sequence):
    """Several actors that share one fused rollout launch
    (``dd_policy_rollout_population``): a checkpoint tournament, the snapshots
    of a training run, the learners of a hyper-parameter sweep.

    ``actors`` is a non-empty sequence of :class:`MlpNet` with ``out_dim ==
    3``, all on one device, of one ``compute`` and one library; anything else
    raises ``ValueError``.  Passed to :meth:`VecDroneEnv.policy_rollout` or
    :meth:`VecDroneEnv.evaluate_policy` in an actor's place, member ``g``
    drives the env's lanes ``lanes(env, g)``, the ``g``-th of ``len(self)``
    equal contiguous groups, exactly as it would drive an env of those lanes
    alone (same ``env_id_base + start``): Philox is keyed by env id, so the
    results are the single-actor ones bit for bit.

    The constructor builds the device table of the members'
    ``packed.data_ptr()`` once and keeps the members alive.  A launch reads
    the table and the images on the device and copies neither, and
    ``MlpNet.packed`` keeps its address through :meth:`MlpNet.load_state_dict`
    and :meth:`AdamW.step`: a member's new weights are seen by the next
    population launch on the stream with nothing rebuilt.
    """

    def __init__(self, actors):
        members = tuple(actors)
        if not members:
            raise ValueError("ActorPopulation needs at least one actor")
        for a in members:
            if not isinstance(a, MlpNet) or a.out_dim != 3:
                raise ValueError("every member must be an actor: an MlpNet with out_dim 3")
        first = members[0]
        for a in members[1:]:
            if a.device != first.device:
                raise ValueError(f"the members are on different devices ({first.device}, {a.device})")
            if a.compute != first.compute:
                raise ValueError(f"the members differ in compute ({first.compute!r}, {a.compute!r}): "
                                 "one launch runs one kernel")
            if a._lib is not first._lib:
                raise ValueError("the members use different builds of the library")
        self._members = members
        self.device, self.compute, self.out_dim = first.device, first.compute, 3
        self._lib = first._lib
        self.table = torch.tensor([a.packed.data_ptr() for a in members], dtype=torch.int64, device=self.device)

    def __len__(self) -> int:
        return len(self._members)

    def __getitem__(self, g):
        return self._members[g]

    def lanes(self, env, g: int) -> slice:
        """The lanes of ``env`` that member ``g`` drives."""
        n, p = len(env), len(self._members)
        if n % p != 0:
            raise ValueError(f"{n} lanes do not split into {p} equal groups")
        g = range(p)[g]
        return slice(g * (n // p), (g + 1) * (n // p))


def population_summary(result: Mapping[str, torch.Tensor], members: int) -> Dict[str, torch.Tensor]:
    """``run_inference_loop``'s table (Actor_Critic_inference.ipynb:229-295)
    for every member of a population: from the dict
    :meth:`VecDroneEnv.evaluate_policy` returned for an
    :class:`ActorPopulation` of ``members`` actors, the ``[members]`` float64
    device tensors ``success_rate`` (the fraction of the member's lanes that
    landed), ``mean_reward``, ``mean_steps`` and ``mean_final_fuel``.  Torch
    reductions over the ``[members, L]`` views; nothing is read back.  Each
    is the float64 sum over the member's lanes divided by ``L`` (a true
    division, so the two integer columns, whose sums are exact, give the
    correctly rounded mean)."""
    members = int(members)
    n = result["steps"].shape[0]
    if members < 1 or n % members != 0:
        raise ValueError(f"{n} lanes do not split into {members} equal groups")
    # a tensor divisor: dividing by a Python number multiplies by its rounded reciprocal
    lanes = torch.full((), n // members, dtype=torch.float64, device=result["steps"].device)

    def mean(t):
        return t.view(members, n // members).to(torch.float64).sum(dim=1) / lanes

    return {"success_rate": mean(result["landed"]), "mean_reward": mean(result["total_reward"]),
            "mean_steps": mean(result["steps"]), "mean_final_fuel": mean(result["final_fuel"])}
