"""A population of PPO learners trained in one fused launch.

:class:`~delivery_drone_amd.ActorPopulation` collects for the learners of a
hyper-parameter sweep in one launch; this module updates them in one.
:func:`ppo_update_population` is ``ppo_update(..., fused=True)`` for every
member of a :class:`LearnerPopulation` at once (``dd_ppo_update_population``,
``csrc/ppo_fused_population.hip``): a grid of two workgroups per member, none
of which waits on another, each reading its member's batch in place through
the keyed permutation, so no shuffled copy of any batch is laid out.  Every
member is left bit for bit as its own fused call would leave it.
:func:`collect_ppo_population` is the collection that goes in front: one
population rollout, then each member's batch from its own lanes.  The loop:
``batches = collect_ppo_population(env, pop); ppo_update_population(pop,
batches, ...)``; the next rollout of ``pop.actors`` sees the new weights with
nothing rebuilt.
"""
from __future__ import annotations

import ctypes
from collections.abc import Sequence
from typing import List, Optional

import torch

from . import _args, abi, adamw
from .adamw import AdamW, FUSED_MAX_ROWS, PpoUpdate
from .policy import ActorPopulation, MlpNet
from .train_batch import PpoBatch, ppo_batch

__all__ = ["LearnerPopulation", "ReinforcePopulation", "ppo_update_population", "collect_ppo_population"]


class _Population(Sequence):
    """What the populations share: ``members`` as a tuple of tuples, none
    empty; every network of a member (``_member_nets``, the subclass's check of
    the member's shape) ``compute="f32"`` and in the population once; one
    device and one library; ``actors``, the members' first networks."""

    def __init__(self, members):
        members = tuple(tuple(m) if isinstance(m, (tuple, list)) else m for m in members)
        if not members:
            raise ValueError(f"{type(self).__name__} needs at least one member")
        seen, nets_of_members = set(), []
        for p, member in enumerate(members):
            nets = self._member_nets(p, member)
            for name, net in nets:
                if net.compute != "f32":
                    raise ValueError(f"member {p}: a population update runs compute='f32' networks only, the {name} "
                                     f"is compute={net.compute!r}")
                if id(net) in seen:
                    raise ValueError(f"member {p}: its {name} is in the population already")
                seen.add(id(net))
            nets_of_members.append([net for _, net in nets])
        self._members = members
        self.device, self._lib = _one_device_and_library(nets_of_members)
        self.actors = ActorPopulation([m[0] for m in members])

    def __len__(self) -> int:
        return len(self._members)

    def __getitem__(self, p):
        return self._members[p]

    @classmethod
    def _of_one(cls, opt, attr: str, member: tuple):
        """The population of the one learner ``member``, built on the first
        call and kept on its optimizer ``opt`` as ``attr``; a refusal speaks
        of the learner, not of "member 0"."""
        pop = getattr(opt, attr, None) if isinstance(opt, AdamW) else None
        if pop is None or tuple(pop[0]) != member:
            try:
                pop = cls([member])
            except ValueError as exc:
                raise ValueError(str(exc).replace("member 0: ", "", 1)) from None
            setattr(opt, attr, pop)
        return pop


def _one_device_and_library(nets_of_members):
    """The device and the library all the members' networks share, or a
    ``ValueError`` naming the first member that differs from member 0."""
    first = nets_of_members[0][0]
    for p, nets in enumerate(nets_of_members):
        for net in nets:
            if net.device != first.device:
                raise ValueError(f"member {p}: on {net.device}, member 0 on {first.device}")
            if net._lib is not first._lib:
                raise ValueError(f"member {p}: uses another build of the library than member 0")
    return first.device, first._lib


class LearnerPopulation(_Population):
    """The learners of a sweep: ``members`` is a non-empty sequence of
    ``(actor, critic, actor_opt, critic_opt)``, each what :func:`ppo_update`
    takes (``actor_opt`` optimizes ``actor``, ``critic_opt`` ``critic``), all
    ``compute="f32"``, on one device and of one library; no network may appear
    twice.  Anything else raises ``ValueError`` naming the member.

    ``actors`` is the :class:`ActorPopulation` of the members' actors, built
    once: an update rewrites each packed image in place, so the next
    ``env.policy_rollout(pop.actors, ...)`` runs the new weights.  The
    population owns the update's workspace (the descriptor table, and per
    workgroup the backward's weight images, the head gradient and the row
    stage), allocated here once and sized for
    :func:`actor_critic_train_population`'s launch as well.
    :func:`ppo_train_population`'s workspace depends on the lanes per member
    and the frames of a call: it is allocated at the first such call and grown
    when a later one needs more."""

    def __init__(self, members):
        super().__init__(members)
        # one workspace for either launch over the members: the PPO update's, or the actor-critic loop's
        size = max(int(self._lib.dd_ppo_update_population_workspace(len(self))),
                   int(self._lib.dd_actor_critic_train_workspace(len(self))))
        self._workspace = torch.empty(size // 8, dtype=torch.int64, device=self.device)
        self._train_workspace = None  # ppo_train_population's: allocated at the first call, grown on demand

    def _train_workspace_for(self, lanes: int, max_steps: int) -> torch.Tensor:
        size = int(self._lib.dd_ppo_train_workspace(len(self), lanes, max_steps))
        if self._train_workspace is None or self._train_workspace.numel() * 8 < size:
            self._train_workspace = torch.empty((size + 7) // 8, dtype=torch.int64, device=self.device)
        return self._train_workspace

    @staticmethod
    def _member_nets(p, member):
        if not isinstance(member, tuple) or len(member) != 4:
            raise ValueError(f"member {p}: expected (actor, critic, actor_opt, critic_opt)")
        actor, critic, actor_opt, critic_opt = member
        if not isinstance(actor, MlpNet) or not isinstance(critic, MlpNet):
            raise ValueError(f"member {p}: the actor and the critic must be MlpNets")
        if not isinstance(actor_opt, AdamW) or not isinstance(critic_opt, AdamW):
            raise ValueError(f"member {p}: actor_opt and critic_opt must be AdamW optimizers")
        if actor_opt.net is not actor or critic_opt.net is not critic:
            raise ValueError(f"member {p}: actor_opt must optimize actor and critic_opt critic")
        try:
            _args.check_actor_critic(actor, critic)
        except ValueError as exc:
            raise ValueError(f"member {p}: {exc}") from None
        return (("actor", actor), ("critic", critic))


class ReinforcePopulation(_Population):
    """The learners of a REINFORCE sweep, which have no critic: ``members`` is
    a non-empty sequence of ``(actor, opt)``, each what
    :func:`reinforce_update` takes (``opt`` optimizes ``actor``), all
    ``compute="f32"``, on one device and of one library; no actor may appear
    twice.  Anything else raises ``ValueError`` naming the member.  The
    critic-less twin of :class:`LearnerPopulation`.

    ``actors`` is the :class:`ActorPopulation` of the members' actors, built
    once: an update rewrites each packed image in place, so the next
    ``env.policy_rollout(pop.actors, ...)`` runs the new weights.  The
    population owns :func:`reinforce_train_population`'s workspace, which
    depends on the lanes per member and the frames of a call: it is allocated
    at the first call and grown when a later call needs more."""

    def __init__(self, members):
        super().__init__(members)
        self._workspace = None

    @staticmethod
    def _member_nets(p, member):
        if not isinstance(member, tuple) or len(member) != 2:
            raise ValueError(f"member {p}: expected (actor, opt)")
        actor, opt = member
        if not isinstance(actor, MlpNet) or actor.out_dim != 3:
            raise ValueError(f"member {p}: the actor must be an MlpNet with out_dim 3")
        if not isinstance(opt, AdamW):
            raise ValueError(f"member {p}: opt must be an AdamW optimizer")
        if opt.net is not actor:
            raise ValueError(f"member {p}: opt must be the AdamW that optimizes actor")
        return (("actor", actor),)

    def _workspace_for(self, lanes: int, max_steps: int) -> torch.Tensor:
        size = int(self._lib.dd_reinforce_train_workspace(len(self), lanes, max_steps))
        if self._workspace is None or self._workspace.numel() * 8 < size:
            self._workspace = torch.empty((size + 7) // 8, dtype=torch.int64, device=self.device)
        return self._workspace


def ppo_update_population(pop: LearnerPopulation, batches, *, num_epochs: int = 4,
                          minibatch_size: Optional[int] = None, drop_last: bool = False, clip_epsilon=0.2,
                          entropy_coef=0.01, value_coef=0.5, max_grad_norm=0.5, shuffle_seed=0,
                          shuffle_epoch: int = 0) -> List[PpoUpdate]:
    """``ppo_update(actor_p, critic_p, batches[p], actor_opt_p, critic_opt_p,
    ..., fused=True)`` for every member ``p`` of ``pop``, in one launch.

    ``batches`` holds one batch per member (a :class:`PpoBatch`, a
    :class:`PpoEpisodesBatch` or the five tensors), of any sizes.
    ``num_epochs``, ``minibatch_size``, ``drop_last`` and ``shuffle_epoch``
    hold for all members; ``clip_epsilon``, ``entropy_coef``, ``value_coef``,
    ``max_grad_norm`` and ``shuffle_seed`` are a scalar or a list with one
    value per member (the sweep).  Each member is checked as
    ``ppo_update(fused=True)`` checks it; a ``ValueError`` names the member.

    Member ``p``'s parameters, moments, optimizer state blocks, packed images,
    gradient buffers and logs end up bit for bit as that single call leaves
    them, and ``result[p]`` is its :class:`PpoUpdate`.  The batches are read in
    place (no shuffled copies).  Runs on the current stream and reads nothing
    back; it cannot be captured into a graph (the members' table is uploaded
    from host memory at every call)."""
    if not isinstance(pop, LearnerPopulation):
        raise ValueError("pop must be a LearnerPopulation")
    members = len(pop)
    batches = list(batches)
    if len(batches) != members:
        raise ValueError(f"batches: {len(batches)} batches for {members} members")
    per = {name: _args.per_member(name, value, members)
           for name, value in (("clip_epsilon", clip_epsilon), ("entropy_coef", entropy_coef),
                               ("value_coef", value_coef), ("max_grad_norm", max_grad_norm),
                               ("shuffle_seed", shuffle_seed))}
    plans, columns = [], []
    for p, ((actor, critic, _, _), batch) in enumerate(zip(pop, batches)):  # every check, before anything is allocated
        five = tuple(batch) if isinstance(batch, (tuple, list)) and not hasattr(batch, "_fields") else (batch,)
        try:
            plan = adamw._plan(actor, critic, five, fused=True, num_epochs=num_epochs, minibatch_size=minibatch_size,
                               drop_last=drop_last, clip_epsilon=per["clip_epsilon"][p],
                               entropy_coef=per["entropy_coef"][p], value_coef=per["value_coef"][p],
                               max_grad_norm=per["max_grad_norm"][p])
            columns.append(adamw._fused_columns(actor, critic, plan))
        except ValueError as exc:
            raise ValueError(f"member {p}: {exc}") from None
        plans.append(plan)
    table = (abi.DDPpoPopulationMember * members)()
    logs = []
    for p, ((actor, critic, actor_opt, critic_opt), plan, cols) in enumerate(zip(pop, plans, columns)):
        log = torch.empty(abi.DD_PPO_FUSED_LOGS, plan.num_epochs, len(plan.ranges), dtype=torch.float64,
                          device=pop.device)
        table[p] = abi.DDPpoPopulationMember(
            adamw._fused_net(actor, actor_opt), adamw._fused_net(critic, critic_opt), *(c.data_ptr() for c in cols),
            _args.action_format(cols[1]), 0 if plan.size is None else 1, plan.m, *plan.coefficients, plan.max_norm,
            int(per["shuffle_seed"][p]) & (2 ** 64 - 1), int(shuffle_epoch) & (2 ** 64 - 1), log.data_ptr())
        logs.append(log)
    size = FUSED_MAX_ROWS if plans[0].size is None else min(plans[0].size, FUSED_MAX_ROWS)
    io = abi.DDPpoPopulationIO(table, members, plans[0].num_epochs, size, 1 if plans[0].drop_last else 0)
    abi.check(pop._lib.dd_ppo_update_population(ctypes.byref(io), pop._workspace.data_ptr(),
                                                _args.stream_ptr(pop.device)), "dd_ppo_update_population")
    return [adamw._update_of(log.view(log.shape[0], log.shape[1]) if plan.size is None else log)
            for log, plan in zip(logs, plans)]


def collect_ppo_population(env, pop: LearnerPopulation, max_steps: int = 300, seed: int = 0, step: int = 0,
                           gamma: float = 0.99, lambda_: float = 0.95, normalize: bool = True) -> List[PpoBatch]:
    """One PPO iteration's data for every member: ``env.reset()``, one
    ``env.policy_rollout(pop.actors, max_steps, seed=seed, step=step)``, then
    :func:`ppo_batch` per member on its lanes ``pop.actors.lanes(env, p)``
    with that member's critic and ``env.obs`` there as the bootstrap state.
    Member ``p``'s batch is what :func:`collect_ppo` gives on an env of those
    lanes alone (``env_id_base`` at the group's start)."""
    if not isinstance(pop, LearnerPopulation):
        raise ValueError("pop must be a LearnerPopulation")
    env.reset()
    obs, acts, lp, reward, done = env.policy_rollout(pop.actors, int(max_steps), seed=seed, step=step)
    final = env.obs
    batches = []
    for p, (_, critic, _, _) in enumerate(pop):
        lanes = pop.actors.lanes(env, p)
        batches.append(ppo_batch(*(t[:, lanes].contiguous() for t in (obs, acts, lp, reward, done)), critic,
                                 bootstrap_obs=final[lanes].contiguous(), gamma=gamma, lambda_=lambda_,
                                 normalize=normalize))
    return batches
