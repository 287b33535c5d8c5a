"""No GPU: the C surface of dd_ppo_update_population
(csrc/ppo_fused_population.hip): the header's declarations and abi.py's
binding of them, the struct layouts against the C compiler, the workspace
size, and every argument error, each returned before any HIP call (fake
pointers throughout, no device present).  One case, the last, passes every
check and ends at the upload for lack of a device; it is not run where there
is one."""
import ctypes
import os
import re
import subprocess

import pytest

from delivery_drone_amd import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(REPO, "include")
EINVAL = 1  # hipErrorInvalidValue
NEW = ("dd_ppo_update_population_workspace", "dd_ppo_update_population")
STRIDE = 1 << 24  # between two members' fake buffers: more than any buffer's bytes


def test_header_declares_and_abi_binds_the_calls():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(HEADER_DIR, "dronestep.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", abi.library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (dd_[a-z0-9_]+)$", out, flags=re.M))
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header) and name in abi.EXPORTS and name in exported, name
    for name in ("DDPpoPopulationMember", "DDPpoPopulationIO"):
        assert name in header and name in abi.__all__, name
    assert abi.DD_ABI_VERSION == 13 and abi.lib().dd_abi_version() == 13  # additions only


def test_struct_layouts_match_the_header(tmp_path):
    structs = (abi.DDPpoPopulationMember, abi.DDPpoPopulationIO)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dronestep.h"', 'int main(void) {']
    for cls in structs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cls.__name__, cls.__name__))
        for name, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cls.__name__, name, cls.__name__, name))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", HEADER_DIR, "-o", str(exe), str(src)], check=True, capture_output=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    for cls in structs:
        assert int(got[cls.__name__]) == ctypes.sizeof(cls), cls.__name__
        for name, _ in cls._fields_:
            assert int(got[f"{cls.__name__}.{name}"]) == getattr(cls, name).offset, (cls.__name__, name)


def test_workspace_grows_linearly_in_members():
    ws = abi.lib().dd_ppo_update_population_workspace
    one = ws(1)
    per_member = ws(2) - one
    # two workgroups' weight images, head gradients and stages, and a descriptor: more than the single call's
    assert per_member > abi.lib().dd_ppo_update_fused_workspace() and one == per_member
    for members in (1, 2, 3, 16, 128, 130, 1000):
        assert ws(members) == members * per_member and ws(members) % 16 == 0, members
    assert ws(0) == 0 and ws(-1) == 0


def _net(base, **kw):
    f = dict(params=base, grads=base + (1 << 18), exp_avg=base + (2 << 18), exp_avg_sq=base + (3 << 18),
             state=base + (4 << 18), packed=base + (5 << 18), lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
             weight_decay=0.01, ln_eps=1e-5)
    f.update(kw)
    return abi.DDPpoFusedNet(f["params"], f["grads"], f["exp_avg"], f["exp_avg_sq"], f["state"], f["packed"],
                             abi.DDAdamWHyper(f["lr"], f["beta1"], f["beta2"], f["eps"], f["weight_decay"]),
                             f["ln_eps"], 0)


def _member(p, actor=None, critic=None, **kw):
    base = (p + 1) * STRIDE
    f = dict(states=16, actions=16, old_log_probs=16, advantages=16, returns=16, action_format=abi.DD_ACT_F32X3,
             shuffle=1, m=200, clip_epsilon=0.2, entropy_coef=0.01, value_coef=0.5, max_grad_norm=0.5,
             shuffle_seed=3, shuffle_epoch=5, logs=16)
    f.update(kw)
    return abi.DDPpoPopulationMember(_net(base, **(actor or {})), _net(base + STRIDE // 2, **(critic or {})),
                                     f["states"], f["actions"], f["old_log_probs"], f["advantages"], f["returns"],
                                     f["action_format"], f["shuffle"], f["m"], f["clip_epsilon"], f["entropy_coef"],
                                     f["value_coef"], f["max_grad_norm"], f["shuffle_seed"], f["shuffle_epoch"],
                                     f["logs"])


def run(bad=None, *, members=3, at=1, io_none=False, table_none=False, workspace=16, num_epochs=2, minibatch_size=64,
        drop_last=0, count=None):
    """The call on `members` good members, member `at` replaced by one built with `bad`."""
    table = (abi.DDPpoPopulationMember * max(members, 1))()
    for p in range(members):
        table[p] = _member(p, **(bad if bad is not None and p == at else {}))
    io = abi.DDPpoPopulationIO(None if table_none else table, members if count is None else count, num_epochs,
                               minibatch_size, drop_last)
    return abi.lib().dd_ppo_update_population(None if io_none else ctypes.byref(io), workspace, None)


def test_launch_wide_argument_errors_without_gpu():
    assert run(io_none=True) == EINVAL and run(table_none=True) == EINVAL
    assert run(workspace=None) == EINVAL and run(workspace=8) == EINVAL
    for count in (0, -1):
        assert run(count=count) == EINVAL, count
    assert run(num_epochs=0) == EINVAL
    for size in (0, -1, 129, 256):
        assert run(minibatch_size=size) == EINVAL, size


def test_every_member_is_checked_as_the_single_call_checks_it():
    for at in (0, 1, 2):  # the first, a middle and the last member
        for name in ("states", "actions", "old_log_probs", "advantages", "returns", "logs"):
            assert run({name: None}, at=at) == EINVAL, (at, name)
        for which in ("actor", "critic"):
            for name in ("params", "grads", "exp_avg", "exp_avg_sq", "state", "packed"):
                assert run({which: {name: None}}, at=at) == EINVAL, (at, which, name)
            assert run({which: dict(state=STRIDE + 12)}, at=at) == EINVAL
            assert run({which: dict(packed=STRIDE + 8)}, at=at) == EINVAL
            assert run({which: dict(ln_eps=0.0)}, at=at) == EINVAL
            for name in ("lr", "beta1", "beta2", "eps", "weight_decay"):
                for bad in (-1e-3, float("nan"), float("inf")):
                    assert run({which: {name: bad}}, at=at) == EINVAL, (at, which, name, bad)
            assert run({which: dict(beta1=1.0)}, at=at) == EINVAL
        for m in (0, -1, 2**31):
            assert run(dict(m=m), at=at) == EINVAL, (at, m)
        assert run(dict(action_format=abi.DD_ACT_U8X3), at=at) == EINVAL
        for bad in (-0.1, float("nan"), float("inf")):
            assert run(dict(clip_epsilon=bad), at=at) == EINVAL, (at, bad)
        for name in ("entropy_coef", "value_coef"):
            for bad in (float("nan"), float("inf")):
                assert run({name: bad}, at=at) == EINVAL, (at, name, bad)
        assert run(dict(max_grad_norm=float("nan")), at=at) == EINVAL
        # drop_last leaves this member no minibatch (the others have three)
        assert run(dict(m=50), at=at, drop_last=1) == EINVAL


def test_members_may_not_share_a_network_buffer():
    other = 1 * STRIDE  # member 0's actor buffers start here
    for which in ("actor", "critic"):
        for name in ("params", "grads", "exp_avg", "exp_avg_sq", "state", "packed"):
            mine = other + ("params", "grads", "exp_avg", "exp_avg_sq", "state", "packed").index(name) * (1 << 18)
            assert run({which: {name: mine}}, at=2) == EINVAL, (which, name)          # the same buffer
            assert run({which: {name: mine + 16}}, at=2) == EINVAL, (which, name)     # inside it
    # a flat buffer that ends inside another member's
    assert run({"actor": dict(grads=other - 64)}, at=1) == EINVAL


def test_a_members_own_networks_may_share_a_buffer():
    """The owner rule from the other side: buffers of one member that overlap pass the check between members (the
    call then fails like a good one, at the upload: no device here), while dd_actor_critic_train and
    dd_reinforce_train refuse any overlap (their own files).  With a device the accepted calls would upload to the
    fake workspace and launch, so the case runs only where there is none."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present: an accepted call would launch on fake pointers")
    good = run()
    assert good != EINVAL  # every check passed; the runtime's error for the missing device
    mine = 2 * STRIDE  # member 1's actor buffers start here
    assert run({"critic": dict(grads=mine + (1 << 18))}, at=1) == good       # its actor's gradient buffer
    assert run({"critic": dict(exp_avg=mine + (1 << 18) + 16)}, at=1) == good  # inside it
    assert run({"critic": dict(grads=mine + (1 << 18))}, at=2) == EINVAL     # another member's: refused
