"""No GPU: the surface of ppo_update(fused=True) and dd_ppo_update_fused
(csrc/ppo_fused.hip): the header's declaration and abi.py's binding of it, the
struct layouts against the C compiler, the argument errors the library
returns before any launch, ppo_update's new keyword, and the helper that
decides whether an update fits the fused path.
"""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

import delivery_drone_amd
from delivery_drone_amd import abi, adamw

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(REPO, "include")
EINVAL = 1  # hipErrorInvalidValue
NEW = ("dd_ppo_update_fused_workspace", "dd_ppo_update_fused")


def test_header_declares_and_abi_binds_the_call():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(HEADER_DIR, "dronestep.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", abi.library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (dd_[a-z0-9_]+)$", out, flags=re.M))
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header) and name in abi.EXPORTS and name in exported, name
    assert abi.DD_ABI_VERSION == 13 and abi.lib().dd_abi_version() == 13  # additions only
    assert abi.lib().dd_ppo_update_fused_workspace() > 0 and abi.lib().dd_ppo_update_fused_workspace() % 16 == 0


def test_struct_layouts_match_the_header(tmp_path):
    structs = (abi.DDPpoFusedNet, abi.DDPpoFusedIO)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dronestep.h"', 'int main(void) {']
    for cls in structs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cls.__name__, cls.__name__))
        for name, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cls.__name__, name, cls.__name__, name))
    lines.append('printf("rows %d\\n", DD_PPO_FUSED_ROWS);')
    lines.append('printf("logs %d %d %d\\n", DD_PPO_POLICY_GRAD_NORM, DD_PPO_CRITIC_GRAD_NORM, DD_PPO_FUSED_LOGS);')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", HEADER_DIR, "-o", str(exe), str(src)], check=True, capture_output=True)
    got = [line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                   text=True).stdout.splitlines()]
    sizes = {g[0]: g[1:] for g in got}
    for cls in structs:
        assert int(sizes[cls.__name__][0]) == ctypes.sizeof(cls), cls.__name__
        for name, _ in cls._fields_:
            assert int(sizes[f"{cls.__name__}.{name}"][0]) == getattr(cls, name).offset, (cls.__name__, name)
    assert ctypes.sizeof(abi.DDPpoFusedNet) == 6 * 8 + 40 + 8
    assert int(sizes["rows"][0]) == abi.DD_PPO_FUSED_ROWS == adamw.FUSED_MAX_ROWS == 128
    assert [int(x) for x in sizes["logs"]] == [abi.DD_PPO_POLICY_GRAD_NORM, abi.DD_PPO_CRITIC_GRAD_NORM,
                                               abi.DD_PPO_FUSED_LOGS] == [9, 10, 11]
    # the log rows are LOG_KEYS' order
    assert len(adamw.LOG_KEYS) == abi.DD_PPO_FUSED_LOGS
    assert adamw.LOG_KEYS.index("policy_grad_norm") == abi.DD_PPO_POLICY_GRAD_NORM
    assert adamw.LOG_KEYS.index("critic_grad_norm") == abi.DD_PPO_CRITIC_GRAD_NORM
    assert adamw.LOG_KEYS.index("clipped_frac") == abi.DD_PPO_CLIPPED_FRAC


def test_argument_errors_without_gpu():
    lib = abi.lib()

    def net(**kw):
        f = dict(params=16, grads=16, exp_avg=16, exp_avg_sq=16, state=16, packed=16, lr=1e-3, beta1=0.9, beta2=0.999,
                 eps=1e-8, weight_decay=0.01, ln_eps=1e-5)
        f.update(kw)
        return abi.DDPpoFusedNet(f["params"], f["grads"], f["exp_avg"], f["exp_avg_sq"], f["state"], f["packed"],
                                 abi.DDAdamWHyper(f["lr"], f["beta1"], f["beta2"], f["eps"], f["weight_decay"]),
                                 f["ln_eps"], 0)

    def run(io_none=False, workspace=16, actor=None, critic=None, **kw):
        f = dict(states=16, actions=16, old_log_probs=16, advantages=16, returns=16, action_format=abi.DD_ACT_F32X3,
                 drop_last=0, m=200, epoch_stride=200, num_epochs=2, minibatch_size=64, clip_epsilon=0.2,
                 entropy_coef=0.01, value_coef=0.5, max_grad_norm=0.5, logs=16)
        f.update(kw)
        io = abi.DDPpoFusedIO(net(**(actor or {})), net(**(critic or {})), f["states"], f["actions"],
                              f["old_log_probs"], f["advantages"], f["returns"], f["action_format"], f["drop_last"],
                              f["m"], f["epoch_stride"], f["num_epochs"], f["minibatch_size"], f["clip_epsilon"],
                              f["entropy_coef"], f["value_coef"], f["max_grad_norm"], f["logs"])
        return lib.dd_ppo_update_fused(None if io_none else ctypes.byref(io), workspace, None)

    assert run(io_none=True) == EINVAL and run(workspace=None) == EINVAL and run(workspace=8) == EINVAL
    for name in ("states", "actions", "old_log_probs", "advantages", "returns", "logs"):
        assert run(**{name: None}) == EINVAL, name
    for which in ("actor", "critic"):
        for name in ("params", "grads", "exp_avg", "exp_avg_sq", "state", "packed"):
            assert run(**{which: {name: None}}) == EINVAL, (which, name)
        assert run(**{which: dict(state=12)}) == EINVAL and run(**{which: dict(packed=8)}) == EINVAL
        assert run(**{which: dict(ln_eps=0.0)}) == EINVAL
        for name in ("lr", "beta1", "beta2", "eps", "weight_decay"):
            for bad in (-1e-3, float("nan"), float("inf")):
                assert run(**{which: {name: bad}}) == EINVAL, (which, name, bad)
        assert run(**{which: dict(beta1=1.0)}) == EINVAL
    for m in (0, -1, 2**31):
        assert run(m=m, epoch_stride=0) == EINVAL, m
    for size in (0, -1, 129, 256):
        assert run(minibatch_size=size) == EINVAL, size
    assert run(num_epochs=0) == EINVAL
    assert run(epoch_stride=-1) == EINVAL and run(epoch_stride=199) == EINVAL
    assert run(m=50, epoch_stride=50, minibatch_size=64, drop_last=1) == EINVAL  # no minibatch
    assert run(action_format=abi.DD_ACT_U8X3) == EINVAL
    for bad in (-0.1, float("nan"), float("inf")):
        assert run(clip_epsilon=bad) == EINVAL, bad
    for name in ("entropy_coef", "value_coef"):
        for bad in (float("nan"), float("inf")):
            assert run(**{name: bad}) == EINVAL, (name, bad)
    assert run(max_grad_norm=float("nan")) == EINVAL


def test_ppo_update_has_the_keyword():
    sig = inspect.signature(delivery_drone_amd.ppo_update)
    fused = sig.parameters["fused"]
    assert fused.default is False and fused.kind is inspect.Parameter.KEYWORD_ONLY
    assert list(sig.parameters)[-1] == "fused"  # after everything that was there


@pytest.mark.parametrize("m,size,drop_last,want", [
    (200, 64, False, [(0, 64), (64, 128), (128, 192), (192, 200)]),
    (200, 64, True, [(0, 64), (64, 128), (128, 192)]),
    (130, 128, False, [(0, 128), (128, 130)]),
    (37, 1, False, [(i, i + 1) for i in range(37)]),
    (100, 200, False, [(0, 100)]),
    (100, 200, True, []),
])
def test_minibatch_ranges_are_unchanged(m, size, drop_last, want):
    assert adamw.minibatch_ranges(m, size, drop_last) == want


def test_which_updates_fit_the_fused_path():
    for size in (1, 64, 128):
        for m in (1, 37, 128, 129, 200, 2048):
            for drop_last in (False, True):
                ranges = adamw.minibatch_ranges(m, size, drop_last)
                assert adamw.fits_fused(m, size, drop_last) == bool(ranges), (m, size, drop_last)
                # a tail larger than one tile cannot occur when the minibatch is at most one tile
                assert all(0 < hi - lo <= size <= 128 for lo, hi in ranges)
                assert adamw.fused_rows(m, size, drop_last) == max((hi - lo for lo, hi in ranges), default=0)
    assert not adamw.fits_fused(200, 129) and not adamw.fits_fused(129, 129)
    assert adamw.fits_fused(100, 129) and adamw.fused_rows(100, 129) == 100  # one step of all 100 rows
    assert not adamw.fits_fused(130, 200) and adamw.fused_rows(130, 200) == 130  # a tail forced above one tile
    for m in (1, 96, 128):
        assert adamw.fits_fused(m) and adamw.fused_rows(m) == m  # the full batch
    assert not adamw.fits_fused(129) and not adamw.fits_fused(2048) and not adamw.fits_fused(0)
