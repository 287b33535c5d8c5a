"""No GPU: the C surface of dd_ppo_train (csrc/ppo_train_fused.hip): the header's
declarations and abi.py's binding of them, the struct layouts against the C
compiler, the workspace size formula, and every argument error, each returned
before any HIP call (fake pointers throughout, no device present)."""
import ctypes
import os
import re
import subprocess

from delivery_drone_amd import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(REPO, "include")
EINVAL = 1  # hipErrorInvalidValue
NEW = ("dd_ppo_train_workspace", "dd_ppo_train")
STRIDE = 1 << 25  # between two members' fake buffers: more than both networks' bytes
BUFFERS = ("params", "grads", "exp_avg", "exp_avg_sq", "state", "packed")


def test_header_declares_and_abi_binds_the_calls():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(HEADER_DIR, "dronestep.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", abi.library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (dd_[a-z0-9_]+)$", out, flags=re.M))
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header) and name in abi.EXPORTS and name in exported, name
    for name in ("DDPpoTrainMember", "DDPpoTrainIO"):
        assert name in header and name in abi.__all__, name
    assert re.search(r"#define DD_ABI_VERSION 13\b", header)
    assert abi.DD_ABI_VERSION == 13 and abi.lib().dd_abi_version() == 13  # additions only
    rows = re.search(r"enum \{ (DD_PT_ROWS.*?) \};", header, flags=re.S).group(1)
    values = dict((k.strip(), int(v)) for k, v in (item.split("=") for item in rows.split(",")))
    assert values.pop("DD_PT_BATCH_LOGS") == abi.DD_PT_BATCH_LOGS == len(abi.PT_BATCH_LOG_NAMES) == 3
    assert [k for k, _ in sorted(values.items(), key=lambda kv: kv[1])] == \
        ["DD_PT_" + name.upper() for name in abi.PT_BATCH_LOG_NAMES]
    assert int(re.search(r"#define DD_PPO_TRAIN_CELL_BYTES (\d+)", header).group(1)) == abi.DD_PPO_TRAIN_CELL_BYTES


def test_struct_layouts_match_the_header(tmp_path):
    structs = (abi.DDPpoTrainMember, abi.DDPpoTrainIO)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dronestep.h"', 'int main(void) {']
    for cls in structs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cls.__name__, cls.__name__))
        for name, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cls.__name__, name, cls.__name__,
                                                                        name.rstrip("_")))
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


def test_workspace_size_formula():
    """members x (a fixed part + DD_PPO_TRAIN_CELL_BYTES per cell, the cells rounded up to a multiple of 4)."""
    ws = abi.lib().dd_ppo_train_workspace
    cell = abi.DD_PPO_TRAIN_CELL_BYTES
    fixed = ws(1, 1, 4) - 4 * cell
    # both networks' backward images and head gradients, one partial gradient set, the accumulators, a stage
    assert fixed > abi.lib().dd_ppo_update_fused_workspace() and fixed % 16 == 0
    for members in (1, 2, 3, 16, 128, 260):
        for lanes, frames in ((1, 1), (1, 2), (1, 4), (3, 5), (6, 300), (33, 7), (64, 300), (128, 257), (128, 300)):
            cells = (lanes * frames + 3) // 4 * 4
            assert ws(members, lanes, frames) == members * (fixed + cells * cell), (members, lanes, frames)
            assert ws(members, lanes, frames) % 16 == 0
    assert ws(1, 128, abi.DD_REINFORCE_MAX_CELLS // 128) > 0
    for bad in ((0, 6, 300), (-1, 6, 300), (1, 0, 300), (1, 129, 300), (1, 6, 0), (1, 6, -3),
                (1, 128, abi.DD_REINFORCE_MAX_CELLS // 128 + 1)):
        assert ws(*bad) == 0, bad


def _net(base, **kw):
    f = dict(params=base, grads=base + (1 << 18), exp_avg=base + (2 << 18), exp_avg_sq=base + (3 << 18),
             state=base + (4 << 18), packed=base + (5 << 18), lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
             weight_decay=0.01, ln_eps=1e-5)
    f.update(kw)
    return abi.DDPpoFusedNet(f["params"], f["grads"], f["exp_avg"], f["exp_avg_sq"], f["state"], f["packed"],
                             abi.DDAdamWHyper(f["lr"], f["beta1"], f["beta2"], f["eps"], f["weight_decay"]),
                             f["ln_eps"], 0)


def _member(p, actor=None, critic=None, **kw):
    f = dict(gamma=0.99, lambda_=0.95, clip_epsilon=0.2, entropy_coef=0.01, value_coef=0.5, max_grad_norm=0.5,
             shuffle_seed=3)
    f.update(kw)
    base = (p + 1) * STRIDE
    return abi.DDPpoTrainMember(_net(base, **(actor or {})), _net(base + STRIDE // 2, **(critic or {})), f["gamma"],
                                f["lambda_"], f["clip_epsilon"], f["entropy_coef"], f["value_coef"],
                                f["max_grad_norm"], f["shuffle_seed"])


def _state(**kw):
    f = dict(precision=abi.DD_F32)
    f.update(kw)
    st = abi.DDState()
    for name, _ in abi.DDState._fields_:
        if name not in ("env_id_base", "precision") and not name.startswith("_"):
            setattr(st, name, f.get(name, 16))
    st.env_id_base, st.precision = 0, f["precision"]
    return st


def run(bad=None, *, members=3, at=1, lanes=64, n=None, cfg_none=False, st_none=False, io_none=False,
        table_none=False, workspace=16, state=None, count=None, auto_reset=0, **io_kw):
    """The call on `members` good members, member `at` replaced by one built with `bad`."""
    table = (abi.DDPpoTrainMember * max(members, 1))()
    for p in range(members):
        table[p] = _member(p, **(bad if bad is not None and p == at else {}))
    f = dict(max_steps=5, obs=16, shaped_hist=None, shaped_mode=abi.DD_SHAPED_REINFORCE, env_max_steps=300,
             normalize=1, num_epochs=4, minibatch_size=0, drop_last=0, shuffle_epoch=0, seed=1, step=0, lengths=16,
             ended=16, episode_return=16, landed=16, record_reward=None, record_done=None, record_values=None,
             record_returns=None, record_advantages=None, logs=16, batch_logs=16)
    f.update(io_kw)
    io = abi.DDPpoTrainIO(None if table_none else table, members if count is None else count, f["max_steps"], lanes,
                          f["obs"], f["shaped_hist"], f["shaped_mode"], f["env_max_steps"], f["normalize"],
                          f["num_epochs"], f["minibatch_size"], f["drop_last"], f["shuffle_epoch"], f["seed"],
                          f["step"], f["lengths"], f["ended"], f["episode_return"], f["landed"], f["record_reward"],
                          f["record_done"], f["record_values"], f["record_returns"], f["record_advantages"],
                          f["logs"], f["batch_logs"])
    cfg, st = abi.DDConfig(), state if state is not None else _state()
    cfg.auto_reset = auto_reset
    return abi.lib().dd_ppo_train(None if cfg_none else ctypes.byref(cfg), None if st_none else ctypes.byref(st),
                                  None if io_none else ctypes.byref(io), members * lanes if n is None else n,
                                  workspace, None)


def test_launch_wide_argument_errors_without_gpu():
    """Everything dd_reinforce_train refuses of the launch, and the update's own three."""
    assert run(cfg_none=True) == EINVAL and run(st_none=True) == EINVAL and run(io_none=True) == EINVAL
    assert run(table_none=True) == EINVAL
    assert run(workspace=None) == EINVAL and run(workspace=8) == EINVAL
    for count in (0, -1):
        assert run(count=count) == EINVAL, count
    for max_steps in (0, -1):
        assert run(max_steps=max_steps) == EINVAL, max_steps
    assert run(lanes=128, max_steps=abi.DD_REINFORCE_MAX_CELLS // 128 + 1) == EINVAL
    for lanes in (0, -1, 129, 256):
        assert run(lanes=lanes) == EINVAL, lanes
    for n in (0, 191, 193, 64):  # members * lanes_per_member is 192
        assert run(n=n) == EINVAL, n
    for name in ("obs", "lengths", "ended", "episode_return", "landed", "logs", "batch_logs"):
        assert run(**{name: None}) == EINVAL, name
    assert run(auto_reset=1) == EINVAL  # one episode per lane
    assert run(state=_state(precision=abi.DD_F64)) == EINVAL and run(state=_state(precision=7)) == EINVAL
    for name in ("x", "fuel", "total_reward", "status", "steps", "episode"):
        assert run(state=_state(**{name: None})) == EINVAL, name
    assert run(shaped_mode=9) == EINVAL
    for name in ("record_reward", "record_done", "record_values", "record_returns", "record_advantages"):
        assert run(**{name: 16}) == EINVAL, name  # one buffer of a group without the others
    assert run(record_values=16, record_returns=16) == EINVAL
    for num_epochs in (0, -1):
        assert run(num_epochs=num_epochs) == EINVAL, num_epochs
    for size in (-1, 129, 1 << 20):
        assert run(minibatch_size=size) == EINVAL, size


def test_every_member_is_checked():
    for at in (0, 1, 2):  # the first, a middle and the last member
        for net in ("actor", "critic"):
            for name in BUFFERS:
                assert run({net: {name: None}}, at=at) == EINVAL, (at, net, name)
            own = (at + 1) * STRIDE + (STRIDE // 2 if net == "critic" else 0)
            assert run({net: dict(state=own + (4 << 18) + 12)}, at=at) == EINVAL
            assert run({net: dict(packed=own + (5 << 18) + 8)}, at=at) == EINVAL
            assert run({net: dict(ln_eps=0.0)}, at=at) == EINVAL
            for name in ("lr", "beta1", "beta2", "eps", "weight_decay"):
                for bad in (-1e-3, float("nan"), float("inf")):
                    assert run({net: {name: bad}}, at=at) == EINVAL, (at, net, name, bad)
        for name in ("gamma", "lambda_", "clip_epsilon", "entropy_coef", "value_coef"):
            for bad in (float("nan"), float("inf"), -float("inf")):
                assert run({name: bad}, at=at) == EINVAL, (at, name, bad)
        assert run(dict(clip_epsilon=-0.1), at=at) == EINVAL
        assert run(dict(max_grad_norm=float("nan")), at=at) == EINVAL


def test_network_buffers_may_not_overlap():
    other = 1 * STRIDE  # member 0's actor starts here, its critic half a stride on
    for name in BUFFERS:
        mine = other + BUFFERS.index(name) * (1 << 18)
        assert run({"actor": {name: mine}}, at=2) == EINVAL, name                     # another member's buffer
        assert run({"critic": {name: mine + 16}}, at=2) == EINVAL, name                # inside it
        assert run({"actor": {name: mine + STRIDE // 2}}, at=0) == EINVAL, name        # the member's own critic's
    assert run({"actor": dict(grads=other - 64)}, at=1) == EINVAL  # a flat buffer that ends inside another member's
