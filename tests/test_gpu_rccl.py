"""GPU: RCCL (torch.distributed's "nccl" backend on ROCm) executes in the
driver's GPU tests, at world size 1 on the one-GPU box (VERDICT r4 "next" 4).

The N>1 path of bench.py and the consumer-side gathers (sharding.gather_obs /
gather_state, the reference's "parallel games", delivery_drone/
socket_server.py:113-124) run over RCCL on device tensors:
  * tools/multirank_check.py under torch.distributed.run --nproc-per-node 1
    --backend nccl: one rank steps its shard, gathers obs / reward / done /
    every SoA field through RCCL and compares them bit for bit with the same
    frames run as one batch in a fresh child process;
  * bench.py --dist-backend nccl --full --gather-point: the process group initialised
    as at N>1, gather_point timed and checked (its rank-0 block unchanged).
The 1->8 scaling curve is the driver's (an 8-GPU node); this pins that the
code path initialises RCCL and moves device tensors correctly on ROCm.
"""
import json
import os
import socket
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _torchrun(script_args, timeout):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node", "1",
           "--master-addr", "127.0.0.1", "--master-port", str(_port())] + script_args
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    return subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=REPO)


def test_rccl_gathers_equal_one_batch(tmp_path, gpu_device):
    total, frames = 65_536 + 777, 60
    r = _torchrun([os.path.join(REPO, "tools", "multirank_check.py"), "--backend", "nccl", "--out", str(tmp_path),
                   "--total", str(total), "--frames", str(frames)], timeout=110)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    res = json.load(open(tmp_path / "multirank.json"))
    assert res["world"] == 1 and res["backend"] == "nccl" and res["total"] == total
    assert res["bit_equal"], res["checks"]
    assert set(res["checks"]) >= {"obs", "reward", "done", "x", "total_reward", "status", "steps", "episode"}


def test_bench_gather_point_over_rccl(gpu_device):
    r = _torchrun([os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5",
                   "--dist-backend", "nccl", "--full", "--gather-point", "--cpu-baseline", "0", "--hbm-point", "0",
                   "--rollout-point", "0", "--no-extra-points"], timeout=110)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    out = json.loads(line)
    gp = out["gather_point"]
    assert gp and "error" not in gp, gp
    assert gp["backend"] == "nccl" and gp["rows"] == out["config"]["global_envs"] and gp["ms"] > 0
    assert out["n_gpus"] == 1 and out["value"] > 0
