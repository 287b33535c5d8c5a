"""CPU: bench.py keeps the driver's contract without running it (that needs a
GPU): the metric is BASELINE.json's, the defaults are one GPU and a bounded
run at config 3, and the CPU-baseline leg (the test-only oracle) reports the
fields the bench line carries."""
import importlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    return importlib.import_module("bench")  # the repo root is on sys.path (conftest.py)


def test_metric_is_baselines():
    base = json.load(open(os.path.join(REPO, "BASELINE.json")))
    assert _bench().METRIC == base["metric"]


def test_defaults_are_one_gpu_config3(monkeypatch):
    b = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = b.parse()
    assert (a.gpus, a.envs_per_gpu, a.precision) == (1, 262_144, "f32")
    assert a.steps > 0 and a.warmup >= 0 and a.graph_steps > 0 and not a.no_obs
    assert a.dist_backend == "nccl"


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch, capsys):
    import pytest
    b = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"])
    a = b.parse()
    assert not a.full and not a.dump_outputs and a.steps == 20 and a.warmup == 5
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = b.parse()
    assert a.full and a.dump_outputs == "d"
    for bad in (["--gather-point"], ["--steps", "0"]):  # a --full measurement asked of a plain run; nothing to time
        monkeypatch.setattr(sys, "argv", ["bench.py"] + bad)
        with pytest.raises(SystemExit):
            b.parse()
    capsys.readouterr()


def test_dump_outputs_writes_the_step_outputs(tmp_path, monkeypatch):
    import types
    import numpy as np
    import torch
    b = _bench()
    n = 1000
    g = torch.Generator().manual_seed(3)
    env = types.SimpleNamespace(num_envs=n, device=torch.device("cpu"), obs=torch.randn(n, 15, generator=g),
                                reward=torch.randn(n, generator=g, dtype=torch.float64),
                                done=torch.rand(n, generator=g) < 0.1)
    assert b.dump_outputs(str(tmp_path / "a"), env, True) == ["done", "obs", "reward"]
    obs, rew, done = (np.load(tmp_path / "a" / f"{k}.npy") for k in ("obs", "reward", "done"))
    assert obs.dtype == np.float32 and rew.dtype == np.float64 and done.dtype == np.float32
    assert np.array_equal(obs, env.obs.numpy()) and np.array_equal(rew, env.reward.numpy())
    assert np.array_equal(done, env.done.numpy().astype(np.float32))
    assert b.dump_outputs(str(tmp_path / "b"), env, False, rank=1, world=2) == ["done", "reward"]
    assert sorted(os.listdir(tmp_path / "b")) == ["done_rank1.npy", "reward_rank1.npy"]
    # over the byte budget: the same fixed sample of lanes in every array, within the budget, on every call
    monkeypatch.setattr(b, "DUMP_BYTES_MAX", 8000)
    for d in ("c", "d"):
        assert b.dump_outputs(str(tmp_path / d), env, True) == ["done", "obs", "reward", "sample_rows"]
    got = {k: np.load(tmp_path / "c" / f"{k}.npy") for k in ("obs", "reward", "done", "sample_rows")}
    lanes = got["sample_rows"].astype(np.int64)
    assert 0 < len(lanes) < n and np.all(np.diff(lanes) > 0) and sum(v.nbytes for v in got.values()) <= 8000
    assert np.array_equal(got["obs"], env.obs.numpy()[lanes]) and np.array_equal(got["reward"], env.reward.numpy()[lanes])
    assert all(np.array_equal(v, np.load(tmp_path / "d" / f"{k}.npy")) for k, v in got.items())


def test_cpu_baseline_fields():
    b = _bench()
    r = b.cpu_baseline(0.3, 2, 0)
    assert set(r) >= {"value", "unit", "cores", "kind", "sample"}
    assert r["kind"] == "port" and r["cores"] == 2 and r["value"] > 0
    assert set(r["legs"]) == {"python_objects", "c_scalar"}
    assert r["value"] == r["legs"]["python_objects"]["value"]
    assert r["legs"]["c_scalar"]["value"] > r["legs"]["python_objects"]["value"]  # C beats Python objects
    assert r["host_cores"] == os.cpu_count() and r["affinity_cores"] >= 1 and r["cpu_model"]
    assert r["baseline_leg"] == "python_objects" and set(r["speedup_basis"]) == set(r["legs"])
    sh = r["cpu_share"]
    assert 1 <= sh["cores"] <= sh["affinity_cores"] and sh["source"]


def test_cpu_share_from_cgroup_files(tmp_path):
    # the worker count follows the cgroup quota when one is set
    b = _bench()
    proc = tmp_path / "cgroup"
    proc.write_text("0::/job\n")
    (tmp_path / "job").mkdir()
    (tmp_path / "job" / "cpu.max").write_text("1600000 100000\n")
    assert b._cgroup_quota(str(tmp_path), str(proc)) == (16.0, str(tmp_path / "job" / "cpu.max"))
    (tmp_path / "job" / "cpu.max").write_text("max 100000\n")
    q, why = b._cgroup_quota(str(tmp_path), str(proc))
    assert q is None and "no CPU quota" in why
    proc.write_text("4:cpu,cpuacct:/c1\n")  # cgroup v1
    d = tmp_path / "cpu,cpuacct" / "c1"
    d.mkdir(parents=True)
    (d / "cpu.cfs_quota_us").write_text("800000\n")
    (d / "cpu.cfs_period_us").write_text("100000\n")
    assert b._cgroup_quota(str(tmp_path), str(proc))[0] == 8.0


def test_pmc_traffic_only_for_the_measured_build(tmp_path):
    # roofline.traffic must come from counters of the loaded build
    from delivery_drone_amd import abi
    b = _bench()
    info = abi.lib().dd_build_info().decode()
    assert info.startswith(f"abi={abi.DD_ABI_VERSION};step_isa=")
    row = {"envs": 262144, "precision": "f32", "obs": True, "hbm_bytes_per_launch": 123}
    p = tmp_path / "pmc.json"
    p.write_text(json.dumps({"rows": [row]}))
    v, note = b.pmc_traffic_row(262144, "f32", True, str(p))
    assert v is None and "build_info" in note
    p.write_text(json.dumps({"rows": [dict(row, build_info="abi=1;step_isa=0000000000000000")]}))
    v, note = b.pmc_traffic_row(262144, "f32", True, str(p))
    assert v is None and "step_isa" in note
    p.write_text(json.dumps({"rows": [dict(row, build_info=info)]}))
    v, note = b.pmc_traffic_row(262144, "f32", True, str(p))
    mine = dict(kv.split("=", 1) for kv in info.split(";"))
    assert v == 123 and f"step_kernel_isa={mine['step_kernel_isa']}" in note  # the note names the matched hash
    # the step kernel's own hash decides: another edit of the translation unit (step_isa) keeps the row
    other = ";".join(f"{k}={'0' * 16 if k == 'step_isa' else v}" for k, v in mine.items())
    p.write_text(json.dumps({"rows": [dict(row, build_info=other)]}))
    assert b.pmc_traffic_row(262144, "f32", True, str(p))[0] == 123
    other = ";".join(f"{k}={'0' * 16 if k == 'step_kernel_isa' else v}" for k, v in mine.items())
    p.write_text(json.dumps({"rows": [dict(row, build_info=other)]}))
    v, note = b.pmc_traffic_row(262144, "f32", True, str(p))
    assert v is None and "step_kernel_isa" in note
    p.write_text(json.dumps({"rows": [dict(row, build_info=info)]}))
    assert b.pmc_traffic_row(4096, "f32", True, str(p))[0] is None
    # rollout rows are keyed by kernel and frames, and never stand in for a step row (or the reverse)
    roll = dict(row, envs=65536, kernel="rollout_kernel", frames=256, hbm_bytes_per_launch=456, build_info=info)
    p.write_text(json.dumps({"rows": [dict(row, build_info=info), roll]}))
    assert b.pmc_traffic_row(65536, "f32", True, str(p), kernel="rollout_kernel", frames=256)[0] == 456
    assert b.pmc_traffic_row(65536, "f32", True, str(p), kernel="rollout_kernel", frames=128)[0] is None
    assert b.pmc_traffic_row(65536, "f32", True, str(p))[0] is None
    assert b.pmc_traffic_row(262144, "f32", True, str(p))[0] == 123


def test_kernel_hashes_are_of_real_functions(tmp_path):
    # a kernel hash of no function at all would equal itself across every edit and keep every PMC row "valid"
    import hashlib
    import importlib.util
    import pytest
    from delivery_drone_amd import abi
    mine = dict(kv.split("=", 1) for kv in abi.lib().dd_build_info().decode().split(";"))
    empty = hashlib.sha256().hexdigest()[:16]
    assert mine["step_kernel_isa"] != empty and mine["rollout_kernel_isa"] != empty
    spec = importlib.util.spec_from_file_location("build_info", os.path.join(REPO, "tools", "build_info.py"))
    build_info = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build_info)
    s = tmp_path / "unit.s"
    s.write_text("_ZN2dd11step_kernelIfEEvv:\n\ts_endpgm\n.Lfunc_end0:\n")
    assert build_info.kernel_digest(str(s), b"_ZN2dd11step_kernel") != empty
    with pytest.raises(ValueError, match="no function"):
        build_info.kernel_digest(str(s), b"_ZN2dd14rollout_kernel")


def _gather_rank(rank, world, port, outdir):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    b = _bench()
    n = 1000
    obs = torch.full((n, 15), float(rank)) + torch.arange(n, dtype=torch.float32)[:, None]
    res = b.gather_point(obs, n, world, "gloo", reps=2)
    mx = b.reduce_max([float(rank), -float(rank)], "gloo", obs.device)
    if rank == 0:
        with open(os.path.join(outdir, "gp.json"), "w") as f:
            json.dump({"gp": res, "max": mx}, f)
    dist.barrier()
    dist.destroy_process_group()


def test_bench_multi_rank_helpers_on_gloo(tmp_path):
    # bench.py's N>1 pieces (the obs gather point and the max-over-ranks timing
    # reduction) on two gloo ranks; on the GPU node the same code runs on RCCL
    import socket
    import torch.multiprocessing as tmp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    tmp.spawn(_gather_rank, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    d = json.load(open(tmp_path / "gp.json"))
    assert d["gp"]["rows"] == 2000 and d["gp"]["bytes_to_rank0"] == 2000 * 60 and d["gp"]["backend"] == "gloo"
    assert d["max"] == [1.0, 0.0]


def test_launcher_refuses_nccl_without_enough_gpus():
    # `python bench.py --gpus 2` (no torch.distributed.run) is its own launcher
    # (VERDICT r05 next #2); with RCCL and fewer visible GPUs than ranks it must
    # fail fast, before starting any rank or measuring anything
    import subprocess
    import torch
    if torch.cuda.device_count() >= 2:
        import pytest
        pytest.skip("this host has two GPUs")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--cpu-baseline", "0"],
                       capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode != 0 and "RCCL needs one GPU per rank" in r.stderr, r.stderr[-2000:]
    assert not r.stdout.strip()
