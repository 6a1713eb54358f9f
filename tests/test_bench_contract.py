"""bench.py's driver contract on the CPU (gloo): ``--gpus N`` started WITHOUT a launcher spawns
the N ranks itself (fail-fast launcher, /root/reference/launch.py:202-259) and reports the
whole-job number; a launcher/flag mismatch is an error, never a silent 1-rank measurement."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def _env():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", CUDA_VISIBLE_DEVICES="",
               HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="2")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


@pytest.mark.timeout(900)
def test_bench_gpus2_self_launches_two_ranks(tmp_path):
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--model", "resnet18",
           "--batch", "8", "--steps", "2", "--warmup", "1"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=_env(), capture_output=True, text=True,
                       timeout=840)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["config"]["parallelism"] == "dp2"
    assert j["config"]["global_batch"] == 16 and j["steps"] == 2 and j["warmup"] == 1
    assert j["value"] > 0 and j["dtype"] == "fp32"


def _bench_one_rank(tmp_path, out, *extra):
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--model", "resnet18",
           "--batch", "8", "--steps", "2", "--warmup", "1", "--dump-outputs", str(out), *extra]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=_env(), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_dump_outputs_and_full(tmp_path):
    """``--dump-outputs`` writes the last timed step's loss / parameters / BatchNorm buffers as
    float32 .npy (64 MB at most), the same arrays from run to run; the idle-device issue cost is
    measured only with ``--full``, after the dump, so it does not change what is written."""
    import numpy as np
    plain = _bench_one_rank(tmp_path, tmp_path / "a")
    full = _bench_one_rank(tmp_path, tmp_path / "b", "--full")
    for j in (plain, full):
        assert j["steps"] == 2 and j["warmup"] == 1 and j["ms_per_step"] > 0
        assert j["value"] == pytest.approx(8 * 1000.0 / j["ms_per_step"], rel=1e-3)
        assert {"metric", "unit", "higher_is_better", "dtype"} <= set(j)
    assert plain["config"]["host_issue_ms_idle_device"] is None
    assert full["config"]["host_issue_ms_idle_device"] > 0
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["buffers.npy", "loss.npy", "params.npy"]
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all(), n
        assert np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 64 << 20
    assert float(np.load(tmp_path / "a" / "loss.npy")[0]) == pytest.approx(
        plain["config"]["final_loss"], rel=1e-6)


@pytest.mark.gpu
def test_bench_flagship_runs_on_pinned_tiles(tmp_path):
    """The flagship configuration times nothing at its first step: every shape takes its recorded
    tile variant (bench/tiles_mi355x.json), so two runs compute bitwise the same.  A kernel change
    that makes a pin inadmissible, or adds a shape, shows here as a tuned entry: record the table
    again (``bench.py --tiles tune --save-tiles bench/tiles_mi355x.json``)."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SIMCLR_AUTOTUNE"):
        env.pop(k, None)
    # the default path: capture, planning replay, execution-mode probe (timing-driven; whichever
    # mode it keeps, the three compute bitwise the same: test_gpu_graph_exec / _forced_comm)
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["config"]["exec_mode"] in ("eager", "graph", "streams")
    assert j["config"]["exec_mode_probe_ms"] is not None
    assert j["config"]["tile_variants"]["unpinned"] == 0, j["config"]["tile_variants"]
    assert j["config"]["tile_variants"]["pinned"] > 0
    assert j["config"]["tile_pins_retimed"] is None  # the stale-pin check belongs to --full


def test_dump_outputs_samples_large_parameter_vectors(tmp_path):
    import importlib.util
    import numpy as np
    import torch
    spec = importlib.util.spec_from_file_location("bench_script", ROOT / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    n = bench.DUMP_PARAMS + 12345
    params = torch.arange(n, dtype=torch.float32)
    bufs = [torch.ones(3), torch.zeros(2, dtype=torch.long), torch.full((2,), 2.0)]
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, torch.tensor(1.5), params, bufs)
    a, b = np.load(tmp_path / "a" / "params.npy"), np.load(tmp_path / "b" / "params.npy")
    assert a.shape == (bench.DUMP_PARAMS,) and a.dtype == np.float32 and np.array_equal(a, b)
    assert 0 <= a.min() and a.max() < n and len(np.unique(a)) > bench.DUMP_PARAMS // 2
    assert np.load(tmp_path / "a" / "buffers.npy").tolist() == [1.0, 1.0, 1.0, 2.0, 2.0]
    assert np.load(tmp_path / "a" / "loss.npy").tolist() == [1.5]


def test_bench_world_mismatch_is_an_error(tmp_path):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(_env(), WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(port))
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--model", "resnet18",
           "--batch", "8", "--steps", "1", "--warmup", "0"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0
    assert "WORLD_SIZE=1" in r.stderr


def test_self_launch_never_touches_hip(monkeypatch):
    """The parent that forks every rank counts GPUs from the visibility variables / KFD
    topology only: torch.cuda.device_count() (which can fall back to hipGetDeviceCount) is never
    called and HIP stays uninitialised in the parent."""
    import argparse
    import torch
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_script", ROOT / "bench.py")
    bench = importlib.util.module_from_spec(spec)  # (the bench/ package shadows the name)
    spec.loader.exec_module(bench)
    from simclr_amd.runtime import launcher

    def boom(*a, **k):
        raise AssertionError("the launcher parent called into torch.cuda")
    monkeypatch.setattr(torch.cuda, "device_count", boom)
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    seen = {}

    def fake_launch(la):
        seen["n"] = la.nproc_per_node
        return 0
    monkeypatch.setattr(launcher, "launch", fake_launch)
    monkeypatch.delenv("HIP_VISIBLE_DEVICES", raising=False)
    monkeypatch.setenv("ROCR_VISIBLE_DEVICES", "0,1,2,3,4,5,6,7")
    rc = bench.self_launch(argparse.Namespace(gpus=8), ["--gpus", "8"])
    assert rc == 0 and seen["n"] == 8
    assert not torch.cuda.is_initialized()
    monkeypatch.setenv("ROCR_VISIBLE_DEVICES", "0,1")
    with pytest.raises(SystemExit, match="only 2 GPU"):
        bench.self_launch(argparse.Namespace(gpus=8), ["--gpus", "8"])


def test_visible_gpu_count_reads_kfd_topology(tmp_path, monkeypatch):
    from simclr_amd.runtime.launcher import visible_gpu_count
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        monkeypatch.delenv(var, raising=False)
    for i, simd in enumerate([0, 1024, 1024, 0]):  # CPU nodes have simd_count 0
        d = tmp_path / str(i)
        d.mkdir()
        (d / "properties").write_text(f"cpu_cores_count 8\nsimd_count {simd}\nmem_banks_count 1\n")
    assert visible_gpu_count(str(tmp_path)) == 2
    assert visible_gpu_count(str(tmp_path / "missing")) is None
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "")
    assert visible_gpu_count(str(tmp_path)) == 0


def test_visible_gpu_count_stacks_variables(monkeypatch):
    """ROCR filters the devices and HIP / CUDA filter what it left: the count is the minimum
    over the variables that are set, and an empty one hides every GPU."""
    from simclr_amd.runtime.launcher import visible_gpu_count
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("ROCR_VISIBLE_DEVICES", "0,1,2,3")
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "0,1")
    assert visible_gpu_count("/nonexistent") == 2
    monkeypatch.setenv("CUDA_VISIBLE_DEVICES", "")
    assert visible_gpu_count("/nonexistent") == 0
