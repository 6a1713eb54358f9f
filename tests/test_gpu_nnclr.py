"""The NNCLR kernels of csrc/nnclr.hip against the torch twin of simclr_amd/loss/nnclr.py: the
lookup on planted and on random support sets, loss / dz / a against the rounded twin given the
kernel's own neighbours, the enqueue, repeatability, the fallbacks and the bindings' size checks;
eager against captured-and-replayed training steps; the CLI.

Shapes (n, D, Q): (16, 32, 256) one query tile, one K step, one loss tile per view;
(48, 64, 768) three loss tiles, 12 queue iterations split 12 ways; (64, 128, 4096) the
workload's D, 64 queue splits; (32, 256, 1024) the widest D; once (512, 128, 16384), the
workload (32 query tiles x 32 queue splits, 8 iterations each; 8 loss splits).

Tolerances: the lookup's δ = 2·D·2^-24·1.01 is the fp32 accumulation bound for two vectors of
norm at most 1 + 2^-8, applied to both sides of the comparison (derived, not tuned; every row is
checked).  The loss at the kernel family's 1e-4·max(1, |ref|); the relative L2 of dz below 1e-2
for a bf16 z and 1e-3 for an fp32 z (tests/test_gpu_supcon.py's).  Everything else is bit for
bit.  Measured values: profiles/nnclr.md."""
import functools
import importlib.util
import json
import subprocess
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = Path(__file__).resolve().parents[1]
T = 0.1

_spec = importlib.util.spec_from_file_location("_nnclr_cpu_tests", ROOT / "tests" / "test_nnclr.py")
_cpu = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_cpu)
views, rand_queue, planted, rel_l2 = _cpu.views, _cpu.rand_queue, _cpu.planted, _cpu.rel_l2

SHAPES = [(16, 32, 256), (48, 64, 768), (64, 128, 4096), (32, 256, 1024)]
BIG = (512, 128, 16384)


def _module(queue, cursor=0):
    from simclr_amd.loss.nnclr import NNCLR
    from simclr_amd.ops import _ext
    _ext.require()
    mod = NNCLR(T, queue_size=queue.shape[0], dim=queue.shape[1], device=torch.device(DEV), seed=0)
    mod.queue.copy_(queue)
    mod.cursor.fill_(cursor)
    return mod


def _hip(z, queue, g=1.0, update=False, cursor=0):
    """One forward + backward through the kernels: loss, dz, idx, a, the module."""
    from simclr_amd.loss.nnclr import hip_path
    n = z.shape[0] // 2
    mod = _module(queue, cursor)
    zd = z.to(DEV).requires_grad_(True)
    assert hip_path(zd, n, queue.shape[0])
    loss, idx, a = mod(zd, update=update, return_nn=True)
    (loss * g).backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), zd.grad.cpu(), idx.cpu(), a.cpu(), mod


def _twin(z, queue, idx, g=1.0):
    from simclr_amd.loss.nnclr import nnclr_torch
    zr = z.clone().requires_grad_(True)
    loss = nnclr_torch(zr, queue, z.shape[0] // 2, T, round_operands=True, nn_idx=idx)
    (loss * g).backward()
    return loss.detach(), zr.grad


@functools.lru_cache(maxsize=None)
def _case(n, D, Q, dtype):
    """z, a random support set, the kernels' results on them and the rounded twin's given the
    kernels' idx: computed once per shape, shared, never modified."""
    z = views(n, D, 100 + n + D).to(dtype)
    queue = rand_queue(Q, D, 200 + n + D)
    g = 2.5
    got = _hip(z, queue, g)[:4]
    ref = _twin(z, queue, got[2], g)
    return z, queue, got, ref


# ------------------------------------------------------------------ lookup
@pytest.mark.parametrize("n,D,Q", SHAPES + [BIG])
def test_lookup_finds_planted_neighbours(n, D, Q):
    z, zb, queue, pos, own, other = planted(n, D, Q, 11 + n)
    print(n, D, Q, "planted", own, "best other", other)
    assert own >= 0.99 and other <= (0.8 if D == 32 else 0.7)
    _, _, idx, a, _ = _hip(z, queue)
    assert idx.dtype == torch.int32 and torch.equal(idx.long(), pos)
    assert torch.equal(a, zb)  # (and so the kernel's ẑb is the twin's, bit for bit)


@pytest.mark.parametrize("n,D,Q", SHAPES + [BIG])
def test_lookup_on_a_random_queue_is_within_the_fp32_bound(n, D, Q):
    from simclr_amd.loss.nnclr import _normalize_exact
    z, queue, (_, _, idx, a), _ = _case(n, D, Q, torch.bfloat16)
    zb = _normalize_exact(z.float())[0].to(torch.bfloat16)
    sim = zb.double() @ queue.double().t()
    chosen = sim.gather(1, idx.long()[:, None]).squeeze(1)
    gap = sim.max(dim=1).values - chosen
    delta = 2 * D * 2.0 ** -24 * 1.01
    print(n, D, Q, "largest gap", float(gap.max()), "bound", delta,
          "rows off the fp64 argmax", int((gap > 0).sum()))
    assert int(idx.min()) >= 0 and int(idx.max()) < Q
    assert bool((gap <= delta).all())
    assert torch.equal(a, queue[idx.long()])


def test_lookup_ties_and_nan():
    n, D, Q = 16, 32, 256
    queue = rand_queue(Q, D, 31)
    queue[130] = queue[7]    # another 64-row iteration and split
    queue[71] = queue[7]     # another tile of the same iteration
    queue[9] = queue[200]
    queue[0] = float("nan")
    z = views(n, D, 32)
    z[0], z[1], z[n] = queue[130].float() * 2, queue[200].float(), queue[71].float()
    _, _, idx, a, _ = _hip(z, queue)
    assert idx[0] == 7 and idx[1] == 9 and idx[n] == 7 and int((idx == 0).sum()) == 0
    queue[:] = float("nan")
    loss, _, idx, _, _ = _hip(z, queue)
    assert idx.tolist() == [0] * (2 * n)


# ------------------------------------------------------------------ loss and dz
# (the workload's shape runs once, with the head's bf16 z)
@pytest.mark.parametrize("n,D,Q,dtype", [(*s, dt) for s in SHAPES
                                         for dt in (torch.bfloat16, torch.float32)]
                         + [(*BIG, torch.bfloat16)])
def test_loss_and_dz_match_the_rounded_twin(n, D, Q, dtype):
    z, queue, (loss, dz, idx, a), (rloss, rdz) = _case(n, D, Q, dtype)
    tol = 1e-2 if dtype == torch.bfloat16 else 1e-3
    print(n, D, Q, dtype, "loss", float(loss), float(rloss), abs(float(loss) - float(rloss)),
          "dz rel L2", rel_l2(dz, rdz))
    assert dz.dtype == dtype and bool(torch.isfinite(dz.float()).all())
    assert abs(float(loss) - float(rloss)) <= 1e-4 * max(1.0, abs(float(rloss)))
    assert rel_l2(dz, rdz) <= tol
    assert torch.equal(a, queue[idx.long()])


# ------------------------------------------------------------------ enqueue
@pytest.mark.parametrize("n,D,Q", [(48, 64, 768), (96, 32, 256)])
def test_enqueue_matches_the_twin_bitwise(n, D, Q):
    from simclr_amd.loss.nnclr import NNCLR, hip_path
    queue = rand_queue(Q, D, 41)
    mod = _module(queue)
    twin = NNCLR(T, queue_size=Q, dim=D, seed=0)
    twin.queue.copy_(queue)
    for step in range(3):
        z = views(n, D, 50 + step).to(torch.bfloat16)
        assert hip_path(z.to(DEV), n, Q)
        before = mod.queue.clone()
        _, idx, a = mod(z.to(DEV), return_nn=True)
        twin(z)
        assert torch.equal(a, before[idx.long()])  # the lookups saw the pre-step queue
        assert torch.equal(mod.queue.cpu(), twin.queue), step
        assert torch.equal(mod.cursor.cpu(), twin.cursor), step
    assert int(mod.cursor) == (3 * n) % Q  # (Q 256, n 96: the third write wrapped mid-batch)
    kept = mod.queue.clone()
    mod(views(n, D, 60).to(torch.bfloat16).to(DEV), update=False)
    assert torch.equal(mod.queue, kept) and int(mod.cursor) == (3 * n) % Q


def test_repeatable():
    n, D, Q = BIG
    z, queue, _, _ = _case(n, D, Q, torch.bfloat16)
    runs = []
    for _ in range(2):
        loss, dz, idx, a, mod = _hip(z, queue, update=True, cursor=Q - 100)
        runs.append((loss, dz, idx, a, mod.queue.cpu(), mod.cursor.cpu()))
    assert all(torch.equal(x, y) for x, y in zip(*runs))
    assert int(runs[0][5]) == n - 100


# ------------------------------------------------------------------ fallbacks, size checks
@pytest.mark.parametrize("n,D,Q", [(24, 64, 256), (32, 48, 256), (32, 64, 16), (32, 64, 320)])
def test_other_sizes_take_the_twin(n, D, Q):
    from simclr_amd.loss.nnclr import NNCLR, hip_path, nnclr_torch
    z = views(n, D, 70).to(torch.bfloat16).to(DEV)
    assert not hip_path(z, n, Q)
    mod = NNCLR(T, queue_size=Q, dim=D, device=torch.device(DEV), seed=3)
    queue = mod.queue.clone()
    za = z.clone().requires_grad_(True)
    la = mod(za)
    la.backward()
    zb = z.clone().requires_grad_(True)
    lb = nnclr_torch(zb, queue, n, T)
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(za.grad, zb.grad)
    assert int(mod.cursor) == n % Q and not torch.equal(mod.queue, queue)


def test_ops_check_their_sizes():
    ops = torch.ops.simclr_amd
    bf, f32, i32 = torch.bfloat16, torch.float32, torch.int32

    def zeros(*shape, dtype=f32):
        return torch.zeros(*shape, device=DEV, dtype=dtype)

    with pytest.raises(RuntimeError, match="nc_normalize: n must be a multiple of 16"):
        ops.nc_normalize(zeros(48, 64, dtype=bf), zeros(48, 64), zeros(48, 64, dtype=bf), zeros(48))
    with pytest.raises(RuntimeError, match="nc_normalize: D must be"):
        ops.nc_normalize(zeros(32, 48, dtype=bf), zeros(32, 48), zeros(32, 48, dtype=bf), zeros(32))
    with pytest.raises(RuntimeError, match="nc_normalize: zb must be"):
        ops.nc_normalize(zeros(32, 64, dtype=bf), zeros(32, 64), zeros(16, 64, dtype=bf), zeros(32))
    zb, q = zeros(32, 64, dtype=bf), zeros(256, 64, dtype=bf)
    good = dict(candv=zeros(4, 32), candi=zeros(4, 32, dtype=i32), idx=zeros(32, dtype=i32),
                a=zeros(32, 64, dtype=bf))
    with pytest.raises(RuntimeError, match="nc_lookup: the queue must be"):
        ops.nc_lookup(zb, zeros(256, 32, dtype=bf), 4, *good.values())
    with pytest.raises(RuntimeError, match="nc_lookup: Q must be"):
        ops.nc_lookup(zb, zeros(320, 64, dtype=bf), 4, *good.values())
    with pytest.raises(RuntimeError, match="nc_lookup: Q must be"):
        ops.nc_lookup(zeros(1024, 64, dtype=bf), q, 4, *good.values())  # n above Q
    with pytest.raises(RuntimeError, match="nc_lookup: 1 <= splits"):
        ops.nc_lookup(zb, q, 5, *good.values())
    with pytest.raises(RuntimeError, match="nc_lookup: candv / candi"):
        ops.nc_lookup(zb, q, 2, *good.values())
    with pytest.raises(RuntimeError, match="nc_lookup: idx"):
        ops.nc_lookup(zb, q, 4, good["candv"], good["candi"], zeros(16, dtype=i32), good["a"])
    with pytest.raises(RuntimeError, match="nc_forward: part"):
        ops.nc_forward(good["a"], zb, 10.0, 2, zeros(2 * 32 * 3))  # more splits than tiles
    with pytest.raises(RuntimeError, match="nc_forward: a must be"):
        ops.nc_forward(zeros(16, 64, dtype=bf), zb, 10.0, 1, zeros(32 * 3))
    with pytest.raises(RuntimeError, match="nc_backward: part"):
        ops.nc_backward(good["a"], zb, zeros(32, 64), zeros(32), zeros(32), 10.0, zeros(1), 1,
                        zeros(32 * 32), zeros(32, 64, dtype=bf), None)
    with pytest.raises(RuntimeError, match="nc_backward: one of"):
        ops.nc_backward(good["a"], zb, zeros(32, 64), zeros(32), zeros(32), 10.0, zeros(1), 1,
                        zeros(32 * 64), None, None)
    with pytest.raises(RuntimeError, match="nc_enqueue: the queue must be"):
        ops.nc_enqueue(zb, zeros(256, 128, dtype=bf), zeros(1, dtype=i32))
    with pytest.raises(RuntimeError, match="nc_enqueue: the cursor"):
        ops.nc_enqueue(zb, q, zeros(2, dtype=i32))


# ------------------------------------------------------------------ training path
def _run_steps(tmp_path, mode):
    out = tmp_path / f"{mode}.pt"
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable,
                        str(ROOT / "tests" / "_nnclr_steps.py"), mode, str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, (mode, r.returncode, r.stdout[-2000:] + r.stderr[-3000:])
    return torch.load(out, weights_only=True)


def _same(a, b, mode):
    for key in ("losses", "master", "momentum", "queue", "cursor"):
        if key in a or key in b:
            assert torch.equal(a[key], b[key]), (mode, key)
    assert a["buffers"].keys() == b["buffers"].keys()
    for key in a["buffers"]:
        assert torch.equal(a["buffers"][key], b["buffers"][key]), (mode, key)


@pytest.mark.timeout(900)
def test_captured_steps_equal_eager_bitwise(tmp_path):
    """Five different batches, eager against captured after the second step and replayed, by
    hipGraphLaunch and by the multi-stream executor (each run starts only after the one before
    ended well): losses, master, momentum, BatchNorm buffers, support set and cursor bit for
    bit."""
    a = _run_steps(tmp_path, "eager")
    assert a["replayed"] == 0 and len(set(a["losses"].tolist())) == 5
    assert int(a["cursor"]) == 160
    for mode in ("graph", "streams"):
        b = _run_steps(tmp_path, mode)
        assert b["replayed"] == 3 and b["mode"] == mode
        print(mode, a["losses"].tolist(), b["losses"].tolist())
        _same(a, b, mode)


@pytest.mark.timeout(600)
def test_key_off_is_the_ntxent_run_bitwise(tmp_path):
    """Without ``loss.kind`` and with ``loss.kind=ntxent`` no NNCLR object exists, no NNCLR
    launch runs, and the five steps are the same NT-Xent steps bit for bit."""
    off, nt = _run_steps(tmp_path, "off"), _run_steps(tmp_path, "ntxent")
    assert "queue" not in off and "queue" not in nt
    _same(off, nt, "off")


@pytest.mark.timeout(900)
def test_cli_pretrains_and_knn_reads_the_checkpoint(tmp_path):
    run = tmp_path / "run"
    common = ["data.synthetic=true", "data.synthetic_size=256", "experiment.batches=32",
              "experiment.base_cnn=resnet18"]
    r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, str(ROOT / "main.py"),
                        "loss.kind=nnclr", "loss.nn_queue=1024", *common, "parameter.epochs=1",
                        "experiment.save_model_epoch=1", f"hydra.run.dir={run}"],
                       cwd=str(tmp_path), capture_output=True, text=True)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "training step captured" in out, out[-4000:]
    line = [l for l in out.splitlines() if "Epoch:1/1 progress:1.000 loss:" in l][0]
    loss = float(line.split("loss:")[1].split(",")[0])
    assert loss == loss and 0.0 < loss < 1e4 and ", lr:" in line
    rec = [json.loads(l) for l in (run / "metrics.jsonl").read_text().splitlines()]
    assert set(rec[0]) == {"epoch", "step", "loss", "lr", "images_per_sec", "seconds", "time"}
    assert rec[0]["step"] == 8
    assert (run / "epoch=1-cifar10.pt").exists()
    entry = torch.load(run / "resume-1.pt", weights_only=False)["nn_queue"]
    assert tuple(entry["queue"].shape) == (1024, 128) and int(entry["cursor"]) == 256
    ev = tmp_path / "ev"
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, str(ROOT / "eval.py"),
                        *common, "parameter.classifier=knn", "parameter.knn_k=3",
                        f"experiment.target_dir={run}", f"hydra.run.dir={ev}"],
                       cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads((ev / "results.json").read_text())["epoch=1-cifar10.pt"]
    assert 0.0 <= res["val_acc"] <= 1.0 and res["knn_k"] == 3
