"""The Barlow Twins kernels of csrc/barlow.hip against the rounded torch twin
(``barlow_twins_torch(..., round_operands=True)``) on the same z: loss, dz, the exposed C (the
twin runs on the host; it evaluates its statistics' quotients and root through fp64, as the
kernel does, so it gives the same bits on the GPU); the
fp32-input variant, degenerate columns, the fallbacks, repeatability; eager against
captured-and-replayed training steps; the CLI.

Shapes (n, D): (32, 64) one K step and a 4 x 4 grid of 16 x 16 tiles; (96, 128) three K steps,
one per split; (512, 128) the workload's split count (16); (128, 512) and (64, 2048) wide D, many
tiles, K steps over D in the backward.  lambda 0.0051 and 1.0 (the off-diagonal path then carries
the gradient).

Tolerances: the loss at the kernel family's 1e-4·max(1, |ref|); the relative L2 of dz below 1e-2
(bf16 output rounding); C within 2·n·2^-24 of the twin's (the standardised columns have mean
square <= 1, so a sum of n terms is at most n and its fp32 summation order moves it by about
n·2^-24; the factor 2 covers the merge of the splits), one entry per 10,000 excepted, which may
exceed it by 2^-8 / n (tests/test_barlow.py checks the same bound on the twin under another
summation order).  Measured values: profiles/barlow.md."""
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

_spec = importlib.util.spec_from_file_location("_barlow_cpu_tests",
                                               ROOT / "tests" / "test_barlow.py")
_cpu = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_cpu)
views, seed_for, check_c, c_bound, SHAPES = (_cpu.views, _cpu.seed_for, _cpu.check_c,
                                             _cpu.c_bound, _cpu.GPU_SHAPES)


def _rel(a, b):
    return float((a.float() - b.float()).norm() / (b.float().norm() + 1e-12))


def _hip(z, n, lambd, g=None):
    from simclr_amd.loss.barlow import BarlowTwins, hip_path
    from simclr_amd.ops import _ext
    _ext.require()
    assert hip_path(z, n)
    zh = z.clone().requires_grad_(True)
    loss, C = BarlowTwins(lambd)(zh, return_c=True)
    (loss if g is None else loss * g).backward()
    return loss.detach(), zh.grad, C


def _twin(z, n, lambd, g=None):
    """The rounded twin on the host; results on z's device."""
    from simclr_amd.loss.barlow import barlow_twins_torch
    zr = z.cpu().requires_grad_(True)
    loss, C = barlow_twins_torch(zr, n, lambd, round_operands=True, return_c=True)
    (loss if g is None else loss * g).backward()
    return loss.detach().to(z.device), zr.grad.to(z.device), C.to(z.device)


_REF = {}


def _reference(n, D, lambd):
    """The rounded twin, once per case (bf16 z)."""
    key = (n, D, lambd)
    if key not in _REF:
        z = views(n, D, seed_for(n, D), DEV).to(torch.bfloat16)
        _REF[key] = (z, *_twin(z, n, lambd))
    return _REF[key]


@pytest.mark.parametrize("lambd", [0.0051, 1.0])
@pytest.mark.parametrize("n,D", SHAPES)
def test_kernels_match_rounded_twin(n, D, lambd):
    """Measured on an MI355X (profiles/barlow.md): the kernel's rstd and bf16 ẑ have the twin's
    bits at every shape, C is within 2.4e-7, the loss within 1.2e-7 relative and dz within 8.9e-5
    relative L2."""
    z, ref, gref, Cref = _reference(n, D, lambd)
    loss, grad, C = _hip(z, n, lambd)
    dc = check_c(C, Cref, n)
    print(f"n {n} D {D} lambda {lambd}: loss {float(loss):.6f} ref {float(ref):.6f} "
          f"|dloss| {abs(float(loss) - float(ref)):.3e} rel dz {_rel(grad, gref):.3e} "
          f"max|dC| {dc:.3e} (bound {c_bound(n):.3e})")
    assert grad.dtype == torch.bfloat16 and gref.dtype == torch.bfloat16
    assert abs(float(loss) - float(ref)) <= 1e-4 * max(1.0, abs(float(ref))), (float(loss),
                                                                               float(ref))
    assert _rel(grad, gref) < 1e-2, _rel(grad, gref)


def test_upstream_gradient_is_read_on_the_device():
    """g != 1: G = bf16(−2g(1 − C)) / bf16(2gλC), with g taken from the incoming gradient."""
    n, D, lambd = 96, 128, 1.0
    z = _reference(n, D, lambd)[0]
    _, grad, _ = _hip(z, n, lambd, g=0.37)
    _, gref, _ = _twin(z, n, lambd, g=0.37)
    assert _rel(grad, gref) < 1e-2, _rel(grad, gref)


def test_fp32_input():
    n, D, lambd = 32, 64, 0.0051
    z = views(n, D, seed_for(n, D), DEV) * 1.0009765625  # (no longer bf16-representable)
    loss, grad, C = _hip(z, n, lambd)
    ref, gref, Cref = _twin(z, n, lambd)
    check_c(C, Cref, n)
    print("fp32", float(loss), float(ref), _rel(grad, gref))
    assert grad.dtype == torch.float32
    assert abs(float(loss) - float(ref)) <= 1e-4 * max(1.0, abs(float(ref)))
    assert _rel(grad, gref) < 1e-2


def test_constant_column_and_identical_views():
    n, D, lambd = 32, 64, 0.0051
    z = views(n, D, 9, DEV)
    z[:n, 7] = 1.25
    z[:, 20] = -3.0  # constant in both views
    z = z.to(torch.bfloat16)
    for zz in (z, torch.cat([z[:n], z[:n]])):
        loss, grad, C = _hip(zz, n, lambd)
        ref, gref, Cref = _twin(zz, n, lambd)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad.float()).all())
        assert torch.equal(C[7], torch.zeros(D, device=DEV))
        assert torch.equal(grad[:, 20], torch.zeros(2 * n, device=DEV, dtype=grad.dtype))
        check_c(C, Cref, n)
        assert abs(float(loss) - float(ref)) <= 1e-4 * max(1.0, abs(float(ref)))
        assert _rel(grad, gref) < 1e-2, _rel(grad, gref)


@pytest.mark.parametrize("n,D", [(24, 64), (32, 96)])
def test_fallback_is_the_twin_bitwise(n, D):
    from simclr_amd.loss.barlow import BarlowTwins, barlow_twins_torch, hip_path
    z = views(n, D, 3, DEV).to(torch.bfloat16)
    assert not hip_path(z, n)
    za = z.clone().requires_grad_(True)
    la = BarlowTwins()(za)
    la.backward()
    zb = z.clone().requires_grad_(True)
    lb = barlow_twins_torch(zb, n, 0.0051)
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(za.grad, zb.grad)


def test_repeatable():
    n, D = 512, 128
    z = _reference(n, D, 0.0051)[0]
    a, b = _hip(z, n, 0.0051), _hip(z, n, 0.0051)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_ops_check_their_shapes():
    ops = torch.ops.simclr_amd
    z = torch.zeros(48, 64, device=DEV, dtype=torch.bfloat16)  # n 24
    with pytest.raises(RuntimeError, match="barlow"):
        ops.bt_standardize(z, 1e-5, torch.zeros(2, 64, device=DEV),
                           torch.zeros_like(z), torch.zeros(2, 64, 24, device=DEV,
                                                            dtype=torch.bfloat16))
    zhT = torch.zeros(2, 64, 32, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="bt_corr"):
        ops.bt_corr(zhT, 32, 2, torch.zeros(2, 64, 64, device=DEV))  # more splits than K steps
    with pytest.raises(RuntimeError, match="bt_backward"):
        ops.bt_backward(torch.zeros(64, 64, device=DEV, dtype=torch.bfloat16),
                        torch.zeros(64, 64, device=DEV, dtype=torch.bfloat16),
                        torch.zeros(64, 64, device=DEV, dtype=torch.bfloat16),
                        torch.zeros(64, 64, device=DEV), torch.zeros(2, 1, 1, 64, device=DEV))


# ------------------------------------------------------------------ training path
def _run_steps(tmp_path, mode):
    out = tmp_path / f"{mode}.pt"
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable,
                        str(ROOT / "tests" / "_barlow_steps.py"), mode, str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, (mode, r.returncode, r.stdout[-2000:] + r.stderr[-3000:])
    return torch.load(out, weights_only=True)


@pytest.mark.timeout(900)
def test_captured_steps_equal_eager_bitwise(tmp_path):
    """Five different batches, eager against captured after the second step and replayed, by
    hipGraphLaunch and by the multi-stream executor (each run starts only after the one before
    ended well): losses and fp32 master weights bit for bit."""
    a = _run_steps(tmp_path, "eager")
    assert a["replayed"] == 0 and len(set(a["losses"].tolist())) == 5
    for mode in ("graph", "streams"):
        b = _run_steps(tmp_path, mode)
        assert b["replayed"] == 3 and b["mode"] == mode
        print(mode, a["losses"].tolist(), b["losses"].tolist())
        assert torch.equal(a["losses"], b["losses"]), (mode, a["losses"], b["losses"])
        assert torch.equal(a["master"], b["master"]), mode


@pytest.mark.timeout(900)
def test_cli_pretrains_and_knn_reads_the_checkpoint(tmp_path):
    run = tmp_path / "run"
    common = ["data.synthetic=true", "data.synthetic_size=256", "experiment.batches=32",
              "experiment.base_cnn=resnet18"]
    r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, str(ROOT / "main.py"),
                        "loss.kind=barlow", *common, "parameter.epochs=1",
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
    ev = tmp_path / "ev"
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, str(ROOT / "eval.py"),
                        *common, "parameter.classifier=knn", "parameter.knn_k=3",
                        f"experiment.target_dir={run}", f"hydra.run.dir={ev}"],
                       cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads((ev / "results.json").read_text())["epoch=1-cifar10.pt"]
    assert 0.0 <= res["val_acc"] <= 1.0 and res["knn_k"] == 3
