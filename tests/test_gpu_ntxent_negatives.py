"""The weighted-negatives kernels of csrc/ntxent.hip (``WeightedNeg<HARD>``: hard-negative,
debiased, decoupled NT-Xent) against the twin ``nt_xent_weighted_torch`` evaluated in fp32 on the
same bf16 z: loss and dz at every shape, setting and clamp regime of tests/_negatives_data.py for
bf16 and fp32 z, the per-row clamp flags against fp64, bitwise identity with the plain loss at
the defaults, the gathered path (in-process fakes of the collectives), repeatability, the
fallbacks to the twin, the bindings' checks, capture + replay and the CLI.

Tolerances: those of tests/test_gpu_supcon.py for the same kernels (exact-fp32 MFMA): loss
1e-4·max(1, |ref|), relative L2 of dz 1e-2 (bf16 output rounding)."""
import json
import math
import subprocess
import sys
import types
from pathlib import Path

import pytest
import torch

import _negatives_data as nd

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = Path(__file__).resolve().parents[1]


def _rel(a, b):
    return float((a.float() - b.float()).norm() / (b.float().norm() + 1e-12))


def _kernel_flags(zb, n, tau, beta, tau_plus, dec):
    """k_i of the kernels: A_i > 0 in the finish kernel's stats.  A_i = k_i·N/(1−τ⁺)·e^{u−c}/T
    and u − c >= −2/τ = −20 at the temperatures used here (u is a weighted mean of logits in
    [−1/τ, 1/τ]), so e^{u−c} cannot underflow and A_i = 0 only where k_i = 0."""
    ops = torch.ops.simclr_amd
    R, D = zb.shape
    zn, inv = torch.empty(R, D, device=DEV), torch.empty(R, device=DEV)
    ops.nt_normalize(zb, zn, inv)
    znT = torch.empty(D, R, device=DEV)
    ops.nt_transpose(zn, znT)
    splits = ops.nt_fwd_splits(R, R)
    part = torch.empty(splits * R * (5 if beta > 0 else 3), device=DEV)
    stats, rows = torch.empty(R, 4, device=DEV), torch.empty(R, device=DEV)
    ops.nt_w_forward_range(znT, R, 0, n, 1.0 / tau, beta, part, 0, R, splits, 0)
    ops.nt_w_finish(part, R, splits, R, 1.0 / tau, beta, tau_plus, dec, stats, rows)
    assert bool(torch.isfinite(stats).all()) and bool(torch.isfinite(rows).all())
    return (stats[:, 1] > 0).cpu(), rows.cpu()


@pytest.mark.parametrize("regime", list(nd.REGIMES))
@pytest.mark.parametrize("setting", nd.SETTINGS, ids=str)
@pytest.mark.parametrize("n,D", nd.SHAPES)
def test_kernels_match_twin(n, D, setting, regime):
    from simclr_amd.loss.ntxent import NTXent, nt_xent_weighted_torch
    from simclr_amd.ops import _ext
    _ext.require()
    beta, tau_plus, dec = setting
    z64, tau = nd.case(n, D, regime)
    k64 = nd.clamp_flags(z64, n, tau, beta, tau_plus)  # (asserts the margin to the kink)
    nd.check_regime(k64, regime, tau_plus)
    fn = NTXent(tau, hard_beta=beta, tau_plus=tau_plus, decoupled=dec)
    zr = z64.float().to(DEV).requires_grad_(True)
    ref = nt_xent_weighted_torch(zr, n, tau, beta, tau_plus, dec)
    ref.backward()
    assert bool(torch.isfinite(zr.grad).all())
    for dtype in (torch.bfloat16, torch.float32):
        zh = z64.to(DEV).to(dtype).requires_grad_(True)
        loss = fn(zh)
        loss.backward()
        loss, ref = loss.detach(), ref.detach()
        print(n, D, setting, regime, dtype, float(loss), float(ref),
              abs(float(loss) - float(ref)) / max(1.0, abs(float(ref))), _rel(zh.grad, zr.grad))
        assert abs(float(loss) - float(ref)) < 1e-4 * max(1.0, abs(float(ref))), (float(loss),
                                                                                  float(ref))
        assert zh.grad.dtype == dtype
        assert _rel(zh.grad, zr.grad) < 1e-2, _rel(zh.grad, zr.grad)
    k, rows = _kernel_flags(z64.to(DEV).to(torch.bfloat16), n, tau, beta, tau_plus, dec)
    assert torch.equal(k, k64), (k.sum(), k64.sum())
    rows64 = nt_xent_weighted_torch(z64, n, tau, beta, tau_plus, dec, "none").reshape(-1)
    assert float((rows.double() - rows64).abs().max()) < 1e-4 * max(1.0, float(rows64.abs().max()))


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_sum_reduction_and_small_temperature(reduction):
    """τ = 0.01 (s up to ±100, (1+β)s ±300) stays finite in the kernels and equal to the twin."""
    from simclr_amd.loss.ntxent import NTXent, nt_xent_weighted_torch
    n, D = 24, 64
    z = nd.make_z(n, D, 3.0, 0)
    for beta, tau_plus, dec in nd.SETTINGS:
        zh = z.to(DEV).to(torch.bfloat16).requires_grad_(True)
        loss = NTXent(0.01, reduction, hard_beta=beta, tau_plus=tau_plus, decoupled=dec)(zh)
        loss.backward()
        ref = nt_xent_weighted_torch(z, n, 0.01, beta, tau_plus, dec, reduction)
        loss = loss.detach()
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(zh.grad.float()).all())
        assert abs(float(loss) - float(ref)) < 1e-4 * max(1.0, abs(float(ref))), (float(loss),
                                                                                  float(ref))


@pytest.mark.parametrize("n,D", nd.SHAPES)
def test_defaults_are_the_plain_loss_bitwise(n, D):
    from simclr_amd.loss.ntxent import NTXent
    z = nd.make_z(n, D, 3.0, 0).to(DEV).to(torch.bfloat16)
    za = z.clone().requires_grad_(True)
    la = NTXent(0.1)(za)
    la.backward()
    zb = z.clone().requires_grad_(True)
    lb = NTXent(0.1, hard_beta=0.0, tau_plus=0.0, decoupled=False)(zb)
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(za.grad, zb.grad)


def test_repeatable():
    from simclr_amd.loss.ntxent import NTXent
    n, D = 64, 128
    z = nd.make_z(n, D, 3.0, 0).to(DEV).to(torch.bfloat16)
    for beta, tau_plus, dec in nd.SETTINGS:
        res = []
        for _ in range(2):
            zh = z.clone().requires_grad_(True)
            loss = NTXent(0.1, hard_beta=beta, tau_plus=tau_plus, decoupled=dec)(zh)
            loss.backward()
            res.append((loss.detach().clone(), zh.grad.clone()))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


# ------------------------------------------------------------------ gathered, in one process
@pytest.mark.parametrize("setting", nd.SETTINGS, ids=str)
@pytest.mark.parametrize("W,r", [(2, 1), (4, 2)])
def test_gathered_kernel_path(monkeypatch, W, r, setting):
    """n = 24, D = 64, the mixed regime; the peers' blocks by the same recipe from other seeds."""
    from simclr_amd.loss import ntxent as mod
    beta, tau_plus, dec = setting
    n, D = 24, 64
    R = 2 * n
    tau, sigma = nd.REGIMES["mixed"]
    z64 = nd.make_z(n, D, sigma, 0)
    peers64 = [nd.make_z(n, D, sigma, 1000 + j) for j in range(W - 1)]
    blocks = list(peers64)
    blocks.insert(r, z64)
    k64 = nd.clamp_flags(z64, n, tau, beta, tau_plus, torch.cat(blocks), r * R)
    nd.check_regime(k64, "mixed", tau_plus)
    peers = [p.to(DEV).to(torch.bfloat16) for p in peers64]
    seen = {}

    def fake_all_gather(out, inp, group=None):
        b = list(peers)
        b.insert(r, inp)
        out.copy_(torch.cat(b))

    def fake_reduce_scatter(out, inp, group=None):
        seen["d_cols"] = inp.clone()
        out.copy_(inp[r * R:(r + 1) * R])

    monkeypatch.setattr(mod.dist, "all_gather_into_tensor", fake_all_gather)
    monkeypatch.setattr(mod.dist, "reduce_scatter_tensor", fake_reduce_scatter)
    st = types.SimpleNamespace(comm=True, world_size=W, rank=r, group=None)
    monkeypatch.setattr(mod.pstate, "get", lambda: st)
    zh = z64.to(DEV).to(torch.bfloat16).requires_grad_(True)
    loss = mod.NTXent(tau, gather=True, hard_beta=beta, tau_plus=tau_plus, decoupled=dec)(zh)
    loss.backward()
    torch.cuda.synchronize()

    # fp32 oracle: the twin's rows on the concatenated columns
    zr = z64.float().to(DEV).requires_grad_(True)
    pr = [p.float().requires_grad_(True) for p in peers]
    b = list(pr)
    b.insert(r, zr)
    cols = torch.nn.functional.normalize(torch.cat(b), dim=1)
    sim = cols[r * R:(r + 1) * R] @ cols.t() / tau
    ref = mod.weighted_rows(sim, n, r * R, tau, beta, tau_plus, dec).sum() / R
    ref.backward()
    loss, ref = loss.detach(), ref.detach()
    print(W, r, setting, float(loss), float(ref), _rel(zh.grad, zr.grad))
    assert abs(float(loss) - float(ref)) < 1e-4 * max(1.0, abs(float(ref))), (float(loss),
                                                                              float(ref))
    assert _rel(zh.grad, zr.grad) < 1e-2, _rel(zh.grad, zr.grad)
    # the column gradient sent to the peers, through the normalisation Jacobian of each block
    # (1e-3: fp32 on both sides, as tests/test_gpu_ntxent_gather.py)
    dc = seen["d_cols"]
    for j, (p, pg) in enumerate(zip(peers, pr)):
        blk = j if j < r else j + 1
        pn = torch.nn.functional.normalize(p.float(), dim=1)
        inv = 1.0 / p.float().norm(dim=1, keepdim=True)
        d = dc[blk * R:(blk + 1) * R]
        dz = (d - pn * (pn * d).sum(1, keepdim=True)) * inv
        assert _rel(dz, pg.grad) < 1e-3, (blk, _rel(dz, pg.grad))


# ------------------------------------------------------------------ fallbacks, bindings
def test_fallbacks_take_the_twin(monkeypatch):
    from simclr_amd.loss import ntxent as mod

    def no_kernels(*a, **k):
        raise AssertionError("the HIP path was taken")

    monkeypatch.setattr(mod._NTXentHipFn, "forward", staticmethod(no_kernels))
    fn = mod.NTXent(0.5, hard_beta=1.0, tau_plus=0.1)
    for n, D, red in ((12, 64, "mean"), (16, 48, "mean"), (16, 64, "none")):  # R % 16, D, none
        z = nd.make_z(n, D, 3.0, 0).to(DEV).to(torch.bfloat16)
        got = mod.NTXent(0.5, red, hard_beta=1.0, tau_plus=0.1)(z)
        want = mod.nt_xent_weighted_torch(z, n, 0.5, 1.0, 0.1, False, red)
        assert torch.equal(got, want) and got.shape == ((2, n) if red == "none" else ())
    with pytest.raises(AssertionError, match="HIP path"):
        fn(nd.make_z(16, 64, 3.0, 0).to(DEV).to(torch.bfloat16))


def test_bindings_check_before_launching():
    ops = torch.ops.simclr_amd
    n, D = 16, 32
    R = 2 * n
    znT = torch.zeros(D, R, device=DEV)
    zn = torch.zeros(R, D, device=DEV)
    part3, part5 = torch.zeros(R * 3, device=DEV), torch.zeros(R * 5, device=DEV)
    stats, rows = torch.zeros(R, 4, device=DEV), torch.zeros(R, device=DEV)
    ws, out = torch.zeros(R * D, device=DEV), torch.zeros(R, D, device=DEV)
    for bad in (-1.0, math.inf, math.nan):
        with pytest.raises(RuntimeError, match="hard_beta"):
            ops.nt_w_forward_range(znT, R, 0, n, 2.0, bad, part5, 0, R, 1, 0)
        with pytest.raises(RuntimeError, match="hard_beta"):
            ops.nt_w_finish(part5, R, 1, R, 2.0, bad, 0.1, False, stats, rows)
        with pytest.raises(RuntimeError, match="hard_beta"):
            ops.nt_w_backward_part(True, zn, znT, stats, R, 0, n, 2.0, bad, 1.0, None, ws, 1, out)
    for bad in (-0.1, 1.0, math.inf, math.nan):
        with pytest.raises(RuntimeError, match="tau_plus"):
            ops.nt_w_finish(part5, R, 1, R, 2.0, 1.0, bad, False, stats, rows)
    with pytest.raises(RuntimeError, match="part"):  # β > 0 needs 5 floats per row
        ops.nt_w_forward_range(znT, R, 0, n, 2.0, 1.0, part3, 0, R, 1, 0)
    with pytest.raises(RuntimeError, match="part"):
        ops.nt_w_finish(part3, R, 1, R, 2.0, 1.0, 0.1, False, stats, rows)
    with pytest.raises(RuntimeError, match="window"):
        ops.nt_w_forward_range(znT, R, 0, n, 2.0, 0.0, part3, 0, R + 16, 1, 0)
    with pytest.raises(RuntimeError, match="stats"):
        ops.nt_w_finish(part3, R, 1, R, 2.0, 0.0, 0.1, False, torch.zeros(R, device=DEV), rows)
    with pytest.raises(RuntimeError, match="loss"):
        ops.nt_w_finish(part3, R, 1, R, 2.0, 0.0, 0.1, False, stats, torch.zeros(R - 1, device=DEV))
    with pytest.raises(RuntimeError, match="stats"):
        ops.nt_w_backward_part(True, zn, znT, torch.zeros(R, device=DEV), R, 0, n, 2.0, 0.0, 1.0,
                               None, ws, 1, out)
    with pytest.raises(RuntimeError, match="stats"):  # not 16-byte aligned
        ops.nt_w_backward_part(True, zn, znT, torch.zeros(R * 4 + 1, device=DEV)[1:], R, 0, n,
                               2.0, 0.0, 1.0, None, ws, 1, out)
    with pytest.raises(RuntimeError, match="sizes"):
        ops.nt_w_backward_part(False, zn, znT, stats, R, 0, n, 2.0, 0.0, 1.0, None, ws[:-1], 1, out)
    with pytest.raises(RuntimeError, match="ntxent"):  # D = 48
        ops.nt_w_forward_range(torch.zeros(48, R, device=DEV), R, 0, n, 2.0, 0.0, part3, 0, R, 1, 0)
    with pytest.raises(RuntimeError, match="ntxent"):  # R != 2 n
        ops.nt_w_backward_part(True, zn, znT, stats, R, 0, n + 1, 2.0, 0.0, 1.0, None, ws, 1, out)
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0 and float(stats.abs().max()) == 0.0  # nothing ran


# ------------------------------------------------------------------ training path
def _run_steps(tmp_path, mode):
    out = tmp_path / f"{mode}.pt"
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable,
                        str(ROOT / "tests" / "_negatives_steps.py"), mode, str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, (mode, r.returncode, r.stdout[-2000:] + r.stderr[-3000:])
    return torch.load(out, weights_only=True)


@pytest.mark.timeout(900)
def test_captured_step_replays_bitwise(tmp_path):
    """Eager against captured-and-replayed (after the second step) through the graph and
    through the multi-stream executor: bitwise equal losses and master weights."""
    a = _run_steps(tmp_path, "eager")
    assert a["replayed"] == 0
    for mode in ("graph", "streams"):  # (each started only after the run before ended well)
        b = _run_steps(tmp_path, mode)
        assert b["replayed"] == 3 and b["mode"] == mode
        print(mode, a["losses"].tolist(), b["losses"].tolist())
        assert torch.equal(a["losses"], b["losses"]), (mode, a["losses"], b["losses"])
        assert torch.equal(a["master"], b["master"]), mode


@pytest.mark.timeout(900)
def test_cli_pretrains_and_evaluates(tmp_path):
    run = tmp_path / "run"
    common = ["data.synthetic=true", "data.synthetic_size=256", "experiment.batches=32",
              "experiment.base_cnn=resnet18"]
    r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, str(ROOT / "main.py"),
                        "+loss.hard_beta=1.0", "+loss.tau_plus=0.1", "+loss.decoupled=true",
                        *common, "parameter.epochs=1", "experiment.save_model_epoch=1",
                        f"hydra.run.dir={run}"],
                       cwd=str(tmp_path), capture_output=True, text=True)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "training step captured" in out, out[-4000:]
    line = [l for l in out.splitlines() if "Epoch:1/1 progress:1.000 loss:" in l][0]
    loss = float(line.split("loss:")[1].split(",")[0])
    assert math.isfinite(loss) and abs(loss) < 100 and ", lr:" in line
    rec = [json.loads(l) for l in (run / "metrics.jsonl").read_text().splitlines()]
    assert rec[0]["step"] == 8 and math.isfinite(rec[0]["loss"])
    assert (run / "epoch=1-cifar10.pt").exists()
    ev = tmp_path / "ev"
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, str(ROOT / "eval.py"),
                        *common, "parameter.classifier=knn", "parameter.knn_k=3",
                        f"experiment.target_dir={run}", f"hydra.run.dir={ev}"],
                       cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads((ev / "results.json").read_text())["epoch=1-cifar10.pt"]
    assert 0.0 <= res["val_acc"] <= 1.0 and res["knn_k"] == 3
