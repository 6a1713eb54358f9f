"""Barlow Twins (``loss.kind=barlow``) on the CPU: the torch twin ``barlow_twins_torch`` against
its own unrounded form in fp64 (autograd), a closed form, affine invariance, a constant column,
the summation-order bound the GPU test puts on C, the config checks, the Trainer and the CLI.

Tolerances against the fp64 oracle (views correlated so that diag C is near 0.7): unrounded fp32
1e-5 on the loss (relative to max(1, |ref|)) and on the relative L2 of dz; with the bf16 operand
rounding 1e-3 and 1e-2, the kernel family's tolerance for a gradient built from bf16 operands."""
import functools
import json
import math
import subprocess
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
LAMBD = 0.0051
SHAPES = [(32, 64), (96, 128), (512, 128), (512, 256), (64, 2048)]
GPU_SHAPES = [(32, 64), (96, 128), (512, 128), (128, 512), (64, 2048)]  # tests/test_gpu_barlow.py


def views(n, D, seed, device="cpu"):
    """z = [z0; z1] in bf16-representable fp32: z0 = bf16(randn), z1 = bf16(0.7 z0 + 0.7 noise).
    Generated on the CPU so that every test (and the GPU tests) sees the same values."""
    g = torch.Generator().manual_seed(seed)
    z0 = torch.randn(n, D, generator=g).to(torch.bfloat16).float()
    z1 = (0.7 * z0 + 0.7 * torch.randn(n, D, generator=g)).to(torch.bfloat16).float()
    return torch.cat([z0, z1]).to(device)


def seed_for(n, D):
    return 1000 * n + D


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def _run(z, n, lambd=LAMBD, eps=1e-5, **kw):
    from simclr_amd.loss.barlow import barlow_twins_torch
    zr = z.clone().requires_grad_(True)
    loss = barlow_twins_torch(zr, n, lambd, eps, **kw)
    loss.backward()
    return loss.detach(), zr.grad


@functools.lru_cache(maxsize=None)
def _oracle(n, D):
    """fp64 autograd on the unrounded function, once per shape."""
    return _run(views(n, D, seed_for(n, D)).double(), n)


@pytest.mark.parametrize("n,D", SHAPES)
def test_twin_matches_fp64_oracle(n, D):
    ref, gref = _oracle(n, D)
    assert 0.5 < float(ref) / (D * 0.09 + LAMBD * D * D / n) < 2.0  # diag near 0.7
    z = views(n, D, seed_for(n, D))
    loss, g = _run(z, n)
    print("plain", n, D, float(ref), abs(float(loss) - float(ref)), _rel(g, gref))
    assert g.dtype == torch.float32
    assert abs(float(loss) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref)))
    assert _rel(g, gref) < 1e-5


@pytest.mark.parametrize("n,D", SHAPES)
def test_rounded_twin_matches_fp64_oracle(n, D):
    ref, gref = _oracle(n, D)
    z = views(n, D, seed_for(n, D))
    loss, g = _run(z, n, round_operands=True)
    print("rounded", n, D, float(ref), abs(float(loss) - float(ref)), _rel(g, gref))
    assert abs(float(loss) - float(ref)) <= 1e-3 * max(1.0, abs(float(ref)))
    assert _rel(g, gref) < 1e-2
    # a bf16 z gets a bf16 gradient, still within the bound
    lb, gb = _run(z.to(torch.bfloat16), n, round_operands=True)
    assert gb.dtype == torch.bfloat16 and torch.equal(lb, loss)
    assert _rel(gb, gref) < 1e-2


def test_closed_form():
    """z0 = z1 = sqrt(n) Q, Q with zero-mean orthonormal columns: mu = 0, var = 1,
    C = I / (1 + eps), loss = D (eps / (1 + eps))^2."""
    from simclr_amd.loss.barlow import barlow_twins_torch
    n, D, eps = 64, 16, 1e-3
    g = torch.Generator().manual_seed(0)
    a = torch.randn(n, D, generator=g, dtype=torch.float64)
    q, _ = torch.linalg.qr(a - a.mean(0, keepdim=True))
    assert float(q.mean(0).abs().max()) < 1e-14
    z = math.sqrt(n) * torch.cat([q, q])
    loss, C = barlow_twins_torch(z, n, LAMBD, eps, return_c=True)
    want = D * (eps / (1.0 + eps)) ** 2
    assert abs(float(loss) - want) <= 1e-9 * want, (float(loss), want)
    assert torch.allclose(C, torch.eye(D, dtype=torch.float64) / (1.0 + eps), rtol=0, atol=1e-13)


def test_affine_invariance():
    from simclr_amd.loss.barlow import barlow_twins_torch
    n, D = 48, 24
    z = views(n, D, 5).double()
    g = torch.Generator().manual_seed(6)
    a = 0.5 + 1.5 * torch.rand(2, 1, D, generator=g, dtype=torch.float64)
    b = torch.randn(2, 1, D, generator=g, dtype=torch.float64)
    za = (z.view(2, n, D) * a + b).reshape(2 * n, D)
    l0 = float(barlow_twins_torch(z, n, LAMBD, 1e-12))
    l1 = float(barlow_twins_torch(za, n, LAMBD, 1e-12))
    assert abs(l0 - l1) < 1e-6 * abs(l0), (l0, l1)


@pytest.mark.parametrize("rounded", [False, True])
def test_constant_column(rounded):
    """A constant column standardises to exactly 0 (never NaN): its row of C is 0, the loss and
    the gradient are finite.  Constant in ONE view its dz is rstd·(dẑ − mean dẑ) with
    dẑ_b = −2g ẑ1[b][i] / n — finite, not 0, and the fp64 oracle agrees; constant in BOTH views
    nothing reaches the column and its dz is exactly 0."""
    from simclr_amd.loss.barlow import barlow_twins_torch
    n, D, col = 32, 64, 7
    z = views(n, D, 9)
    z[:n, col] = 1.25
    zr = z.clone().requires_grad_(True)
    loss, C = barlow_twins_torch(zr, n, LAMBD, round_operands=rounded, return_c=True)
    loss.backward()
    loss = loss.detach()
    assert math.isfinite(float(loss)) and bool(torch.isfinite(zr.grad).all())
    assert torch.equal(C[col], torch.zeros(D))
    ref, gref = _run(z.double(), n)
    assert abs(float(loss) - float(ref)) <= 1e-3 * max(1.0, abs(float(ref)))
    assert _rel(zr.grad, gref) < 1e-2
    assert float(gref[:n, col].abs().max()) > 0.0
    z[n:, col] = -3.0
    l2, g2 = _run(z, n, round_operands=rounded)
    assert math.isfinite(float(l2)) and bool(torch.isfinite(g2).all())
    assert torch.equal(g2[:, col], torch.zeros(2 * n))


def c_bound(n):
    return 2.0 * n * 2.0 ** -24


def check_c(C, Cref, n):
    """max |C − Cref| <= 2 n 2^-24, but for at most one entry per 10,000, which may pass it by
    2^-8 / n (a bf16 rounding of ẑ flipped by a 1-ulp difference in the statistics)."""
    d = (C.double() - Cref.double()).abs()
    over = d > c_bound(n)
    assert int(over.sum()) <= C.numel() // 10000, (int(over.sum()), float(d.max()))
    assert float(d.max()) <= c_bound(n) + 2.0 ** -8 / n, float(d.max())
    return float(d.max())


@pytest.mark.parametrize("n,D", GPU_SHAPES)
def test_c_bound_holds_under_another_summation_order(n, D):
    """The bound tests/test_gpu_barlow.py puts on the kernels' C, met by the twin itself when the
    rows are summed in reverse order (same seeds as there)."""
    from simclr_amd.loss.barlow import barlow_twins_torch
    z = views(n, D, seed_for(n, D))
    _, C = barlow_twins_torch(z, n, LAMBD, round_operands=True, return_c=True)
    zr = z.view(2, n, D).flip(1).reshape(2 * n, D)
    _, Cr = barlow_twins_torch(zr, n, LAMBD, round_operands=True, return_c=True)
    print(n, D, check_c(Cr, C, n), c_bound(n))


def test_module_forms_and_fallback():
    from simclr_amd.loss import BarlowTwins, barlow_twins_torch
    n, D = 24, 96
    z = views(n, D, 3)
    mod = BarlowTwins()
    assert mod.lambd == LAMBD and mod.eps == 1e-5
    a = mod(z[:n], z[n:])
    assert a.dim() == 0 and torch.equal(a, mod(z))
    assert torch.equal(a, barlow_twins_torch(z, n, LAMBD))
    with pytest.raises(ValueError, match="barlow_lambda"):
        BarlowTwins(lambd=0.0)
    with pytest.raises(ValueError, match="2n"):
        mod(z[:-1])


# ------------------------------------------------------------------ config, Trainer, CLI
def _cfg(ov):
    from simclr_amd.config import compose, task_config, CONF_DIR
    return task_config(compose(str(CONF_DIR), "config", ov))


def test_configuration_keys():
    from simclr_amd.config import check_pretrain_conf
    check_pretrain_conf(_cfg([]))
    check_pretrain_conf(_cfg(["loss.kind=ntxent", "loss.gather=true", "loss.supervised=true"]))
    check_pretrain_conf(_cfg(["loss.kind=barlow"]))
    check_pretrain_conf(_cfg(["loss.kind=barlow", "loss.barlow_lambda=0.01",
                              "loss.gather=false", "loss.supervised=false"]))
    with pytest.raises(AssertionError, match=r"loss\.kind"):
        check_pretrain_conf(_cfg(["loss.kind=vicreg"]))
    for bad in ("0", "-0.5", "lots", "true"):
        with pytest.raises(AssertionError, match=r"loss\.barlow_lambda"):
            check_pretrain_conf(_cfg([f"loss.barlow_lambda={bad}"]))
    with pytest.raises(AssertionError, match=r"loss\.kind.*loss\.supervised"):
        check_pretrain_conf(_cfg(["loss.kind=barlow", "loss.supervised=true"]))
    for gather in ("true", "ring"):
        with pytest.raises(AssertionError, match=r"loss\.kind.*loss\.gather"):
            check_pretrain_conf(_cfg(["loss.kind=barlow", f"loss.gather={gather}"]))
    with pytest.raises(AssertionError, match=r"parameter\.temperature"):
        check_pretrain_conf(_cfg(["loss.kind=barlow", "parameter.temperature=0"]))


def _trainer(ov):
    from simclr_amd.parallel import state as pstate
    from simclr_amd.train.pretrain import Trainer
    cfg = _cfg(["experiment.base_cnn=resnet18", "experiment.batches=8", "data.synthetic=true",
                "runtime.precision=fp32", "parameter.epochs=10", "parameter.warmup_epochs=1",
                *ov])
    pstate.reset()
    st = pstate.get()
    st.device = torch.device("cpu")
    torch.manual_seed(0)
    return Trainer(cfg, st, 64, precision="fp32")


@pytest.mark.timeout(300)
def test_trainer_picks_the_loss_and_steps():
    from simclr_amd.data.datasets import synthetic_dataset
    from simclr_amd.data.loader import ContrastiveLoader
    from simclr_amd.loss import BarlowTwins, barlow_twins_torch
    from simclr_amd.loss.ntxent import NTXent
    assert type(_trainer([]).loss_fn) is NTXent
    assert type(_trainer(["loss.kind=ntxent"]).loss_fn) is NTXent
    tr = _trainer(["loss.kind=barlow", "loss.barlow_lambda=0.02"])
    assert type(tr.loss_fn) is BarlowTwins and tr.loss_fn.lambd == 0.02
    loader = ContrastiveLoader(synthetic_dataset(32, 3), 8, torch.device("cpu"), seed=7)
    xs = [x.clone() for x, _ in loader][:2]
    losses = [tr.step(x).clone() for x in xs]
    # the same two steps by hand on an identically initialised trainer (the first step's warm-up
    # lr is 0, the second moves the weights): the same torch ops in the same order, so the
    # default allclose tolerance is ample
    hand = _trainer(["loss.kind=barlow", "loss.barlow_lambda=0.02"])
    start = hand.store.master.clone()
    for x, loss in zip(xs, losses):
        z = hand.model(hand.prepare(x), segments=2)
        want = barlow_twins_torch(z, 8, 0.02)
        hand.store.zero_grad()
        want.backward()
        hand.store.finish()
        hand.opt.step()
        assert math.isfinite(float(loss))
        assert torch.allclose(loss, want.detach()), (float(loss), float(want))
    assert torch.allclose(tr.store.master, hand.store.master)
    assert not torch.equal(tr.store.master, start)
    x = xs[0]
    with pytest.raises(ValueError, match="labels"):
        tr.step(x, torch.zeros(8, dtype=torch.int64))


@pytest.mark.timeout(600)
def test_cli_pretrains_with_barlow(tmp_path):
    run = tmp_path / "run"
    r = subprocess.run([sys.executable, str(ROOT / "main.py"), "loss.kind=barlow",
                        "data.synthetic=true", "data.synthetic_size=32", "experiment.batches=8",
                        "experiment.base_cnn=resnet18", "parameter.epochs=1",
                        "experiment.save_model_epoch=1", "runtime.max_steps=2",
                        f"hydra.run.dir={run}"], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=500)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    line = [l for l in out.splitlines() if "Epoch:1/1 progress:1.000 loss:" in l][0]
    loss = float(line.split("loss:")[1].split(",")[0])
    assert math.isfinite(loss) and ", lr:" in line
    ck = torch.load(run / "epoch=1-cifar10.pt", weights_only=True)
    assert len(ck) == 128 and all(k.startswith("module.") for k in ck)
    rec = [json.loads(l) for l in (run / "metrics.jsonl").read_text().splitlines()]
    assert set(rec[0]) == {"epoch", "step", "loss", "lr", "images_per_sec", "seconds", "time"}
    assert rec[0]["step"] == 2
