"""Weighted negatives of NT-Xent (``loss.hard_beta`` / ``loss.tau_plus`` / ``loss.decoupled``) on
the CPU: the torch twin ``nt_xent_weighted_torch`` against a literal fp64 double loop of the
published hard-negative / debiased expression, its autograd dS against the closed form of the
contract, its reductions to NT-Xent and to −s_p + LSE_Neg, the clamp, small temperatures, the
gathered twin on 2 gloo ranks, the config checks, the Trainer's fp32 path and the CLI.

Inputs, clamp regimes and the margin to the clamp's kink: tests/_negatives_data.py."""
import math
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _negatives_data as nd

ROOT = Path(__file__).resolve().parents[1]
SMALL = nd.SHAPES[:2]  # the double loop is quadratic in python


@pytest.mark.parametrize("regime", list(nd.REGIMES))
@pytest.mark.parametrize("setting", nd.SETTINGS, ids=str)
@pytest.mark.parametrize("n,D", SMALL)
def test_twin_matches_published_double_loop(n, D, setting, regime):
    from simclr_amd.loss.ntxent import nt_xent_weighted_torch
    beta, tau_plus, dec = setting
    z, tau = nd.case(n, D, regime)
    nd.check_regime(nd.clamp_flags(z, n, tau, beta, tau_plus), regime, tau_plus)
    want = nd.hcl_rows(z, n, tau, beta, tau_plus, dec)
    got = nt_xent_weighted_torch(z, n, tau, beta, tau_plus, dec, "none")
    assert got.dtype == torch.float64 and got.shape == (2, n)
    err = float((got.reshape(-1) - want).abs().max())
    print(n, D, setting, regime, err)
    assert err < 1e-12, err  # fp64 on both sides; |loss_i| is O(10)


def _closed_form_ds(s, n, tau, beta, tau_plus, dec):
    """dS of Σ_i loss_i by the contract's formulas (g = 1), fp64, local columns."""
    R = s.shape[0]
    idx = torch.arange(R)
    pcol = torch.where(idx < n, idx + n, idx - n)
    neg = torch.ones_like(s, dtype=torch.bool)
    neg[idx, idx] = False
    neg[idx, pcol] = False
    N = R - 2
    sn = s.masked_fill(~neg, float("-inf"))
    L1 = torch.logsumexp((1 + beta) * sn, 1)
    L0 = torch.logsumexp(beta * sn, 1) if beta > 0 else math.log(N) * torch.ones(R, dtype=s.dtype)
    sp = s[idx, pcol]
    u = L1 - L0
    c = torch.maximum(u, sp)
    raw = N * (torch.exp(u - c) - tau_plus * torch.exp(sp - c)) / (1 - tau_plus)
    floor = N * torch.exp(-1 / tau - c)
    k = (raw >= floor).double()
    kappa = 0.0 if dec else 1.0
    T = kappa * torch.exp(sp - c) + torch.maximum(raw, floor)
    A = k * N / (1 - tau_plus) * torch.exp(u - c) / T
    B = -1 + (kappa - k * tau_plus * N / (1 - tau_plus)) * torch.exp(sp - c) / T
    w = (1 + beta) * torch.exp((1 + beta) * s - L1[:, None])
    if beta > 0:
        w = w - beta * torch.exp(beta * s - L0[:, None])
    ds = torch.where(neg, A[:, None] * w, torch.zeros_like(s))
    ds[idx, pcol] = B
    return ds, k.bool(), neg


@pytest.mark.parametrize("regime", list(nd.REGIMES))
@pytest.mark.parametrize("setting", nd.SETTINGS, ids=str)
@pytest.mark.parametrize("n,D", SMALL)
def test_autograd_ds_matches_closed_form(n, D, setting, regime):
    """... and a clamped row has no gradient into its negatives, exactly."""
    from simclr_amd.loss.ntxent import weighted_rows
    beta, tau_plus, dec = setting
    z, tau = nd.case(n, D, regime)
    k64 = nd.clamp_flags(z, n, tau, beta, tau_plus)
    s, _, _ = nd.sims(z, None, 0, n, tau)
    sl = s.clone().requires_grad_(True)
    weighted_rows(sl, n, 0, tau, beta, tau_plus, dec).sum().backward()
    ds, k, neg = _closed_form_ds(s, n, tau, beta, tau_plus, dec)
    assert torch.equal(k, k64)
    err = float((sl.grad - ds).abs().max())
    print(n, D, setting, regime, int(k.sum()), err)
    assert err < 1e-13, err  # |dS| <= 1 + β
    clamped = ~k
    assert bool((sl.grad[clamped][neg[clamped]] == 0).all())
    assert float(sl.grad.diagonal().abs().max()) == 0.0


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_defaults_are_ntxent_exactly(reduction):
    from simclr_amd.loss.ntxent import NTXent, nt_xent_torch, nt_xent_weighted_torch
    n, tau = 10, 0.1
    z = nd.make_z(n, 16, 3.0, 0)
    za, zb, zc = (z.clone().requires_grad_(True) for _ in range(3))
    a = nt_xent_torch(za, n, tau, reduction)
    b = nt_xent_weighted_torch(zb, n, tau, 0.0, 0.0, False, reduction)
    c = NTXent(tau, reduction, hard_beta=0.0, tau_plus=0.0, decoupled=False)(zc)
    assert torch.equal(a, b) and torch.equal(a, c)
    for t in (a, b, c):
        t.sum().backward()
    assert torch.equal(za.grad, zb.grad) and torch.equal(za.grad, zc.grad)
    assert not NTXent(tau).weighted and NTXent(tau, decoupled=True).weighted


def test_formula_at_defaults_is_ntxent():
    """β = τ⁺ = 0, κ = 1 through the weighted formula itself (not the shortcut to nt_xent_torch)."""
    from simclr_amd.loss.ntxent import nt_xent_torch, weighted_rows
    n, tau = 12, 0.1
    z = nd.make_z(n, 16, 3.0, 1)
    s, _, _ = nd.sims(z, None, 0, n, tau)
    rows = weighted_rows(s, n, 0, tau, 0.0, 0.0, False)
    want = nt_xent_torch(z, n, tau, "none").reshape(-1)
    assert float((rows - want).abs().max()) < 1e-13


def test_decoupled_alone_is_lse_over_negatives():
    from simclr_amd.loss.ntxent import nt_xent_weighted_torch
    n, tau = 12, 0.5
    z = nd.make_z(n, 16, 3.0, 2)
    s, pcol, neg = nd.sims(z, None, 0, n, tau)
    want = -s[torch.arange(2 * n), pcol] + torch.logsumexp(s.masked_fill(~neg, -math.inf), 1)
    got = nt_xent_weighted_torch(z, n, tau, 0.0, 0.0, True, "none").reshape(-1)
    assert float((got - want).abs().max()) < 1e-13


@pytest.mark.parametrize("setting", nd.SETTINGS, ids=str)
def test_small_temperature_stays_finite(setting):
    """τ = 0.01: s reaches ±100 and (1+β)s ±300; the shifted form keeps fp32 finite."""
    from simclr_amd.loss.ntxent import nt_xent_weighted_torch
    beta, tau_plus, dec = setting
    n = 24
    z = nd.make_z(n, 64, 3.0, 0).float().requires_grad_(True)
    loss = nt_xent_weighted_torch(z, n, 0.01, beta, tau_plus, dec)
    loss.backward()
    loss = loss.detach()
    assert loss.dtype == torch.float32 and bool(torch.isfinite(loss))
    assert bool(torch.isfinite(z.grad).all())
    ref = nt_xent_weighted_torch(z.detach().double(), n, 0.01, beta, tau_plus, dec)
    assert abs(float(loss) - float(ref)) < 1e-4 * max(1.0, abs(float(ref)))


def test_reductions_and_module_forms():
    from simclr_amd.loss.ntxent import NTXent, nt_xent_weighted_torch
    n, tau = 8, 0.1
    z = nd.make_z(n, 32, 3.0, 1)
    none = nt_xent_weighted_torch(z, n, tau, 1.0, 0.1, False, "none")
    assert none.shape == (2, n)
    assert torch.allclose(nt_xent_weighted_torch(z, n, tau, 1.0, 0.1, False, "sum"), none.sum(),
                          rtol=1e-14)
    assert torch.allclose(nt_xent_weighted_torch(z, n, tau, 1.0, 0.1, False, "mean"),
                          none.sum() / (2 * n), rtol=1e-14)
    mod = NTXent(tau, "sum", hard_beta=1.0, tau_plus=0.1)
    assert torch.equal(mod(z[:n], z[n:]), mod(z))
    assert torch.allclose(mod(z), none.sum(), rtol=1e-14)
    assert torch.equal(NTXent(tau, "none", hard_beta=1, tau_plus=0.1)(z), none)  # an integer β


def test_module_argument_checks():
    from simclr_amd.loss.ntxent import NTXent
    for kw, key in (({"hard_beta": -0.5}, "hard_beta"), ({"hard_beta": True}, "hard_beta"),
                    ({"hard_beta": "1"}, "hard_beta"), ({"hard_beta": math.inf}, "hard_beta"),
                    ({"tau_plus": 1.0}, "tau_plus"), ({"tau_plus": -0.1}, "tau_plus"),
                    ({"tau_plus": math.nan}, "tau_plus"), ({"tau_plus": False}, "tau_plus"),
                    ({"decoupled": 1}, "decoupled")):
        with pytest.raises(ValueError, match=key):
            NTXent(0.5, **kw)
    for kw, key in (({"hard_beta": 1.0}, "hard_beta"), ({"tau_plus": 0.1}, "tau_plus"),
                    ({"decoupled": True}, "decoupled")):
        with pytest.raises(ValueError, match=rf"{key}.*loss\.supervised"):
            NTXent(0.5, supervised=True, **kw)
        with pytest.raises(ValueError, match=rf"{key}.*loss\.gather"):
            NTXent(0.5, gather="ring", **kw)
        assert NTXent(0.5, gather=True, **kw).weighted
    # the defaults spelled out stay compatible with everything
    NTXent(0.5, gather="ring", hard_beta=0.0, tau_plus=0.0, decoupled=False)
    NTXent(0.5, supervised=True, hard_beta=0, tau_plus=0, decoupled=False)


# ------------------------------------------------------------------ 2-rank gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


GLOO = (1.0, 0.1, False, 0.1)  # β, τ⁺, decoupled, τ: clamped and unclamped rows


def _dist_data(world, n):
    z = nd.make_z(world * n, 16, 3.0, 3)
    return z[:world * n], z[world * n:]


def _worker(rank, world, port, n, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from simclr_amd.loss.ntxent import NTXent
    from simclr_amd.parallel import state as pstate
    pstate.set_state(rank=rank, world_size=world, local_rank=rank, group=dist.group.WORLD)
    torch.set_num_threads(1)
    v0, v1 = _dist_data(world, n)
    sl = slice(rank * n, (rank + 1) * n)
    z = torch.cat([v0[sl], v1[sl]]).requires_grad_(True)
    beta, tau_plus, dec, tau = GLOO
    loss = NTXent(tau, gather=True, hard_beta=beta, tau_plus=tau_plus, decoupled=dec)(z)
    loss.backward()
    torch.save({"loss": loss.detach(), "grad": z.grad}, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_gathered_twin_two_ranks(tmp_path):
    """Each rank's gathered loss is the mean over its own anchors of the one-process loss on the
    concatenated batch, and its gradient (summed over the ranks by the differentiable gather) W
    times the one-process gradient's rows."""
    from simclr_amd.loss.ntxent import nt_xent_weighted_torch
    world, n = 2, 8
    beta, tau_plus, dec, tau = GLOO
    mp.spawn(_worker, args=(world, _free_port(), n, str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(tmp_path / f"r{r}.pt", weights_only=True) for r in range(world)]
    v0, v1 = _dist_data(world, n)
    zfull = torch.cat([v0, v1])
    k = nd.clamp_flags(zfull, world * n, tau, beta, tau_plus)
    assert bool(k.any()) and not bool(k.all())
    order = torch.cat([torch.cat([torch.arange(r * n, (r + 1) * n),
                                  world * n + torch.arange(r * n, (r + 1) * n)])
                       for r in range(world)])
    zfull.requires_grad_(True)
    rows = nt_xent_weighted_torch(zfull, world * n, tau, beta, tau_plus, dec, "none").reshape(-1)
    rows.mean().backward()
    for r in range(world):
        mine = order[r * 2 * n:(r + 1) * 2 * n]
        assert torch.allclose(got[r]["loss"], rows[mine].mean().detach(), rtol=1e-12, atol=0.0)
        assert torch.allclose(got[r]["grad"], world * zfull.grad[mine], rtol=1e-9, atol=1e-14)


# ------------------------------------------------------------------ config, Trainer, CLI
def _cfg(ov):
    from simclr_amd.config import compose, task_config, CONF_DIR
    return task_config(compose(str(CONF_DIR), "config", ov))


def test_keys_are_opt_in():
    loss = _cfg([]).get("loss") or {}
    assert not {"hard_beta", "tau_plus", "decoupled"} & set(loss)


def test_configuration_keys():
    from simclr_amd.config import check_pretrain_conf
    for ok in ([], ["+loss.hard_beta=1.0"], ["+loss.hard_beta=1"], ["+loss.tau_plus=0.1"],
               ["+loss.decoupled=true"], ["+loss.hard_beta=0.5", "+loss.tau_plus=0.05",
                                         "+loss.decoupled=true", "loss.gather=true"],
               ["+loss.hard_beta=1.0", "loss.kind=ntxent"],
               # the defaults spelled out are not a weighted loss
               ["+loss.hard_beta=0", "+loss.tau_plus=0.0", "+loss.decoupled=false",
                "loss.gather=ring"],
               ["+loss.hard_beta=0.0", "loss.supervised=true"],
               ["+loss.decoupled=false", "loss.kind=barlow"]):
        check_pretrain_conf(_cfg(ok))
    for bad, key in ((["+loss.hard_beta=true"], "loss.hard_beta"),
                     (["+loss.hard_beta=strong"], "loss.hard_beta"),
                     (["+loss.hard_beta=-1"], "loss.hard_beta"),
                     (["+loss.tau_plus=false"], "loss.tau_plus"),
                     (["+loss.tau_plus=some"], "loss.tau_plus"),
                     (["+loss.tau_plus=1.0"], "loss.tau_plus"),
                     (["+loss.tau_plus=-0.1"], "loss.tau_plus"),
                     (["+loss.decoupled=1"], "loss.decoupled"),
                     (["+loss.decoupled=0.5"], "loss.decoupled"),
                     (["+loss.decoupled=yes_please"], "loss.decoupled")):
        with pytest.raises(AssertionError, match=key):
            check_pretrain_conf(_cfg(bad))
    for val in (math.inf, math.nan):  # (a value a composed file could carry)
        for key in ("hard_beta", "tau_plus"):
            cfg = _cfg([])
            cfg.setdefault("loss", {})
            cfg["loss"][key] = val
            with pytest.raises(AssertionError, match=f"loss.{key}"):
                check_pretrain_conf(cfg)
    for key in ("+loss.hard_beta=1.0", "+loss.tau_plus=0.1", "+loss.decoupled=true"):
        name = key.split("=")[0][1:].replace(".", r"\.")
        for other, oname in (("loss.kind=barlow", r"loss\.kind"), ("loss.kind=nnclr", r"loss\.kind"),
                             ("loss.supervised=true", r"loss\.supervised"),
                             ("loss.gather=ring", r"loss\.gather")):
            with pytest.raises(AssertionError, match=rf"{name}.*{oname}"):
                check_pretrain_conf(_cfg([key, other]))


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
def test_trainer_fp32_path():
    from simclr_amd.data.datasets import synthetic_dataset
    from simclr_amd.data.loader import ContrastiveLoader
    loader = ContrastiveLoader(synthetic_dataset(32, 3), 8, torch.device("cpu"), seed=7)
    batches = [x.clone() for x, _ in loader][:2]
    hard = _trainer(["+loss.hard_beta=1.0", "+loss.tau_plus=0.1", "+loss.decoupled=true"])
    plain = _trainer([])
    fn = hard.loss_fn
    assert fn.weighted and (fn.hard_beta, fn.tau_plus, fn.decoupled) == (1.0, 0.1, True)
    assert not plain.loss_fn.weighted
    lh = [float(hard.step(x)) for x in batches]
    lp = [float(plain.step(x)) for x in batches]
    assert all(math.isfinite(v) for v in lh + lp)
    assert abs(lh[0] - lp[0]) > 1e-3, (lh, lp)
    with pytest.raises(ValueError, match=r"loss\.hard_beta.*loss\.kind"):
        _trainer(["+loss.hard_beta=1.0", "loss.kind=barlow"])


@pytest.mark.timeout(600)
def test_cli_pretrains_with_the_keys(tmp_path):
    run = tmp_path / "run"
    r = subprocess.run([sys.executable, str(ROOT / "main.py"), "data.synthetic=true",
                        "data.synthetic_size=32", "experiment.batches=8",
                        "experiment.base_cnn=resnet18", "parameter.epochs=1",
                        "+loss.hard_beta=1.0", "+loss.tau_plus=0.1", "+loss.decoupled=true",
                        f"hydra.run.dir={run}"], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=500)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    line = [l for l in out.splitlines() if "Epoch:1/1" in l][0]
    loss = float(line.split("loss:")[1].split(",")[0])
    assert math.isfinite(loss) and abs(loss) < 100
    r = subprocess.run([sys.executable, str(ROOT / "main.py"), "data.synthetic=true",
                        "data.synthetic_size=32", "experiment.batches=8",
                        "experiment.base_cnn=resnet18", "parameter.epochs=1",
                        "+loss.hard_beta=1.0", "loss.supervised=true",
                        f"hydra.run.dir={tmp_path / 'bad'}"], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=500)
    assert r.returncode != 0 and "loss.hard_beta" in r.stdout + r.stderr
