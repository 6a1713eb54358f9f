"""Barlow Twins over all ranks (``loss.barlow_global``) on the CPU: the torch twin on 2 and 4
gloo ranks holding slices of one batch against ``barlow_twins_torch`` of the concatenated batch
in one process (fp64: loss and the parameter gradient of a small linear map), the 1-rank identity
with and without rounding, the two constant-column cases, the rank-order merge of the
statistics, the config checks, the Trainer, and ``main.py`` on 2 gloo ranks.

Tolerances are those of tests/test_barlow.py: 1e-5 on the loss (relative to max(1, |ref|)) and on
the relative L2 of the gradient for the twin against the oracle (both are fp64 here, so the
measured differences are near 1e-15); ``c_bound`` for a sum under another summation order."""
import importlib.util
import json
import math
import os
import socket
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = Path(__file__).resolve().parents[1]
LAMBD = 0.0051
N_ALL, D = 64, 64  # W · n and the embedding width of the multi-rank cases


def _cpu():
    """tests/test_barlow.py's data and bounds (loaded by path: tests/ is no package)."""
    spec = importlib.util.spec_from_file_location("_barlow_cpu_tests",
                                                  ROOT / "tests" / "test_barlow.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def _batch():
    """x = [x0; x1] fp64 [2 N][D] and the linear map P [D][D]: z = x P."""
    x = _cpu().views(N_ALL, D, 4242).double()
    g = torch.Generator().manual_seed(17)
    P = torch.eye(D, dtype=torch.float64) + 0.1 * torch.randn(D, D, generator=g,
                                                             dtype=torch.float64)
    return x, P


def _slice(x, rank, n):
    """Rank ``rank``'s n rows of each view of x = [view0; view1]."""
    N = x.shape[0] // 2
    return torch.cat([x[rank * n:(rank + 1) * n], x[N + rank * n:N + (rank + 1) * n]])


def _const_cases(x):
    """Contract item 2.  Column 7: constant over the global batch in view 0.  Column 20:
    constant within each rank (the value r + 0.5 on rank r) in view 0, so every M2_r is 0 and the
    variance comes from the means alone."""
    N = x.shape[0] // 2
    x = x.clone()
    x[:N, 7] = 1.25
    return x, 7, 20


def _init(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)


def _worker(rank, world, port, out_dir):
    _init(rank, world, port)
    from simclr_amd.loss.barlow import BarlowTwins, barlow_twins_torch
    from simclr_amd.parallel import state as pstate
    kw = dict(group=dist.group.WORLD, world_size=world, rank=rank)
    n = N_ALL // world
    x, P = _batch()
    res = {}
    # fp64 oracle: loss and the gradient of P
    Pr = P.clone().requires_grad_(True)
    loss, C = barlow_twins_torch(_slice(x, rank, n) @ Pr, n, LAMBD, return_c=True, **kw)
    loss.backward()
    res.update(loss=loss.detach(), gradP=Pr.grad, C=C.detach())
    # the module takes the same path from pstate
    pstate.set_state(rank=rank, world_size=world, local_rank=rank, group=dist.group.WORLD)
    z = (_slice(x, rank, n) @ P)
    res["module_loss"] = BarlowTwins(LAMBD, global_batch=True)(z).detach()
    res["module_local"] = BarlowTwins(LAMBD)(z).detach()
    pstate.reset()
    # rounded twin, fp32: the mean of dz over a linear map, as above
    Pf = P.float().requires_grad_(True)
    lr_ = barlow_twins_torch(_slice(x, rank, n).float() @ Pf, n, LAMBD, round_operands=True, **kw)
    lr_.backward()
    res.update(rloss=lr_.detach(), rgradP=Pf.grad)
    # constant columns, unrounded and rounded
    xc, c_all, c_rank = _const_cases(x)
    for rounded in (False, True):
        zc = _slice(xc, rank, n).float()
        zc[:n, c_rank] = rank + 0.5
        zc.requires_grad_(True)
        lc, Cc = barlow_twins_torch(zc, n, LAMBD, round_operands=rounded, return_c=True, **kw)
        lc.backward()
        res[f"const{int(rounded)}"] = (lc.detach(), Cc.detach(), zc.grad)
    torch.save(res, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def oracle():
    """The one-process loss of the whole batch, fp64 and rounded fp32, once."""
    from simclr_amd.loss.barlow import barlow_twins_torch
    x, P = _batch()
    Pr = P.clone().requires_grad_(True)
    loss, C = barlow_twins_torch(x @ Pr, N_ALL, LAMBD, return_c=True)
    loss.backward()
    Pf = P.float().requires_grad_(True)
    rl = barlow_twins_torch(x.float() @ Pf, N_ALL, LAMBD, round_operands=True)
    rl.backward()
    return dict(loss=loss.detach(), gradP=Pr.grad, C=C.detach(), rloss=rl.detach(),
                rgradP=Pf.grad)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 4])
def test_twin_over_ranks_matches_single_process_oracle(tmp_path, oracle, world):
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(tmp_path / f"r{r}.pt", weights_only=True) for r in range(world)]
    ref = float(oracle["loss"])
    for r, g in enumerate(got):
        print(world, r, float(g["loss"]), ref, abs(float(g["loss"]) - ref))
        assert abs(float(g["loss"]) - ref) <= 1e-5 * max(1.0, abs(ref))
        assert torch.equal(g["loss"], got[0]["loss"])  # the same number on every rank
        assert torch.equal(g["module_loss"], g["loss"])
        assert not torch.equal(g["module_local"], g["loss"])  # (the per-rank loss differs)
        assert float((g["C"] - oracle["C"]).abs().max()) < 1e-12
    # the data-parallel mean of the ranks' parameter gradients is the global loss's gradient
    mean = sum(g["gradP"] for g in got) / world
    print(world, "gradP", _rel(mean, oracle["gradP"]))
    assert _rel(mean, oracle["gradP"]) < 1e-5
    # the rounded twin: the bf16-operand bounds of tests/test_barlow.py against the fp64 oracle
    rmean = sum(g["rgradP"] for g in got) / world
    print(world, "rounded", float(got[0]["rloss"]), _rel(rmean, oracle["gradP"]),
          _rel(rmean, oracle["rgradP"]))
    assert abs(float(got[0]["rloss"]) - ref) <= 1e-3 * max(1.0, abs(ref))
    assert all(torch.equal(g["rloss"], got[0]["rloss"]) for g in got)
    assert _rel(rmean, oracle["gradP"]) < 1e-2
    # constant columns
    n = N_ALL // world
    for rounded in (0, 1):
        for r, g in enumerate(got):
            loss, C, grad = g[f"const{rounded}"]
            assert math.isfinite(float(loss)) and bool(torch.isfinite(grad).all())
            # constant over the global batch: ẑ = 0 exactly, so C's row is 0
            assert torch.equal(C[7], torch.zeros(D))
            # constant within each rank, different between them: a live column (σ² > 0 from the
            # mean term), with a finite, non-zero gradient
            assert float(C[20].abs().max()) > 1e-3
            assert float(grad[:n, 20].abs().max()) > 0.0


def _worker_one(rank, world, port, out_dir):
    """A 1-rank group: the global path with W = 1 against today's per-rank path."""
    _init(rank, world, port)
    from simclr_amd.loss.barlow import barlow_twins_torch
    cpu = _cpu()
    res = {}
    for n, Dd in ((32, 64), (96, 128)):
        z32 = cpu.views(n, Dd, cpu.seed_for(n, Dd))
        for name, z, rounded in (("plain32", z32, False), ("plain64", z32.double(), False),
                                 ("round32", z32, True),
                                 ("roundbf", z32.to(torch.bfloat16), True)):
            out = []
            for kw in ({}, dict(group=dist.group.WORLD, world_size=1, rank=0)):
                zr = z.clone().requires_grad_(True)
                loss, C = barlow_twins_torch(zr, n, LAMBD, round_operands=rounded,
                                             return_c=True, **kw)
                loss.backward()
                out.append((loss.detach(), C.detach(), zr.grad))
            res[f"{name}-{n}-{Dd}"] = out
    torch.save(res, os.path.join(out_dir, "one.pt"))
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_one_rank_group_is_the_per_rank_loss_bitwise(tmp_path):
    mp.spawn(_worker_one, args=(1, _free_port(), str(tmp_path)), nprocs=1, join=True)
    res = torch.load(tmp_path / "one.pt", weights_only=True)
    assert len(res) == 8
    for name, (local, glob) in res.items():
        for a, b, what in zip(local, glob, ("loss", "C", "dz")):
            assert a.dtype == b.dtype and torch.equal(a, b), (name, what)


@pytest.mark.parametrize("world", [2, 4, 8, 3])
def test_rank_order_merge_of_the_statistics(world):
    """The merged σ² against a two-pass variance over all N rows in fp32, within the bound
    tests/test_barlow.py puts on a sum of N terms under another summation order (unit-variance
    columns: Σ (z − μ)² is about N); the merged μ likewise."""
    from simclr_amd.loss.barlow import _local_stats, _merge_moments, _merge_stats
    cpu = _cpu()
    n = 32
    N = world * n
    z = cpu.views(N, D, 99) + 3.0  # (a mean well away from 0)
    gst = torch.stack([_local_stats(_slice(z, r, n), n) for r in range(world)])
    assert gst.shape == (world, 2, 2, D) and gst.dtype == torch.float32
    mu, var = _merge_moments(gst, n)
    zv = z.view(2, N, D)
    mu2 = zv.double().mean(dim=1)
    ref32 = ((zv - zv.mean(dim=1, keepdim=True)) ** 2).mean(dim=1)  # two passes, fp32
    ref64 = ((zv.double() - mu2.unsqueeze(1)) ** 2).mean(dim=1)
    print(world, float((var - ref32).abs().max()), float((var.double() - ref64).abs().max()),
          cpu.c_bound(N) / N)
    assert 0.5 < float(ref64.min()) and float(ref64.max()) < 2.0
    assert float((var - ref32).abs().max()) <= cpu.c_bound(N)
    assert float((var.double() - ref64).abs().max()) <= cpu.c_bound(N)
    assert float((mu.double() - mu2).abs().max()) <= cpu.c_bound(N)
    # rstd is the correctly rounded 1 / sqrt of the merged variance
    _, rstd = _merge_stats(gst, n, 1e-5)
    want = 1.0 / torch.sqrt((var + 1e-5).double())
    assert float((rstd.squeeze(1).double() / want - 1.0).abs().max()) < 2.0 ** -22


# ------------------------------------------------------------------ config, Trainer, CLI
def _cfg(ov):
    from simclr_amd.config import compose, task_config, CONF_DIR
    return task_config(compose(str(CONF_DIR), "config", ov))


def test_configuration_key():
    from simclr_amd.config import check_pretrain_conf
    check_pretrain_conf(_cfg(["loss.kind=barlow", "loss.barlow_global=true"]))
    check_pretrain_conf(_cfg(["loss.kind=barlow", "loss.barlow_global=false"]))
    check_pretrain_conf(_cfg(["loss.kind=ntxent", "loss.barlow_global=false"]))
    with pytest.raises(AssertionError, match=r"loss\.barlow_global"):
        check_pretrain_conf(_cfg(["loss.kind=ntxent", "loss.barlow_global=true"]))
    with pytest.raises(AssertionError, match=r"loss\.barlow_global"):
        check_pretrain_conf(_cfg(["loss.barlow_global=true"]))  # (the default kind)
    for bad in ("1", "yes_please", "0.5"):
        with pytest.raises(AssertionError, match=r"loss\.barlow_global"):
            check_pretrain_conf(_cfg(["loss.kind=barlow", f"loss.barlow_global={bad}"]))
    for gather in ("true", "ring"):  # still rejected, with or without the new key
        with pytest.raises(AssertionError, match=r"loss\.kind.*loss\.gather"):
            check_pretrain_conf(_cfg(["loss.kind=barlow", "loss.barlow_global=true",
                                      f"loss.gather={gather}"]))


@pytest.mark.timeout(300)
def test_trainer_passes_the_key_through():
    from simclr_amd.loss import BarlowTwins
    from simclr_amd.parallel import state as pstate
    from simclr_amd.train.pretrain import Trainer

    def trainer(ov):
        cfg = _cfg(["experiment.base_cnn=resnet18", "experiment.batches=8", "data.synthetic=true",
                    "runtime.precision=fp32", "parameter.epochs=10", "parameter.warmup_epochs=1",
                    "loss.kind=barlow", *ov])
        pstate.reset()
        st = pstate.get()
        st.device = torch.device("cpu")
        torch.manual_seed(0)
        return Trainer(cfg, st, 64, precision="fp32")

    tr = trainer(["loss.barlow_global=true", "loss.barlow_lambda=0.02"])
    assert type(tr.loss_fn) is BarlowTwins
    assert tr.loss_fn.global_batch is True and tr.loss_fn.lambd == 0.02
    assert trainer([]).loss_fn.global_batch is False
    assert trainer(["loss.barlow_global=false"]).loss_fn.global_batch is False
    assert BarlowTwins().global_batch is False
    # without a communicating group the key changes nothing: the per-rank loss, bit for bit
    z = _cpu().views(24, 96, 3)
    assert torch.equal(BarlowTwins(global_batch=True)(z), BarlowTwins()(z))


def _worker_cli(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    os.chdir(out_dir)
    sys.path.insert(0, str(ROOT))
    import main as entry
    import simclr_amd.train.pretrain as P
    from simclr_amd.runtime.dist import cleanup
    losses, kinds = [], []
    orig_step = P.Trainer.step

    def step(self, x):
        loss = orig_step(self, x)
        losses.append(float(loss))
        kinds.append(bool(self.loss_fn.global_batch))
        return loss

    P.Trainer.step = step
    try:
        entry.main(["loss.kind=barlow", "loss.barlow_global=true", "data.synthetic=true",
                    "data.synthetic_size=64", "experiment.batches=8",
                    "experiment.base_cnn=resnet18", "parameter.epochs=1",
                    "experiment.save_model_epoch=1", "parameter.use_cuda=false",
                    "runtime.save_resume=false", f"hydra.run.dir={out_dir}/run{rank}"])
    finally:
        cleanup()
    with open(os.path.join(out_dir, f"losses{rank}.json"), "w") as f:
        json.dump({"losses": losses, "global": kinds}, f)


@pytest.mark.timeout(600)
def test_main_on_two_gloo_ranks_logs_one_global_loss(tmp_path):
    """``main.py loss.kind=barlow loss.barlow_global=true`` on 2 gloo ranks, synthetic data, one
    epoch: every step's loss is the same number on both ranks (each rank sees other images, so
    the per-rank losses would differ), and rank 0's ``metrics.jsonl`` holds the last one."""
    mp.spawn(_worker_cli, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    a, b = (json.loads((tmp_path / f"losses{r}.json").read_text()) for r in range(2))
    assert len(a["losses"]) == 4 and all(a["global"]) and all(b["global"])
    assert all(math.isfinite(v) for v in a["losses"])
    assert a["losses"] == b["losses"], (a["losses"], b["losses"])
    rec = [json.loads(l) for l in (tmp_path / "run0" / "metrics.jsonl").read_text().splitlines()]
    assert set(rec[0]) == {"epoch", "step", "loss", "lr", "images_per_sec", "seconds", "time"}
    assert rec[0]["step"] == 4 and rec[0]["loss"] == a["losses"][-1]
    assert not (tmp_path / "run1" / "metrics.jsonl").exists()
