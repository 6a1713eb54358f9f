"""SupCon (``loss.supervised``) on the CPU: the torch twin ``sup_con_torch`` against a literal
fp64 double loop, its reductions to NT-Xent / to the one-class closed form, the gathered twin on
2 gloo ranks, the config checks and the Trainer's fp32 path."""
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F


def _brute(z, labels, tau):
    """loss_i = LSE_{a != i} s_ia - mean_{p != i, y_p = y_i} s_ip, one anchor and one column at
    a time; returns the per-row losses as a differentiable fp64 tensor."""
    n = len(labels)
    R = 2 * n
    zn = [z[i] / z[i].norm().clamp_min(1e-12) for i in range(R)]
    rows = []
    for i in range(R):
        logits, pos = [], []
        for c in range(R):
            if c == i:
                continue
            s = (zn[i] * zn[c]).sum() / tau
            logits.append(s)
            if labels[c % n] == labels[i % n]:
                pos.append(s)
        m = max(float(v.detach()) for v in logits)
        lse = m + torch.log(sum(torch.exp(v - m) for v in logits))
        rows.append(lse - sum(pos) / len(pos))
    return torch.stack(rows)


def test_twin_matches_brute_force():
    from simclr_amd.loss.ntxent import sup_con_torch
    n, d, tau = 6, 8, 0.5
    labels = [0, 0, 1, 2, 2, 2]  # a class seen twice, once and three times
    torch.manual_seed(3)
    z = torch.randn(2 * n, d, dtype=torch.float64)
    y = torch.tensor(labels)
    za = z.clone().requires_grad_(True)
    zb = z.clone().requires_grad_(True)
    rows = _brute(zb, labels, tau)
    got = sup_con_torch(za, n, y, tau, "mean")
    want = rows.sum() / (2 * n)
    assert torch.allclose(got, want, rtol=1e-12, atol=0.0), (float(got), float(want))
    assert torch.allclose(sup_con_torch(za, n, y, tau, "none").reshape(-1), rows, rtol=1e-12,
                          atol=0.0)
    got.backward()
    want.backward()
    assert torch.allclose(za.grad, zb.grad, rtol=1e-9, atol=1e-14), \
        float((za.grad - zb.grad).abs().max())


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_distinct_labels_equal_ntxent_exactly(reduction):
    from simclr_amd.loss.ntxent import nt_xent_torch, sup_con_torch
    n, d, tau = 10, 16, 0.1
    torch.manual_seed(0)
    z = torch.randn(2 * n, d, dtype=torch.float64)
    y = torch.randperm(n) * 5 - 7
    za = z.clone().requires_grad_(True)
    zb = z.clone().requires_grad_(True)
    a = nt_xent_torch(za, n, tau, reduction)
    b = sup_con_torch(zb, n, y, tau, reduction)
    assert torch.equal(a, b)
    a.sum().backward()
    b.sum().backward()
    assert torch.equal(za.grad, zb.grad)


def test_one_class_for_all():
    from simclr_amd.loss.ntxent import sup_con_torch
    n, d, tau = 7, 8, 0.5
    torch.manual_seed(1)
    z = torch.randn(2 * n, d, dtype=torch.float64)
    R = 2 * n
    zn = F.normalize(z, dim=1)
    s = zn @ zn.t() / tau
    off = ~torch.eye(R, dtype=torch.bool)
    want = torch.stack([torch.logsumexp(s[i][off[i]], 0) - s[i][off[i]].mean()
                        for i in range(R)]).mean()
    got = sup_con_torch(z, n, torch.full((n,), 3), tau)
    assert torch.allclose(got, want, rtol=1e-12, atol=0.0)


def test_reductions_are_consistent():
    from simclr_amd.loss.ntxent import NTXent, sup_con_torch
    n, d, tau = 6, 8, 0.5
    torch.manual_seed(2)
    z = torch.randn(2 * n, d, dtype=torch.float64)
    y = torch.tensor([0, 0, 1, 2, 2, 2])
    none = sup_con_torch(z, n, y, tau, "none")
    assert none.shape == (2, n)
    assert torch.allclose(sup_con_torch(z, n, y, tau, "sum"), none.sum(), rtol=1e-14)
    assert torch.allclose(sup_con_torch(z, n, y, tau, "mean"), none.sum() / (2 * n), rtol=1e-14)
    # the module: (view0, view1) and z forms, int32 labels
    mod = NTXent(tau, "sum", supervised=True)
    assert torch.equal(mod(z[:n], z[n:], labels=y.to(torch.int32)), mod(z, labels=y))
    assert torch.allclose(mod(z, labels=y), none.sum(), rtol=1e-14)


def test_label_checks():
    from simclr_amd.loss.ntxent import NTXent, SupCon, sup_con_torch
    z = torch.randn(8, 4)
    with pytest.raises(ValueError, match="labels"):
        sup_con_torch(z, 4, torch.zeros(5, dtype=torch.int64), 0.5)
    with pytest.raises(TypeError, match="labels"):
        sup_con_torch(z, 4, torch.zeros(4), 0.5)
    with pytest.raises(ValueError, match="labels"):
        NTXent(0.5, supervised=True)(z)
    with pytest.raises(ValueError, match="supervised"):
        NTXent(0.5)(z, labels=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"loss\.supervised.*loss\.gather"):
        SupCon(0.5, gather="ring")


# ------------------------------------------------------------------ 2-rank gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dist_data(world, n, d=8):
    g = torch.Generator().manual_seed(5)
    v0 = torch.randn(world * n, d, generator=g, dtype=torch.float64)
    v1 = torch.randn(world * n, d, generator=g, dtype=torch.float64)
    y = torch.tensor([0, 1, 1, 2, 0, 0, 1, 3][:world * n])  # labels repeat across the ranks
    return v0, v1, y


def _worker(rank, world, port, n, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from simclr_amd.loss.ntxent import NTXent
    from simclr_amd.parallel import state as pstate
    pstate.set_state(rank=rank, world_size=world, local_rank=rank, group=dist.group.WORLD)
    torch.set_num_threads(1)
    v0, v1, y = _dist_data(world, n)
    sl = slice(rank * n, (rank + 1) * n)
    z = torch.cat([v0[sl], v1[sl]]).requires_grad_(True)
    loss = NTXent(0.5, gather=True, supervised=True)(z, labels=y[sl])
    loss.backward()
    ring = ""
    try:
        NTXent(0.5, gather="ring", supervised=True)
    except ValueError as e:
        ring = str(e)
    torch.save({"loss": loss.detach(), "grad": z.grad, "ring": ring},
               os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_gathered_twin_two_ranks(tmp_path):
    """Each rank's gathered loss is the mean over its own anchors; the mean over the ranks is the
    single-process loss on the concatenated batch, and the ranks' local gradients (which the
    differentiable gather sums over the ranks) are W times the single-process gradient's rows."""
    from simclr_amd.loss.ntxent import sup_con_torch
    world, n = 2, 4
    mp.spawn(_worker, args=(world, _free_port(), n, str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(tmp_path / f"r{r}.pt", weights_only=True) for r in range(world)]
    v0, v1, y = _dist_data(world, n)
    # single process, columns in the gathered (rank-major, view-expanded) order
    order = torch.cat([torch.cat([torch.arange(r * n, (r + 1) * n),
                                  world * n + torch.arange(r * n, (r + 1) * n)])
                       for r in range(world)])
    zfull = torch.cat([v0, v1]).requires_grad_(True)
    rows = sup_con_torch(zfull, world * n, y, 0.5, "none").reshape(-1)
    full = rows.mean()
    full.backward()
    for r in range(world):
        mine = order[r * 2 * n:(r + 1) * 2 * n]
        assert torch.allclose(got[r]["loss"], rows[mine].mean().detach(), rtol=1e-12, atol=0.0)
        assert torch.allclose(got[r]["grad"], world * zfull.grad[mine], rtol=1e-9, atol=1e-14)
        assert "loss.supervised" in got[r]["ring"] and "loss.gather" in got[r]["ring"]
    mean = sum(g["loss"] for g in got) / world
    assert torch.allclose(mean, full.detach(), rtol=1e-12, atol=0.0)


# ------------------------------------------------------------------ config, Trainer
def _cfg(ov):
    from simclr_amd.config import compose, task_config, CONF_DIR
    return task_config(compose(str(CONF_DIR), "config", ov))


def test_configuration_key():
    from simclr_amd.config import check_pretrain_conf
    check_pretrain_conf(_cfg([]))
    check_pretrain_conf(_cfg(["loss.supervised=true"]))
    check_pretrain_conf(_cfg(["loss.supervised=true", "loss.gather=true"]))
    check_pretrain_conf(_cfg(["loss.supervised=false", "loss.gather=ring"]))
    for bad in ("1", "yes_please", "0.5"):
        with pytest.raises(AssertionError, match="loss.supervised"):
            check_pretrain_conf(_cfg([f"loss.supervised={bad}"]))
    with pytest.raises(AssertionError, match="loss.supervised"):
        check_pretrain_conf(_cfg(["loss.supervised=true", "loss.gather=ring"]))


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
    ds = synthetic_dataset(32, 3)
    loader = ContrastiveLoader(ds, 8, torch.device("cpu"), seed=7)
    loader.label_i32 = True
    batches = [(x.clone(), y.clone()) for x, y in loader][:2]
    assert batches[0][1].dtype == torch.int32 and batches[0][1].shape == (8,)
    sup = _trainer(["loss.supervised=true"])
    plain = _trainer([])
    ls = [float(sup.step(x, y)) for x, y in batches]
    lp = [float(plain.step(x)) for x, _ in batches]
    assert all(math.isfinite(v) for v in ls + lp)
    assert abs(ls[0] - lp[0]) > 1e-3, (ls, lp)  # 8 images of 3 classes: labels repeat
    with pytest.raises(ValueError, match="labels"):
        sup.step(batches[0][0])
    with pytest.raises(ValueError, match="loss.supervised"):
        plain.step(*batches[0])
