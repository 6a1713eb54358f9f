"""Online linear probe (``online_probe.enabled``) on the CPU: the torch twin of
``ops/online_probe.py`` against fp64 ``nn.Linear`` + ``F.cross_entropy`` + ``torch.optim.SGD``,
its progressive metrics, its schedule, the config checks, the Trainer's fp32 path (isolation,
label bookkeeping), 2 gloo ranks and resume."""
import json
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
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
U = 2.0 ** -24


def _op():
    from simclr_amd.ops import online_probe
    return online_probe


def _data(n, Fdim, C, steps, seed):
    g = torch.Generator().manual_seed(seed)
    centers = torch.randn(C, Fdim, generator=g)
    out = []
    for _ in range(steps):
        y = torch.randint(0, C, (n,), generator=g)
        h = torch.cat([centers[y] + torch.randn(n, Fdim, generator=g) for _ in range(2)])
        out.append((h, y.to(torch.int32)))
    return out


def _torch_run(lin, batches, lr0, decay, warmup, total, dtype):
    """The literal reference: autograd through nn.Linear + mean CE, SGD(nesterov=True), the LR of
    ``lr_at`` set per step."""
    from simclr_amd.optim.schedule import MODE_WARMUP_COSINE, lr_at
    m = torch.nn.Linear(lin.in_features, lin.out_features).to(dtype)
    m.load_state_dict({k: v.to(dtype) for k, v in lin.state_dict().items()})
    opt = torch.optim.SGD(m.parameters(), lr=lr0, momentum=0.9, nesterov=True, weight_decay=decay)
    losses = []
    for s, (h, y) in enumerate(batches):
        for g in opt.param_groups:
            g["lr"] = lr_at(MODE_WARMUP_COSINE, s, lr0, warmup, total)
        opt.zero_grad()
        loss = F.cross_entropy(m(h.to(dtype)), y.long().repeat(2))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return m, losses


def test_twin_matches_autograd_sgd():
    """4 steps, operand rounding off.  The twin and the fp32 autograd run are both fp32 with
    different summation orders (sums over F = 48 features and 2n = 48 rows), so the bound of every
    quantity is 4x the gap the autograd run itself shows between fp32 and fp64 execution,
    measured here on every run.  Measured: fp32/fp64 gap weights 8.5e-8, bias 1.1e-8, loss
    6.0e-8; the twin's distance to the fp64 run: 1.4e-7, 1.1e-8, 6.0e-8."""
    op = _op()
    Fd, C, n = 48, 10, 24
    torch.manual_seed(3)
    lin = torch.nn.Linear(Fd, C)
    batches = _data(n, Fd, C, 4, 0)
    lr0, decay, warmup, total = 0.4, 1e-3, 2, 8
    m32, l32 = _torch_run(lin, batches, lr0, decay, warmup, total, torch.float32)
    m64, l64 = _torch_run(lin, batches, lr0, decay, warmup, total, torch.float64)
    pr = op.OnlineProbe(lin.weight, lin.bias, lr0, decay, 0.9, 5, warmup, total,
                        round_operands=False)
    assert not pr.hip
    pr.reset_metrics()
    lt = [float(pr.step(h, y)["loss"].double().mean()) for h, y in batches]
    W, b = pr.weights()
    for name, a32, a64, tw in (("weights", m32.weight, m64.weight, W), ("bias", m32.bias, m64.bias, b),
                               ("loss", torch.tensor(l32), torch.tensor(l64), torch.tensor(lt))):
        gap = float((a32.detach().double() - a64.detach().double()).abs().max())
        d = float((tw.detach().double() - a64.detach().double()).abs().max())
        print(f"{name}: autograd fp32/fp64 gap {gap:.3e}, twin vs fp64 {d:.3e}")
        assert gap > 0 and d <= 4 * gap, (name, d, gap)
    assert float((W - lin.weight.detach()).abs().max()) > 1e-3  # it did train
    assert pr.host_step == 4 and int(pr.step_t) == 4
    # progressive mean loss = mean of the per-step losses (each on the weights before its update)
    assert abs(pr.metrics()["loss"] - sum(lt) / 4) <= 1e-6
    assert pr.metrics()["rows"] == 4 * 2 * n


def test_metrics_against_direct_count():
    """W = I, b = 0, no rounding: h holds the logits.  Rows with a NaN target logit (never
    correct: 0 · NaN makes the whole row of logits NaN) and exact ties below and above the target
    (ties go to the lower class)."""
    op = _op()
    C = 6
    nan = float("nan")
    y = torch.tensor([2, 0, 3, 1], dtype=torch.int32)
    h = torch.tensor([
        [0.0, 1.0, 3.0, 2.0, -1.0, 0.5],   # y 2: top-1
        [1.0, 1.0, 0.0, 0.0, 0.0, 0.0],    # y 0: tie with class 1, the lower class wins: rank 0
        [5.0, 4.0, 3.5, 3.5, 3.5, 0.0],    # y 3: two above, tie with 2 (lower, above) and 4: rank 3
        [2.0, nan, 1.0, 0.0, 0.0, 0.0],    # y 1: NaN target logit: never correct
        [9.0, 8.0, 7.0, 0.0, 0.0, 0.0],    # y 2: rank 2
        [nan, 0.0, 0.0, 0.0, 0.0, 0.0],    # y 0: NaN target
        [0.0, 0.0, 0.5, 1.0, 2.0, 0.0],    # y 3: one class above: rank 1
        [0.0, 1.0, 1.0, 0.0, 0.0, 0.0],    # y 1: tie with class 2 (higher): rank 0
    ])
    want_rank = [0, 0, 3, C, 2, C, 1, 0]
    for k in (1, 2, 3):
        pr = op.OnlineProbe(torch.eye(C), torch.zeros(C), 0.1, top_k=k, round_operands=False)
        out = pr.step(h, y)
        assert out["rank"].tolist() == want_rank
        m = pr.metrics()
        assert m["rows"] == 8 and m["acc"] == sum(r == 0 for r in want_rank) / 8
        assert m["top_k_acc"] == sum(r < k for r in want_rank) / 8
        assert math.isnan(m["loss"])  # a NaN target logit poisons the mean loss, as it should
    # the loss sum on the finite rows, and progressive accumulation over two steps
    yk = torch.tensor([2, 0], dtype=torch.int32)
    hk = torch.stack([h[0], h[1], h[4], torch.tensor([3.0, 1.0, 0.0, 0.0, 0.0, 0.0])])
    pr = op.OnlineProbe(torch.eye(C), torch.zeros(C), 0.1, top_k=2, round_operands=False)
    want = F.cross_entropy(hk.double(), yk.long().repeat(2), reduction="sum")
    pr.step(hk, yk)
    assert abs(pr.metrics()["loss"] * 4 - float(want)) <= 4 * (C + 16) * 2 * U * (1 + float(want))
    W1, b1 = (t.clone() for t in pr.weights())
    pr.step(hk, yk)
    z = hk.double() @ W1.double().t() + b1.double()
    want2 = want + F.cross_entropy(z, yk.long().repeat(2), reduction="sum")
    m = pr.metrics()
    assert m["rows"] == 8 and abs(m["loss"] * 8 - float(want2)) <= 1e-5
    pr.reset_metrics()
    assert pr.metrics()["rows"] == 0 and pr.metrics()["loss"] == 0.0


def test_lr_per_step_follows_the_pretraining_schedule():
    from simclr_amd.optim.schedule import MODE_WARMUP_COSINE, lr_at
    op = _op()
    warmup, total, lr0 = 3, 9, op.initial_lr(0.1, 512, True)
    assert lr0 == 0.1 * 512 / 256 and op.initial_lr(0.1, 64, False) == 0.1 * 8
    (h, y), = _data(8, 16, 4, 1, 1)
    pr = op.OnlineProbe(torch.zeros(4, 16), torch.zeros(4), lr0, warmup_steps=warmup,
                        total_steps=total)
    for s in range(total):
        pr.step(h, y)
        want = torch.tensor(lr_at(MODE_WARMUP_COSINE, s, lr0, warmup, total), dtype=torch.float32)
        assert torch.equal(pr.lr_t, want.view(1)), (s, float(pr.lr_t), float(want))
        assert int(pr.step_t) == s + 1 == pr.host_step


def test_padding_never_moves_and_limits():
    op = _op()
    (h, y), = _data(8, 40, 10, 1, 2)
    torch.manual_seed(0)
    lin = torch.nn.Linear(40, 10)
    pr = op.OnlineProbe(lin.weight, lin.bias, 0.5, decay=1e-2)
    assert (pr.Cp, pr.Fp) == (16, 64) and pr.master.numel() == 16 * 64 + 16
    for _ in range(3):
        pr.step(h, y)
    assert not pr.W[10:].any() and not pr.W[:, 40:].any() and not pr.b[10:].any()
    assert not pr.mom[:16 * 64].view(16, 64)[10:].any()
    assert torch.equal(pr.Wsh, pr.W.to(torch.bfloat16))
    assert not op.hip_shape_ok(1025, 64) and not op.hip_shape_ok(10, 4097)
    assert op.hip_shape_ok(1024, 4096)
    with pytest.raises(ValueError, match="labels"):
        pr.step(h, y[:3])
    with pytest.raises(TypeError, match="labels"):
        pr.step(h, y.float())


# ------------------------------------------------------------------ config, Trainer
def _cfg(ov):
    from simclr_amd.config import compose, task_config, CONF_DIR
    return task_config(compose(str(CONF_DIR), "config", ov))


def test_configuration_keys():
    from simclr_amd.config import check_pretrain_conf
    cfg = _cfg([])
    assert dict(cfg["online_probe"]) == {"enabled": False, "lr": 0.1, "decay": 0.0,
                                         "momentum": 0.9, "top_k": 5}
    check_pretrain_conf(cfg)
    check_pretrain_conf(_cfg(["online_probe.enabled=true", "online_probe.lr=0.3",
                              "online_probe.decay=1e-4", "online_probe.top_k=3"]))
    for ov, key in (("online_probe.enabled=1", "online_probe.enabled"),
                    ("online_probe.enabled=maybe", "online_probe.enabled"),
                    ("online_probe.lr=0", "online_probe.lr"),
                    ("online_probe.lr=-0.1", "online_probe.lr"),
                    ("online_probe.lr=fast", "online_probe.lr"),
                    ("online_probe.decay=-1e-4", "online_probe.decay"),
                    ("online_probe.momentum=1.0", "online_probe.momentum"),
                    ("online_probe.momentum=-0.1", "online_probe.momentum"),
                    ("online_probe.top_k=0", "online_probe.top_k"),
                    ("online_probe.top_k=2.5", "online_probe.top_k")):
        with pytest.raises(AssertionError, match=key.replace(".", r"\.")):
            check_pretrain_conf(_cfg([ov]))


def _trainer(ov, classes=3):
    from simclr_amd.parallel import state as pstate
    from simclr_amd.train.pretrain import Trainer
    cfg = _cfg(["experiment.base_cnn=resnet18", "experiment.batches=8", "data.synthetic=true",
                "runtime.precision=fp32", "parameter.epochs=10", "parameter.warmup_epochs=1",
                *ov])
    pstate.reset()
    st = pstate.get()
    st.device = torch.device("cpu")
    torch.manual_seed(0)
    return Trainer(cfg, st, 64, precision="fp32", num_classes=classes)


def _batches(k):
    from simclr_amd.data.datasets import synthetic_dataset
    from simclr_amd.data.loader import ContrastiveLoader
    loader = ContrastiveLoader(synthetic_dataset(32, 3), 8, torch.device("cpu"), seed=7)
    loader.label_i32 = True
    return [(x.clone(), y.clone()) for x, y in loader][:k]


@pytest.mark.timeout(600)
def test_trainer_fp32_isolation_and_labels():
    """The probe never touches the encoder: loss, master, momentum and BatchNorm buffers are
    bitwise what they are without it, over 3 steps; and the label bookkeeping of step()."""
    batches = _batches(3)
    on = _trainer(["online_probe.enabled=true", "online_probe.top_k=2"])
    off = _trainer([])
    assert off.probe is None and on.probe is not None and not on.probe.hip
    assert (on.probe.C, on.probe.F, on.probe.top_k) == (3, 512, 2)
    assert not on.probe.round_operands  # the fp32 path keeps fp32 operands
    assert torch.equal(on.store.master, off.store.master)  # same model initialisation
    W0 = on.probe.W.clone()
    for x, y in batches:
        a, b = on.step(x, y), off.step(x)
        assert torch.equal(a, b), (float(a), float(b))
    assert torch.equal(on.store.master, off.store.master)
    assert torch.equal(on.opt.mom, off.opt.mom)
    for u, v in zip(on.model.buffers(), off.model.buffers()):
        assert torch.equal(u, v)
    m = on.probe.metrics()
    assert m["rows"] == 3 * 16 and math.isfinite(m["loss"]) and 0.0 <= m["acc"] <= 1.0
    assert on.probe.host_step == 3 and int(on.probe.step_t) == 3
    assert not torch.equal(on.probe.W, W0)
    assert on.probe.lr0 == 0.1 * 8 / 256 and on.probe.total == on.total_steps
    with pytest.raises(ValueError, match=r"online_probe\.enabled.*labels"):
        on.step(batches[0][0])
    with pytest.raises(ValueError, match="labels"):
        on.step(batches[0][0], batches[0][1][:3])
    with pytest.raises(ValueError, match=r"online_probe\.enabled"):
        off.step(*batches[0])
    assert on.probe.host_step == 3  # a refused step trained nothing


def test_trainer_needs_the_class_count():
    with pytest.raises(ValueError, match="class count"):
        _trainer(["online_probe.enabled=true", "experiment.name=other"], classes=None)
    assert _trainer(["online_probe.enabled=true"], classes=None).probe.C == 10  # cifar10


# ------------------------------------------------------------------ 2-rank gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


DIST = dict(n=8, Fd=40, C=10, steps=3, lr0=0.3, decay=1e-3, warmup=1, total=6)


def _dist_probe(**kw):
    torch.manual_seed(5)
    lin = torch.nn.Linear(DIST["Fd"], DIST["C"])
    return _op().OnlineProbe(lin.weight, lin.bias, DIST["lr0"], DIST["decay"], 0.9, 3,
                             DIST["warmup"], DIST["total"], **kw)


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    n = DIST["n"]
    pr = _dist_probe(group=dist.group.WORLD, world_size=world)
    assert pr.comm and pr.gscale == 1.0 / world
    pr.broadcast_from(0)
    sl = slice(rank * n, (rank + 1) * n)
    for h, y in _data(world * n, DIST["Fd"], DIST["C"], DIST["steps"], 9):
        v0, v1 = h[:world * n], h[world * n:]
        pr.step(torch.cat([v0[sl], v1[sl]]), y[sl])
    m = pr.metrics(group=dist.group.WORLD)
    torch.save({"master": pr.master, "mom": pr.mom, "metrics": m}, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_average_the_gradient(tmp_path):
    """Both ranks hold bitwise the same probe; it is the single-process probe on the concatenated
    batch up to summation order (the mean over 2 x 8 rows of a rank, then over the ranks, against
    one mean over 32 rows): the bound is 4x the twin's own fp32 / fp64-accumulation gap.  The
    counts are equal; the mean loss moves by at most twice the logit change those weights allow,
    plus the fp32 error of the per-row loss."""
    world, n = 2, DIST["n"]
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(tmp_path / f"r{r}.pt", weights_only=True) for r in range(world)]
    assert torch.equal(got[0]["master"], got[1]["master"]) and torch.equal(got[0]["mom"], got[1]["mom"])
    assert got[0]["metrics"] == got[1]["metrics"]
    batches = _data(world * n, DIST["Fd"], DIST["C"], DIST["steps"], 9)
    one32, one64 = _dist_probe(), _dist_probe(accumulate=torch.float64)
    for h, y in batches:
        one32.step(h, y)
        one64.step(h, y)
    gap = float((one32.master.double() - one64.master.double()).abs().max())
    d = float((got[0]["master"].double() - one64.master.double()).abs().max())
    print(f"twin fp32/fp64 gap {gap:.3e}, 2 ranks vs fp64 twin {d:.3e}")
    assert gap > 0 and d <= 4 * gap
    m2, m1 = got[0]["metrics"], one32.metrics()
    assert m2["rows"] == m1["rows"] == DIST["steps"] * 2 * world * n
    assert m2["acc"] == m1["acc"] and m2["top_k_acc"] == m1["top_k_acc"]
    habs = max(float(h.to(torch.bfloat16).float().abs().sum(1).max()) for h, _ in batches)
    tol = 2 * 4 * gap * (habs + 1) + (DIST["C"] + 16) * 2 * U * (1 + abs(m1["loss"]))
    assert abs(m2["loss"] - m1["loss"]) <= tol, (m2["loss"], m1["loss"], tol)


# ------------------------------------------------------------------ resume
def test_state_dict_resumes_bitwise():
    batches = _data(8, 40, 10, 4, 4)
    straight = _dist_probe()
    for h, y in batches:
        straight.step(h, y)
    first = _dist_probe()
    for h, y in batches[:2]:
        first.step(h, y)
    sd = first.state_dict()
    assert set(sd) == {"master", "momentum", "step"} and sd["step"] == 2
    torch.manual_seed(99)
    lin = torch.nn.Linear(40, 10)  # another initialisation: everything comes from the file
    second = _op().OnlineProbe(lin.weight, lin.bias, DIST["lr0"], DIST["decay"], 0.9, 3,
                               DIST["warmup"], DIST["total"])
    second.load_state_dict(sd)
    assert second.host_step == 2 and int(second.step_t) == 2
    assert torch.equal(second.Wsh, second.W.to(torch.bfloat16))
    for h, y in batches[2:]:
        second.step(h, y)
    assert torch.equal(second.master, straight.master) and torch.equal(second.mom, straight.mom)
    assert torch.equal(second.lr_t, straight.lr_t)
    with pytest.raises(ValueError, match="online_probe"):
        _op().OnlineProbe(torch.zeros(10, 100), torch.zeros(10), 0.1).load_state_dict(sd)


COMMON = ["data.synthetic=true", "data.synthetic_size=32", "experiment.batches=8",
          "experiment.base_cnn=resnet18", "parameter.epochs=2", "parameter.warmup_epochs=1",
          "experiment.save_model_epoch=1"]


def _main(args, cwd):
    r = subprocess.run([sys.executable, str(ROOT / "main.py"), *args], cwd=str(cwd),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout + r.stderr


def _online_line(out, epoch):
    return [l for l in out.splitlines() if f"Epoch:{epoch}/2 online_loss:" in l][0].split(" - ")[-1]


@pytest.mark.timeout(900)
def test_cli_logs_checkpoints_and_resumes(tmp_path):
    run = tmp_path / "run"
    out = _main(COMMON + ["online_probe.enabled=true", f"hydra.run.dir={run}"], tmp_path)
    assert "Epoch:2/2 progress:1.000 loss:" in out and "online_acc:" in _online_line(out, 2)
    rec = [json.loads(l) for l in (run / "metrics.jsonl").read_text().splitlines()]
    assert len(rec) == 2
    for r in rec:
        assert {"online_loss", "online_acc", "online_top_k_acc"} <= set(r)
        assert math.isfinite(r["online_loss"]) and 0.0 <= r["online_acc"] <= r["online_top_k_acc"] <= 1.0
    # the reference-format checkpoint has no probe keys; the resume file has the entry
    ck = torch.load(run / "epoch=2-cifar10.pt", weights_only=True)
    assert len(ck) == 128 and not any("probe" in k and "projection" not in k for k in ck)
    blob = torch.load(run / "resume-1.pt", weights_only=True)
    assert set(blob["online_probe"]) == {"master", "momentum", "step"}
    assert blob["online_probe"]["step"] == 4  # 32 images / 8 per step
    # resuming after epoch 1 reproduces epoch 2's online metrics to the digit
    run2 = tmp_path / "run2"
    out2 = _main(COMMON + ["online_probe.enabled=true", f"hydra.run.dir={run2}",
                           f"runtime.resume={run / 'resume-1.pt'}"], tmp_path)
    assert _online_line(out2, 2) == _online_line(out, 2)
    assert "starts fresh" not in out2
    # a run without the probe: no second line, no field, no entry; resuming from it with the
    # probe on starts a fresh probe and says so
    run3 = tmp_path / "run3"
    out3 = _main(COMMON + [f"hydra.run.dir={run3}"], tmp_path)
    assert "online_" not in out3
    assert "online_loss" not in (run3 / "metrics.jsonl").read_text()
    assert "online_probe" not in torch.load(run3 / "resume-1.pt", weights_only=True)
    ref = [l.split("loss:")[1] for l in out.splitlines() if "Epoch:2/2 progress" in l][0]
    off = [l.split("loss:")[1] for l in out3.splitlines() if "Epoch:2/2 progress" in l][0]
    assert ref == off  # the reference's line is what it is without the probe
    run4 = tmp_path / "run4"
    out4 = _main(COMMON + ["online_probe.enabled=true", f"hydra.run.dir={run4}",
                           f"runtime.resume={run3 / 'resume-1.pt'}"], tmp_path)
    assert "online_probe entry" in out4 and "starts fresh" in out4
    assert "online_acc:" in _online_line(out4, 2)
