"""The online probe's HIP kernels (csrc/probe.hip) against the torch twin of
``ops/online_probe.py`` (fp64 accumulation on the same bf16 operands) and bitwise against the
sweep's ops, which run the same kernels; the captured pre-training step with the probe in it, and
the CLI.

Bounds, with u = 2^-24 (fp32 unit roundoff), as tests/test_gpu_probe_sweep.py derives them:

* logits: ``Fp · u · (Σ|x_i||w_i| + |b|)``, the fp32 accumulation bound of the dot product with the
  bias counted as one more term;
* loss = lse(z) - z_t: ``2 ez`` for the largest logit error ``ez`` of the row plus
  ``(C + 16) · 2u · (1 + |lse| + |z_t|)`` for expf / logf and the sum of C terms;
* dlogits: softmax moves by ``p · (2.1 ez + (C + 16) · 2u)``, divided by rows, plus the bf16
  rounding ``2^-8`` of the value;
* dW (on the kernel's own dlogits): ``rows · u · Σ|dl||x|``; db: the dlogits bounds summed over
  the rows plus ``rows · u · Σ|dl|``;
* ranks: exactly equal.  The data puts the target's logit at least 100 logit bounds away from
  every other logit of its row, which the test asserts on the twin alone.
"""
import json
import subprocess
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
ROOT = Path(__file__).resolve().parents[1]
# (rows, F, C, seed): seeds for which the twin's smallest gap between the target's logit and any
# other exceeds 100 logit bounds (found on the CPU; the test asserts the gap)
SHAPES = [(16, 64, 10, 11), (48, 96, 100, 7), (32, 2048, 1000, 11), (1024, 512, 10, 11)]


def _op():
    from simclr_amd.ops import _ext, online_probe
    _ext.require()
    return online_probe


def _problem(rows, Fd, C, seed, steps=1):
    """Class-structured rows: image i of true class t mixes the centres of t, t + 1, t + 2 with
    weights 1, 0.6, 0.3 and carries the label t + (i mod 3), so the target's rank is i mod 3 once
    the weights are near the centres (scaled to logits of about 4, 2.4, 1.2 and 0 +- 4 / sqrt(F))."""
    g = torch.Generator().manual_seed(seed)
    n = rows // 2
    centers = torch.randn(C, Fd, generator=g)
    W = centers * (4.0 / Fd) + 0.02 / Fd ** 0.5 * torch.randn(C, Fd, generator=g)
    b = 0.05 * torch.randn(C, generator=g)
    batches = []
    for _ in range(steps):
        t = torch.randint(0, C, (n,), generator=g)
        y = ((t + torch.arange(n) % 3) % C).to(torch.int32)
        mix = centers[t] + 0.6 * centers[(t + 1) % C] + 0.3 * centers[(t + 2) % C]
        h = torch.cat([mix + 0.1 * torch.randn(n, Fd, generator=g) for _ in range(2)])
        batches.append((h.to(torch.bfloat16), y))
    return W, b, batches


def _pair(rows, Fd, C, seed, steps=1, **kw):
    op = _op()
    W, b, batches = _problem(rows, Fd, C, seed, steps)
    args = dict(lr0=0.2, decay=1e-3, momentum=0.9, top_k=2, warmup_steps=2, total_steps=12)
    args.update(kw)
    dev = op.OnlineProbe(W, b, device=DEV, **args)
    tw = op.OnlineProbe(W, b, device="cpu", accumulate=torch.float64, **args)
    assert dev.hip and not tw.hip
    return dev, tw, batches


@pytest.mark.parametrize("rows, Fd, C, seed", SHAPES)
def test_step_against_twin(rows, Fd, C, seed):
    dev, tw, ((h, y),) = _pair(rows, Fd, C, seed)
    # non-zero momentum, so the update's every term is exercised
    g = torch.Generator().manual_seed(1)
    tw.mom[:tw.Cp * tw.Fp].view(tw.Cp, tw.Fp)[:C, :Fd] = 0.01 * torch.randn(C, Fd, generator=g)
    tw.mom[tw.Cp * tw.Fp:][:C] = 0.01 * torch.randn(C, generator=g)
    dev.mom.copy_(tw.mom)
    for p in (dev, tw):
        p.host_step = 5
        p.step_t.fill_(5)
    W0, M0 = tw.master.double().clone(), tw.mom.double().clone()
    ref = tw.step(h, y)
    out = dev.step(h.to(DEV), y.to(DEV))
    torch.cuda.synchronize()
    assert dev.hip_steps == 1 and torch.equal(dev.lr_t.cpu(), tw.lr_t)
    x = h.double()
    Wb = W0[:tw.Cp * tw.Fp].view(tw.Cp, tw.Fp)[:C, :Fd].to(torch.bfloat16).double()
    bb = W0[tw.Cp * tw.Fp:][:C]
    z = ref["logits"].double()
    ez = dev.Fp * U * (x.abs() @ Wb.abs().t() + bb.abs())
    got = out["logits"].cpu().double()
    assert bool(((got - z).abs() <= ez).all()), float(((got - z).abs() / ez).max())
    # the twin alone: the target's logit is 100 bounds away from every other logit of its row
    t = y.long().repeat(2)
    zt = z.gather(1, t[:, None])
    other = torch.ones_like(z, dtype=torch.bool).scatter_(1, t[:, None], False)
    margin = float(((z - zt).abs()[other]).min())
    print(f"({rows}, {Fd}, {C}): smallest target gap {margin:.3e}, logit bound {float(ez.max()):.3e}")
    assert margin > 100 * float(ez.max())
    assert torch.equal(out["rank"].cpu(), ref["rank"])
    assert {0, 1, 2} <= set(ref["rank"].tolist())  # (the data does rank targets below the top)
    lse = torch.logsumexp(z, 1)
    ezr = ez.max(1).values
    fn = (C + 16) * 2 * U
    tol = 2 * ezr + fn * (1 + lse.abs() + zt[:, 0].abs())
    assert bool(((out["loss"].cpu().double() - (lse - zt[:, 0])).abs() <= tol).all())
    p = torch.softmax(z, 1)
    onehot = torch.zeros_like(p).scatter_(1, t[:, None], 1.0)
    dl = (p - onehot) / rows
    edl32 = p * (2.1 * ezr[:, None] + fn) / rows + U * dl.abs()
    edl = edl32 + 2.0 ** -8 * (dl.abs() + edl32) + 1e-38
    kdl = out["dl"].float().cpu().double()
    assert bool(((kdl - dl).abs() <= edl).all())
    # gradients: dW on the kernel's own dlogits, db in tile order
    nw = dev.Cp * dev.Fp
    gW = dev.grad[:nw].view(dev.Cp, dev.Fp).cpu().double()
    dW = kdl.t() @ x
    assert bool(((gW[:C, :Fd] - dW).abs() <= rows * U * (kdl.abs().t() @ x.abs()) + 1e-38).all())
    assert not gW[C:].any() and not gW[:, Fd:].any()
    gb = dev.grad[nw:].cpu().double()
    assert bool(((gb[:C] - dl.sum(0)).abs() <= edl32.sum(0) + rows * U * dl.abs().sum(0)).all())
    assert not gb[C:].any()
    # update: the twin's formula on the kernel's own gradient, a few roundings per term
    lr, m, wd = float(tw.lr_t), 0.9, 1e-3
    G = dev.grad.cpu().double()
    d = G + wd * W0
    nb = m * M0 + d
    want = W0 - lr * (d + m * nb)
    terms = G.abs() + wd * W0.abs() + m * M0.abs()
    mask = torch.zeros(nw + dev.Cp, dtype=torch.bool)
    mask[:nw].view(dev.Cp, dev.Fp)[:C, :Fd] = True
    mask[nw:][:C] = True
    assert bool(((dev.mom.cpu().double() - nb).abs()[mask] <= (8 * U * terms)[mask]).all())
    assert bool(((dev.master.cpu().double() - want).abs()[mask]
                 <= (8 * U * (W0.abs() + lr * (1 + m) * terms))[mask]).all())
    # padding columns and features of master, momentum and shadow never move
    assert torch.equal(dev.master.cpu()[~mask], W0.float()[~mask]) and not dev.master.cpu()[~mask].any()
    assert torch.equal(dev.mom.cpu()[~mask], M0.float()[~mask])
    assert torch.equal(dev.Wsh, dev.W.to(torch.bfloat16))
    assert float((dev.master.cpu().double() - W0).abs().max()) > 0
    # metrics of this one step: the weights before the update
    md, mt = dev.metrics(), tw.metrics()
    assert (md["rows"], md["acc"], md["top_k_acc"]) == (rows, mt["acc"], mt["top_k_acc"])
    assert abs(md["loss"] - mt["loss"]) <= float(tol.max())


def _trajectory(device, steps, **kw):
    op = _op()
    W, b, batches = _problem(64, 96, 10, 5, steps)
    pr = op.OnlineProbe(W, b, 0.3, 1e-3, 0.9, 3, 2, 12, device=device, **kw)
    losses = [pr.step(h.to(device), y.to(device))["loss"].double().mean().cpu() for h, y in batches]
    return pr, torch.stack(losses)


def test_trajectory_against_fp64_twin():
    """5 steps of ``OnlineProbe.step``: the kernels against the twin with fp64 accumulation on the
    same rounded operands.  As in the sweep's trajectory test the bound is 4x the gap the twin
    itself shows between fp32 and fp64 accumulation, computed here on the CPU on every run."""
    t32, l32 = _trajectory("cpu", 5, hip=False)
    t64, l64 = _trajectory("cpu", 5, hip=False, accumulate=torch.float64)
    pr, lg = _trajectory(DEV, 5)
    assert pr.hip_steps == 5 and int(pr.step_t) == 5
    nw = pr.Cp * pr.Fp
    for name, a32, a64, got in (("weights", t32.master[:nw], t64.master[:nw], pr.master[:nw].cpu()),
                                ("bias", t32.master[nw:], t64.master[nw:], pr.master[nw:].cpu()),
                                ("loss", l32, l64, lg)):
        gap = float((a32.double() - a64.double()).abs().max())
        d = float((got.double() - a64.double()).abs().max())
        print(f"{name}: twin fp32/fp64 gap {gap:.3e}, kernels vs fp64 twin {d:.3e}")
        assert gap > 0 and d <= 4 * gap, (name, d, gap)
    assert pr.metrics()["rows"] == 5 * 64 == t64.metrics()["rows"]
    assert pr.metrics()["acc"] == t64.metrics()["acc"]


def test_repeatable_bitwise_and_padding():
    a, la = _trajectory(DEV, 5)
    b, lb = _trajectory(DEV, 5)
    assert torch.equal(a.master, b.master) and torch.equal(a.mom, b.mom) and torch.equal(la, lb)
    assert torch.equal(a.acc_loss, b.acc_loss) and torch.equal(a.acc_cnt, b.acc_cnt)
    assert torch.equal(a.Wsh, b.Wsh) and torch.equal(a.Wsh, a.W.to(torch.bfloat16))
    for p in (a.W, a.mom[:a.Cp * a.Fp].view(a.Cp, a.Fp), a.Wsh):
        assert not p[10:].any() and not p[:, 96:].any()
    assert not a.b[10:].any() and float(a.W.abs().max()) > 0


def test_shapes_outside_the_limits_take_the_twin_and_ops_check_by_name():
    op = _op()
    W, b, ((h, y),) = _problem(24, 64, 10, 3)  # 24 rows: not a multiple of 16
    pr = op.OnlineProbe(W, b, 0.1, device=DEV)
    pr.step(h.to(DEV), y.to(DEV))
    assert pr.hip and pr.hip_steps == 0 and pr.metrics()["rows"] == 24
    ops = torch.ops.simclr_amd
    with pytest.raises(RuntimeError, match="online_probe_forward: rows"):
        ops.online_probe_forward(h.to(DEV), y.to(DEV), pr.Wsh, pr.b, 10,
                                 torch.empty(24, 16, device=DEV), torch.empty(24, device=DEV),
                                 torch.empty(24, device=DEV, dtype=torch.int32),
                                 torch.empty(16, 32, device=DEV, dtype=torch.bfloat16),
                                 torch.empty(2, 16, device=DEV))
    with pytest.raises(RuntimeError, match="acc_cnt"):
        ops.online_probe_metrics(torch.empty(16, device=DEV),
                                 torch.empty(16, device=DEV, dtype=torch.int32), 5, pr.acc_loss,
                                 pr.acc_cnt.to(torch.int32))
    with pytest.raises(RuntimeError, match="online_probe_update: master"):
        ops.online_probe_update(pr.master[:-1], pr.grad, pr.mom, pr.Wsh, pr.lr_t, 0.0, 0.9, 1.0,
                                10, 64, 64)


# ------------------------------------------------------------------ one kernel family
# (rows, F, C): Cp 16 (one column tile at a time) with a pure-padding row tile (Rp 32); Cp 112
# (seven column tiles: the last group of four is clamped); Cp 32 with a mostly-padding column tile
FAMILY_SHAPES = [(16, 64, 10), (48, 96, 100), (32, 64, 17)]


def _family_operands(rows, Fd, C):
    op = _op()
    W, b, ((h, y32),) = _problem(rows, Fd, C, 3)
    Cp, Fp, Rp = op.padded_classes(C), op.padded_features(Fd), (rows + 31) // 32 * 32
    X = torch.zeros(rows, Fp, dtype=torch.bfloat16)
    X[:, :Fd] = h
    Wsh = torch.zeros(Cp, Fp, dtype=torch.bfloat16)
    Wsh[:C, :Fd] = W.to(torch.bfloat16)
    bias = torch.zeros(Cp)
    bias[:C] = b
    return X.to(DEV), y32.to(DEV), Wsh.to(DEV), bias.to(DEV), Cp, Fp, Rp


@pytest.mark.parametrize("rows, Fd, C", FAMILY_SHAPES)
def test_forward_is_bitwise_the_sweeps_forward(rows, Fd, C):
    """The online probe's forward and the sweep's (G = 1, idx = arange, the labels repeated per
    view) are one kernel under two row policies: every output has the same bits."""
    X, y32, Wsh, bias, Cp, Fp, Rp = _family_operands(rows, Fd, C)
    ops = torch.ops.simclr_amd
    f32, i32, bf = (dict(device=DEV, dtype=t) for t in (torch.float32, torch.int32, torch.bfloat16))
    # every output starts from a value that neither kernel writes
    Zo, Zs = torch.full((rows, Cp), 7.0, **f32), torch.full((rows, Cp), 7.0, **f32)
    lo, ls = torch.full((rows,), 7.0, **f32), torch.full((rows,), 7.0, **f32)
    ro, rs = torch.full((rows,), -7, **i32), torch.full((1, rows), -7, **i32)
    do, ds = torch.full((Cp, Rp), 7.0, **bf), torch.full((Cp, Rp + 32), 7.0, **bf)
    po, ps = torch.full((rows // 16, Cp), 7.0, **f32), torch.full((rows // 16, Cp), 7.0, **f32)
    ops.online_probe_forward(X, y32, Wsh, bias, C, Zo, lo, ro, do, po)
    y = y32.long().repeat(rows // y32.numel())
    ops.probe_forward(X, y, torch.arange(rows, device=DEV), Wsh, bias, 1, C, Zs, ls, rows, rs, ds,
                      ps)
    torch.cuda.synchronize()
    assert torch.equal(Zo[:rows, :C], Zs[:rows, :C])
    assert torch.equal(lo, ls) and torch.equal(ro, rs[0])
    assert torch.equal(do.view(torch.int16), ds[:, :Rp].view(torch.int16))
    assert not do[C:].any() and not do[:, rows:].any()  # the padding columns and rows: zeros
    assert bool((ds[:, Rp:] == 7.0).all())              # (the sweep's wider dlT: untouched)
    assert torch.equal(po, ps)
    assert bool(torch.isfinite(lo).all()) and int(ro.min()) >= 0 and int(ro.max()) < C
    assert float(do.float().abs().max()) > 0


@pytest.mark.parametrize("rows, Fd, C", FAMILY_SHAPES)
def test_weight_gradient_is_bitwise_the_sweeps(rows, Fd, C):
    """The same dlogits and bias partials through ``online_probe_wgrad`` (stores the gradient) and
    ``probe_update`` (G = 1, zero weights and momentum, lr 1, no decay, step 0, momentum 0: its
    Nesterov epilogue returns exactly ``-grad``)."""
    X, _, _, _, Cp, Fp, Rp = _family_operands(rows, Fd, C)
    ops = torch.ops.simclr_amd
    g = torch.Generator().manual_seed(rows + C)
    dlT = torch.zeros(Cp, Rp, dtype=torch.bfloat16)
    dlT[:C, :rows] = (0.01 * torch.randn(C, rows, generator=g)).to(torch.bfloat16)
    dlT, dbp = dlT.to(DEV), torch.randn(rows // 16, Cp, generator=g).to(DEV)
    grad = torch.full((Cp * Fp + Cp,), 7.0, device=DEV)
    ops.online_probe_wgrad(X, dlT, dbp, grad, C)
    W, Mw = torch.zeros(Cp, Fp, device=DEV), torch.zeros(Cp, Fp, device=DEV)
    b, Mb = torch.zeros(Cp, device=DEV), torch.zeros(Cp, device=DEV)
    Wsh = torch.zeros(Cp, Fp, device=DEV, dtype=torch.bfloat16)
    one, zero = torch.ones(1, device=DEV), torch.zeros(1, device=DEV)
    ops.probe_update(X, torch.arange(rows, device=DEV), dlT, dbp, W, Mw, Wsh, b, Mb, one, zero,
                     one, 0, 0.0, 1, C)
    torch.cuda.synchronize()
    assert torch.equal(W[:C], -grad[:Cp * Fp].view(Cp, Fp)[:C])
    assert torch.equal(b[:C], -grad[Cp * Fp:][:C])
    assert float(W.abs().max()) > 0 and float(b.abs().max()) > 0
    assert not W[C:].any() and not b[C:].any()  # the sweep never moves a padding column


# ------------------------------------------------------------------ training path
def _run_steps(tmp_path, mode, *flags):
    out = tmp_path / f"{'-'.join((mode,) + flags)}.pt"
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable,
                        str(ROOT / "tests" / "_online_probe_steps.py"), mode, str(out), *flags],
                       capture_output=True, text=True)
    assert r.returncode == 0, (mode, flags, r.returncode, r.stdout[-2000:] + r.stderr[-3000:])
    return torch.load(out, weights_only=True)


PROBE_KEYS = ("probe_master", "probe_mom", "probe_step", "acc_loss", "acc_cnt")


@pytest.mark.timeout(900)
def test_captured_step_carries_the_probe(tmp_path):
    """ResNet-18 at batch 32, deterministic tiles, five batches with different labels: eager issue,
    graph replay and streams replay give bitwise the same probe and accumulators, and the
    contrastive loss and the encoder are bitwise those of the run without the probe."""
    off = _run_steps(tmp_path, "eager", "off")
    eager = _run_steps(tmp_path, "eager")
    assert eager["hip_steps"] == 5 and int(eager["acc_cnt"][2]) == 5 * 64
    assert torch.equal(eager["losses"], off["losses"]) and torch.equal(eager["master"], off["master"])
    for mode in ("graph", "streams"):
        r = _run_steps(tmp_path, mode)  # (started only after the runs before it ended well)
        assert r["replayed"] == 3 and r["mode"] == mode
        assert torch.equal(r["losses"], off["losses"]) and torch.equal(r["master"], off["master"])
        for k in PROBE_KEYS:
            assert torch.equal(r[k], eager[k]), (mode, k)
    assert int(eager["probe_step"]) == 5


@pytest.mark.timeout(600)
def test_supcon_and_probe_share_the_label_buffer(tmp_path):
    sup = _run_steps(tmp_path, "eager", "supcon")
    cap = _run_steps(tmp_path, "streams", "supcon")
    assert cap["replayed"] == 3 and cap["shared_labels"] == 1
    assert torch.equal(cap["losses"], sup["losses"]) and torch.equal(cap["master"], sup["master"])
    for k in PROBE_KEYS:
        assert torch.equal(cap[k], sup[k]), k


@pytest.mark.timeout(600)
def test_forced_comm_all_reduce_is_captured(tmp_path):
    """A 1-rank RCCL group: the probe's gradient all-reduce is issued (eager and captured) and
    everything is bitwise what the run without collectives gives."""
    plain = _run_steps(tmp_path, "eager")
    eager = _run_steps(tmp_path, "eager", "comm")
    cap = _run_steps(tmp_path, "streams", "comm")
    assert plain["all_reduces"] == 0 and eager["all_reduces"] == 5
    assert cap["all_reduces"] == 3 and cap["replayed"] == 3  # 2 eager steps + the capture
    for r in (eager, cap):
        for k in PROBE_KEYS:
            assert torch.equal(r[k], plain[k]), k


@pytest.mark.timeout(600)
def test_cli_pretrains_with_the_probe(tmp_path):
    run = tmp_path / "run"
    r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, str(ROOT / "main.py"),
                        "data.synthetic=true", "data.synthetic_size=256", "experiment.batches=32",
                        "online_probe.enabled=true", "parameter.epochs=2",
                        f"hydra.run.dir={run}"], cwd=str(tmp_path), capture_output=True, text=True)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "Epoch:2/2 progress:1.000 loss:" in out and "Epoch:2/2 online_loss:" in out
    assert "training step captured" in out
    rec = [json.loads(l) for l in (run / "metrics.jsonl").read_text().splitlines()]
    assert len(rec) == 2
    for e in rec:
        for k in ("online_loss", "online_acc", "online_top_k_acc"):
            assert e[k] == e[k] and abs(e[k]) < 1e4
        assert 0.0 <= e["online_acc"] <= e["online_top_k_acc"] <= 1.0
    rows = [float(l.split("online_rows:")[1].split()[0]) for l in out.splitlines()
            if "online_rows:" in l]
    assert rows == [8 * 64, 8 * 64]  # steps x 2n per epoch
