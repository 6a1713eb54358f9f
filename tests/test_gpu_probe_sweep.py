"""HIP kernels of csrc/probe.hip (fused forward / CE / gradient, fused weight gradient / Nesterov
update) against fp64 torch on the kernels' own bf16 operands and against the torch twin of
``ops/probe_sweep.py``.

Bounds, with u = 2^-24 (fp32 unit roundoff):

* logits: ``Fp · u · (Σ|x_i||w_i| + |b|)``, the fp32 accumulation bound of the dot product with the
  bias counted as one more term;
* loss = lse(z) - z_t: the log-sum-exp moves by at most the largest logit error ``ez`` of the row,
  so ``2 ez`` plus ``(C + 16) · 2u · (1 + |lse| + |z_t|)`` for expf / logf and the sum of C terms;
* dlogits: softmax moves by ``p · (2.1 ez + (C + 16) · 2u)`` (the exponent ``z - lse`` moves by
  ``2 ez``), divided by rows, plus the bf16 rounding ``2^-8`` of the value;
* dW: ``rows · u · Σ|dl||x|``; master and momentum follow with the update's own factors plus a few
  roundings of every term of the update.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
SHAPES = [(37, 96, 10, 3), (512, 2048, 100, 8), (130, 512, 1000, 1), (1, 64, 10, 16)]


def _ps():
    from simclr_amd.ops import _ext, probe_sweep
    if DEV == "cuda":
        _ext.require()
    return probe_sweep


def _random_sweep(rows, F, C, G, seed, steps=10, device=None):
    """A sweep with different random weights, biases and momentum per configuration, a feature
    matrix of rows + 13 rows and a permuted index vector of ``rows`` of them."""
    ps = _ps()
    dev = device or DEV
    g = torch.Generator().manual_seed(seed)
    sw = ps.LinearSweep(torch.zeros(C, F), torch.zeros(C), [0.05 * (i + 1) for i in range(G)],
                        [1e-4 * (i + 1) for i in range(G)], 0.9, ps.cosine_table(steps), device=dev)
    Wv, Mv = sw.W.view(G, sw.Cp, sw.Fp), sw.Mw.view(G, sw.Cp, sw.Fp)
    Wv[:, :C, :F] = (0.2 * torch.randn(G, C, F, generator=g)).to(dev)
    Mv[:, :C, :F] = (0.01 * torch.randn(G, C, F, generator=g)).to(dev)
    sw.b.view(G, sw.Cp)[:, :C] = (0.1 * torch.randn(G, C, generator=g)).to(dev)
    sw.Mb.view(G, sw.Cp)[:, :C] = (0.01 * torch.randn(G, C, generator=g)).to(dev)
    sw.Wsh.copy_(sw.W.to(torch.bfloat16))
    N = rows + 13
    X = ps.prepare_features(torch.randn(N, F, generator=g).to(dev))
    y = torch.randint(0, C, (N,), generator=g).to(dev)
    idx = torch.randperm(N, generator=g)[:rows].to(dev)
    return sw, X, y, idx


def _ref_rank(z, t):
    C = z.shape[-1]
    zt = z.gather(-1, t[..., None])
    cls = torch.arange(C, device=z.device)
    return ((z > zt) | ((z == zt) & (cls < t[..., None]))).sum(-1)


@pytest.mark.parametrize("rows, F, C, G", SHAPES)
def test_forward_ce_against_fp64(rows, F, C, G):
    sw, X, y, idx = _random_sweep(rows, F, C, G, 11)
    assert sw.hip == (DEV == "cuda")
    fwd = sw.forward(X, y, idx, train=True)
    loss, rank = fwd["loss"].clone(), fwd["rank"].clone()
    ev = sw.forward(X, y, idx, train=False)  # the evaluation variant of the kernel
    assert torch.equal(ev["loss"], loss) and torch.equal(ev["rank"], rank)
    x = X[idx].double()                                         # [rows][Fp]
    W = sw.Wsh.view(G, sw.Cp, sw.Fp)[:, :C].double()            # [G][C][Fp]
    b = sw.b.view(G, sw.Cp)[:, :C].double()
    z = torch.einsum("rf,gcf->grc", x, W) + b[:, None, :]       # [G][rows][C]
    ez = sw.Fp * U * (torch.einsum("rf,gcf->grc", x.abs(), W.abs()) + b.abs()[:, None, :])
    got = fwd["logits"].permute(1, 0, 2).double()
    assert bool(((got - z).abs() <= ez).all()), float(((got - z).abs() / ez).max())
    t = y[idx].expand(G, rows)
    lse = torch.logsumexp(z, 2)
    zt = z.gather(2, t[..., None])[..., 0]
    ezr = ez.max(2).values
    fn = (C + 16) * 2 * U
    tol = 2 * ezr + fn * (1 + lse.abs() + zt.abs())
    assert bool(((loss.double() - (lse - zt)).abs() <= tol).all())
    p = torch.softmax(z, 2)
    onehot = torch.zeros_like(p).scatter_(2, t[..., None], 1.0)
    dl = (p - onehot) / rows
    edl32 = p * (2.1 * ezr[..., None] + fn) / rows + U * dl.abs()
    edl = edl32 + 2.0 ** -8 * (dl.abs() + edl32) + 1e-38
    assert bool(((fwd["dl"].double() - dl).abs() <= edl).all())
    db = fwd["db"].double()
    db = db.sum(0) if db.dim() == 3 else db
    assert bool(((db - dl.sum(1)).abs() <= edl32.sum(1) + rows * U * dl.abs().sum(1)).all())
    # ranks: equal unless another class's logit lies within the bound of the target's
    ref = _ref_rank(z, t)
    bad = ref != rank.long()
    ezt = ez.gather(2, t[..., None])
    near = ((z - zt[..., None]).abs() <= ez + ezt) & (onehot == 0)
    assert bool((~bad | near.any(2)).all())
    assert int(rank.min()) >= 0 and int(rank.max()) < C


@pytest.mark.parametrize("rows, F, C, G", SHAPES)
def test_update_against_twin(rows, F, C, G):
    """One update from non-zero momentum, decay > 0, a permuted index vector: the kernel against
    the twin (fp64 weight-gradient accumulation) fed with the kernel's own dlogits."""
    ps = _ps()
    sw, X, y, idx = _random_sweep(rows, F, C, G, 12)
    sw.step = 3
    tw = ps.LinearSweep(torch.zeros(C, F), torch.zeros(C), [1.0] * G, [0.0] * G, 0.9, sw.ftab,
                        device="cpu", accumulate=torch.float64)
    for k in ("W", "b", "Mw", "Mb", "Wsh", "lr0", "wd"):
        setattr(tw, k, getattr(sw, k).cpu().clone())
    tw.step = sw.step
    W0, M0, b0, Mb0 = tw.W.clone(), tw.Mw.clone(), tw.b.clone(), tw.Mb.clone()
    fwd = sw.forward(X, y, idx, train=True)
    dl = fwd["dl"].float().cpu().contiguous()                   # [G][rows][C] bf16 values
    dbp = fwd["db"].double().cpu()
    db = (dbp.sum(0) if dbp.dim() == 3 else dbp)
    x = X[idx].double().cpu()
    tw.update(X.cpu(), idx.cpu(), {"dl": dl, "db": db.float(), "x": x})
    sw.update(X, idx, fwd)
    assert sw.step == 4 and torch.equal(sw.Wsh, sw.W.to(torch.bfloat16))
    Cp, Fp, m = sw.Cp, sw.Fp, 0.9
    lr = (tw.lr0 * tw.ftab[3]).double().view(G, 1, 1)
    wd = tw.wd.double().view(G, 1, 1)
    edW = torch.zeros(G, Cp, Fp, dtype=torch.float64)
    dW = torch.zeros(G, Cp, Fp, dtype=torch.float64)
    edW[:, :C] = rows * U * torch.einsum("grc,rf->gcf", dl.double().abs(), x.abs())
    dW[:, :C] = torch.einsum("grc,rf->gcf", dl.double(), x)
    W0v, M0v = W0.view(G, Cp, Fp).double().abs(), M0.view(G, Cp, Fp).double().abs()
    terms = dW.abs() + wd * W0v + m * M0v
    eM = edW + 8 * U * terms
    eW = lr * (1 + m) * edW + 8 * U * (W0v + lr * (1 + m) * terms)
    assert bool(((sw.Mw.cpu().double() - tw.Mw.double()).abs().view(G, Cp, Fp) <= eM).all())
    assert bool(((sw.W.cpu().double() - tw.W.double()).abs().view(G, Cp, Fp) <= eW).all())
    assert float((sw.W.cpu() - W0).abs().max()) > 0
    # bias: the partials of the 16-row tiles are summed in fp32 in tile order
    RT = (rows + 15) // 16
    edb = torch.zeros(G, Cp, dtype=torch.float64)
    dbf = torch.zeros(G, Cp, dtype=torch.float64)
    part = dbp.abs().sum(0) if dbp.dim() == 3 else dbp.abs()
    edb[:, :C] = (RT + 1) * U * part
    dbf[:, :C] = db.abs()
    lrb, wdb = lr.view(G, 1), wd.view(G, 1)
    tb = dbf + wdb * b0.view(G, Cp).double().abs() + m * Mb0.view(G, Cp).double().abs()
    assert bool(((sw.Mb.cpu().double() - tw.Mb.double()).abs().view(G, Cp) <= edb + 8 * U * tb).all())
    assert bool(((sw.b.cpu().double() - tw.b.double()).abs().view(G, Cp)
                 <= lrb * (1 + m) * edb + 8 * U * (b0.view(G, Cp).double().abs() + lrb * (1 + m) * tb)).all())
    # padding columns and padding features never move
    assert not sw.W.view(G, Cp, Fp)[:, C:].any() and not sw.W.view(G, Cp, Fp)[:, :, F:].any()
    assert not sw.b.view(G, Cp)[:, C:].any()


def _structured(n, F, C, seed, centers=None, noise=1.5):
    g = torch.Generator().manual_seed(seed)
    if centers is None:
        centers = torch.randn(C, F, generator=g)
    y = torch.randint(0, C, (n,), generator=g)
    return centers[y] + noise * torch.randn(n, F, generator=g), y, centers


def _trajectory(device, steps, lr0, decay, n=1200, bs=512, F=128, C=10, seed=5, hip=None,
                accumulate=torch.float32):
    ps = _ps()
    Xf, y, _ = _structured(n, F, C, seed)
    torch.manual_seed(seed)
    lin = torch.nn.Linear(F, C)
    sw = ps.LinearSweep(lin.weight, lin.bias, lr0, decay, 0.9, ps.cosine_table(steps),
                        device=device, accumulate=accumulate, hip=hip)
    X, y = ps.prepare_features(Xf.to(device)), y.to(device)
    gen = torch.Generator().manual_seed(seed)
    losses = []
    while sw.step < steps:
        perm = torch.randperm(n, generator=gen).to(device)
        for s in range(0, n, bs):
            if sw.step < steps:
                losses.append(sw.train_step(X, y, perm[s:s + bs]).double().mean(1).cpu())
    return sw, torch.stack(losses), X, y


LR4, WD4 = [0.1, 0.2, 0.4, 0.8], [0.0, 1e-4, 1e-3, 1e-4]


def test_trajectory_against_fp64_twin():
    """20 steps (ragged third batch of 176), G = 4: the kernels against the twin with fp64
    accumulation on the same rounded operands.  The bound is 4x the gap the twin itself shows
    between fp32 and fp64 accumulation, computed here on the CPU on every run.  Measured twin
    gap on the MI355X host: weights 3.1e-5, bias 5.5e-6, per-step mean loss 2.4e-6 (the bf16
    rounding of dlogits and shadow amplifies accumulation differences; a CPU whose BLAS sums in
    another order showed 6.0e-7 / 2.2e-8 / 1.3e-8); the kernels' distance to the fp64 twin:
    weights 3.1e-6, bias 6.3e-8, loss 6.2e-8."""
    t32, l32, _, _ = _trajectory("cpu", 20, LR4, WD4, hip=False)
    t64, l64, _, _ = _trajectory("cpu", 20, LR4, WD4, hip=False, accumulate=torch.float64)
    sw, lg, _, _ = _trajectory(DEV, 20, LR4, WD4)
    assert sw.step == 20 and lg.shape == (20, 4)
    for name, a32, a64, got in (("weights", t32.W, t64.W, sw.W.cpu()), ("bias", t32.b, t64.b, sw.b.cpu()),
                                ("loss", l32, l64, lg)):
        gap = float((a32.double() - a64.double()).abs().max())
        d = float((got.double() - a64.double()).abs().max())
        print(f"{name}: twin fp32/fp64 gap {gap:.3e}, kernels vs fp64 twin {d:.3e}")
        assert gap > 0 and d <= 4 * gap, (name, d, gap)


def test_repeatable_and_independent_bitwise():
    a, la, _, _ = _trajectory(DEV, 7, LR4, WD4)
    b, lb, _, _ = _trajectory(DEV, 7, LR4, WD4)
    assert torch.equal(a.W, b.W) and torch.equal(a.b, b.b) and torch.equal(la, lb)
    # configuration j alone against j inside G = 16, C = 10 (one column tile) and C = 100 (seven)
    for C, G, F in ((10, 16, 128), (100, 8, 96)):
        lr0 = [0.05 * (i + 1) for i in range(G)]
        wd = [1e-4 * (i % 3) for i in range(G)]
        j = G - 3
        many, lm, _, _ = _trajectory(DEV, 5, lr0, wd, n=700, bs=300, F=F, C=C)
        one, lo, _, _ = _trajectory(DEV, 5, [lr0[j]], [wd[j]], n=700, bs=300, F=F, C=C)
        for p, q in zip(many.weights(j), one.weights(0)):
            assert torch.equal(p, q)
        assert torch.equal(many.Mw.view(G, many.Cp, many.Fp)[j], one.Mw.view(1, one.Cp, one.Fp)[0])
        assert torch.equal(many.Wsh.view(G, many.Cp, many.Fp)[j], one.Wsh.view(1, one.Cp, one.Fp)[0])
        assert torch.equal(lm[:, j], lo[:, 0])
        assert not torch.equal(many.weights(0)[0], many.weights(j)[0])


def test_divergence_is_contained():
    """lr0 = 1e6 with decay 1e-2 multiplies the weights by about -1e4 per step: inf after ten
    steps, NaN after.  Its neighbours stay bitwise what they are without it."""
    lr0, wd = [0.1, 0.2, 1e6, 0.4], [0.0, 1e-4, 1e-2, 1e-3]
    keep = [0, 1, 3]
    bad, lb, X, y = _trajectory(DEV, 30, lr0, wd)
    sane, ls, _, _ = _trajectory(DEV, 30, [lr0[i] for i in keep], [wd[i] for i in keep])
    for k, i in enumerate(keep):
        for p, q in zip(bad.weights(i), sane.weights(k)):
            assert torch.equal(p, q) and bool(torch.isfinite(p).all())
        assert torch.equal(lb[:, i], ls[:, k])
    loss, top1, topk = bad.evaluate(X, y, 5)
    assert math.isnan(loss[2]) and top1[2] == 0.0 and topk[2] == 0.0
    l2, t2, k2 = sane.evaluate(X, y, 5)
    assert [loss[i] for i in keep] == l2 and [top1[i] for i in keep] == t2
    assert all(math.isfinite(v) for v in l2) and min(t2) > 0.2


def test_run_probe_end_to_end():
    """``run_probe`` with a 2 x 2 sweep on class-structured features against the twin with fp64
    accumulation, after the last epoch.  As in the trajectory test the kernels may be 4x as far
    from it as the twin's own fp32 accumulation is, measured on the final validation logits
    (``zgap``, a maximum over 500 x 4 x 10 values; the gap of a mean loss can cancel to nothing).
    A row's loss moves by at most twice its logit error, plus expf / logf and the sum of C terms
    as in the forward test.  Accuracy: 4x the twin's accuracy gap plus the share of rows whose
    top-2 margin is within 2 · 4 zgap, the only rows whose argmax can change.  Measured: zgap
    2e-6, val-loss distance 4e-7, accuracy distance 0."""
    from simclr_amd.evaluation.probes import DownstreamDataset, run_probe, sweep_eval
    from simclr_amd.models.heads import LinearClassifier
    ps = _ps()
    F, C = 64, 10
    Xtr, ytr, centers = _structured(2000, F, C, 21, noise=2.0)
    Xva, yva, _ = _structured(500, F, C, 22, centers, noise=2.0)
    lrs, decays = [0.05, 0.2], [0.0, 1e-4]
    cfg = {"parameter": {"epochs": 5, "momentum": 0.9, "linear_schedule": True, "seed": 7,
                         "sweep_lr": lrs, "sweep_decay": decays},
           "experiment": {"batches": 256, "lr": 0.1, "decay": 0.0}}
    torch.manual_seed(3)
    res = run_probe(cfg, "linear", DownstreamDataset(Xtr.to(DEV), ytr.to(DEV)),
                    DownstreamDataset(Xva.to(DEV), yva.to(DEV)), C, 5, torch.device(DEV))
    tw = {}
    for name, acc in (("32", torch.float32), ("64", torch.float64)):
        torch.manual_seed(3)
        tw[name] = sweep_eval(cfg, LinearClassifier(F, C), DownstreamDataset(Xtr, ytr),
                              DownstreamDataset(Xva, yva), lrs, decays, 5, seed=7, hip=False,
                              accumulate=acc)
    Xv = ps.prepare_features(Xva)
    idx = torch.arange(len(Xva))
    z32 = tw["32"][1].forward(Xv, yva, idx, train=False)["logits"].double()
    z64 = tw["64"][1].forward(Xv, yva, idx, train=False)["logits"].double()
    zgap = float((z32 - z64).abs().max())
    top2 = z64.topk(2, dim=2).values
    flip = ((top2[..., 0] - top2[..., 1]) <= 8 * zgap).double().mean(0)  # per configuration
    assert res["best"] in range(4) and len(res["sweep"]) == 4
    for g, entry in enumerate(res["sweep"]):
        r32, r64 = tw["32"][0][g], tw["64"][0][g]
        agap = max(abs(a - b) for a, b in zip(r32[3], r64[3]))
        d = abs(entry["val_losses"][-1] - r64[5][-1])
        da = abs(entry["val_accuracies"][-1] - r64[3][-1])
        ltol = 2 * 4 * zgap + (C + 16) * 2 * U * (1 + abs(r64[5][-1]))
        print(f"config {g}: zgap {zgap:.3e} val loss tol {ltol:.3e} got {d:.3e}; acc gap "
              f"{agap:.3e} flip share {float(flip[g]):.3e} got {da:.3e}")
        assert zgap > 0 and d <= ltol and len(entry["val_losses"]) == 5
        assert da <= 4 * agap + float(flip[g]) + 1e-12
    best32 = max(max(r[3]) for r in tw["32"][0])
    assert best32 > 0.2  # chance is 0.1
    assert res["highest_val_acc"] == res["sweep"][res["best"]]["highest_val_acc"]
