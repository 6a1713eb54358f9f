"""Downstream probes on frozen features: centroid, weighted k-NN, linear and nonlinear classifiers.

Parity: ``centroid_eval`` (``/root/reference/eval.py:61-85``), ``learnable_eval``
(eval.py:88-190) and the results-dict schema of eval.py:279-319:

* centroid: class-mean weights (unnormalised) · dot-product scores, top-1 / top-k accuracy;
* knn: the weighted k-nearest-neighbour classifier of Wu et al. (InstDisc), not in the reference:
  cosine neighbours in the train features, votes ``exp((sim - 1) / T)``; the train numbers are
  leave-one-out (``ops/knn.py`` holds the contract);
* kmeans / geometry: the label-free probes of ``ops/kmeans.py`` (spherical k-means scored against
  the labels) and ``ops/geometry.py`` (uniformity, alignment and the covariance spectrum), not in
  the reference; neither trains anything;
* linear / nonlinear: SGD(lr = lr·batches/256, momentum, **nesterov=True**, wd = decay),
  ``CosineAnnealingLR(T_max = epochs·ceil(N/batches))`` stepped every batch, shuffled batches;
  after every epoch train and val (top-1, top-k, mean CE) are recomputed; the JSON reports the
  per-epoch lists and ``lowest_val_loss``, ``highest_val_acc``, ``highest_val_top_k_acc``;
* linear with ``parameter.sweep_lr`` / ``parameter.sweep_decay`` (not in the reference): the grid
  of lr x weight decay trained in one pass (``sweep_eval``, contract in ``ops/probe_sweep.py``);
  the JSON holds one linear entry per configuration under ``sweep``, the ``best`` index and that
  entry's fields at the top level.

Fixed reference defects: ``top_k <= 1`` no longer accumulates cumulative top-1 counts (Q4), and
``NonLinearClassifier`` exists (Q1).  Features and labels stay on the device; batches are index
permutations (no per-batch host copies).
"""
from __future__ import annotations

import logging
import math
from dataclasses import dataclass
from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F

from ..models.heads import CentroidClassifier, LinearClassifier, NonLinearClassifier
from ..ops.classify import ce_rank, cross_entropy
from ..ops import geometry, kmeans, probe_sweep
from ..ops.knn import knn_topk, knn_vote
from ..utils.misc import cfg_get
from ..optim.schedule import cosine_lr

log = logging.getLogger(__name__)


@dataclass
class DownstreamDataset:
    """(data, targets) tensor dataset over extracted features (reference dataset.py:5-16)."""
    data: torch.Tensor
    targets: torch.Tensor

    def __post_init__(self):
        assert len(self.data) == len(self.targets)

    def __len__(self) -> int:
        return len(self.data)

    def __getitem__(self, i):
        return self.data[i], self.targets[i]


def _batches(n: int, bs: int, shuffle: bool, gen: torch.Generator, device):
    if shuffle:
        perm = torch.randperm(n, generator=gen).to(device)
    else:
        perm = torch.arange(n, device=device)
    for s in range(0, n, bs):
        yield perm[s:s + bs]


def _topk_correct(scores: torch.Tensor, y: torch.Tensor, top_k: int) -> Tuple[int, int]:
    """(top-1, top-k) correct counts: the target's rank (classes scoring above it) < k."""
    _, rank = ce_rank(scores, y)
    k = max(1, min(top_k, scores.shape[1]))
    return int((rank == 0).sum().item()), int((rank < k).sum().item())


@torch.no_grad()
def centroid_eval(ds: DownstreamDataset, classifier: CentroidClassifier, top_k: int = 5,
                  batch_size: int = 4096) -> Tuple[float, float]:
    _, c1, ck = _eval_counts(classifier, ds, top_k, batch_size, with_loss=False)
    return c1, ck


@torch.no_grad()
def knn_eval(bank: DownstreamDataset, query: DownstreamDataset, num_classes: int, k: int = 200,
             temperature: float = 0.1, top_k: int = 5, leave_one_out: bool = False,
             return_scores: bool = False):
    """(top-1, top-k) accuracy of the weighted k-NN vote of ``query`` against ``bank``.  With
    ``leave_one_out`` the queries are the bank itself and a row is never its own neighbour."""
    vals, idx = knn_topk(query.data, bank.data.to(query.data.device), k,
                         self_offset=0 if leave_one_out else None)
    scores, rank = knn_vote(vals, idx, bank.targets, num_classes, temperature, query.targets)
    kk = max(1, min(top_k, num_classes))
    n = max(1, len(query))
    c = torch.stack([(rank == 0).sum(), (rank < kk).sum()]).cpu().tolist()
    if return_scores:
        return c[0] / n, c[1] / n, scores
    return c[0] / n, c[1] / n


@torch.no_grad()
def kmeans_eval(cfg, train: DownstreamDataset, val: DownstreamDataset, num_classes: int) -> Dict:
    """Spherical k-means on the train features (``ops/kmeans.py`` holds the contract): R restarts
    in one pass, the best by objective scored against the labels on train and val (NMI, ARI, purity
    and the matched accuracy; val with the train matching)."""
    K = cfg_get(cfg, "parameter.kmeans_k", None)
    K = int(num_classes if K is None else K)
    R = int(cfg_get(cfg, "parameter.kmeans_restarts", 8))
    T = int(cfg_get(cfg, "parameter.kmeans_iters", 50))
    if sweep_values(cfg) is not None:
        raise ValueError("parameter.sweep_lr / parameter.sweep_decay need parameter.classifier=linear")
    fit = kmeans.kmeans_fit(train.data, K, R, T, seed=int(cfg_get(cfg, "parameter.seed", 0)))
    b = fit.best
    tr_table = kmeans.contingency(fit.a[b], train.targets, K, num_classes)
    va_a, _ = kmeans.kmeans_assign(val.data.to(train.data.device), fit.centroids[b])
    va_table = kmeans.contingency(va_a, val.targets, K, num_classes)
    match = kmeans.cluster_matching(tr_table)
    tr, va = kmeans.cluster_scores(tr_table, match), kmeans.cluster_scores(va_table, match)
    logging.info("train acc: {}, val acc: {}".format(tr["acc"], va["acc"]))
    n = max(1, len(train))
    out = {}
    for m in ("acc", "nmi", "ari", "purity"):
        out["train_" + m] = tr[m]
        out["val_" + m] = va[m]
    out.update({
        "kmeans_k": K,
        "kmeans_restarts": R,
        "kmeans_iters": T,
        "best": b,
        "objective": [float(j) / n for j in fit.objective.tolist()],
        "iterations": kmeans.iterations(fit.changed),
        "cluster_sizes": [int(c) for c in fit.counts[b].tolist()],
    })
    return out


@torch.no_grad()
def geometry_eval(cfg, train: DownstreamDataset, val: DownstreamDataset) -> Dict:
    """Uniformity / alignment and the covariance spectrum of the train and the val features
    (``ops/geometry.py`` holds the contract).  Nothing is trained and ``parameter.top_k`` is not
    used.  The metrics carry a ``train_`` / ``val_`` prefix, as do ``rows`` and ``nonfinite`` (the
    count of non-finite feature values: with any, the split's metrics may be NaN)."""
    t = cfg_get(cfg, "parameter.geometry_t", 2.0)
    try:
        geometry.check_limits(t=t)
    except ValueError as err:
        raise ValueError("parameter." + str(err)) from None
    if sweep_values(cfg) is not None:
        raise ValueError("parameter.sweep_lr / parameter.sweep_decay need parameter.classifier=linear")
    dev = train.data.device
    out = {"geometry_t": float(t), "dims": int(train.data.shape[1])}
    for name, ds in (("train", train), ("val", val)):
        x = ds.data.to(dev)
        sums = geometry.pair_stats(x, ds.targets, float(t))
        spec = geometry.spectrum(x)
        m = dict(geometry.pair_metrics(sums), **geometry.spectrum_metrics(spec.eig, spec.cov_diag))
        m["rows"] = int(x.shape[0])
        m["nonfinite"] = int((~torch.isfinite(x)).sum())
        logging.info("{} uniformity: {}, alignment: {}, effective rank: {}".format(
            name, m["uniformity"], m["class_alignment"], m["effective_rank"]))
        out.update({name + "_" + k: v for k, v in m.items()})
    return out


def _eval_counts(classifier, ds: DownstreamDataset, top_k: int, batch_size: int,
                 with_loss: bool = True) -> Tuple[float, float, float]:
    """Mean CE, top-1 and top-k accuracy over ``ds``, accumulated on the device (one host sync
    per call instead of three per batch, reference eval.py:104-136)."""
    n = len(ds)
    k = None
    acc = None
    for s in range(0, n, batch_size):
        x = ds.data[s:s + batch_size]
        y = ds.targets[s:s + batch_size].to(x.device)
        out = classifier(x).float()
        if k is None:
            k = max(1, min(top_k, out.shape[1]))
            acc = torch.zeros(3, dtype=torch.float64, device=out.device)
        loss, rank = ce_rank(out, y)
        acc[0] += loss.double().sum() if with_loss else 0.0
        acc[1] += (rank == 0).sum()
        acc[2] += (rank < k).sum()
    a = acc.cpu().tolist() if acc is not None else [0.0, 0.0, 0.0]
    return a[0] / n, a[1] / n, a[2] / n


@torch.no_grad()
def accuracies_loss(classifier, ds: DownstreamDataset, top_k: int = 5,
                    batch_size: int = 4096) -> Tuple[float, float, float]:
    classifier.eval()
    loss, c1, ck = _eval_counts(classifier, ds, top_k, batch_size)
    return c1, ck, loss


def learnable_eval(cfg, classifier, train: DownstreamDataset, val: DownstreamDataset,
                   top_k: int = 5, seed: int = 0) -> Tuple[List[float], ...]:
    p, e = cfg["parameter"], cfg["experiment"]
    epochs = p["epochs"]
    bs = e["batches"]
    n = len(train)
    total_steps = epochs * int(math.ceil(n / bs))
    if p["linear_schedule"]:
        lr0 = e["lr"] * bs / 256.0
    else:
        lr0 = e["lr"] * math.sqrt(bs)
    opt = torch.optim.SGD(classifier.parameters(), lr=lr0, momentum=p["momentum"], nesterov=True,
                          weight_decay=e["decay"])
    gen = torch.Generator()
    gen.manual_seed(seed)
    step = 0
    tr_acc, tr_topk, tr_loss, va_acc, va_topk, va_loss = [], [], [], [], [], []
    dev = train.data.device
    for epoch in range(1, epochs + 1):
        classifier.train()
        sum_loss = 0.0
        for idx in _batches(n, bs, True, gen, dev):
            for g in opt.param_groups:
                g["lr"] = cosine_lr(step, lr0, total_steps)
            x = train.data[idx]
            y = train.targets[idx].to(dev)
            opt.zero_grad()
            out = classifier(x).float()
            loss = cross_entropy(out, y)
            loss.backward()
            opt.step()
            step += 1
            sum_loss = sum_loss + loss.detach() * len(y)  # device-side: no sync per batch
        logging.info("Epoch:{}/{} progress:{:.3f} loss:{:.3f}, lr:{:.7f}".format(
            epoch, epochs, epoch / epochs, float(sum_loss) / n, cosine_lr(step, lr0, total_steps)))
        a, b, c = accuracies_loss(classifier, train, top_k)
        tr_acc.append(a)
        tr_topk.append(b)
        tr_loss.append(c)
        a, b, c = accuracies_loss(classifier, val, top_k)
        va_acc.append(a)
        va_topk.append(b)
        va_loss.append(c)
    return tr_acc, tr_topk, tr_loss, va_acc, va_topk, va_loss


def sweep_values(cfg) -> Tuple[List[float], List[float]] | None:
    """(lrs, decays) of ``parameter.sweep_lr`` / ``parameter.sweep_decay``, an unset key meaning the
    one value of ``experiment.lr`` / ``experiment.decay``; ``None`` without either key."""
    lrs, decays = cfg_get(cfg, "parameter.sweep_lr", None), cfg_get(cfg, "parameter.sweep_decay", None)
    if lrs is None and decays is None:
        return None
    e = cfg["experiment"]
    return ([float(v) for v in lrs] if lrs is not None else [float(e["lr"])],
            [float(v) for v in decays] if decays is not None else [float(e["decay"])])


@torch.no_grad()
def sweep_eval(cfg, classifier: LinearClassifier, train: DownstreamDataset, val: DownstreamDataset,
               lrs: List[float], decays: List[float], top_k: int = 5, seed: int = 0,
               round_operands: bool = True, accumulate: torch.dtype = torch.float32,
               hip: bool | None = None):
    """``learnable_eval`` for the grid ``lrs`` x ``decays`` in one pass over the shuffled features
    (``ops/probe_sweep.py`` holds the contract).  Every configuration starts from ``classifier``'s
    weights and sees the batches an unswept run with the same seed sees.  Returns (one
    ``learnable_eval`` tuple per configuration, decay-major and lr-minor; the ``LinearSweep``)."""
    p, e = cfg["parameter"], cfg["experiment"]
    epochs, bs, n = p["epochs"], e["batches"], len(train)
    configs = probe_sweep.grid(lrs, decays)
    lin = classifier.classifier
    probe_sweep.check_limits(len(configs), lin.out_features, lin.in_features, bs)
    total_steps = epochs * int(math.ceil(n / bs))
    dev = train.data.device
    lr0 = probe_sweep.initial_lrs([c[0] for c in configs], bs, bool(p["linear_schedule"]))
    sweep = probe_sweep.LinearSweep(lin.weight, lin.bias, lr0, [c[1] for c in configs],
                                    p["momentum"], probe_sweep.cosine_table(total_steps),
                                    device=dev, round_operands=round_operands,
                                    accumulate=accumulate, hip=hip)
    Xtr = probe_sweep.prepare_features(train.data, round_operands)
    Xva = probe_sweep.prepare_features(val.data.to(dev), round_operands)
    ytr = train.targets.to(device=dev, dtype=torch.long).contiguous()
    yva = val.targets.to(device=dev, dtype=torch.long).contiguous()
    gen = torch.Generator()
    gen.manual_seed(seed)
    G = len(configs)
    out = [([], [], [], [], [], []) for _ in range(G)]
    losses = torch.empty(G, n, device=dev, dtype=torch.float32)
    for epoch in range(1, epochs + 1):
        pos = 0
        for idx in _batches(n, bs, True, gen, dev):
            sweep.train_step(Xtr, ytr, idx, losses, pos)
            pos += len(idx)
        mean = (losses.double().sum(1) / n).cpu().tolist()
        logging.info("Epoch:{}/{} progress:{:.3f} loss:[{}]".format(
            epoch, epochs, epoch / epochs, ", ".join("{:.3f}".format(v) for v in mean)))
        tl, t1, tk = sweep.evaluate(Xtr, ytr, top_k)
        vl, v1, vk = sweep.evaluate(Xva, yva, top_k)
        for g in range(G):
            for lst, v in zip(out[g], (t1[g], tk[g], tl[g], v1[g], vk[g], vl[g])):
                lst.append(v)
    return out, sweep


def _nanmin(v: List[float]) -> float:
    ok = [x for x in v if x == x]
    return min(ok) if ok else float("nan")


def _linear_result(t, top_k: int) -> Dict:
    tr_acc, tr_topk, tr_loss, va_acc, va_topk, va_loss = t
    return {
        "train_accuracies": tr_acc,
        "val_accuracies": va_acc,
        "train_losses": tr_loss,
        "val_losses": va_loss,
        "train_top_{}_accuracies".format(top_k): tr_topk,
        "val_top_{}_accuracies".format(top_k): va_topk,
        "lowest_val_loss": _nanmin(va_loss),
        "highest_val_acc": max(va_acc),
        "highest_val_top_k_acc": max(va_topk),
    }


def run_probe(cfg, kind: str, train: DownstreamDataset, val: DownstreamDataset, num_classes: int,
              top_k: int, device) -> Dict:
    if kind == "centroid":
        clf = CentroidClassifier(CentroidClassifier.create_weights(train, num_classes).to(device))
        train_acc, train_topk = centroid_eval(train, clf, top_k)
        val_acc, val_topk = centroid_eval(val, clf, top_k)
        logging.info("train acc: {}, val acc: {}".format(train_acc, val_acc))
        return {
            "train_acc": train_acc,
            "train_top_{}_acc".format(top_k): train_topk,
            "val_acc": val_acc,
            "val_top_{}_acc".format(top_k): val_topk,
        }
    if kind == "knn":
        k = int(cfg_get(cfg, "parameter.knn_k", 200))
        t = float(cfg_get(cfg, "parameter.knn_t", 0.1))
        train_acc, train_topk = knn_eval(train, train, num_classes, k, t, top_k, leave_one_out=True)
        val_acc, val_topk = knn_eval(train, val, num_classes, k, t, top_k)
        logging.info("train acc: {}, val acc: {}".format(train_acc, val_acc))
        return {
            "train_acc": train_acc,
            "train_top_{}_acc".format(top_k): train_topk,
            "val_acc": val_acc,
            "val_top_{}_acc".format(top_k): val_topk,
            "knn_k": k,
            "knn_t": t,
        }
    if kind == "kmeans":
        return kmeans_eval(cfg, train, val, num_classes)
    if kind == "geometry":
        return geometry_eval(cfg, train, val)
    F_ = train.data.shape[1]
    if kind == "linear":
        clf = LinearClassifier(F_, num_classes).to(device)
    elif kind.replace("-", "") == "nonlinear":
        clf = NonLinearClassifier(F_, num_classes).to(device)
    else:
        raise ValueError(f"unknown classifier {kind!r} "
                         "(centroid | knn | kmeans | geometry | linear | nonlinear)")
    sv = sweep_values(cfg)
    if sv is not None:
        if kind != "linear":
            raise ValueError("parameter.sweep_lr / parameter.sweep_decay need parameter.classifier=linear")
        per_cfg, _ = sweep_eval(cfg, clf, train, val, sv[0], sv[1], top_k,
                                seed=cfg["parameter"]["seed"])
        entries = []
        for (lr, decay), t in zip(probe_sweep.grid(*sv), per_cfg):
            entries.append(dict(_linear_result(t, top_k), lr=lr, decay=decay))
        best = max(range(len(entries)), key=lambda i: (entries[i]["highest_val_acc"], -i))
        logging.info("sweep best: lr {} decay {} val acc {}".format(
            entries[best]["lr"], entries[best]["decay"], entries[best]["highest_val_acc"]))
        return dict(entries[best], sweep=entries, best=best)
    tr_acc, tr_topk, tr_loss, va_acc, va_topk, va_loss = learnable_eval(
        cfg, clf, train, val, top_k, seed=cfg["parameter"]["seed"])
    logging.info("train acc: {}, val acc: {}".format(max(tr_acc), max(va_acc)))
    return {
        "train_accuracies": tr_acc,
        "val_accuracies": va_acc,
        "train_losses": tr_loss,
        "val_losses": va_loss,
        "train_top_{}_accuracies".format(top_k): tr_topk,
        "val_top_{}_accuracies".format(top_k): va_topk,
        "lowest_val_loss": min(va_loss),
        "highest_val_acc": max(va_acc),
        "highest_val_top_k_acc": max(va_topk),
    }
