"""Per-entry-point config validation (``check_hydra_conf`` of the reference scripts,
SURVEY C4): main.py:39-50, eval.py:20-28 (momentum strictly > 0), save_features.py:15-17,
supervised.py:18-27.  Raises ``AssertionError`` with the failing key (the reference asserts)."""
from __future__ import annotations


def _check(cond: bool, msg: str) -> None:
    if not cond:
        raise AssertionError(msg)


def _check_blur(cfg) -> None:
    """The opt-in ``data.blur_kernel``: 0 (derive from the output size) or odd within the
    augmentation op's limits (``data.augment_ref.MAX_BLUR_KERNEL``)."""
    from ..data.augment_ref import MAX_BLUR_KERNEL
    data = cfg.get("data") if hasattr(cfg, "get") else None
    ks = (data or {}).get("blur_kernel")
    if ks is None:
        return
    _check(isinstance(ks, int) and not isinstance(ks, bool), "data.blur_kernel must be an integer")
    _check(ks >= 0, "data.blur_kernel must be >= 0")
    _check(ks == 0 or (ks % 2 == 1 and ks >= 3), "data.blur_kernel must be 0 or odd and >= 3")
    _check(ks <= MAX_BLUR_KERNEL, f"data.blur_kernel must be <= {MAX_BLUR_KERNEL}")


def _check_supervised(cfg) -> None:
    """The opt-in ``loss.supervised`` (SupCon, loss/ntxent.py): a boolean; not with the ring."""
    loss = (cfg.get("loss") if hasattr(cfg, "get") else None) or {}
    sup = loss.get("supervised")
    if sup is None:
        return
    _check(isinstance(sup, bool), "loss.supervised must be a boolean")
    _check(not (sup and str(loss.get("gather")).lower() == "ring"),
           "loss.supervised=true is not available with loss.gather=ring")


def _check_negatives(cfg) -> None:
    """The opt-in weighted negatives of NT-Xent (loss/ntxent.py): ``loss.hard_beta`` >= 0,
    ``loss.tau_plus`` in [0, 1), ``loss.decoupled`` a boolean.  A loss with any of them off its
    default is NT-Xent's only: not with ``loss.kind`` barlow / nnclr, ``loss.supervised`` or the
    ring (``loss.gather=true`` is fine)."""
    import math
    loss = (cfg.get("loss") if hasattr(cfg, "get") else None) or {}
    beta, tau_plus, dec = loss.get("hard_beta"), loss.get("tau_plus"), loss.get("decoupled")
    for key, v in (("loss.hard_beta", beta), ("loss.tau_plus", tau_plus)):
        if v is not None:
            _check(isinstance(v, (int, float)) and not isinstance(v, bool),
                   f"{key} must be a number")
            _check(math.isfinite(v), f"{key} must be finite")
    _check(beta is None or beta >= 0, "loss.hard_beta must be >= 0")
    _check(tau_plus is None or 0 <= tau_plus < 1, "loss.tau_plus must be in [0, 1)")
    _check(dec is None or isinstance(dec, bool), "loss.decoupled must be a boolean")
    on = [k for k, v in (("loss.hard_beta", beta), ("loss.tau_plus", tau_plus),
                         ("loss.decoupled", dec)) if v]
    if not on:
        return
    kind = loss.get("kind")
    _check(kind in (None, "ntxent"), f"{on[0]} is not available with loss.kind={kind}")
    _check(not loss.get("supervised"), f"{on[0]} is not available with loss.supervised=true")
    _check(str(loss.get("gather")).lower() != "ring",
           f"{on[0]} is not available with loss.gather=ring")


LOSS_KINDS = ("ntxent", "barlow", "nnclr")
NN_QUEUE_DEFAULT = 16384
NN_QUEUE_MULTIPLE, NN_QUEUE_MAX = 256, 131072


def _check_nnclr(cfg, loss, kind) -> None:
    """``loss.kind=nnclr`` (loss/nnclr.py: per rank, no labels, no gather) and its support-set
    size ``loss.nn_queue``: a multiple of 256 in [256, 131072], at least ``experiment.batches``;
    the key is valid with ``nnclr`` only."""
    q = loss.get("nn_queue")
    if q is not None:
        _check(kind == "nnclr", "loss.nn_queue needs loss.kind=nnclr")
        _check(isinstance(q, int) and not isinstance(q, bool), "loss.nn_queue must be an integer")
        _check(NN_QUEUE_MULTIPLE <= q <= NN_QUEUE_MAX and q % NN_QUEUE_MULTIPLE == 0,
               f"loss.nn_queue must be a multiple of {NN_QUEUE_MULTIPLE} in "
               f"[{NN_QUEUE_MULTIPLE}, {NN_QUEUE_MAX}]")
    if kind != "nnclr":
        return
    _check(not loss.get("supervised"),
           "loss.kind=nnclr is not available with loss.supervised=true")
    _check(loss.get("gather") in (None, False),
           "loss.kind=nnclr is not available with loss.gather (the loss is per rank)")
    _check(not loss.get("barlow_global"),
           "loss.kind=nnclr is not available with loss.barlow_global=true")
    batches = cfg["experiment"]["batches"]
    _check((NN_QUEUE_DEFAULT if q is None else q) >= batches,
           f"loss.nn_queue must be at least experiment.batches ({batches})")


def _check_loss_kind(cfg) -> None:
    """The opt-in ``loss.kind`` (``ntxent`` | ``barlow``, loss/barlow.py | ``nnclr``,
    loss/nnclr.py) and ``loss.barlow_lambda``; Barlow Twins has no labels and is per rank unless
    ``loss.barlow_global`` (a boolean, only with ``barlow``) asks for the loss over all ranks."""
    loss = (cfg.get("loss") if hasattr(cfg, "get") else None) or {}
    kind = loss.get("kind")
    _check(kind is None or (isinstance(kind, str) and kind in LOSS_KINDS),
           f"loss.kind must be one of {', '.join(LOSS_KINDS)}")
    lam = loss.get("barlow_lambda")
    if lam is not None:
        _check(isinstance(lam, (int, float)) and not isinstance(lam, bool),
               "loss.barlow_lambda must be a number")
        _check(lam > 0.0, "loss.barlow_lambda must be > 0")
    glob = loss.get("barlow_global")
    if glob is not None:
        _check(isinstance(glob, bool), "loss.barlow_global must be a boolean")
        _check(not glob or kind == "barlow", "loss.barlow_global=true needs loss.kind=barlow")
    if kind == "barlow":
        _check(not loss.get("supervised"),
               "loss.kind=barlow is not available with loss.supervised=true")
        _check(loss.get("gather") in (None, False),
               "loss.kind=barlow is not available with loss.gather (the loss is per rank)")
    _check_nnclr(cfg, loss, kind)


def _check_online_probe(cfg) -> None:
    """The opt-in ``online_probe`` group (ops/online_probe.py): a linear classifier trained on
    the encoder output inside the pre-training step."""
    from ..ops import online_probe
    conf = (cfg.get("online_probe") if hasattr(cfg, "get") else None) or {}
    try:
        online_probe.validate(conf)
    except ValueError as err:
        raise AssertionError(str(err)) from None


def check_pretrain_conf(cfg) -> None:
    p, e = cfg["parameter"], cfg["experiment"]
    _check_blur(cfg)
    _check_supervised(cfg)
    _check_loss_kind(cfg)
    _check_negatives(cfg)
    _check_online_probe(cfg)
    _check(p["temperature"] > 0.0, "parameter.temperature must be > 0")
    _check(p["epochs"] > 0, "parameter.epochs must be > 0")
    _check(e["batches"] > 0, "experiment.batches must be > 0")
    _check(1.0 > p["momentum"] >= 0, "parameter.momentum must be in [0, 1)")
    _check(p["warmup_epochs"] >= 0, "parameter.warmup_epochs must be >= 0")
    _check(p["d"] > 0, "parameter.d must be > 0")
    _check(e["base_cnn"] in {"resnet18", "resnet50"}, "experiment.base_cnn must be resnet18/50")
    _check(e["lr"] > 0.0, "experiment.lr must be > 0")
    _check(e["strength"] > 0.0, "experiment.strength must be > 0")
    _check(e["decay"] >= 0.0, "experiment.decay must be >= 0")


def _check_sweep(cfg) -> None:
    """The opt-in ``parameter.sweep_lr`` / ``parameter.sweep_decay`` lists of the linear probe,
    within the sweep op's limits (``ops.probe_sweep.check_limits``)."""
    from ..ops import probe_sweep
    p, e = cfg["parameter"], cfg["experiment"]
    lrs, decays = p.get("sweep_lr"), p.get("sweep_decay")
    if lrs is None and decays is None:
        return
    _check(p.get("classifier") == "linear",
           "parameter.sweep_lr / parameter.sweep_decay need parameter.classifier=linear")
    for key, vals in (("parameter.sweep_lr", lrs), ("parameter.sweep_decay", decays)):
        if vals is None:
            continue
        _check(isinstance(vals, (list, tuple)) and len(vals) > 0,
               f"{key} must be a non-empty list")
        _check(all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in vals),
               f"{key} must hold numbers")
    _check(lrs is None or all(v > 0.0 for v in lrs), "parameter.sweep_lr: every lr must be > 0")
    _check(decays is None or all(v >= 0.0 for v in decays),
           "parameter.sweep_decay: every decay must be >= 0")
    G = len(lrs or [0]) * len(decays or [0])
    classes = {"cifar10": 10, "cifar100": 100}.get(e.get("name"))
    try:
        probe_sweep.check_limits(G, classes, None, e["batches"])
    except ValueError as err:
        raise AssertionError(str(err)) from None


def check_eval_conf(cfg) -> None:
    p, e = cfg["parameter"], cfg["experiment"]
    _check_sweep(cfg)
    _check(p["epochs"] > 0, "parameter.epochs must be > 0")
    _check(e["batches"] > 0, "experiment.batches must be > 0")
    _check(1.0 > p["momentum"] > 0.0, "parameter.momentum must be in (0, 1)")
    _check(p["warmup_epochs"] >= 0, "parameter.warmup_epochs must be >= 0")
    _check(e["base_cnn"] in {"resnet18", "resnet50"}, "experiment.base_cnn must be resnet18/50")
    _check(e["lr"] > 0.0, "experiment.lr must be > 0")
    _check(e["decay"] >= 0.0, "experiment.decay must be >= 0")
    if p.get("classifier") == "knn":
        k, t = p.get("knn_k"), p.get("knn_t")
        _check(k is None or k >= 1, "parameter.knn_k must be >= 1")
        _check(t is None or t > 0.0, "parameter.knn_t must be > 0")
    if p.get("classifier") == "kmeans":
        _check_kmeans(cfg)
    if p.get("classifier") == "geometry":
        _check_geometry(cfg)


def _check_kmeans(cfg) -> None:
    """The ``parameter.kmeans_*`` keys of the k-means probe, within the op's limits
    (``ops.kmeans.check_limits``); an unset ``kmeans_k`` is the data set's class count."""
    from ..ops import kmeans
    p, e = cfg["parameter"], cfg["experiment"]
    _check(p.get("sweep_lr") is None and p.get("sweep_decay") is None,
           "parameter.sweep_lr / parameter.sweep_decay need parameter.classifier=linear")
    K = p.get("kmeans_k")
    if K is None:
        K = {"cifar10": 10, "cifar100": 100}.get(e.get("name"))
    R, T = p.get("kmeans_restarts"), p.get("kmeans_iters")
    try:
        kmeans.check_limits(K, 8 if R is None else R, 50 if T is None else T)
    except ValueError as err:
        raise AssertionError("parameter." + str(err)) from None


def _check_geometry(cfg) -> None:
    """The geometry probe's one key ``parameter.geometry_t`` (the uniformity temperature, a finite
    number > 0; ``ops.geometry.check_limits``); nothing is swept."""
    from ..ops import geometry
    p = cfg["parameter"]
    _check(p.get("sweep_lr") is None and p.get("sweep_decay") is None,
           "parameter.sweep_lr / parameter.sweep_decay need parameter.classifier=linear")
    t = p.get("geometry_t")
    try:
        geometry.check_limits(t=t)
    except ValueError as err:
        raise AssertionError("parameter." + str(err)) from None


def check_save_features_conf(cfg) -> None:
    _check(cfg["parameter"]["epochs"] > 0, "parameter.epochs must be > 0")
    _check(cfg["experiment"]["base_cnn"] in {"resnet18", "resnet50"},
           "experiment.base_cnn must be resnet18/50")


def check_supervised_conf(cfg) -> None:
    p, e = cfg["parameter"], cfg["experiment"]
    _check_blur(cfg)
    _check(p["epochs"] > 0, "parameter.epochs must be > 0")
    _check(e["batches"] > 0, "experiment.batches must be > 0")
    _check(1.0 > p["momentum"] >= 0, "parameter.momentum must be in [0, 1)")
    _check(p["warmup_epochs"] >= 0, "parameter.warmup_epochs must be >= 0")
    _check(e["base_cnn"] in {"resnet18", "resnet50"}, "experiment.base_cnn must be resnet18/50")
    _check(e["lr"] > 0.0, "experiment.lr must be > 0")
    _check(e["strength"] > 0.0, "experiment.strength must be > 0")
    _check(e["decay"] >= 0.0, "experiment.decay must be >= 0")
