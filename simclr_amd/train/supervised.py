"""Supervised baseline (the ``supervised`` entry point).

Reference: ``/root/reference/supervised.py``: SupervisedModel (same backbone
surgery, ``fc = Linear(H, classes)``) + SyncBN + DDP, trained on SimCLR-augmented single views
with cross entropy, ``SGD(all params, momentum, weight_decay=decay)`` wrapped in LARC, the same
warmup + cosine schedule as pre-training; every epoch a distributed validation (Σ CE and Σ
correct reduced to rank 0), log line ``... val loss:{:.3f}, val acc:{:.2f}%`` and a "best"
checkpoint by ``parameter.metric`` (loss or 1 − acc).

Fixed defect Q14: the reference never updates ``best_metric``, so it rewrote the checkpoint
every epoch; here the best value is tracked and only improvements are saved (the previous best
file is removed, as the reference intends).
"""
from __future__ import annotations

import logging
import os
import time

import torch
import torch.distributed as dist

from ..comm.ipc import StepGuard
from ..config import check_supervised_conf
from ..data.datasets import load_dataset
from ..data.loader import ContrastiveLoader, blur_kernel_from_cfg
from ..models.contrastive import SupervisedModel
from ..ops import registry
from ..ops.classify import ce_rank, cross_entropy
from ..optim.lars import FusedLARS
from ..optim.schedule import MODE_WARMUP_COSINE, calculate_initial_lr
from ..parallel.flat import FlatParamStore
from ..parallel.invariant import require_replicas
from ..runtime.dist import init_distributed
from ..utils.checkpoint import checkpoint_name, save_reference_checkpoint
from ..utils.misc import MetricsWriter, cfg_get, refuse_experiment_knobs, seed_everything

log = logging.getLogger(__name__)


def _prep(x, precision, device):
    if precision == "bf16" and device.type == "cuda":
        return x
    x = x.float()
    return (x[:, :3] if x.shape[1] != 3 else x).contiguous()


@torch.no_grad()
def validation(model, loader, precision, device):
    model.eval()
    sum_loss = torch.zeros(1, device=device, dtype=torch.float64)
    correct = torch.zeros(1, device=device, dtype=torch.float64)
    for x, y in loader:
        out = model(_prep(x, precision, device)).float()
        # one HIP kernel (csrc/eval.hip ce_topk) gives per-row CE and the target's rank;
        # rank 0 <=> argmax == y (ties to the lower class, as argmax)
        loss, rank = ce_rank(out, y)
        sum_loss += loss.sum().double()
        correct += (rank == 0).sum().double()
    model.train()
    return sum_loss, correct


def supervised(cfg) -> dict:
    refuse_experiment_knobs("supervised")
    check_supervised_conf(cfg)
    st = init_distributed(cfg, use_cuda=cfg["parameter"].get("use_cuda", True))
    registry.set_backend(cfg_get(cfg, "runtime.backend", "auto"))
    seed = cfg["parameter"]["seed"]
    seed_everything(seed)
    dev = st.device
    precision = cfg_get(cfg, "runtime.precision", "bf16") if dev.type == "cuda" else "fp32"
    logging.info("Using {}".format(dev))
    kw = dict(root=cfg_get(cfg, "data.root", "~/pytorch_datasets"),
              synthetic=bool(cfg_get(cfg, "data.synthetic", False)),
              allow_synthetic_fallback=bool(cfg_get(cfg, "data.synthetic_fallback", False)),
              synthetic_noise=float(cfg_get(cfg, "data.synthetic_noise", 25.0)),
              synthetic_colour=bool(cfg_get(cfg, "data.synthetic_colour", True)),
              synthetic_kind=str(cfg_get(cfg, "data.synthetic_kind", "template")),
              seed=seed)
    size = cfg_get(cfg, "data.synthetic_size", None)
    train_ds = load_dataset(cfg["experiment"]["name"], train=True, synthetic_size=size, **kw)
    val_ds = load_dataset(cfg["experiment"]["name"], train=False,
                          synthetic_size=(max(1, size // 5) if size else None), **kw)
    bs = cfg["experiment"]["batches"]
    train_loader = ContrastiveLoader(train_ds, bs, dev, rank=st.rank, world=st.world_size,
                                     strength=cfg["experiment"]["strength"], seed=seed, views=1,
                                     blur_kernel=blur_kernel_from_cfg(cfg,
                                                                      train_ds.images.shape[1]))
    val_loader = ContrastiveLoader(val_ds, bs, dev, rank=st.rank, world=st.world_size, views=1,
                                   augment=False, shuffle=False, drop_last=False)
    model = SupervisedModel(cfg["experiment"]["base_cnn"], num_classes=train_ds.num_classes,
                            cifar_stem=cfg_get(cfg, "model.cifar_stem", None),
                            stem_padding=cfg_get(cfg, "model.stem_padding", 3)).to(dev)
    store = FlatParamStore(model, dev,
                           shadow_dtype=torch.bfloat16 if precision == "bf16" and dev.type == "cuda"
                           else None, bucket_mb=cfg_get(cfg, "runtime.bucket_mb", 32.0),
                           last_bucket_mb=cfg_get(cfg, "runtime.last_bucket_mb", 2.0))
    store.broadcast_from(0)
    store.defer_side_join = True  # every step ends with store.finish() before the optimizer
    steps_per_epoch = max(1, int(len(train_ds) / (bs * st.world_size)))
    epochs = cfg["parameter"]["epochs"]
    total, warm = epochs * steps_per_epoch, cfg["parameter"]["warmup_epochs"] * steps_per_epoch
    # reference: weight decay on ALL parameters (supervised.py:87-93)
    opt = FusedLARS(store, [cfg["experiment"]["decay"]] * len(store.params),
                    lr0=calculate_initial_lr(cfg), momentum=cfg["parameter"]["momentum"],
                    schedule_mode=MODE_WARMUP_COSINE, warmup_steps=warm, total_steps=total)
    hip = dev.type == "cuda" and precision == "bf16" and registry.use_hip(store.master)
    metric_kind = cfg["parameter"]["metric"]
    best = float("inf")
    best_file = None
    max_steps = cfg_get(cfg, "runtime.max_steps", None)
    metrics = MetricsWriter("metrics.jsonl" if st.rank == 0 else None)
    step = 0
    loss = torch.zeros(())
    summary = {}
    model.train()
    guard = StepGuard(st)  # RCCL statistics while tuning, per-step IPC error check

    def train_step(x, y):
        out = model(_prep(x, precision, dev)).float()
        loss = cross_entropy(out, y)  # HIP CE kernel: the forward also writes the gradient
        if not hip:
            store.zero_grad()
        loss.backward()
        store.finish()
        opt.step()
        return loss

    for epoch in range(1, epochs + 1):
        train_loader.set_epoch(epoch)
        t0 = time.time()
        for x, y in train_loader:
            loss = guard.run(train_step, x, y)
            step += 1
            guard.check(step)
            if max_steps is not None and step >= max_steps:
                break
        guard.flush(step)  # the epoch's last flag copy
        line = None
        if st.rank == 0:
            line = "Epoch:{}/{} progress:{:.3f} loss:{:.3f}, lr:{:.7f}".format(
                epoch, epochs, epoch / epochs, float(loss.item()), opt.logged_lr)
        sum_loss, correct = validation(model, val_loader, precision, dev)
        if st.world_size > 1:
            # every rank must still hold bitwise the same replicated state (ReplicaDivergence)
            require_replicas(store, opt, model, group=st.group, where=f"after epoch {epoch}")
            dist.barrier()
            dist.reduce(sum_loss, dst=0)
            dist.reduce(correct, dst=0)
        if st.rank == 0:
            n_val = len(val_ds)
            vloss = float(sum_loss.item()) / n_val
            vacc = float(correct.item()) / n_val
            logging.info(line + " val loss:{:.3f}, val acc:{:.2f}%".format(vloss, vacc * 100.0))
            metrics.write(epoch=epoch, step=step, val_loss=vloss, val_acc=vacc,
                          seconds=time.time() - t0)
            metric = vloss if metric_kind == "loss" else 1.0 - vacc
            summary.update(val_loss=vloss, val_acc=vacc, epoch=epoch)
            if metric <= best:
                best = metric
                if best_file is not None and os.path.exists(best_file):
                    os.remove(best_file)
                best_file = checkpoint_name(epoch, cfg["experiment"]["output_model_name"])
                save_reference_checkpoint(model, best_file)
                summary["best_checkpoint"] = best_file
        if st.world_size > 1:
            # nobody starts the next epoch's first statistics exchange while rank 0 is still
            # saving (a multi-second save would exceed the IPC exchange's spin bound)
            dist.barrier()
        if max_steps is not None and step >= max_steps:
            break
    metrics.close()
    return summary
