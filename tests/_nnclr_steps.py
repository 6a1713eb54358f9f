"""Five NNCLR training steps of ResNet-18 (CIFAR stem, batch 32 at 32x32, synthetic data,
deterministic tiles; n 32, D 128, Q 256: the loss kernels' path, the support set written 160
rows deep), eager throughout (``eager``) or captured after the second step and replayed by
hipGraphLaunch (``graph``) or by the multi-stream executor (``streams``): losses, master
weights, momentum, BatchNorm buffers, the support set and its cursor go to a file for
tests/test_gpu_nnclr.py, which runs each mode in a process of its own.  ``off`` / ``ntxent``:
the same five eager steps without ``loss.kind`` / with ``loss.kind=ntxent`` (no NNCLR object
may exist and no ``nc_*`` op may run).

Usage: python tests/_nnclr_steps.py {eager|graph|streams|off|ntxent} OUT.pt
"""
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def _no_twin(*a, **k):
    raise AssertionError("the step fell back to the torch twin")


def main(mode: str, out: str) -> None:
    from simclr_amd.config import compose, task_config, CONF_DIR
    from simclr_amd.data.datasets import synthetic_dataset
    from simclr_amd.data.loader import ContrastiveLoader
    from simclr_amd.loss import nnclr
    from simclr_amd.ops import tuning
    from simclr_amd.parallel import state as pstate
    from simclr_amd.train.pretrain import Trainer
    from simclr_amd.utils.misc import seed_everything
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    on = mode in ("eager", "graph", "streams")
    kind = {"off": [], "ntxent": ["loss.kind=ntxent"]}.get(
        mode, ["loss.kind=nnclr", "loss.nn_queue=256"])
    cfg = task_config(compose(str(CONF_DIR), "config", [
        "experiment.base_cnn=resnet18", "model.cifar_stem=true", "experiment.batches=32",
        "data.synthetic=true", *kind, "runtime.deterministic=true",
        "parameter.epochs=10", "parameter.warmup_epochs=1"]))
    seed_everything(7, deterministic=True)
    tuning.set_enabled(False)
    pstate.reset()
    st = pstate.get()
    st.device = dev
    tr = Trainer(cfg, st, 512, precision="bf16")
    assert tr.hip and isinstance(tr.loss_fn, nnclr.NNCLR) == on
    nnclr.nnclr_torch = _no_twin
    if not on:
        nnclr._NNCLRHipFn.forward = staticmethod(_no_twin)
    ds = synthetic_dataset(256, 10)
    loader = ContrastiveLoader(ds, 32, dev, seed=7)
    losses, replayed = [], 0
    for i, (x, _) in enumerate(loader):
        if i == 5:
            break
        if mode in ("graph", "streams") and i == 2:
            tr.capture(x, warmup=0)
            assert mode == "graph" or tr.sreplay is not None
            tr.replay_mode = mode
            loader.out = tr._static_x
        replayed += int(tr.graph is not None)
        losses.append(tr.step(x).clone())
    torch.cuda.synchronize()
    res = {"losses": torch.stack(losses).cpu(), "master": tr.store.master.cpu(),
           "momentum": tr.opt.mom.cpu(),
           "buffers": {k: v.cpu() for k, v in tr.model.named_buffers()},
           "replayed": replayed, "mode": tr.replay_mode}
    if on:
        res["queue"] = tr.loss_fn.queue.cpu()
        res["cursor"] = tr.loss_fn.cursor.cpu()
    torch.save(res, out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
