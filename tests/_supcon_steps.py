"""Five SupCon training steps of ResNet-18 (CIFAR stem, batch 32 at 32x32, synthetic data with
labels, deterministic tiles), eager throughout (``eager``) or captured after the second step
and replayed (``captured``): losses and final master weights go to a file for
tests/test_gpu_supcon.py, which runs each mode in a process of its own.

Usage: python tests/_supcon_steps.py {eager|captured} OUT.pt
"""
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main(mode: str, out: str) -> None:
    from simclr_amd.config import compose, task_config, CONF_DIR
    from simclr_amd.data.datasets import synthetic_dataset
    from simclr_amd.data.loader import ContrastiveLoader
    from simclr_amd.ops import tuning
    from simclr_amd.parallel import state as pstate
    from simclr_amd.train.pretrain import Trainer
    from simclr_amd.utils.misc import seed_everything
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = task_config(compose(str(CONF_DIR), "config", [
        "experiment.base_cnn=resnet18", "model.cifar_stem=true", "experiment.batches=32",
        "data.synthetic=true", "loss.supervised=true", "runtime.deterministic=true",
        "parameter.epochs=10", "parameter.warmup_epochs=1"]))
    seed_everything(7, deterministic=True)
    tuning.set_enabled(False)
    pstate.reset()
    st = pstate.get()
    st.device = dev
    tr = Trainer(cfg, st, 512, precision="bf16")
    assert tr.hip and tr.supervised
    ds = synthetic_dataset(256, 10)
    loader = ContrastiveLoader(ds, 32, dev, seed=7)
    loader.label_i32 = True
    losses, replayed = [], 0
    for i, (x, y) in enumerate(loader):
        if i == 5:
            break
        if mode == "captured" and i == 2:
            tr.capture(x, y, warmup=0)
            tr.replay_mode = "streams" if tr.sreplay is not None else "graph"
            loader.out, loader.label_out = tr._static_x, tr._static_y
        replayed += int(tr.graph is not None)
        losses.append(tr.step(x, y).clone())
    torch.cuda.synchronize()
    torch.save({"losses": torch.stack(losses).cpu(), "master": tr.store.master.cpu(),
                "replayed": replayed, "mode": tr.replay_mode}, out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
