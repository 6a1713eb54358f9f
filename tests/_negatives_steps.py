"""Five training steps of ResNet-18 (CIFAR stem, batch 32 at 32x32, synthetic data,
deterministic tiles) with the weighted-negatives NT-Xent (β = 1, τ⁺ = 0.1, decoupled), eager
throughout (``eager``) or captured after the second step and replayed through the graph
(``graph``) or the multi-stream executor (``streams``): losses and final master weights go to a
file for tests/test_gpu_ntxent_negatives.py, which runs each mode in a process of its own.

Usage: python tests/_negatives_steps.py {eager|graph|streams} OUT.pt
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
        "data.synthetic=true", "+loss.hard_beta=1.0", "+loss.tau_plus=0.1",
        "+loss.decoupled=true", "runtime.deterministic=true", "parameter.epochs=10",
        "parameter.warmup_epochs=1"]))
    seed_everything(7, deterministic=True)
    tuning.set_enabled(False)
    pstate.reset()
    st = pstate.get()
    st.device = dev
    tr = Trainer(cfg, st, 512, precision="bf16")
    assert tr.hip and tr.loss_fn.weighted
    loader = ContrastiveLoader(synthetic_dataset(256, 10), 32, dev, seed=7)
    losses, replayed = [], 0
    for i, (x, _) in enumerate(loader):
        if i == 5:
            break
        if mode != "eager" and i == 2:
            tr.capture(x, warmup=0)
            if mode == "streams":
                assert tr.sreplay is not None, "the multi-stream executor is not available"
            tr.replay_mode = mode
            loader.out = tr._static_x
        replayed += int(tr.graph is not None)
        losses.append(tr.step(x).clone())
    torch.cuda.synchronize()
    torch.save({"losses": torch.stack(losses).cpu(), "master": tr.store.master.cpu(),
                "replayed": replayed, "mode": tr.replay_mode}, out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
