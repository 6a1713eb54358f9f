"""Five training steps of ResNet-18 (CIFAR stem, batch 32 at 32x32, synthetic data with labels,
deterministic tiles) with the online probe, eager throughout (``eager``) or captured after the
second step and replayed by hipGraphLaunch (``graph``) or the multi-stream executor
(``streams``): losses, encoder master, the probe's state and its accumulators go to a file for
tests/test_gpu_online_probe.py, which runs each mode in a process of its own.

Flags: ``off`` (no probe), ``supcon`` (``loss.supervised=true`` as well), ``comm`` (the probe's
gradient all-reduce on a 1-rank RCCL group).

Usage: python tests/_online_probe_steps.py {eager|graph|streams} OUT.pt [FLAG ...]
"""
import datetime
import os
import sys
from pathlib import Path

import torch
import torch.distributed as dist

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main(mode: str, out: str, flags) -> None:
    from simclr_amd.config import compose, task_config, CONF_DIR
    from simclr_amd.data.datasets import synthetic_dataset
    from simclr_amd.data.loader import ContrastiveLoader
    from simclr_amd.ops import online_probe, tuning
    from simclr_amd.parallel import state as pstate
    from simclr_amd.train.pretrain import Trainer
    from simclr_amd.utils.misc import seed_everything
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    probe_on = "off" not in flags
    ov = ["experiment.base_cnn=resnet18", "model.cifar_stem=true", "experiment.batches=32",
          "data.synthetic=true", "runtime.deterministic=true", "parameter.epochs=10",
          "parameter.warmup_epochs=1", f"online_probe.enabled={'true' if probe_on else 'false'}",
          f"loss.supervised={'true' if 'supcon' in flags else 'false'}"]
    cfg = task_config(compose(str(CONF_DIR), "config", ov))
    seed_everything(7, deterministic=True)
    tuning.set_enabled(False)
    pstate.reset()
    st = pstate.get()
    st.device = dev
    tr = Trainer(cfg, st, 512, precision="bf16", num_classes=10)
    assert tr.hip and (tr.probe is not None) == probe_on
    calls = [0]
    if "comm" in flags:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29547")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev,
                                timeout=datetime.timedelta(seconds=120))
        tr.probe.group, tr.probe.comm = dist.group.WORLD, True
        real = dist.all_reduce

        def counted(t, *a, **k):
            calls[0] += int(t.data_ptr() == tr.probe.grad.data_ptr())
            return real(t, *a, **k)
        online_probe.dist.all_reduce = counted
    need_y = probe_on or "supcon" in flags
    loader = ContrastiveLoader(synthetic_dataset(256, 10), 32, dev, seed=7)
    loader.with_labels = loader.label_i32 = need_y
    losses, replayed = [], 0
    for i, (x, y) in enumerate(loader):
        if i == 5:
            break
        args = (x, y) if need_y else (x,)
        if mode != "eager" and i == 2:
            tr.capture(*args, warmup=0)
            tr.replay_mode = mode
            assert mode == "graph" or tr.sreplay is not None, "multi-stream executor refused"
            loader.out, loader.label_out = tr._static_x, tr._static_y
        replayed += int(tr.graph is not None)
        losses.append(tr.step(*args).clone())
    torch.cuda.synchronize()
    res = {"losses": torch.stack(losses).cpu(), "master": tr.store.master.cpu(),
           "replayed": replayed, "mode": tr.replay_mode, "all_reduces": calls[0],
           "shared_labels": int(tr._static_y is not None and loader.label_out is tr._static_y)}
    if probe_on:
        p = tr.probe
        res.update(probe_master=p.master.cpu(), probe_mom=p.mom.cpu(), probe_step=p.step_t.cpu(),
                   acc_loss=p.acc_loss.cpu(), acc_cnt=p.acc_cnt.cpu(), hip_steps=p.hip_steps)
    torch.save(res, out)
    if tr.sreplay is not None:
        tr.sreplay.close()
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], sys.argv[3:])
