"""Worker of tests/test_gpu_barlow_global.py (a process of its own: it owns a 1-rank RCCL group,
which the pytest process must not inherit).  With ``SIMCLR_FORCE_COMM=1`` every collective of the
data-parallel step is issued on that group, the three of ``loss.barlow_global`` among them.

``identity``: the loss, C and dz of ``BarlowTwins(global_batch=True)`` and of the per-rank module
on the same z at (n, D) = (32, 64) and (512, 128), bf16 and fp32 z.

``eager`` / ``graph`` / ``streams``: five training steps of ResNet-18 (CIFAR stem, batch 32 at
32x32, synthetic data, deterministic tiles; n 32, D 128) with the key ``on`` or ``off``, eager
throughout or captured after the second step and replayed by hipGraphLaunch or by the
multi-stream executor: losses, master weights, momentum and BatchNorm buffers go to a file.

Usage: SIMCLR_FORCE_COMM=1 python tests/_barlow_global_steps.py MODE {on|off} OUT.pt [PORT]
"""
import datetime
import os
import sys
from pathlib import Path

import torch
import torch.distributed as dist

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def _no_twin(*a, **k):
    raise AssertionError("the step fell back to the torch twin")


def _forced_state(dev, port):
    from simclr_amd.parallel import state as pstate
    assert os.environ.get("SIMCLR_FORCE_COMM") == "1", "run with SIMCLR_FORCE_COMM=1"
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", port)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev,
                            timeout=datetime.timedelta(seconds=120))
    pstate.reset()
    st = pstate.set_state(rank=0, world_size=1, local_rank=0, group=dist.group.WORLD,
                          backend="nccl", force_comm=True)
    st.device = dev
    pstate.make_stat_group(st)
    assert st.comm, "the forced 1-rank group did not enable the collectives"
    return st


def identity(dev, out):
    from simclr_amd.loss import barlow
    from simclr_amd.ops import _ext
    _ext.require()
    calls = {"gather": 0, "reduce": 0}
    gather, reduce = dist.all_gather_into_tensor, dist.all_reduce

    def counted_gather(*a, **k):
        calls["gather"] += 1
        return gather(*a, **k)

    def counted_reduce(*a, **k):
        calls["reduce"] += 1
        return reduce(*a, **k)

    barlow.dist.all_gather_into_tensor = counted_gather
    barlow.dist.all_reduce = counted_reduce
    barlow.barlow_twins_torch = _no_twin
    res = {}
    for n, D in ((32, 64), (512, 128)):
        g = torch.Generator().manual_seed(1000 * n + D)
        z0 = torch.randn(n, D, generator=g)
        z = torch.cat([z0, 0.7 * z0 + 0.7 * torch.randn(n, D, generator=g)]).to(dev)
        for name, zz in (("bf16", z.to(torch.bfloat16)), ("fp32", z * 1.0009765625)):
            arms = []
            for glob in (False, True):
                before = dict(calls)
                zr = zz.clone().requires_grad_(True)
                loss, C = barlow.BarlowTwins(0.0051, global_batch=glob)(zr, return_c=True)
                (loss * 0.37).backward()
                torch.cuda.synchronize()
                issued = (calls["gather"] - before["gather"], calls["reduce"] - before["reduce"])
                assert issued == ((2, 1) if glob else (0, 0)), (glob, issued)
                arms.append((loss.detach().cpu(), C.cpu(), zr.grad.cpu()))
            res[f"{name}-{n}-{D}"] = arms
    torch.save(res, out)


def steps(dev, st, mode, key, out):
    from simclr_amd.config import compose, task_config, CONF_DIR
    from simclr_amd.data.datasets import synthetic_dataset
    from simclr_amd.data.loader import ContrastiveLoader
    from simclr_amd.loss import barlow
    from simclr_amd.ops import tuning
    from simclr_amd.train.pretrain import Trainer
    from simclr_amd.utils.misc import seed_everything
    cfg = task_config(compose(str(CONF_DIR), "config", [
        "experiment.base_cnn=resnet18", "model.cifar_stem=true", "experiment.batches=32",
        "data.synthetic=true", "loss.kind=barlow",
        f"loss.barlow_global={'true' if key == 'on' else 'false'}", "runtime.deterministic=true",
        "parameter.epochs=10", "parameter.warmup_epochs=1"]))
    seed_everything(7, deterministic=True)
    tuning.set_enabled(False)
    tr = Trainer(cfg, st, 512, precision="bf16")
    assert tr.hip and isinstance(tr.loss_fn, barlow.BarlowTwins)
    assert tr.loss_fn.global_batch is (key == "on")
    barlow.barlow_twins_torch = _no_twin
    used = {"global": 0}
    apply = barlow._BarlowHipFn.apply

    def counted(*a):
        used["global"] += int(a[-1] is not None)  # (the state: the loss over all ranks)
        return apply(*a)

    barlow._BarlowHipFn.apply = counted
    loader = ContrastiveLoader(synthetic_dataset(256, 10), 32, dev, seed=7)
    losses, replayed = [], 0
    for i, (x, _) in enumerate(loader):
        if i == 5:
            break
        if mode != "eager" and i == 2:
            tr.capture(x, warmup=0)
            assert mode == "graph" or tr.sreplay is not None
            tr.replay_mode = mode
            loader.out = tr._static_x
        replayed += int(tr.graph is not None)
        losses.append(tr.step(x).clone())
    torch.cuda.synchronize()
    torch.save({"losses": torch.stack(losses).cpu(), "master": tr.store.master.cpu(),
                "momentum": tr.opt.mom.cpu(),
                "buffers": [b.detach().cpu() for b in tr.model.buffers()],
                "replayed": replayed, "mode": tr.replay_mode, "global_calls": used["global"]},
               out)
    if tr.sreplay is not None:
        tr.sreplay.close()


def main(mode: str, key: str, out: str, port: str) -> None:
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    st = _forced_state(dev, port)
    if mode == "identity":
        identity(dev, out)
    else:
        steps(dev, st, mode, key, out)
    torch.cuda.synchronize()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else "29547")
