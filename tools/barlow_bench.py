"""Barlow Twins kernel cost on one GPU at n = 512 images per view: every launch of
csrc/barlow.hip on its own, then forward + backward of the whole loss (autograd included) for
the kernels, for the torch twin on stock ops (fp32, unrounded) and for NT-Xent at R 1024 / D 128,
the arms alternating round by round in one process; medians over the rounds.

``--global``: on a forced 1-rank RCCL group, every new launch of ``loss.barlow_global`` on its own
and forward + backward of the per-rank and the global module alternating in one run (the three
collectives are 1-rank calls: their cost among several GPUs is not measured here)."""
import argparse
import datetime
import os
import sys

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])


def timeit(fn, reps):
    fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def launches(ops, z, n, lambd=0.0051, eps=1e-5):
    """name -> callable for each launch, on buffers filled by one real pass."""
    dev, D = z.device, z.shape[1]
    rstd = torch.empty(2, D, device=dev)
    zh = torch.empty(2 * n, D, device=dev, dtype=torch.bfloat16)
    zhT = torch.empty(2, D, n, device=dev, dtype=torch.bfloat16)
    splits = ops.bt_corr_splits(n, D)
    part = torch.empty(splits, D, D, device=dev)
    C = torch.empty(D, D, device=dev)
    lpart = torch.empty(ops.bt_loss_blocks(D), device=dev)
    out, g = torch.empty(1, device=dev), torch.ones(1, device=dev)
    G = torch.empty(D, D, device=dev, dtype=torch.bfloat16)
    GT = torch.empty_like(G)
    dzh = torch.empty(2 * n, D, device=dev)
    colpart = torch.empty(2, n // 32, 2, D, device=dev)
    dz = torch.empty_like(zh)
    fns = {
        "standardize": lambda: ops.bt_standardize(z, eps, rstd, zh, zhT),
        "corr": lambda: ops.bt_corr(zhT, n, splits, part),
        "loss": lambda: ops.bt_loss(part, splits, n, lambd, C, lpart),
        "reduce": lambda: ops.nt_reduce_loss(lpart, 1.0, out),
        "grad": lambda: ops.bt_grad(C, lambd, g, G, GT),
        "bwd": lambda: ops.bt_backward(zh, G, GT, dzh, colpart),
        "std_bwd": lambda: ops.bt_std_backward(zh, rstd, dzh, colpart, dz, None),
    }
    for f in fns.values():
        f()
    return fns, splits


def global_launches(ops, z, n):
    """name -> callable for each launch loss.barlow_global adds (W = 1 buffers)."""
    dev, D = z.device, z.shape[1]
    stats = torch.empty(1, 2, 2, D, device=dev)
    rstd = torch.empty(2, D, device=dev)
    zh = torch.empty(2 * n, D, device=dev, dtype=torch.bfloat16)
    zhT = torch.empty(2, D, n, device=dev, dtype=torch.bfloat16)
    splits = ops.bt_corr_splits(n, D)
    part = torch.randn(splits, D, D, device=dev)
    S = torch.empty(D, D, device=dev)
    colpart = torch.randn(2, n // 32, 2, D, device=dev)
    csum = torch.empty(1, 2, 2, D, device=dev)
    dzh = torch.randn(2 * n, D, device=dev)
    dz = torch.empty_like(zh)
    fns = {
        "stats": lambda: ops.bt_stats(z, stats[0]),
        "merge_standardize": lambda: ops.bt_merge_standardize(z, stats, 1e-5, rstd, zh, zhT),
        "slab_merge": lambda: ops.bt_slab_merge(part, splits, S),
        "colsum": lambda: ops.bt_colsum(colpart, csum[0]),
        "std_bwd_global": lambda: ops.bt_std_backward_global(zh, rstd, dzh, csum, dz, None),
    }
    for f in fns.values():
        f()
    return fns, splits


def main_global(dims, n, rounds, reps):
    import torch.distributed as dist
    from simclr_amd.loss.barlow import BarlowTwins
    from simclr_amd.ops import _ext
    from simclr_amd.parallel import state as pstate
    ops = _ext.ops()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29546")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev,
                            timeout=datetime.timedelta(seconds=120))
    pstate.set_state(rank=0, world_size=1, local_rank=0, group=dist.group.WORLD, backend="nccl",
                     force_comm=True)
    g = torch.Generator(device=dev).manual_seed(0)
    for D in dims:
        z0 = torch.randn(n, D, device=dev, generator=g)
        z = torch.cat([z0, 0.7 * z0 + 0.7 * torch.randn(n, D, device=dev, generator=g)])
        z = z.to(torch.bfloat16)
        fns, splits = global_launches(ops, z, n)
        per = {k: _median([timeit(f, reps) for _ in range(rounds)]) for k, f in fns.items()}
        arms = {"per rank": step_of(BarlowTwins(), z),
                "global (1-rank group)": step_of(BarlowTwins(global_batch=True), z)}
        tot = {k: [] for k in arms}
        for _ in range(rounds):
            for k, f in arms.items():
                tot[k].append(timeit(f, reps))
        print(f"global n={n} D={D} splits={splits}: " +
              "  ".join(f"{k} {v:.1f}" for k, v in per.items()) + " us | fwd+bwd: " +
              "  ".join(f"{k} {_median(v):.1f} [{min(v):.1f}, {max(v):.1f}]"
                        for k, v in tot.items()) + " us", flush=True)
    torch.cuda.synchronize()
    dist.destroy_process_group()


def step_of(mod, z):
    zr = z.clone().requires_grad_(True)

    def step():
        zr.grad = None
        mod(zr).backward()
    return step


def main(dims, n, rounds, reps):
    from simclr_amd.loss.barlow import BarlowTwins, barlow_twins_torch
    from simclr_amd.loss.ntxent import NTXent
    from simclr_amd.ops import _ext
    ops = _ext.ops()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    znt = torch.randn(2 * n, 128, device=dev, generator=g).to(torch.bfloat16)
    nt = step_of(NTXent(0.5), znt)
    for D in dims:
        z0 = torch.randn(n, D, device=dev, generator=g)
        z = torch.cat([z0, 0.7 * z0 + 0.7 * torch.randn(n, D, device=dev, generator=g)])
        z = z.to(torch.bfloat16)
        fns, splits = launches(ops, z, n)
        per = {k: _median([timeit(f, reps) for _ in range(rounds)]) for k, f in fns.items()}
        arms = {"kernels": step_of(BarlowTwins(), z),
                "twin": step_of(lambda t: barlow_twins_torch(t, n, 0.0051), z.float()),
                "nt-xent R 1024 D 128": nt}
        tot = {k: [] for k in arms}
        for _ in range(rounds):
            for k, f in arms.items():
                tot[k].append(timeit(f, reps))
        print(f"n={n} D={D} splits={splits}: " +
              "  ".join(f"{k} {v:.1f}" for k, v in per.items()) +
              f"  sum {sum(per.values()):.1f} us | fwd+bwd: " +
              "  ".join(f"{k} {_median(v):.1f} [{min(v):.1f}, {max(v):.1f}]"
                        for k, v in tot.items()) + " us", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--dims", type=int, nargs="+", default=[128, 512, 2048])
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--global", dest="global_batch", action="store_true",
                    help="the launches and the step of loss.barlow_global on a 1-rank RCCL group")
    a = ap.parse_args()
    (main_global if a.global_batch else main)(a.dims, a.n, a.rounds, a.reps)
