"""NNCLR kernel cost on one GPU at n = 512 images per view, D 128: every launch of
csrc/nnclr.hip on its own for each support-set size, then forward + backward of the whole loss
(autograd and the enqueue included) beside NT-Xent at R 1024 / D 128, the arms alternating round
by round in one process; medians over the rounds."""
import argparse
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


def launches(ops, z, queue, n, inv_t=10.0):
    """name -> callable for each launch, on buffers filled by one real pass."""
    dev, (R, D), Q = z.device, z.shape, queue.shape[0]
    zn = torch.empty(R, D, device=dev)
    zb = torch.empty(R, D, device=dev, dtype=torch.bfloat16)
    inv = torch.empty(R, device=dev)
    qs = ops.nc_top1_splits(R, Q)
    candv = torch.empty(qs, R, device=dev)
    candi = torch.empty(qs, R, device=dev, dtype=torch.int32)
    idx = torch.empty(R, device=dev, dtype=torch.int32)
    a = torch.empty_like(zb)
    ls = ops.nc_loss_splits(n)
    part = torch.empty(ls * R * 3, device=dev)
    lse, rows = torch.empty(R, device=dev), torch.empty(R, device=dev)
    out, g = torch.empty(1, device=dev), torch.ones(1, device=dev)
    bpart = torch.empty(ls * R * D, device=dev)
    dz = torch.empty_like(zb)
    cursor = torch.zeros(1, device=dev, dtype=torch.int32)
    fns = {
        "normalize": lambda: ops.nc_normalize(z, zn, zb, inv),
        "top1+select": lambda: ops.nc_lookup(zb, queue, qs, candv, candi, idx, a),
        "fwd": lambda: ops.nc_forward(a, zb, inv_t, ls, part),
        "finish": lambda: ops.nt_finish(part, R, ls, lse, rows),
        "reduce": lambda: ops.nt_reduce_loss(rows, 1.0 / R, out),
        "enqueue": lambda: ops.nc_enqueue(zb, queue, cursor),
        "bwd+norm_bwd": lambda: ops.nc_backward(a, zb, zn, inv, lse, inv_t, g, ls, bpart, dz, None),
    }
    for f in fns.values():
        f()
    return fns, qs, ls


def step_of(mod, z):
    zr = z.clone().requires_grad_(True)

    def step():
        zr.grad = None
        mod(zr).backward()
    return step


def main(queues, n, D, rounds, reps):
    from simclr_amd.loss.nnclr import NNCLR
    from simclr_amd.loss.ntxent import NTXent
    from simclr_amd.ops import _ext
    ops = _ext.ops()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    z0 = torch.randn(n, D, device=dev, generator=g)
    z = torch.cat([z0, 0.7 * z0 + 0.7 * torch.randn(n, D, device=dev, generator=g)])
    z = z.to(torch.bfloat16)
    nt = step_of(NTXent(0.1), torch.randn(1024, 128, device=dev, generator=g).to(torch.bfloat16))
    for Q in queues:
        mod = NNCLR(0.1, queue_size=Q, dim=D, device=dev, seed=0)
        fns, qs, ls = launches(ops, z, mod.queue.clone(), n)
        per = {k: _median([timeit(f, reps) for _ in range(rounds)]) for k, f in fns.items()}
        arms = {"nnclr": step_of(mod, z), "nt-xent R 1024 D 128": nt}
        tot = {k: [] for k in arms}
        for _ in range(rounds):
            for k, f in arms.items():
                tot[k].append(timeit(f, reps))
        print(f"n={n} D={D} Q={Q} queue splits={qs} loss splits={ls}: " +
              "  ".join(f"{k} {v:.1f}" for k, v in per.items()) +
              f"  sum {sum(per.values()):.1f} us | fwd+bwd: " +
              "  ".join(f"{k} {_median(v):.1f} [{min(v):.1f}, {max(v):.1f}]"
                        for k, v in tot.items()) + " us", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--queues", type=int, nargs="+", default=[16384, 65536])
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=100)
    a = ap.parse_args()
    main(a.queues, a.n, a.dim, a.rounds, a.reps)
