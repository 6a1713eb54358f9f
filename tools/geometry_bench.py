"""Geometry probe: the HIP kernels of ops/geometry.py against stock ops on the same GPU.

    python tools/geometry_bench.py [--n 50000] [--dims 512,2048] [--t 2.0] [--rounds 3]
                                   [--md profiles/geometry.md]

Pair part: ``pair_stats`` (normalise, the triangle's tiles, the read-back of the tile partials)
against chunked bf16 ``torch.matmul`` + ``exp`` + ``sum`` over the row blocks' columns from the
block's first row on (the upper blocks; the diagonal block masked), with and without labels.
Spectrum part: the centre and the product kernels (to S on the device) against a bf16 ``matmul``
of the centred features; the host eigendecomposition is the same work for both and is timed once.
The two paths alternate within every round; the tables report the median over the rounds (device
events around each call, which ends in a synchronise).  A kernel's rate counts the products of the
triangle it computes (N (N - 1) / 2 · Dp and N · Dp (Dp + 64) / 2 multiply-adds) and is also given
as a share of 1.24 PF/s, the lower end of the bf16 GEMM rate measured in this project.
"""
import argparse
import statistics
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
GEMM_RATE = 1.24e15


def stock_pair(x, y, t, block=4096):
    xn = torch.nn.functional.normalize(x, dim=1).to(torch.bfloat16)
    N = x.shape[0]
    E = torch.zeros((), device=x.device, dtype=torch.float64)
    A, A_same = E.clone(), E.clone()
    for b in range(0, N, block):
        s = (xn[b:b + block] @ xn[b:].t()).float()
        n = s.shape[0]
        keep = torch.ones_like(s, dtype=torch.bool)
        keep[:, :n] = torch.triu(keep[:, :n], diagonal=1)
        e = torch.where(keep, torch.exp(2 * t * (s - 1)), torch.zeros_like(s))
        d = torch.where(keep, 2 - 2 * s, torch.zeros_like(s))
        E += e.sum(dtype=torch.float64)
        A += d.sum(dtype=torch.float64)
        if y is not None:
            eq = y[b:b + block].view(-1, 1) == y[b:].view(1, -1)
            A_same += torch.where(eq, d, torch.zeros_like(d)).sum(dtype=torch.float64)
    return float(E), float(A), float(A_same)


def stock_second_moment(x):
    c = (x - x.mean(0, keepdim=True)).to(torch.bfloat16)
    return (c.t() @ c).float()


def timed(fn):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


def alternate(fa, fb, rounds):
    """Medians (and ranges) of two paths that alternate within every round, after one warm-up."""
    fa()
    fb()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(fa)[0])
        tb.append(timed(fb)[0])
    return (statistics.median(ta), min(ta), max(ta)), (statistics.median(tb), min(tb), max(tb))


def median_ms(fn, rounds):
    fn()
    return statistics.median(timed(fn)[0] for _ in range(rounds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--dims", default="512,2048")
    ap.add_argument("--t", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--md", default=None, help="append the tables to this markdown file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "geometry_bench needs a GPU"
    from simclr_amd.ops import _ext, geometry as geo
    _ext.require()
    ops = _ext.ops()
    dev = torch.device("cuda", 0)
    N, t = a.n, a.t
    pair_rows, spec_rows = [], []
    for D in [int(v) for v in a.dims.split(",")]:
        torch.manual_seed(0)
        y = torch.randint(0, 10, (N,), device=dev)
        x = torch.randn(10, D, device=dev)[y] + 2.0 * torch.randn(N, D, device=dev)
        Dp = geo.padded_d(D)
        for labels in (y, None):
            (f, f0, f1), (s, s0, s1) = alternate(lambda: geo.pair_stats(x, labels, t),
                                                 lambda: stock_pair(x, labels, t), a.rounds)
            got, ref = geo.pair_stats(x, labels, t), stock_pair(x, labels, t)
            Xn = geo.normalize_bf16(x)
            tiles = geo.pair_tiles(N)
            fpart = torch.empty(tiles, 3, device=dev)
            ipart = torch.empty(tiles, 2, device=dev, dtype=torch.int32)
            lab = None if labels is None else labels.to(torch.int32)
            tk = median_ms(lambda: ops.geometry_pair(Xn, lab, t, fpart, ipart), a.rounds)
            rate = N * (N - 1) * Dp / (tk * 1e-3)  # 2 flops per multiply-add, half the square
            pair_rows.append((D, labels is not None, f, f0, f1, s, s0, s1, tk, rate,
                              abs(got.E - ref[0]) / ref[0], abs(got.A - ref[1]) / ref[1]))
            print(f"pair D={D} labels={labels is not None}: hip {f:.1f} ms [{f0:.1f}, {f1:.1f}]  stock "
                  f"{s:.1f} ms [{s0:.1f}, {s1:.1f}]  kernel {tk:.1f} ms = {rate / 1e12:.0f} TF/s "
                  f"({rate / GEMM_RATE:.1%} of the GEMM rate)  E rel diff {pair_rows[-1][10]:.1e} "
                  f"A rel diff {pair_rows[-1][11]:.1e}", flush=True)
            del fpart, ipart, Xn
        Np = (N + 63) // 64 * 64
        mu = torch.empty(Dp, device=dev)
        cT = torch.empty(Dp, Np, device=dev, dtype=torch.bfloat16)
        S = torch.empty(Dp, Dp, device=dev, dtype=torch.float64)

        def hip_second_moment():
            ops.geometry_center(x, mu, cT)
            ops.geometry_syrk(cT, N, S)
            return S

        (f, f0, f1), (s, s0, s1) = alternate(hip_second_moment, lambda: stock_second_moment(x), a.rounds)
        tc = median_ms(lambda: ops.geometry_center(x, mu, cT), a.rounds)
        tp = median_ms(lambda: ops.geometry_syrk(cT, N, S), a.rounds)
        rate = N * Dp * (Dp + 64) / (tp * 1e-3)
        ref = stock_second_moment(x).double()
        diff = float((S[:D, :D] - ref).norm() / ref.norm())
        t0 = time.perf_counter()
        sp = geo.spectrum(x)
        total = (time.perf_counter() - t0) * 1e3
        er = geo.effective_rank(sp.eig)
        spec_rows.append((D, f, f0, f1, s, s0, s1, tc, tp, rate, geo.syrk_splits(N, Dp), diff, total, er))
        print(f"spectrum D={D}: hip {f:.1f} ms [{f0:.1f}, {f1:.1f}]  stock {s:.1f} ms [{s0:.1f}, {s1:.1f}]  "
              f"centre {tc:.2f} ms  product + merge {tp:.2f} ms = {rate / 1e12:.0f} TF/s "
              f"({rate / GEMM_RATE:.1%} of the GEMM rate, {spec_rows[-1][10]} splits)  S rel diff {diff:.1e}  "
              f"spectrum() with the host eigvalsh {total:.0f} ms  effective rank {er:.1f}", flush=True)
        del mu, cT, S
    if a.md:
        with open(a.md, "a") as fh:
            fh.write(f"\n`python tools/geometry_bench.py --n {N} --dims {a.dims} --t {t} --rounds "
                     f"{a.rounds}` on one MI355X\n\n")
            fh.write("| D | labels | pair_stats ms | stock ms | stock / hip | pair kernel ms | TF/s | share "
                     "of 1.24 PF/s | E rel diff | A rel diff |\n|---|---|---|---|---|---|---|---|---|---|\n")
            for D, lab, f, f0, f1, s, s0, s1, tk, rate, de, da in pair_rows:
                fh.write(f"| {D} | {'yes' if lab else 'no'} | {f:.1f} [{f0:.1f}, {f1:.1f}] | {s:.1f} "
                         f"[{s0:.1f}, {s1:.1f}] | {s / f:.2f} | {tk:.1f} | {rate / 1e12:.0f} | "
                         f"{rate / GEMM_RATE:.1%} | {de:.1e} | {da:.1e} |\n")
            fh.write("\n| D | centre + product ms | stock ms | stock / hip | centre ms | product + merge ms | "
                     "TF/s | share of 1.24 PF/s | splits | S rel diff | spectrum() with eigvalsh ms |\n"
                     "|---|---|---|---|---|---|---|---|---|---|---|\n")
            for D, f, f0, f1, s, s0, s1, tc, tp, rate, sp_, diff, total, er in spec_rows:
                fh.write(f"| {D} | {f:.1f} [{f0:.1f}, {f1:.1f}] | {s:.1f} [{s0:.1f}, {s1:.1f}] | {s / f:.2f} | "
                         f"{tc:.2f} | {tp:.2f} | {rate / 1e12:.0f} | {rate / GEMM_RATE:.1%} | {sp_} | "
                         f"{diff:.1e} | {total:.0f} |\n")


if __name__ == "__main__":
    main()
