"""k-means probe: the fused HIP fit (ops/kmeans.py: normalise, R restarts in the same launches,
assign + update + finish per iteration) against a stock-op fit on the same GPU (chunked bf16
torch.matmul + argmax + index_add_ + F.normalize, the restarts one after another), both from raw
fp32 features to the final assignments.

    python tools/kmeans_bench.py [--n 50000] [--dims 512,2048] [--ks 10,100] [--restarts 1,8]
                                 [--iters 20] [--rounds 3] [--md profiles/kmeans.md]

The two paths alternate within every round; the table reports the median over the rounds (device
events around each call) as total time and time per iteration (total / (T + 1) assign passes), and
the medians of the assign and the update + finish launches on their own (prepared operands, the
fit's final centroids and assignments).  The partitions of the two paths are compared by ARI on
the first restart.
"""
import argparse
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])


def stock_fit(x, K, R, T, init, chunk=8192):
    xn = torch.nn.functional.normalize(x, dim=1).to(torch.bfloat16)
    xf = xn.float()
    N = x.shape[0]
    out = []
    for r in range(R):
        C = xn[init[r]]
        a = torch.empty(N, device=x.device, dtype=torch.long)
        for t in range(T + 1):
            for s in range(0, N, chunk):
                a[s:s + chunk] = (xn[s:s + chunk] @ C.t()).float().argmax(1)
            if t < T:
                S = torch.zeros(K, xf.shape[1], device=x.device).index_add_(0, a, xf)
                n = torch.bincount(a, minlength=K)
                C = torch.where((n > 0)[:, None], torch.nn.functional.normalize(S, dim=1)
                                .to(torch.bfloat16), C)
        out.append(a.clone())
    return out


def timed(fn):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


def median_ms(fn, rounds):
    fn()
    return statistics.median(timed(fn)[0] for _ in range(rounds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--dims", default="512,2048")
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--restarts", default="1,8")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--md", default=None, help="write the table to this markdown file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kmeans_bench needs a GPU"
    from simclr_amd.ops import _ext, kmeans
    _ext.require()
    dev = torch.device("cuda", 0)
    T = a.iters
    rows = []
    for D in [int(v) for v in a.dims.split(",")]:
        torch.manual_seed(0)
        # clustered features (a frozen encoder's are): 2 K centres, so that restarts differ
        for K in [int(v) for v in a.ks.split(",")]:
            centres = torch.randn(2 * K, D, device=dev)
            x = centres[torch.randint(0, 2 * K, (a.n,), device=dev)] + 2.0 * torch.randn(a.n, D, device=dev)
            for R in [int(v) for v in a.restarts.split(",")]:
                init = kmeans.draw_init(a.n, K, R, 0)
                init_dev = init.to(dev)
                run_f = lambda: kmeans.kmeans_fit(x, K, R, T, init=init)
                run_s = lambda: stock_fit(x, K, R, T, init_dev)
                _, fit = timed(run_f)  # warm-up of both paths at the timed shape
                _, st = timed(run_s)
                table = kmeans.contingency(fit.a[0], st[0], K, K)
                ari = kmeans.cluster_scores(table)["ari"]
                tf, ts = [], []
                for _ in range(a.rounds):
                    tf.append(timed(run_f)[0])
                    ts.append(timed(run_s)[0])
                Xn = kmeans.normalize_bf16(x)
                t_as = median_ms(lambda: kmeans._assign_hip(Xn, fit.centroids), a.rounds)
                t_up = median_ms(lambda: kmeans._update_hip(Xn, fit.a, fit.centroids), a.rounds)
                f, s = statistics.median(tf), statistics.median(ts)
                rows.append((D, K, R, f, min(tf), max(tf), s, min(ts), max(ts), t_as, t_up, ari))
                print(f"F={D} K={K} R={R}: fused {f:.1f} ms [{min(tf):.1f}, {max(tf):.1f}] "
                      f"({f / (T + 1):.2f} ms / iteration)  stock {s:.1f} ms [{min(ts):.1f}, "
                      f"{max(ts):.1f}] ({s / (T + 1):.2f} ms / iteration)  assign call {t_as:.2f} ms  "
                      f"update call {t_up:.2f} ms  ARI fused vs stock (restart 0) {ari:.4f}",
                      flush=True)
                del fit, st, Xn
    if a.md:
        with open(a.md, "a") as fh:
            fh.write(f"\n`python tools/kmeans_bench.py --n {a.n} --dims {a.dims} --ks {a.ks} "
                     f"--restarts {a.restarts} --iters {T} --rounds {a.rounds}` on one MI355X\n\n")
            fh.write("| F | K | R | fused total ms | fused ms / iteration | stock total ms | stock ms / "
                     "iteration | stock / fused | assign call ms | update call ms | ARI fused vs "
                     "stock |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
            for D, K, R, f, f0, f1, s, s0, s1, t_as, t_up, ari in rows:
                fh.write(f"| {D} | {K} | {R} | {f:.1f} [{f0:.1f}, {f1:.1f}] | {f / (T + 1):.2f} | "
                         f"{s:.1f} [{s0:.1f}, {s1:.1f}] | {s / (T + 1):.2f} | {s / f:.2f} | "
                         f"{t_as:.2f} | {t_up:.2f} | {ari:.4f} |\n")


if __name__ == "__main__":
    main()
