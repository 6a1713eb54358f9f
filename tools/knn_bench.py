"""Weighted k-NN probe: the fused HIP path (ops/knn.py: normalise, similarity + top-k, vote)
against a stock-op path on the same GPU (chunked bf16 torch.matmul + torch.topk + scatter_add),
both from raw fp32 features to class scores.

    python tools/knn_bench.py [--q 10000] [--n 50000] [--dims 2048,512] [--k 200] [--rounds 5]
                              [--stock-chunk 2048] [--md profiles/knn_probe.md]

The two paths alternate within every round; the table reports the median over the rounds (device
events around each call), the peak memory either path allocates beyond its inputs, and the fused
path's similarity rate (2·Q·N·D useful operations over its whole time, so a lower bound on the
kernel's own rate).  The neighbour sets of the two paths are compared on the first round.
"""
import argparse
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])


def stock(query, bank, labels, k, T, C, chunk):
    qn = torch.nn.functional.normalize(query, dim=1).to(torch.bfloat16)
    bn = torch.nn.functional.normalize(bank, dim=1).to(torch.bfloat16)
    scores = torch.zeros(query.shape[0], C, device=query.device)
    idx = torch.empty(query.shape[0], k, device=query.device, dtype=torch.long)
    for s in range(0, query.shape[0], chunk):
        sim = qn[s:s + chunk] @ bn.t()  # [chunk][N] bf16
        v, i = torch.topk(sim.float(), k, dim=1)
        scores[s:s + chunk].scatter_add_(1, labels[i], torch.exp((v - 1.0) / T))
        idx[s:s + chunk] = i
    return scores, idx


def fused(query, bank, labels, targets, k, T, C):
    from simclr_amd.ops.knn import knn_topk, knn_vote
    vals, idx = knn_topk(query, bank, k)
    scores, _ = knn_vote(vals, idx, labels, C, T, targets)
    return scores, idx


def timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e), torch.cuda.max_memory_allocated() - base, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--q", type=int, default=10000)
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--dims", default="2048,512")
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--t", type=float, default=0.1)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--stock-chunk", type=int, default=2048)
    ap.add_argument("--md", default=None, help="write the table to this markdown file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "knn_bench needs a GPU"
    from simclr_amd.ops import _ext
    ops = _ext.ops()
    dev = torch.device("cuda", 0)
    rows = []
    for D in [int(d) for d in a.dims.split(",")]:
        torch.manual_seed(0)
        query = torch.randn(a.q, D, device=dev)
        bank = torch.randn(a.n, D, device=dev)
        labels = torch.randint(0, a.classes, (a.n,), device=dev)
        targets = torch.randint(0, a.classes, (a.q,), device=dev)
        run_f = lambda: fused(query, bank, labels, targets, a.k, a.t, a.classes)
        run_s = lambda: stock(query, bank, labels, a.k, a.t, a.classes, a.stock_chunk)
        _, _, (sf, i_f) = timed(run_f)  # warm-up of both paths at the timed shape
        _, _, (ss, i_s) = timed(run_s)
        same = (i_f.long().sort(1)[0] == i_s.sort(1)[0]).all(1).float().mean().item()
        close = torch.allclose(sf, ss, rtol=2e-2)  # the stock similarities are rounded to bf16
        del sf, ss, i_f, i_s
        tf, ts, mf, ms = [], [], 0, 0
        for _ in range(a.rounds):
            t, m, _ = timed(run_f)
            tf.append(t)
            mf = max(mf, m)
            t, m, _ = timed(run_s)
            ts.append(t)
            ms = max(ms, m)
        f, s = statistics.median(tf), statistics.median(ts)
        scratch = ops.knn_scratch_bytes(min(a.q, 8192), a.n, a.k)
        rate = 2.0 * a.q * a.n * D / (f * 1e-3) / 1e12
        rows.append((D, f, min(tf), max(tf), s, min(ts), max(ts), mf, ms, scratch, rate, same,
                     close))
        print(f"D={D}: fused {f:.1f} ms [{min(tf):.1f}, {max(tf):.1f}]  stock {s:.1f} ms "
              f"[{min(ts):.1f}, {max(ts):.1f}]  peak extra memory fused {mf / 2**20:.0f} MiB "
              f"(kernel scratch {scratch / 2**20:.0f} MiB) stock {ms / 2**20:.0f} MiB  "
              f"fused {rate:.1f} TF/s  identical neighbour sets {same * 100:.2f} % of rows, "
              f"scores close {close}", flush=True)
    if a.md:
        with open(a.md, "w") as fh:
            fh.write("# Weighted k-NN probe: fused HIP path vs stock ops\n\n")
            fh.write(f"`python tools/knn_bench.py --q {a.q} --n {a.n} --dims {a.dims} --k {a.k} "
                     f"--rounds {a.rounds} --stock-chunk {a.stock_chunk}` on one MI355X.  Both "
                     "paths go from raw fp32 features to class scores; they alternate within each "
                     "round; times are medians over the rounds [min, max] after one warm-up call "
                     "of each.  Stock path: `F.normalize`, bf16 `torch.matmul` in query chunks of "
                     f"{a.stock_chunk}, `torch.topk`, `scatter_add_`.  Peak memory is what a call "
                     "allocates beyond its inputs (`torch.cuda.max_memory_allocated`).  TF/s is "
                     "2·Q·N·D over the fused path's whole time (normalise, top-k, merge and vote "
                     "included), not a kernel's share of peak.\n\n")
            fh.write("| D | fused ms | stock ms | stock / fused | fused peak MiB (kernel scratch) | "
                     "stock peak MiB | fused TF/s | rows with identical neighbour sets |\n")
            fh.write("|---|---|---|---|---|---|---|---|\n")
            for D, f, f0, f1, s, s0, s1, mf, ms, scratch, rate, same, close in rows:
                fh.write(f"| {D} | {f:.1f} [{f0:.1f}, {f1:.1f}] | {s:.1f} [{s0:.1f}, {s1:.1f}] | "
                         f"{s / f:.2f} | {mf / 2**20:.0f} ({scratch / 2**20:.0f}) | "
                         f"{ms / 2**20:.0f} | {rate:.1f} | {same * 100:.2f} % |\n")
            fh.write("\nThe stock path rounds its similarities to bf16 before `torch.topk`, so its "
                     "neighbour sets differ from the exact ones near the k-th similarity; the "
                     "fused path selects on fp32 accumulators.\n")


if __name__ == "__main__":
    main()
