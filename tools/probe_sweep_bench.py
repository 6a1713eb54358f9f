"""Times the fused linear-probe sweep (ops/probe_sweep.py, csrc/probe.hip) at G in {1, 4, 16}
against G sequential runs of ``learnable_eval`` (nn.Linear, autograd, torch.optim.SGD) on the same
device and the same synthetic features: N 50,000, C 10, batch 512, F 512 and 2048.  Both sides
include the per-epoch train / val evaluation, as ``eval.py`` runs them.

    python tools/probe_sweep_bench.py [--epochs 2] [--out profiles/probe_sweep.md]
"""
import argparse
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from simclr_amd.evaluation.probes import DownstreamDataset, learnable_eval, sweep_eval  # noqa: E402
from simclr_amd.models.heads import LinearClassifier  # noqa: E402


def _features(n, F, C, dev, seed):
    centers = torch.randn(C, F, generator=torch.Generator().manual_seed(0))  # shared by train / val
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, C, (n,), generator=g)
    x = 0.2 * centers[y] + torch.randn(n, F, generator=g)
    return DownstreamDataset(x.to(dev), y.to(dev))


def _cfg(epochs, bs, lr=0.1, decay=0.0):
    return {"parameter": {"epochs": epochs, "momentum": 0.9, "linear_schedule": True, "seed": 7},
            "experiment": {"batches": bs, "lr": lr, "decay": decay}}


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--features", type=int, nargs="+", default=[512, 2048])
    ap.add_argument("--configs", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    C, bs = a.classes, a.batch
    steps = a.epochs * -(-a.n // bs)
    lines = [f"N {a.n}, C {C}, batch {bs}, {a.epochs} epochs ({steps} steps), "
             f"{torch.cuda.get_device_name(0)}; seconds include the per-epoch evaluation", "",
             "| F | G | fused sweep s | ms / step | G sequential runs s | ms / step / run | speed-up | best val acc (sweep / sequential) |",
             "|---|---|---|---|---|---|---|---|"]
    for F in a.features:
        train, val = _features(a.n, F, C, dev, 1), _features(a.n // 5, F, C, dev, 2)
        for G in a.configs:
            lrs = [0.02 * 1.3 ** i for i in range(G)]
            torch.manual_seed(0)
            init = LinearClassifier(F, C)
            # warm-up: allocations, kernel load
            sweep_eval(_cfg(1, bs), init, DownstreamDataset(train.data[:2048], train.targets[:2048]),
                       val, lrs, [0.0], 5, seed=7)
            res = {}
            t_sweep = _timed(lambda: res.setdefault("s", sweep_eval(
                _cfg(a.epochs, bs), init, train, val, lrs, [0.0], 5, seed=7)))
            assert res["s"][1].hip and res["s"][1].step == steps
            best_sweep = max(max(r[3]) for r in res["s"][0])

            def sequential():
                best = 0.0
                for lr in lrs:
                    clf = LinearClassifier(F, C)
                    clf.load_state_dict(init.state_dict())
                    r = learnable_eval(_cfg(a.epochs, bs, lr), clf.to(dev), train, val, 5, seed=7)
                    best = max(best, max(r[3]))
                res["q"] = best
            clf = LinearClassifier(F, C).to(dev)
            learnable_eval(_cfg(1, bs), clf, DownstreamDataset(train.data[:2048], train.targets[:2048]),
                           val, 5, seed=7)
            t_seq = _timed(sequential)
            lines.append(f"| {F} | {G} | {t_sweep:.3f} | {1e3 * t_sweep / steps:.3f} | {t_seq:.3f} | "
                         f"{1e3 * t_seq / steps / G:.3f} | {t_seq / t_sweep:.2f}x | "
                         f"{best_sweep:.4f} / {res['q']:.4f} |")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
