"""NT-Xent kernel cost vs the number of columns (global negatives: W ranks x 1024 rows), one
GPU: normalise/transpose, forward (+finish/reduce) and both backward passes, R = 1024 local rows."""
import sys

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])


def timeit(fn, reps=20):
    fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def main():
    from simclr_amd.ops import _ext
    ops = _ext.ops()
    dev = torch.device("cuda", 0)
    R, D, n = 1024, 128, 512
    for W in (1, 2, 4, 8):
        C = W * R
        zall = torch.nn.functional.normalize(torch.randn(C, D, device=dev), dim=1)
        znT = torch.empty(D, C, device=dev)
        ops.nt_transpose(zall, znT)
        off = 0
        splits = ops.nt_fwd_splits(R, C)
        part = torch.empty(splits * R * 3, device=dev)
        lse = torch.empty(R, device=dev)
        rows = torch.empty(R, device=dev)
        out = torch.empty(1, device=dev)
        g = torch.ones(1, device=dev)

        def fwd():
            ops.nt_forward(znT, R, off, n, 2.0, part, splits, lse, rows)
            ops.nt_reduce_loss(rows, 1.0 / R, out)
        s_col, s_row = ops.nt_bwd_splits(C, R), ops.nt_bwd_splits(R, C)
        p2 = torch.empty(s_col * C * D, device=dev)
        dc = torch.empty(C, D, device=dev)
        p1 = torch.empty(s_row * R * D, device=dev)
        dr = torch.empty(R, D, device=dev)
        t_t = timeit(lambda: ops.nt_transpose(zall, znT))
        t_f = timeit(fwd)
        t_bc = timeit(lambda: ops.nt_backward_part(False, zall, znT, lse, R, off, n, 2.0, 1.0 / R,
                                                   g, p2, s_col, dc))
        t_br = timeit(lambda: ops.nt_backward_part(True, zall, znT, lse, R, off, n, 2.0, 1.0 / R,
                                                   g, p1, s_row, dr))
        fl = 2.0 * R * C * D
        print(f"W={W} cols={C}: transpose {t_t:.1f}  fwd {t_f:.1f}  bwd cols {t_bc:.1f}  "
              f"bwd rows {t_br:.1f} us  (fwd {fl / t_f / 1e6:.1f} TF/s, splits {splits}/{s_col}/{s_row})",
              flush=True)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main_supervised(classes, widths, rounds, reps):
    """``--supervised``: the label-mode (SupCon) kernels against the NT-Xent ones on the same
    ẑ, alternating the two losses round by round in one process: forward (+finish/reduce),
    column pass, row pass; medians over the rounds, min-max of the per-round ratio."""
    from simclr_amd.ops import _ext
    ops = _ext.ops()
    dev = torch.device("cuda", 0)
    R, D, n = 1024, 128, 512
    for W in widths:
        C = W * R
        zall = torch.nn.functional.normalize(torch.randn(C, D, device=dev), dim=1)
        znT = torch.empty(D, C, device=dev)
        ops.nt_transpose(zall, znT)
        splits = ops.nt_fwd_splits(R, C)
        s_col, s_row = ops.nt_bwd_splits(C, R), ops.nt_bwd_splits(R, C)
        part3 = torch.empty(splits * R * 3, device=dev)
        part4 = torch.empty(splits * R * 4, device=dev)
        lse, rows, icnt = (torch.empty(R, device=dev) for _ in range(3))
        out, g = torch.empty(1, device=dev), torch.ones(1, device=dev)
        p2, dc = torch.empty(s_col * C * D, device=dev), torch.empty(C, D, device=dev)
        p1, dr = torch.empty(s_row * R * D, device=dev), torch.empty(R, D, device=dev)
        for K in classes:
            y = torch.randint(0, K, (n,), device=dev, dtype=torch.int32)
            ycol = torch.empty(C, device=dev, dtype=torch.int32)
            for w in range(W):  # every rank's block: view-expanded labels of the same classes
                yw = y if w == 0 else torch.randint(0, K, (n,), device=dev, dtype=torch.int32)
                ops.nt_expand_labels(yw, None, 2, ycol[w * R:(w + 1) * R])

            def fwd_nt():
                ops.nt_forward(znT, R, 0, n, 2.0, part3, splits, lse, rows)
                ops.nt_reduce_loss(rows, 1.0 / R, out)

            def fwd_sup():
                ops.nt_sup_forward_range(znT, ycol, 0, R, 0, n, 2.0, part4, 0, C, splits, 0)
                ops.nt_sup_finish(part4, R, splits, lse, icnt, rows)
                ops.nt_reduce_loss(rows, 1.0 / R, out)
            arms = {
                "fwd": (fwd_nt, fwd_sup),
                "bwd cols": (
                    lambda: ops.nt_backward_part(False, zall, znT, lse, R, 0, n, 2.0, 1.0 / R, g,
                                                 p2, s_col, dc),
                    lambda: ops.nt_sup_backward_part(False, zall, znT, lse, icnt, ycol, R, 0, n,
                                                     2.0, 1.0 / R, g, p2, s_col, dc)),
                "bwd rows": (
                    lambda: ops.nt_backward_part(True, zall, znT, lse, R, 0, n, 2.0, 1.0 / R, g,
                                                 p1, s_row, dr),
                    lambda: ops.nt_sup_backward_part(True, zall, znT, lse, icnt, ycol, R, 0, n,
                                                     2.0, 1.0 / R, g, p1, s_row, dr)),
            }
            fwd_sup()  # (lse / inv_cnt of this label set for the backward arms)
            line = [f"cols={C} classes={K}:"]
            for name, (f_nt, f_sup) in arms.items():
                t_nt, t_sup = [], []
                for _ in range(rounds):
                    t_nt.append(timeit(f_nt, reps))
                    t_sup.append(timeit(f_sup, reps))
                ratios = [b / a for a, b in zip(t_nt, t_sup)]
                line.append(f"{name} nt-xent {_median(t_nt):.1f} supcon {_median(t_sup):.1f} us "
                            f"ratio {_median(ratios):.3f} [{min(ratios):.3f}, {max(ratios):.3f}];")
            print(" ".join(line) + f" splits {splits}/{s_col}/{s_row}", flush=True)


def main_negatives(widths, rounds, reps):
    """``--negatives``: the weighted-negatives kernels (``HARD`` off: β = 0, τ⁺ = 0.1; ``HARD``
    on: β = 1, τ⁺ = 0.1) against the plain NT-Xent ones on the same ẑ, the three alternating
    round by round in one process: forward (+finish/reduce), column pass, row pass; medians over
    the rounds, median and min-max of the per-round ratio to the plain loss."""
    from simclr_amd.ops import _ext
    ops = _ext.ops()
    dev = torch.device("cuda", 0)
    R, D, n = 1024, 128, 512
    inv_t, tau_plus = 2.0, 0.1
    for W in widths:
        C = W * R
        zall = torch.nn.functional.normalize(torch.randn(C, D, device=dev), dim=1)
        znT = torch.empty(D, C, device=dev)
        ops.nt_transpose(zall, znT)
        splits = ops.nt_fwd_splits(R, C)
        s_col, s_row = ops.nt_bwd_splits(C, R), ops.nt_bwd_splits(R, C)
        part = torch.empty(splits * R * 5, device=dev)
        lse, rows = torch.empty(R, device=dev), torch.empty(R, device=dev)
        stats = {b: torch.empty(R, 4, device=dev) for b in (0.0, 1.0)}
        out, g = torch.empty(1, device=dev), torch.ones(1, device=dev)
        p2, dc = torch.empty(s_col * C * D, device=dev), torch.empty(C, D, device=dev)
        p1, dr = torch.empty(s_row * R * D, device=dev), torch.empty(R, D, device=dev)

        def fwd_nt():
            ops.nt_forward(znT, R, 0, n, inv_t, part, splits, lse, rows)
            ops.nt_reduce_loss(rows, 1.0 / R, out)

        def fwd_w(beta):
            ops.nt_w_forward_range(znT, R, 0, n, inv_t, beta, part, 0, C, splits, 0)
            ops.nt_w_finish(part, R, splits, C, inv_t, beta, tau_plus, False, stats[beta], rows)
            ops.nt_reduce_loss(rows, 1.0 / R, out)

        def bwd_w(row_mode, beta):
            ws, sp, dst = (p1, s_row, dr) if row_mode else (p2, s_col, dc)
            ops.nt_w_backward_part(row_mode, zall, znT, stats[beta], R, 0, n, inv_t, beta,
                                   1.0 / R, g, ws, sp, dst)
        arms = {
            "fwd": (fwd_nt, lambda: fwd_w(0.0), lambda: fwd_w(1.0)),
            "bwd cols": (
                lambda: ops.nt_backward_part(False, zall, znT, lse, R, 0, n, inv_t, 1.0 / R, g,
                                             p2, s_col, dc),
                lambda: bwd_w(False, 0.0), lambda: bwd_w(False, 1.0)),
            "bwd rows": (
                lambda: ops.nt_backward_part(True, zall, znT, lse, R, 0, n, inv_t, 1.0 / R, g,
                                             p1, s_row, dr),
                lambda: bwd_w(True, 0.0), lambda: bwd_w(True, 1.0)),
        }
        fwd_nt(), fwd_w(0.0), fwd_w(1.0)  # (lse / stats for the backward arms)
        for name, fns in arms.items():
            t = [[], [], []]
            for _ in range(rounds):
                for k, f in enumerate(fns):
                    t[k].append(timeit(f, reps))
            line = f"cols={C} {name}: plain {_median(t[0]):.1f} us"
            for k, label in ((1, "weighted"), (2, "weighted hard")):
                ratios = [b / a for a, b in zip(t[0], t[k])]
                line += (f"; {label} {_median(t[k]):.1f} us ratio {_median(ratios):.3f} "
                         f"[{min(ratios):.3f}, {max(ratios):.3f}]")
            print(line + f"; splits {splits}/{s_col}/{s_row}", flush=True)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--supervised", action="store_true",
                    help="time the label-mode (SupCon) kernels against the NT-Xent ones")
    ap.add_argument("--classes", type=int, nargs="+", default=[10, 100],
                    help="--supervised: number of distinct labels (one run per value)")
    ap.add_argument("--ranks", type=int, nargs="+", default=[1, 8],
                    help="--supervised / --negatives: column counts as multiples of the 1024 "
                         "local rows")
    ap.add_argument("--negatives", action="store_true",
                    help="time the weighted-negatives kernels (HARD off and on) against the "
                         "plain ones")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    if a.negatives:
        main_negatives(a.ranks, a.rounds, a.reps)
    elif a.supervised:
        main_supervised(a.classes, a.ranks, a.rounds, a.reps)
    else:
        main()
