"""Debug: every launch of the persistent 3x3 kernel (variant 20) inside a real training step is
re-run with the per-tile patch kernel (variant 15) into scratch outputs and compared."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_main", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from simclr_amd.ops.conv_hip import Igemm
    orig = Igemm.launch

    def wrapped(job, ops, v, stats=None):
        args = (stats,) if stats is not None else ()
        orig(job, ops, v, *args)
        if v != 20:
            return
        mode = job.epi.mode if job.epi is not None else 0
        if mode not in (0, 3):
            print("skip compare mode", mode, flush=True)
            return
        job2 = job._replace(out=torch.empty_like(job.out))
        stats2 = stats._replace(stats=torch.empty_like(stats.stats)) if stats is not None else None
        orig(job2, ops, 15, *((stats2,) if stats2 is not None else ()))
        torch.cuda.synchronize()
        d = (job.out.float() - job2.out.float()).abs().max().item()
        s = job2.out.float().abs().max().item()
        ds = ((stats.stats - stats2.stats).abs().max().item() if stats is not None else 0.0)
        print(f"v20 mode {mode} M={job.geom.M} out maxdiff {d:.3e} (max {s:.3e})"
              f" stats maxdiff {ds:.3e} nan={bool(torch.isnan(job.out).any())}", flush=True)

    Igemm.launch = wrapped
    sys.argv = ["bench.py", "--steps", "2", "--warmup", "1", "--no-graph"]
    bench.main()


if __name__ == "__main__":
    main()
