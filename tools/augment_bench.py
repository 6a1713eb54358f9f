"""On-device augmentation launch time, Gaussian blur off and on (csrc/augment.hip).

    python tools/augment_bench.py [--launches 100] [--warmup 10] [--repeats 3] [--md FILE]

Cases: 32x32 from 32x32 sources (n 512, 2 views, blur kernel 3: the register-resident kernel) and
224x224 from 224x224 sources (n 128, 2 views, blur kernel 23: the two-pass kernel).  Every launch
sits between two device events on an otherwise idle device and advances the step counter, so it
draws fresh parameters (half of the images blurred); a row is the median over the launches and
the [min, max] of that median over the repeats.  On a build whose op has no ``blur_kernel``
argument only the blur-off rows are timed, with the argument left out.
"""
import argparse
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])

CASES = [(32, 512, 3), (224, 128, 23)]  # (side, n, blur kernel)


def time_case(ops, imgs, idx, out, n, size, ks, launches, warmup, pass_ks):
    extra = (ks,) if pass_ks else ()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(launches)]
    for i in range(warmup):
        ops.augment(imgs, idx, n, 2, size, size, 8, 0.5, 7, i, 0, 1, out, None, *extra)
    torch.cuda.synchronize()
    for i, (s, e) in enumerate(ev):
        s.record()
        ops.augment(imgs, idx, n, 2, size, size, 8, 0.5, 7, warmup + i, 0, 1, out, None, *extra)
        e.record()
    torch.cuda.synchronize()
    return statistics.median(s.elapsed_time(e) * 1e3 for s, e in ev)  # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--md", default=None, help="write the table to this markdown file")
    a = ap.parse_args()
    assert a.launches >= 50, "the median needs at least 50 launches"
    assert torch.cuda.is_available(), "augment_bench needs a GPU"
    from simclr_amd.ops import _ext
    ops = _ext.ops()
    has_blur = "blur_kernel" in str(torch.ops.simclr_amd.augment.default._schema)
    dev = torch.device("cuda", 0)
    rows = []
    for size, n, ks in CASES:
        g = torch.Generator().manual_seed(size)
        imgs = torch.randint(0, 256, (n, size, size, 3), dtype=torch.uint8, generator=g).to(dev)
        idx = torch.arange(n, device=dev)
        out = torch.empty((2 * n, size, size, 8), device=dev, dtype=torch.bfloat16)
        off, on = [], []
        for _ in range(a.repeats):  # off and on alternate within a repeat
            off.append(time_case(ops, imgs, idx, out, n, size, 0, a.launches, a.warmup, has_blur))
            if has_blur:
                on.append(time_case(ops, imgs, idx, out, n, size, ks, a.launches, a.warmup, True))
        rows.append((size, n, ks, off, on))
        line = (f"{size}x{size} n={n} views=2: blur off {statistics.median(off):.1f} us "
                f"[{min(off):.1f}, {max(off):.1f}]")
        if on:
            line += (f"  blur on (ks {ks}) {statistics.median(on):.1f} us "
                     f"[{min(on):.1f}, {max(on):.1f}]  "
                     f"on / off {statistics.median(on) / statistics.median(off):.2f}")
        print(line, flush=True)
    if a.md:
        with open(a.md, "w") as fh:
            fh.write(f"`python tools/augment_bench.py --launches {a.launches} --warmup {a.warmup} "
                     f"--repeats {a.repeats}`: median launch time in microseconds [min, max over "
                     "the repeats], 2 views.\n\n")
            fh.write("| output | n | blur kernel | blur off | blur on | on / off |\n")
            fh.write("|---|---|---|---|---|---|\n")
            for size, n, ks, off, on in rows:
                o = statistics.median(off)
                fh.write(f"| {size}x{size} | {n} | {ks} | {o:.1f} [{min(off):.1f}, {max(off):.1f}] | ")
                if on:
                    b = statistics.median(on)
                    fh.write(f"{b:.1f} [{min(on):.1f}, {max(on):.1f}] | {b / o:.2f} |\n")
                else:
                    fh.write("- | - |\n")


if __name__ == "__main__":
    main()
