"""Cost of the online probe in the replayed training step: the headline configuration of bench.py
(ResNet-50 CIFAR stem, 512 images x 2 views, one GPU, streams replay) with ``online_probe.enabled``
off and on, alternating A B A B in one process, and the probe's own launches timed serialized.

Prints one JSON line per round and a summary line.

Usage: python tools/online_probe_bench.py [--steps 20] [--warmup 5] [--rounds 3] [--batch 512]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def build(args, dev, probe: bool):
    """Trainer + loader the way bench.py builds them, captured, on the streams replay."""
    from simclr_amd.config import compose, task_config, CONF_DIR
    from simclr_amd.data.datasets import synthetic_dataset
    from simclr_amd.data.loader import ContrastiveLoader
    from simclr_amd.ops import tuning
    from simclr_amd.parallel import state as pstate
    from simclr_amd.train.pretrain import Trainer
    from simclr_amd.utils.misc import seed_everything
    ov = [f"experiment.base_cnn={args.model}", f"experiment.batches={args.batch}",
          "model.cifar_stem=true", "data.synthetic=true", "runtime.precision=bf16",
          "parameter.epochs=100", f"online_probe.enabled={'true' if probe else 'false'}"]
    cfg = task_config(compose(str(CONF_DIR), "config", ov, job_name="bench"))
    seed_everything(cfg["parameter"]["seed"])
    tiles = ROOT / "bench" / "tiles_mi355x.json"
    if tiles.exists():
        tuning.load_pinned(tiles)
    st = pstate.get()
    st.device = dev
    ds = synthetic_dataset(50000, 10, size=32, seed=0)
    loader = ContrastiveLoader(ds, args.batch, dev, strength=cfg["experiment"]["strength"],
                               seed=7, views=2)
    loader.with_labels = loader.label_i32 = probe
    tr = Trainer(cfg, st, 50000, num_classes=10)
    assert tr.hip, "HIP path not active"
    it = iter(loader)

    def step():
        x, y = next(it)
        return tr.step(x, y) if probe else tr.step(x)

    for _ in range(2):
        step()
    x, y = next(it)
    tr.capture(*((x, y) if probe else (x,)))
    tr.replay_mode = "streams" if tr.sreplay is not None else "graph"
    loader.out, loader.label_out = tr._static_x, tr._static_y
    step()  # the executor's planning replay
    return tr, step


def timed(step, k: int) -> float:
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(k):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / k * 1000.0


def probe_kernels_ms(tr, reps: int = 20) -> dict:
    """The probe's launches of one step, serialized on one stream, per launch (hip events)."""
    p = tr.probe
    ops = torch.ops.simclr_amd
    rows = 2 * tr.cfg["experiment"]["batches"]
    h = torch.randn(rows, p.F, device=p.device).to(torch.bfloat16)
    y = torch.randint(0, p.C, (rows // 2,), device=p.device, dtype=torch.int32)
    out = p._forward_hip(h, y, rows)  # allocates the scratch
    Rp = (rows + 31) // 32 * 32
    s = p._scratch
    Z, loss, rank = s[f"Z{(rows, p.Cp)}"], s[f"loss{(rows,)}"], s[f"rank{(rows,)}"]
    dlT, dbp = s[f"dlT{(p.Cp, Rp)}"], s[f"dbp{(rows // 16, p.Cp)}"]
    acc_l, acc_c = p.acc_loss.clone(), p.acc_cnt.clone()
    launches = {
        "k_oprobe_fwd": lambda: ops.online_probe_forward(out["x"], y, p.Wsh, p.b, p.C, Z, loss,
                                                         rank, dlT, dbp),
        "k_oprobe_metrics": lambda: ops.online_probe_metrics(loss, rank, p.top_k, acc_l, acc_c),
        "k_oprobe_wgrad": lambda: ops.online_probe_wgrad(out["x"], dlT, dbp, p.grad, p.C),
        "k_lr_step": lambda: ops.lr_step(p.step_t.clone(), p.lr_t.clone(), p.lr0, p.warmup,
                                         p.total, 0),
        "k_oprobe_update": lambda: ops.online_probe_update(
            p.master.clone(), p.grad, p.mom.clone(), p.Wsh.clone(), p.lr_t, p.decay, p.momentum,
            p.gscale, p.C, p.F, p.Fp),
    }
    res = {}
    for name, fn in launches.items():
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        res[name] = a.elapsed_time(b) / reps
    res["sum"] = sum(res.values())
    return res


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--model", default="resnet50")
    args = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    arms = {"off": build(args, dev, False), "on": build(args, dev, True)}
    ms = {k: [] for k in arms}
    for r in range(args.rounds):
        for name, (tr, step) in arms.items():
            timed(step, args.warmup)
            ms[name].append(timed(step, args.steps))
        print(json.dumps({"round": r, **{k: round(v[-1], 3) for k, v in ms.items()}}), flush=True)
    tr_on = arms["on"][0]
    kern = probe_kernels_ms(tr_on)
    print(json.dumps({
        "config": f"{args.model} cifar-stem {args.batch}x2 streams-replay",
        "replay": {k: arms[k][0].replay_mode for k in arms},
        "off_ms": [round(v, 3) for v in ms["off"]], "on_ms": [round(v, 3) for v in ms["on"]],
        "on_minus_off_ms": round(min(ms["on"]) - min(ms["off"]), 3),
        "probe_kernels_ms": {k: round(v, 4) for k, v in kern.items()},
        "probe_stream": "side stream of the step (forked after the encoder, joined at the end)",
        "online_rows": int(tr_on.probe.acc_cnt[2])}), flush=True)
    for tr, _ in arms.values():
        if tr.sreplay is not None:
            tr.sreplay.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
