"""Linear-probe sweep on the CPU: the torch twin of ``ops/probe_sweep.py`` against the established
``learnable_eval``, its independence and padding properties, the config limits and the CLI."""
import json
import math
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from simclr_amd.config.validate import check_eval_conf
from simclr_amd.evaluation.probes import DownstreamDataset, learnable_eval, sweep_eval
from simclr_amd.models.heads import LinearClassifier
from simclr_amd.ops import probe_sweep as ps

ROOT = Path(__file__).resolve().parents[1]


def _cfg(epochs=3, bs=512, lr=0.1, decay=1e-4, **extra):
    return {"parameter": dict({"epochs": epochs, "momentum": 0.9, "linear_schedule": True,
                               "seed": 7, "warmup_epochs": 0, "classifier": "linear"}, **extra),
            "experiment": {"batches": bs, "lr": lr, "decay": decay, "base_cnn": "resnet18",
                           "name": "cifar10"}}


def _data(n, F, C, seed, centers=None, noise=1.5):
    g = torch.Generator().manual_seed(seed)
    if centers is None:
        centers = torch.randn(C, F, generator=g)
    y = torch.randint(0, C, (n,), generator=g)
    return DownstreamDataset(centers[y] + noise * torch.randn(n, F, generator=g), y), centers


def _clf(F, C, seed=3):
    torch.manual_seed(seed)
    return LinearClassifier(F, C)


def _copy(clf, dtype):
    c = LinearClassifier(clf.classifier.in_features, clf.classifier.out_features).to(dtype)
    c.load_state_dict({k: v.to(dtype) for k, v in clf.state_dict().items()})
    return c


def _gap(a, b):
    return max(abs(x - y) for x, y in zip(a, b))


def test_twin_matches_learnable_eval():
    """The twin with operand rounding off, G = 1, reproduces ``learnable_eval`` (batch order, the
    cosine table, Nesterov momentum, weight decay on the bias).  Both are fp32 with different
    summation orders, so the tolerance of every quantity is 4x the gap ``learnable_eval`` itself
    shows between fp32 and fp64 execution of this run, measured here on every run.  Measured:
    fp32/fp64 gap of the train / val losses 6.3e-9 / 1.2e-8, of the accuracies 0, of the final
    weight / bias 9.8e-8 / 1.7e-8; the twin's distance to the fp32 run: losses 6.1e-9 / 2.2e-8,
    accuracies 0, weight / bias 6.0e-8 / 1.5e-8."""
    n, F, C = 1200, 48, 10
    train, centers = _data(n, F, C, 0)
    val, _ = _data(300, F, C, 1, centers)
    cfg = _cfg()
    init = _clf(F, C)
    c32, c64 = _copy(init, torch.float32), _copy(init, torch.float64)
    r32 = learnable_eval(cfg, c32, train, val, 5, seed=7)
    r64 = learnable_eval(cfg, c64, DownstreamDataset(train.data.double(), train.targets),
                         DownstreamDataset(val.data.double(), val.targets), 5, seed=7)
    out, sweep = sweep_eval(cfg, _copy(init, torch.float32), train, val, [0.1], [1e-4], 5, seed=7,
                            round_operands=False)
    assert sweep.step == 3 * math.ceil(n / 512) and not sweep.hip
    names = ("train_acc", "train_topk", "train_loss", "val_acc", "val_topk", "val_loss")
    for name, a32, a64, tw in zip(names, r32, r64, out[0]):
        gap, d = _gap(a32, a64), _gap(a32, tw)
        print(f"{name}: fp32/fp64 gap {gap:.3e}, twin vs fp32 {d:.3e}")
        assert len(tw) == 3 and d <= 4 * gap, (name, d, gap)
    W, b = sweep.weights(0)
    for name, p32, p64, tw in (("weight", c32.classifier.weight, c64.classifier.weight, W),
                               ("bias", c32.classifier.bias, c64.classifier.bias, b)):
        gap = float((p32.detach().double() - p64.detach()).abs().max())
        d = float((p32.detach() - tw).abs().max())
        print(f"{name}: fp32/fp64 gap {gap:.3e}, twin vs fp32 {d:.3e}")
        assert gap > 0 and d <= 4 * gap, (name, d, gap)


def test_configuration_is_independent_of_the_sweep():
    """(0.1, 1e-4) inside a 2 x 3 sweep is bitwise the run of that configuration alone."""
    train, centers = _data(700, 40, 10, 2)
    val, _ = _data(200, 40, 10, 3, centers)
    cfg = _cfg(epochs=2, bs=256)
    init = _clf(40, 10)
    lrs, decays = [0.05, 0.1], [0.0, 1e-4, 1e-3]
    j = ps.grid(lrs, decays).index((0.1, 1e-4))
    assert j == 3  # decay-major, lr-minor
    many, sm = sweep_eval(cfg, init, train, val, lrs, decays, 5, seed=7)
    one, s1 = sweep_eval(cfg, init, train, val, [0.1], [1e-4], 5, seed=7)
    assert many[j] == one[0]
    for a, b in zip(sm.weights(j), s1.weights(0)):
        assert torch.equal(a, b)
    assert torch.equal(sm.Wsh.view(6, sm.Cp, sm.Fp)[j], s1.Wsh.view(1, s1.Cp, s1.Fp)[0])
    assert many[j] != many[0]  # the configurations do differ


@pytest.mark.parametrize("C, Cp", [(10, 16), (100, 112)])
def test_padding_columns_never_move(C, Cp):
    n, F = 300, 40
    train, _ = _data(n, F, C, 4)
    init = _clf(F, C)
    lin = init.classifier
    sw = ps.LinearSweep(lin.weight, lin.bias, [0.2, 0.4], [1e-3, 0.0], 0.9, ps.cosine_table(6))
    assert sw.Cp == Cp and sw.Fp == 64 and sw.W.shape == (2 * Cp, 64)
    X = ps.prepare_features(train.data)
    assert X.dtype == torch.bfloat16 and X.shape == (n, 64) and not X[:, F:].any()
    gen = torch.Generator().manual_seed(0)
    for _ in range(2):
        perm = torch.randperm(n, generator=gen)
        for s in range(0, n, 128):
            fwd = sw.forward(X, train.targets, perm[s:s + 128])
            # no probability mass outside the C classes: the softmax of the real columns sums to 1
            prob = torch.softmax(fwd["logits"], 2).sum(2)
            assert fwd["logits"].shape[2] == C and torch.allclose(prob, torch.ones_like(prob))
            # softmax - onehot sums to zero: what is left is the bf16 rounding (2^-8 relative) of C
            # terms of at most 1 / rows each
            rows = fwd["dl"].shape[1]
            assert float(fwd["dl"].sum(2).abs().max()) <= C / rows * 2.0 ** -8 + 1e-6
            sw.update(X, perm[s:s + 128], fwd)
    Wv, bv = sw.W.view(2, Cp, 64), sw.b.view(2, Cp)
    assert not Wv[:, C:].any() and not bv[:, C:].any() and not Wv[:, :, F:].any()
    assert not sw.Mw.view(2, Cp, 64)[:, C:].any() and not sw.Wsh.view(2, Cp, 64)[:, C:].any()
    assert torch.equal(sw.Wsh, sw.W.to(torch.bfloat16))
    assert (sw.weights(0)[0] - lin.weight).abs().max() > 1e-3  # the real columns did move


@pytest.mark.parametrize("extra, exp, msg", [
    ({"sweep_lr": []}, {}, "sweep_lr"),
    ({"sweep_decay": []}, {}, "sweep_decay"),
    ({"sweep_lr": [0.1, 0.0]}, {}, "sweep_lr"),
    ({"sweep_lr": [0.1, -1.0]}, {}, "sweep_lr"),
    ({"sweep_decay": [1e-4, -1e-6]}, {}, "sweep_decay"),
    ({"sweep_lr": [0.01 * (i + 1) for i in range(17)]}, {}, "configurations"),
    ({"sweep_lr": [0.1, 0.2, 0.3], "sweep_decay": [0, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1]}, {},
     "configurations"),
    ({"sweep_lr": [0.01 * (i + 1) for i in range(10)]}, {"name": "cifar100"}, "columns"),
    ({"sweep_lr": [0.1, 0.2], "classifier": "nonlinear"}, {}, "classifier=linear"),
    ({"sweep_lr": [0.1, 0.2]}, {"batches": 8192}, "experiment.batches"),
])
def test_check_eval_conf_rejects(extra, exp, msg):
    cfg = _cfg(**extra)
    cfg["experiment"].update(exp)
    with pytest.raises(AssertionError, match=msg):
        check_eval_conf(cfg)


def test_check_eval_conf_accepts():
    check_eval_conf(_cfg())
    check_eval_conf(_cfg(sweep_lr=None, sweep_decay=None))
    check_eval_conf(_cfg(sweep_lr=[0.05, 0.1, 0.2, 0.4], sweep_decay=[0, 1e-4, 1e-3, 1e-2]))
    c100 = _cfg(sweep_lr=[0.01 * (i + 1) for i in range(9)])  # 9 x 112 = 1008 columns
    c100["experiment"]["name"] = "cifar100"
    check_eval_conf(c100)
    with pytest.raises(ValueError, match="columns"):
        ps.check_limits(2, 1000)
    with pytest.raises(ValueError, match="feature width"):
        ps.check_limits(1, 10, 5000)


def _run(script, args, cwd):
    r = subprocess.run([sys.executable, str(ROOT / script), *args], cwd=str(cwd),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout + r.stderr


@pytest.mark.timeout(600)
def test_cli_sweep_results_schema(tmp_path):
    from simclr_amd.models.contrastive import ContrastiveModel
    run = tmp_path / "run"
    run.mkdir()
    torch.manual_seed(0)
    model = ContrastiveModel("resnet18", 128)
    torch.save({"module." + k: v for k, v in model.state_dict().items()}, run / "epoch=1-cifar10.pt")
    common = ["data.synthetic=true", "data.synthetic_size=32", "experiment.batches=8",
              "parameter.use_cuda=false", f"experiment.target_dir={run}",
              "parameter.classifier=linear", "parameter.epochs=2"]
    ev = tmp_path / "ev"
    _run("eval.py", common + ["parameter.sweep_lr=[0.05,0.2]", "parameter.sweep_decay=[0,1e-4]",
                              f"hydra.run.dir={ev}"], tmp_path)
    res = json.loads((ev / "results.json").read_text())["epoch=1-cifar10.pt"]
    sw = res["sweep"]
    assert [(s["lr"], s["decay"]) for s in sw] == [(0.05, 0.0), (0.2, 0.0), (0.05, 1e-4), (0.2, 1e-4)]
    linear_keys = {"train_accuracies", "val_accuracies", "train_losses", "val_losses",
                   "train_top_5_accuracies", "val_top_5_accuracies", "lowest_val_loss",
                   "highest_val_acc", "highest_val_top_k_acc"}
    for s in sw:
        assert set(s) == linear_keys | {"lr", "decay"} and len(s["val_accuracies"]) == 2
        assert s["highest_val_acc"] == max(s["val_accuracies"])
    accs = [s["highest_val_acc"] for s in sw]
    assert res["best"] == accs.index(max(accs))  # ties to the lowest index
    assert {k: v for k, v in res.items() if k not in ("sweep", "best")} == sw[res["best"]]
    # without the keys: today's schema
    ev2 = tmp_path / "ev2"
    _run("eval.py", common + [f"hydra.run.dir={ev2}"], tmp_path)
    plain = json.loads((ev2 / "results.json").read_text())["epoch=1-cifar10.pt"]
    assert set(plain) == linear_keys
