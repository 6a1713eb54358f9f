"""HIP kernels of csrc/geometry.hip (pair statistics of the Gram triangle, centring, the
second-moment product and its merge) against fp64 torch on the kernels' own bf16 operands and
against the torch twin of ops/geometry.py run on the host on the same inputs.

Pair sums.  The counts are exact.  A and A_same: the fp32 similarity (Dp products) and the tile's
fp32 chain of L = PAIR_CHAIN roundings give (L + Dp) · 2^-24 relative on Σ|d_ij|.  E also carries
the device exp; its error was measured on the MI355X at these shapes (profiles/geometry.md: the
largest relative error of E against the fp64 evaluation is 8.03e-8, at the one pair of N = 2,
where nothing averages out; 2.0e-8 to 3.9e-8 at the larger shapes) and E_RTOL is four times that.
At these shapes one missing tile moves E by more than 10 %; single-pair masking errors are caught
by the exact counts and the one-hot case.

Spectrum.  c is bitwise the twin's.  Every entry of S is within 2 · min(N, 2048) · 2^-24 ·
Σ_b |c_bi c_bj| of the fp64 product of the same c; S is bitwise symmetric; the eigenvalues are
within |S_gpu - S_twin|_F / N of the twin's (Weyl) plus D · 2^-52 · λ_max for each of the two
decompositions' own backward error."""
import functools
import json
import math
import subprocess
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = Path(__file__).resolve().parents[1]
E_RTOL = 3.2e-7  # 4 x 8.03e-8, the largest relative error of E measured at PAIR_SHAPES


def _geo():
    from simclr_amd.ops import _ext
    _ext.require()
    from simclr_amd.ops import geometry
    return geometry


# (2, 64): one pair; (130, 100): D padded to 128, 2 tile rows = 3 tiles, a ragged last tile;
# (257, 64): 3 tile rows = 6 tiles, one row in the last; (384, 512): 6 full tiles, 8 K-steps
PAIR_SHAPES = [(2, 64), (130, 100), (257, 64), (384, 512)]


@functools.lru_cache(maxsize=None)
def _pair_case(N, D):
    """(x, y, the bf16 rows the kernel sees, their fp64 similarities) of one shape, made once."""
    from simclr_amd.ops.knn import normalize_bf16
    g = torch.Generator().manual_seed(100 * N + D)
    x = torch.randn(N, D, generator=g) + 0.3
    y = torch.randint(0, 5, (N,), generator=g)
    y[N - 1] = 5 if N > 2 else y[0]  # a class with a single member; N = 2: one same-class pair
    U = normalize_bf16(x.to(DEV)).cpu().double()
    return x, y, U, U @ U.t()


def _pair_reference(N, D, t):
    _, y, _, S = _pair_case(N, D)
    upper = torch.triu(torch.ones(N, N, dtype=torch.bool), diagonal=1)
    same = upper & (y.view(-1, 1) == y.view(1, -1))
    d = 2.0 - 2.0 * S
    return (float(torch.exp(2 * t * (S - 1))[upper].sum()), float(d[upper].sum()),
            float(d[same].sum()), float(d[upper].abs().sum()), float(d[same].abs().sum()))


@pytest.mark.parametrize("t", [2.0, 0.5])
@pytest.mark.parametrize("labelled", [True, False])
@pytest.mark.parametrize("N,D", PAIR_SHAPES)
def test_pair_sums_match_fp64_reference(N, D, labelled, t):
    geo = _geo()
    x, y, _, _ = _pair_case(N, D)
    got = geo.pair_stats(x.to(DEV), y.to(DEV) if labelled else None, t)
    twin = geo.pair_stats(x, y if labelled else None, t)
    E, A, A_same, abs_d, abs_same = _pair_reference(N, D, t)
    rel = (geo.PAIR_CHAIN + geo.padded_d(D)) * 2.0 ** -24
    print(f"pair {N}x{D} t={t} labelled={labelled}: E rel err {abs(got.E - E) / E:.3e} "
          f"A err {abs(got.A - A):.3e} (bound {rel * abs_d:.3e}) twin E rel err {abs(twin.E - E) / E:.3e}")
    assert got.pairs == twin.pairs == N * (N - 1) // 2
    assert abs(got.A - A) <= rel * abs_d
    assert abs(got.E - E) <= E_RTOL * E
    if labelled:
        assert got.same_pairs == twin.same_pairs
        assert abs(got.A_same - A_same) <= rel * abs_same
    else:
        assert got.A_same is None and got.same_pairs is None and twin.same_pairs is None
    again = geo.pair_stats(x.to(DEV), y.to(DEV) if labelled else None, t)
    assert again == got, "not repeatable"


@pytest.mark.parametrize("t", [2.0, 0.5])
def test_onehot_and_duplicate_rows_are_exact(t):
    """Rows e_{i mod 120} of 130: distinct rows have s = 0, d = 2, e = exp(-2t); the 10 duplicate
    pairs s = 1, d = 0, e = 1 and share their label.  Counts and A are exact; E within the exp's
    3 ulp (the OpenCL bound the device library keeps) on the distinct pairs plus the tile chain."""
    geo = _geo()
    N, distinct = 130, 120
    idx = torch.arange(N) % distinct
    x = torch.zeros(N, 192)
    x[torch.arange(N), idx] = 1.0
    y = idx % 7
    pairs, dup = N * (N - 1) // 2, N - distinct
    same = sum(c * (c - 1) // 2 for c in torch.bincount(y).tolist())
    got = geo.pair_stats(x.to(DEV), y.to(DEV), t)
    assert got.pairs == pairs and got.same_pairs == same
    assert got.A == 2.0 * (pairs - dup) and got.A_same == 2.0 * (same - dup)
    ref = dup + (pairs - dup) * math.exp(-2 * t)
    tol = (pairs - dup) * math.exp(-2 * t) * 3 * 2.0 ** -23 + ref * geo.PAIR_CHAIN * 2.0 ** -24
    print(f"one-hot t={t}: E err {abs(got.E - ref):.3e} tol {tol:.3e}")
    assert abs(got.E - ref) <= tol


# (33, 64): less than a K-step of rows; (2049, 64): one row past a chunk, 2 splits; (300, 192):
# 3 tile columns = 6 tiles; (4100, 128): 3 chunks on 3 splits; (64, 2048): 528 tiles, unsplit;
# (2049, 2048): unsplit with two chunks merged in registers
SPEC_SHAPES = [(33, 64), (2049, 64), (300, 192), (4100, 128), (64, 2048), (2049, 2048)]


@pytest.mark.parametrize("N,D", SPEC_SHAPES)
def test_spectrum_matches_twin_and_fp64_product(N, D):
    geo = _geo()
    from simclr_amd.ops import _ext
    g = torch.Generator().manual_seed(7 * N + D)
    x = torch.randn(N, D, generator=g) * torch.linspace(0.1, 3.0, D) + 1.0
    got = geo.spectrum(x.to(DEV), return_centered=True)
    twin = geo.spectrum(x, return_centered=True)
    Dp = geo.padded_d(D)
    assert _ext.ops().geometry_syrk_splits(N, Dp) == geo.syrk_splits(N, Dp)
    assert torch.equal(got.mean.cpu(), twin.mean)
    assert torch.equal(got.c.cpu().view(torch.int16), twin.c.view(torch.int16))
    c64 = twin.c.double()
    ref = c64.t() @ c64
    bound = 2.0 * min(N, 2048) * 2.0 ** -24 * (c64.abs().t() @ c64.abs())
    err = (got.S - ref).abs()
    print(f"spectrum {N}x{D}: S err max {float(err.max()):.3e} bound at it "
          f"{float(bound.view(-1)[err.argmax()]):.3e} worst ratio {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    assert torch.equal(got.S, got.S.t())
    weyl = float((got.S - twin.S).norm()) / N + 2 * D * 2.0 ** -52 * float(twin.eig[0])
    assert float((got.eig - twin.eig).abs().max()) <= weyl
    again = geo.spectrum(x.to(DEV), return_centered=True)
    assert torch.equal(again.S, got.S) and torch.equal(again.c.view(torch.int16), got.c.view(torch.int16))


def test_signed_axes_effective_rank_on_the_device():
    geo = _geo()
    k, m = 10, 6
    x = torch.zeros(2 * k * m, 64)
    for j in range(k):
        x[2 * j * m:(2 * j + 1) * m, j] = 1.0
        x[(2 * j + 1) * m:(2 * j + 2) * m, j] = -1.0
    x[:, 20] = 3.5
    sp = geo.spectrum(x.to(DEV))
    assert torch.equal(sp.S, torch.diag(torch.tensor([12.0] * k + [0.0] * (64 - k), dtype=torch.float64)))
    met = geo.spectrum_metrics(sp.eig, sp.cov_diag)
    assert met["effective_rank"] == pytest.approx(k, rel=1e-12)
    assert met["participation_ratio"] == pytest.approx(k, rel=1e-12)
    assert met["dims_90"] == 9 and met["dims_99"] == 10 and met["dim_std_min"] == 0.0


def test_limits_raise_before_any_launch():
    geo = _geo()
    from simclr_amd.ops import _ext
    ops = _ext.ops()
    bf = dict(device=DEV, dtype=torch.bfloat16)

    def pair(N=64, Dp=64, t=2.0, xn=None, tiles=None, labels=None):
        xn = torch.zeros(N, Dp, **bf) if xn is None else xn
        tiles = geo.pair_tiles(N) if tiles is None else tiles
        ops.geometry_pair(xn, labels, t, torch.zeros(tiles, 3, device=DEV),
                          torch.zeros(tiles, 2, device=DEV, dtype=torch.int32))

    pair()  # the base case is accepted
    big = torch.zeros(1, 64, **bf).expand(2 ** 25, 64)
    for kw, name in ((dict(N=1), "N must be >= 2"), (dict(Dp=96), "Dp must"), (dict(Dp=4160), "Dp must"),
                     (dict(t=0.0), "t must"), (dict(t=-1.0), "t must"), (dict(t=float("inf")), "t must"),
                     (dict(t=float("nan")), "t must"), (dict(xn=big, tiles=1), r"N \* Dp must"),
                     (dict(tiles=2), "fpart must"),
                     (dict(labels=torch.zeros(63, device=DEV, dtype=torch.int32)), "labels must")):
        with pytest.raises(RuntimeError, match=name):
            pair(**kw)
    x = torch.zeros(100, 70, device=DEV)
    mu = torch.zeros(128, device=DEV)
    with pytest.raises(RuntimeError, match="cT must"):
        ops.geometry_center(x, mu, torch.zeros(128, 100, **bf))
    with pytest.raises(RuntimeError, match="mu must"):
        ops.geometry_center(x, mu[:64], torch.zeros(128, 128, **bf))
    with pytest.raises(RuntimeError, match="N must be >= 2"):
        ops.geometry_center(x[:1], mu, torch.zeros(128, 64, **bf))
    S = torch.zeros(128, 128, device=DEV, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="cT must"):
        ops.geometry_syrk(torch.zeros(128, 128, **bf), 200, S)
    with pytest.raises(RuntimeError, match="S must"):
        ops.geometry_syrk(torch.zeros(128, 128, **bf), 100, S[:64])
    with pytest.raises(RuntimeError, match="Dp must"):
        ops.geometry_syrk(torch.zeros(96, 128, **bf), 100, S)
    # the op's own checks, with the argument named
    with pytest.raises(ValueError, match="N must be >= 2"):
        geo.pair_stats(torch.zeros(1, 64, device=DEV))
    with pytest.raises(ValueError, match="geometry_t"):
        geo.pair_stats(torch.zeros(4, 64, device=DEV), t=float("nan"))
    with pytest.raises(ValueError, match="exceeds 4096"):
        geo.spectrum(torch.zeros(2, 4100, device=DEV))
    with pytest.raises(ValueError, match="2\\^31"):
        geo.spectrum(torch.zeros(1, 2048, device=DEV).expand(2 ** 20, 2048))


def test_nonfinite_features_are_counted_and_nothing_faults():
    geo = _geo()
    from simclr_amd.evaluation.probes import DownstreamDataset, run_probe
    g = torch.Generator().manual_seed(12)
    x = torch.randn(200, 100, generator=g)
    y = torch.arange(200) % 4
    x[3, 2] = float("nan")
    x[150, 99] = float("inf")
    s = geo.pair_stats(x.to(DEV), y.to(DEV))
    assert s.pairs == 19900 and s.same_pairs == 4 * (50 * 49 // 2) and math.isnan(s.E)
    sp = geo.spectrum(x.to(DEV))
    assert bool(torch.isnan(sp.eig).all())
    ds = DownstreamDataset(x.to(DEV), y.to(DEV))
    res = run_probe({"parameter": {}}, "geometry", ds, ds, 4, 5, torch.device(DEV))
    assert res["train_nonfinite"] == 2 and res["train_rows"] == 200 and res["train_pairs"] == 19900
    json.dumps(res)


def test_declined_inputs_take_the_twin(monkeypatch):
    geo = _geo()
    from simclr_amd.ops import registry

    def boom(*a, **k):
        raise AssertionError("the HIP path ran")

    g = torch.Generator().manual_seed(13)
    x = torch.randn(150, 64, generator=g)
    y = torch.arange(150) % 3
    want, want_sp = geo.pair_stats(x, y), geo.spectrum(x)  # CPU tensors: the twin
    prev = registry.get_backend()
    monkeypatch.setattr(geo, "_pair_hip", boom)
    registry.set_backend("torch")
    try:
        got = geo.pair_stats(x.to(DEV), y.to(DEV))
        got_sp = geo.spectrum(x.to(DEV))
    finally:
        registry.set_backend(prev)
    assert got.pairs == want.pairs and got.same_pairs == want.same_pairs
    assert got.E == pytest.approx(want.E, rel=1e-5) and got.A == pytest.approx(want.A, rel=1e-5)
    assert torch.allclose(got_sp.eig, want_sp.eig, rtol=1e-4, atol=1e-9)
    with pytest.raises(AssertionError, match="HIP path ran"):
        geo.pair_stats(x.to(DEV), y.to(DEV))


def test_run_probe_matches_the_cpu_twin():
    _geo()
    from simclr_amd.evaluation.probes import DownstreamDataset, run_probe
    g = torch.Generator().manual_seed(8)
    y = torch.arange(1280) % 10
    x = torch.randn(10, 96, generator=g)[y] + 0.5 * torch.randn(1280, 96, generator=g)
    out = []
    for dev in ("cpu", DEV):
        tr = DownstreamDataset(x[:1024].to(dev), y[:1024].to(dev))
        va = DownstreamDataset(x[1024:].to(dev), y[1024:].to(dev))
        out.append(run_probe({"parameter": {"geometry_t": 1.0}}, "geometry", tr, va, 10, 5,
                             torch.device(dev)))
    cpu, gpu = out
    assert set(cpu) == set(gpu)
    for k in cpu:
        if isinstance(cpu[k], int) or k == "geometry_t":
            assert gpu[k] == cpu[k], k
        else:
            assert gpu[k] == pytest.approx(cpu[k], rel=1e-5, abs=1e-7), k


@pytest.mark.timeout(600)
def test_eval_cli_geometry_on_the_device(tmp_path):
    from simclr_amd.models.contrastive import ContrastiveModel
    torch.manual_seed(5)
    run = tmp_path / "run"
    run.mkdir()
    model = ContrastiveModel(base_cnn="resnet18", d=128)
    torch.save({"module." + k: v for k, v in model.state_dict().items()}, run / "epoch=1-cifar10.pt")
    ev = tmp_path / "ev"
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, str(ROOT / "eval.py"),
                        "data.synthetic=true", "data.synthetic_size=256", "experiment.batches=32",
                        "experiment.base_cnn=resnet18", "parameter.classifier=geometry",
                        "runtime.backend=hip", f"experiment.target_dir={run}", f"hydra.run.dir={ev}"],
                       cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Using cuda" in r.stdout
    res = json.loads((ev / "results.json").read_text())["epoch=1-cifar10.pt"]
    assert res["geometry_t"] == 2.0 and res["dims"] == 512
    assert res["train_rows"] == 256 and res["train_pairs"] == 256 * 255 // 2 and res["val_rows"] == 51
    assert res["train_nonfinite"] == 0 and res["train_uniformity"] <= 0.0
    assert 1.0 <= res["train_effective_rank"] <= 256 and len(res["train_eig_shares"]) == 32
    assert res["train_same_class_pairs"] + res["val_same_class_pairs"] > 0
