"""Geometry probe on the CPU: the torch implementation of the contract in ops/geometry.py against
plain fp64 loops and crafted exact cases, the host metric functions, the configuration checks and
the ``eval.py parameter.classifier=geometry`` command line.

Bounds used below, for unit rows of width Dp (|u_i| <= 1 + 2^-8 after the bf16 rounding):
an fp32 similarity is within ds = Dp · 2^-24 · (1 + 2^-7) of the fp64 one; d = 2 - 2 s adds one
rounding of a value <= 4, so |Δd| <= 2 ds + 2^-22; e = exp(c (s - 1)) with |c (s - 1)| <= 4 t + 1
has the relative error c · ds (the similarity) + (4 t + 1) · 2^-23 (the two roundings of the
argument) + EXP_ULPS · 2^-23 (the exp itself: 3 ulp, the OpenCL bound the device library keeps
and more than the host's)."""
import json
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from simclr_amd.ops import geometry as geo
from simclr_amd.ops.knn import normalize_bf16

ROOT = Path(__file__).resolve().parents[1]
EXP_ULPS = 3
PAIR_KEYS = {"uniformity", "mean_sq_dist", "class_alignment", "class_separation", "pairs",
             "same_class_pairs"}
SPEC_KEYS = {"effective_rank", "rankme", "participation_ratio", "top_eig_share", "dims_90",
             "dims_99", "dim_std_min", "dim_std_median", "dim_std_max", "eig_shares"}
RESULT_KEYS = {"geometry_t", "dims"} | {s + k for s in ("train_", "val_")
                                        for k in PAIR_KEYS | SPEC_KEYS | {"rows", "nonfinite"}}


def term_bounds(Dp, t):
    """(|Δd| per pair, relative error of e) of the module docstring."""
    ds = Dp * 2.0 ** -24 * (1 + 2.0 ** -7)
    return 2 * ds + 2.0 ** -22, 2 * t * ds + (4 * t + 1 + EXP_ULPS) * 2.0 ** -23


def loop_sums(Xn, y, t):
    """The raw sums by a plain fp64 double loop over the pairs i < j of the bf16 rows."""
    U = Xn.double().numpy()
    E = A = A_same = 0.0
    pairs = same = 0
    for i in range(U.shape[0]):
        for j in range(i + 1, U.shape[0]):
            s = float(U[i] @ U[j])
            E += math.exp(2 * t * (s - 1))
            A += 2 - 2 * s
            pairs += 1
            if y is not None and int(y[i]) == int(y[j]):
                A_same += 2 - 2 * s
                same += 1
    return E, A, A_same, pairs, same


# ------------------------------------------------------------------------------ pair part

@pytest.mark.parametrize("t", [2.0, 0.5])
def test_twin_matches_fp64_double_loop(t):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(37, 20, generator=g)
    y = torch.arange(37) % 2
    y[11] = 2  # a class with a single member
    got = geo.pair_stats(x, y, t)
    E, A, A_same, pairs, same = loop_sums(normalize_bf16(x), y, t)
    dd, de = term_bounds(64, t)
    assert got.pairs == pairs == 37 * 36 // 2 and got.same_pairs == same
    assert abs(got.A - A) <= pairs * dd and abs(got.A_same - A_same) <= same * dd
    assert abs(got.E - E) <= de * E
    free = geo.pair_stats(x, None, t)
    assert free.A_same is None and free.same_pairs is None
    assert (free.E, free.A, free.pairs) == (got.E, got.A, got.pairs)
    m = geo.pair_metrics(got)
    assert m["uniformity"] == pytest.approx(math.log(E / pairs), abs=2 * de)
    assert m["class_alignment"] == pytest.approx(A_same / same, abs=dd)
    assert m["class_separation"] == pytest.approx((A - A_same) / (pairs - same), abs=2 * dd)
    assert m["mean_sq_dist"] == pytest.approx(A / pairs, abs=dd)


def test_sum_of_distances_closed_form():
    """Σ_{i<j} |u_i - u_j|² = N Σ|u_i|² - |Σ u_i|²; the bf16 rows are unit only to 2^-8, and
    d_ij = 2 - 2 s_ij differs from |u_i - u_j|² by (|u_i|² - 1) + (|u_j|² - 1), which the right
    side takes out: A = [N Σ|u_i|² - |Σ u_i|²] - (N - 1)(Σ|u_i|² - N), all in fp64."""
    g = torch.Generator().manual_seed(4)
    N = 300  # three tiles of 128 rows: 6 tiles of the triangle
    x = torch.randn(N, 100, generator=g) + 0.5
    U = normalize_bf16(x).double()
    sq = float(U.pow(2).sum())
    closed = N * sq - float(U.sum(0).pow(2).sum()) - (N - 1) * (sq - N)
    got = geo.pair_stats(x)
    assert got.pairs == N * (N - 1) // 2
    assert abs(got.A - closed) <= got.pairs * term_bounds(128, 2.0)[0]


def onehot_case(N=130, D=192, distinct=120, classes=7):
    """Rows e_{i mod distinct}: rows i and i + distinct are duplicates and share their label."""
    idx = torch.arange(N) % distinct
    x = torch.zeros(N, D)
    x[torch.arange(N), idx] = 1.0
    y = idx % classes
    pairs, dup = N * (N - 1) // 2, N - distinct
    cnt = torch.bincount(y).tolist()
    return x, y, pairs, dup, sum(c * (c - 1) // 2 for c in cnt)


def check_onehot(sums, t, pairs, dup, same):
    """Distinct one-hot rows: s = 0, d = 2, e = fp32 exp(-2t); duplicates: s = 1, d = 0, e = 1.
    The counts and A are exact (sums of twos).  E: the exp's EXP_ULPS ulp on every distinct pair
    plus the tile's fp32 chain of PAIR_CHAIN roundings on everything."""
    assert sums.pairs == pairs and sums.same_pairs == same
    assert sums.A == 2.0 * (pairs - dup) and sums.A_same == 2.0 * (same - dup)
    ref = dup + (pairs - dup) * math.exp(-2 * t)
    tol = (pairs - dup) * math.exp(-2 * t) * EXP_ULPS * 2.0 ** -23 + ref * geo.PAIR_CHAIN * 2.0 ** -24
    assert abs(sums.E - ref) <= tol, (sums.E, ref, tol)


@pytest.mark.parametrize("t", [2.0, 0.5])
def test_onehot_rows_are_exact(t):
    x, y, pairs, dup, same = onehot_case()
    check_onehot(geo.pair_stats(x, y, t), t, pairs, dup, same)


def test_pair_metrics_null_on_zero_denominators():
    m = geo.pair_metrics(geo.PairSums(1.5, 3.0, 0.0, 3, 0))  # no two rows share a label
    assert m["class_alignment"] is None and m["class_separation"] == 1.0
    m = geo.pair_metrics(geo.PairSums(1.5, 3.0, 3.0, 3, 3))  # one class
    assert m["class_alignment"] == 1.0 and m["class_separation"] is None
    m = geo.pair_metrics(geo.PairSums(1.5, 3.0, None, 3, None))
    assert m["class_alignment"] is None and m["same_class_pairs"] is None
    assert m["uniformity"] == math.log(0.5) and m["mean_sq_dist"] == 1.0 and m["pairs"] == 3


# ------------------------------------------------------------------------------ spectrum part

def signed_axes(k, m, D=64):
    """m rows +e_j and m rows -e_j for each of k directions: μ = 0, S = diag(N / k)."""
    x = torch.zeros(2 * k * m, D)
    for j in range(k):
        x[2 * j * m:(2 * j + 1) * m, j] = 1.0
        x[(2 * j + 1) * m:(2 * j + 2) * m, j] = -1.0
    return x


@pytest.mark.parametrize("k", [10, 7])
def test_signed_axes_spectrum_is_exact(k):
    x = signed_axes(k, 6)
    x[:, 20] = 3.5  # a constant column: centred away exactly
    N = x.shape[0]
    sp = geo.spectrum(x, return_centered=True)
    assert torch.equal(sp.mean[:64], torch.tensor([0.0] * 20 + [3.5] + [0.0] * 43))
    ref = x.clone()
    ref[:, 20] = 0.0
    assert torch.equal(sp.c.float(), ref)
    assert torch.equal(sp.S, torch.diag(torch.tensor([N / k] * k + [0.0] * (64 - k), dtype=torch.float64)))
    m = geo.spectrum_metrics(sp.eig, sp.cov_diag)
    assert m["effective_rank"] == pytest.approx(k, rel=1e-12)
    assert m["participation_ratio"] == pytest.approx(k, rel=1e-12)
    assert geo.rankme(sp.eig, eps=0.0) == pytest.approx(k, rel=1e-12)
    q = np.sqrt(sp.eig.numpy()) / np.sqrt(sp.eig.numpy()).sum() + 1e-7
    assert m["rankme"] == pytest.approx(float(np.exp(-(q * np.log(q)).sum())), rel=1e-12)
    assert m["dims_90"] == math.ceil(0.9 * k) and m["dims_99"] == k
    assert m["top_eig_share"] == pytest.approx(1 / k, rel=1e-12)
    assert m["dim_std_min"] == 0.0 and m["dim_std_max"] == pytest.approx(math.sqrt(1 / k), rel=1e-12)
    assert len(m["eig_shares"]) == 32 and sum(m["eig_shares"]) == pytest.approx(1.0, rel=1e-12)


def test_rank_one_input():
    v = torch.zeros(64)
    v[:5] = torch.tensor([1.0, -2.0, 0.5, 3.0, 4.0])
    a = torch.tensor([1.0, -1.0] * 20)
    sp = geo.spectrum(a[:, None] * v[None, :])
    m = geo.spectrum_metrics(sp.eig, sp.cov_diag)
    assert m["effective_rank"] == pytest.approx(1.0, abs=1e-9)
    assert m["participation_ratio"] == pytest.approx(1.0, abs=1e-9)
    assert m["dims_90"] == m["dims_99"] == 1 and m["top_eig_share"] == pytest.approx(1.0, abs=1e-12)
    # every row the same point: no variance at all
    z = geo.spectrum(torch.ones(8, 64))
    mz = geo.spectrum_metrics(z.eig, z.cov_diag)
    assert mz["effective_rank"] is None and mz["rankme"] is None and mz["dims_90"] is None
    assert mz["dim_std_max"] == 0.0 and mz["eig_shares"] is None


def test_host_metrics_on_a_written_spectrum():
    lam = np.array([4.0, 2.0, 1.0, 1.0, 0.0])
    p = lam / 8.0
    nz = p[p > 0]
    m = geo.spectrum_metrics(lam, np.array([0.25, 4.0, 1.0, 9.0, 0.0]))
    assert m["effective_rank"] == pytest.approx(float(np.exp(-(nz * np.log(nz)).sum())), rel=1e-15)
    assert m["effective_rank"] == pytest.approx(2 ** 1.75, rel=1e-12)  # H = 1.75 bits
    sv = np.sqrt(lam)
    q = sv / sv.sum() + 1e-7
    assert m["rankme"] == pytest.approx(float(np.exp(-(q * np.log(q)).sum())), rel=1e-15)
    assert m["participation_ratio"] == pytest.approx(64.0 / 22.0, rel=1e-15)
    assert m["top_eig_share"] == 0.5 and m["eig_shares"] == [0.5, 0.25, 0.125, 0.125, 0.0]
    assert m["dims_90"] == 4 and m["dims_99"] == 4  # 0.875 after three
    assert geo.dims_for_share(lam, 0.5) == 1 and geo.dims_for_share(lam, 0.75) == 2
    assert (m["dim_std_min"], m["dim_std_median"], m["dim_std_max"]) == (0.0, 1.0, 3.0)
    nan = geo.spectrum_metrics(np.full(4, np.nan), np.full(4, np.nan))
    assert math.isnan(nan["effective_rank"]) and nan["dims_90"] is None


def product_bound(c, N):
    """(fp64 cᵀc, the per-entry bound 2 · min(N, 2048) · 2^-24 · Σ_b |c_bi c_bj|)."""
    c64 = c.double()
    return c64.t() @ c64, 2.0 * min(N, 2048) * 2.0 ** -24 * (c64.abs().t() @ c64.abs())


@pytest.mark.parametrize("N,D", [(300, 192), (2049, 64), (4100, 128)])
def test_twin_product_meets_the_entry_bound_in_either_row_order(N, D):
    g = torch.Generator().manual_seed(N)
    x = torch.randn(N, D, generator=g) * torch.linspace(0.1, 3.0, D) + 1.0
    sp = geo.spectrum(x, return_centered=True)
    # the mean to an fp32 ulp of the exactly rounded column sums, c from it
    exact = torch.tensor([math.fsum(col) for col in x.double().t().tolist()], dtype=torch.float64) / N
    assert bool(((sp.mean[:D].double() - exact).abs() <= 2.0 ** -23 * exact.abs()).all())
    assert torch.equal(sp.c[:, :D].view(torch.int16),
                       (x - sp.mean[:D]).to(torch.bfloat16).view(torch.int16))
    assert not bool(sp.c[:, D:].any()) and sp.c.shape == (N, geo.padded_d(D))
    ref, bound = product_bound(sp.c, N)
    assert bool(((sp.S - ref).abs() <= bound).all())
    assert bool(((geo._syrk_torch(sp.c.flip(0)) - ref).abs() <= bound).all())
    assert torch.equal(sp.S, sp.S.t())
    cov = ref[:D, :D] / N
    want = torch.linalg.eigvalsh(cov).clamp_min(0).flip(0)
    weyl = float((sp.S - ref).norm()) / N
    assert float((sp.eig - want).abs().max()) <= weyl + 1e-12 * float(want[0])
    assert torch.equal(sp.cov_diag, (sp.S[:D, :D] / N).diagonal())


def test_syrk_splits_rule():
    assert geo.syrk_splits(64, 2048) == 1 and geo.syrk_splits(50000, 2048) == 1  # 528 tiles
    assert geo.syrk_splits(2049, 64) == 2 and geo.syrk_splits(4100, 128) == 3
    assert geo.syrk_splits(33, 64) == 1 and geo.syrk_splits(50000, 512) == 13  # 36 tiles, 25 chunks
    assert geo.pair_tiles(2) == 1 and geo.pair_tiles(130) == 3 and geo.pair_tiles(257) == 6


def test_nonfinite_features_do_not_raise():
    x = torch.randn(40, 16, generator=torch.Generator().manual_seed(1))
    x[3, 2] = float("nan")
    x[7, 0] = float("inf")
    s = geo.pair_stats(x, torch.arange(40) % 3)
    assert s.pairs == 780 and math.isnan(s.E)
    sp = geo.spectrum(x)
    m = geo.spectrum_metrics(sp.eig, sp.cov_diag)
    assert math.isnan(m["effective_rank"]) and m["dims_90"] is None


# ------------------------------------------------------------------------------ limits, configuration

def test_limits_name_the_argument():
    with pytest.raises(ValueError, match="N must be >= 2"):
        geo.pair_stats(torch.randn(1, 8))
    with pytest.raises(ValueError, match="N must be >= 2"):
        geo.spectrum(torch.randn(1, 8))
    with pytest.raises(ValueError, match="Dp 4160 exceeds 4096"):
        geo.check_limits(10, 4160)
    with pytest.raises(ValueError, match="2\\^31"):
        geo.check_limits(2 ** 20, 2048)
    with pytest.raises(ValueError, match="pair statistics"):
        geo.check_limits(128 * 65535 + 1, 64)
    geo.check_limits(128 * 65535 + 1, 64, pairs=False)
    for bad in (0, -1, float("inf"), float("nan"), "lots", True, None):
        if bad is None:
            geo.check_limits(t=bad)
            continue
        with pytest.raises(ValueError, match="geometry_t"):
            geo.check_limits(t=bad)
    with pytest.raises(ValueError, match="geometry_t"):
        geo.pair_stats(torch.randn(4, 8), t=0.0)
    with pytest.raises(ValueError, match="labels"):
        geo.pair_stats(torch.randn(4, 8), torch.zeros(5, dtype=torch.long))
    geo.pair_stats(torch.randn(4, 8), torch.arange(4) * 5000)  # labels are only compared


BASE = {"parameter": {"epochs": 1, "momentum": 0.9, "warmup_epochs": 0, "classifier": "geometry"},
        "experiment": {"batches": 8, "base_cnn": "resnet18", "lr": 0.1, "decay": 0.0,
                       "name": "cifar10"}}


@pytest.mark.parametrize("bad", [0, -1, "lots", True])
def test_validate_rejects_bad_t_and_names_the_key(bad):
    from simclr_amd.config import check_eval_conf
    check_eval_conf(BASE)  # the key is optional
    check_eval_conf({"parameter": dict(BASE["parameter"], geometry_t=0.5),
                     "experiment": BASE["experiment"]})
    cfg = {"parameter": dict(BASE["parameter"], geometry_t=bad), "experiment": BASE["experiment"]}
    with pytest.raises(AssertionError, match="parameter.geometry_t"):
        check_eval_conf(cfg)
    for other in ("centroid", "knn", "kmeans", "linear", "nonlinear"):  # validated with geometry only
        cfg["parameter"]["classifier"] = other
        check_eval_conf(cfg)


def test_validate_rejects_sweep_keys():
    from simclr_amd.config import check_eval_conf
    for key in ("sweep_lr", "sweep_decay"):
        with pytest.raises(AssertionError, match="sweep"):
            check_eval_conf({"parameter": dict(BASE["parameter"], **{key: [0.1]}),
                             "experiment": BASE["experiment"]})


def test_override_parses_from_the_command_line():
    from simclr_amd.config import compose, task_config, CONF_DIR
    cfg = task_config(compose(str(CONF_DIR), "eval", ["parameter.classifier=geometry",
                                                      "+parameter.geometry_t=0.5"]))
    assert cfg["parameter"]["geometry_t"] == 0.5 and cfg["parameter"]["classifier"] == "geometry"
    assert "geometry_t" not in task_config(compose(str(CONF_DIR), "eval", []))["parameter"]


# ------------------------------------------------------------------------------ probe and CLI

def check_result(res, n_train, n_val, dims, t):
    assert set(res) == RESULT_KEYS
    assert res["geometry_t"] == t and isinstance(res["geometry_t"], float) and res["dims"] == dims
    for s, n in (("train_", n_train), ("val_", n_val)):
        assert res[s + "rows"] == n and res[s + "pairs"] == n * (n - 1) // 2
        assert res[s + "nonfinite"] == 0
        for k in ("pairs", "same_class_pairs", "dims_90", "dims_99", "rows", "nonfinite"):
            assert isinstance(res[s + k], int), k
        for k in ("uniformity", "mean_sq_dist", "effective_rank", "rankme", "participation_ratio",
                  "top_eig_share", "dim_std_min", "dim_std_median", "dim_std_max"):
            assert isinstance(res[s + k], float) and math.isfinite(res[s + k]), k
        assert res[s + "uniformity"] <= 0.0 and 0.0 <= res[s + "mean_sq_dist"] <= 4.0
        assert 1.0 <= res[s + "effective_rank"] <= min(n, dims) + 1e-6
        assert 1 <= res[s + "dims_90"] <= res[s + "dims_99"] <= dims
        assert res[s + "dim_std_min"] <= res[s + "dim_std_median"] <= res[s + "dim_std_max"]
        shares = res[s + "eig_shares"]
        assert len(shares) == min(32, dims) and shares == sorted(shares, reverse=True)
        assert shares[0] == res[s + "top_eig_share"]


def test_run_probe_geometry_schema():
    from simclr_amd.evaluation.probes import DownstreamDataset, run_probe
    g = torch.Generator().manual_seed(2)
    y = torch.arange(240) % 4
    centres = torch.randn(4, 40, generator=g)
    x = centres[y] + 0.3 * torch.randn(240, 40, generator=g)
    tr, va = DownstreamDataset(x[:200], y[:200]), DownstreamDataset(x[200:], y[200:])
    res = run_probe({"parameter": {"top_k": 5}}, "geometry", tr, va, 4, 5, torch.device("cpu"))
    check_result(res, 200, 40, 40, 2.0)  # the default temperature
    assert res["train_class_alignment"] < res["train_class_separation"]  # planted classes
    assert res["train_same_class_pairs"] == 4 * (50 * 49 // 2)
    r2 = run_probe({"parameter": {"geometry_t": 0.5, "top_k": 1}}, "geometry", tr, va, 4, 1,
                   torch.device("cpu"))
    assert r2["geometry_t"] == 0.5 and r2["train_uniformity"] > res["train_uniformity"]
    assert r2["train_mean_sq_dist"] == res["train_mean_sq_dist"]
    json.dumps(res)
    for bad in (0, "lots", True):
        with pytest.raises(ValueError, match="parameter.geometry_t"):
            run_probe({"parameter": {"geometry_t": bad}}, "geometry", tr, va, 4, 5, torch.device("cpu"))
    with pytest.raises(ValueError, match="sweep"):
        run_probe({"parameter": {"sweep_lr": [0.1]}, "experiment": {"lr": 0.1, "decay": 0.0}},
                  "geometry", tr, va, 4, 5, torch.device("cpu"))
    with pytest.raises(ValueError, match="geometry"):
        run_probe({"parameter": {}}, "bogus", tr, va, 4, 5, torch.device("cpu"))
    # a non-finite feature is counted and nothing raises
    xb = x.clone()
    xb[5, 3] = float("nan")
    rb = run_probe({"parameter": {}}, "geometry", DownstreamDataset(xb[:200], y[:200]), va, 4, 5,
                   torch.device("cpu"))
    assert rb["train_nonfinite"] == 1 and rb["val_nonfinite"] == 0 and rb["train_pairs"] == 19900
    assert math.isnan(rb["train_uniformity"]) and rb["val_uniformity"] == res["val_uniformity"]


@pytest.mark.timeout(600)
def test_eval_cli_geometry(tmp_path):
    from simclr_amd.models.contrastive import ContrastiveModel
    torch.manual_seed(5)
    run = tmp_path / "run"
    run.mkdir()
    model = ContrastiveModel(base_cnn="resnet18", d=128)
    torch.save({"module." + k: v for k, v in model.state_dict().items()}, run / "epoch=1-cifar10.pt")
    ev = tmp_path / "ev"
    r = subprocess.run([sys.executable, str(ROOT / "eval.py"), "data.synthetic=true",
                        "data.synthetic_size=32", "experiment.batches=8",
                        "experiment.base_cnn=resnet18", "parameter.classifier=geometry",
                        "+parameter.geometry_t=1.5", f"experiment.target_dir={run}",
                        f"hydra.run.dir={ev}"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads((ev / "results.json").read_text())["epoch=1-cifar10.pt"]
    check_result(res, 32, 6, 512, 1.5)
