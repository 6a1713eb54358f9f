"""k-means probe on the CPU: the torch implementation of the contract in ops/kmeans.py against a
naive fp64 Lloyd loop, the partition scores against sklearn / scipy and a brute-force matching, the
rules of the contract (ties, NaN, padding columns, empty clusters, fixed point, restart
independence, repeatability), the configuration checks, the probe's result schema and the
``eval.py parameter.classifier=kmeans`` command line."""
import itertools
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from simclr_amd.ops import kmeans as km
from simclr_amd.ops.knn import normalize_bf16

ROOT = Path(__file__).resolve().parents[1]
SCORE_KEYS = {"train_acc", "val_acc", "train_nmi", "val_nmi", "train_ari", "val_ari",
              "train_purity", "val_purity"}
RUN_KEYS = {"kmeans_k", "kmeans_restarts", "kmeans_iters", "best", "objective", "iterations",
            "cluster_sizes"}


def planted(N, F, K, noise, seed):
    """(features, labels, one row index per cluster): K far-apart unit centres plus noise."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.nn.functional.normalize(torch.randn(K, F, generator=g), dim=1)
    y = torch.arange(N) % K
    x = centres[y] + noise * torch.randn(N, F, generator=g) / F ** 0.5
    return x, y, torch.arange(K)


def _naive_lloyd(features, init_rows, T):
    """fp64 spherical Lloyd on the bf16 operands, centroids rounded to bf16 as the contract does."""
    X = normalize_bf16(features).double()
    C = X[init_rows].clone()
    for _ in range(T):
        a = (X @ C.t()).argmax(1)
        for k in range(C.shape[0]):
            rows = X[a == k]
            if len(rows):
                S = rows.sum(0).float()
                den = S.double().pow(2).sum().sqrt().float().clamp_min(1e-12)
                C[k] = (S / den).to(torch.bfloat16).double()
    a = (X @ C.t()).argmax(1)
    return a, torch.bincount(a, minlength=C.shape[0])


def test_twin_matches_naive_fp64_lloyd_on_planted_clusters():
    x, y, rows = planted(600, 48, 7, 0.3, 0)
    fit = km.kmeans_fit(x, 7, restarts=1, iters=6, init=[rows.tolist()])
    a, counts = _naive_lloyd(x, rows, 6)
    assert fit.a.dtype == torch.int32 and fit.s.dtype == torch.float32
    assert fit.centroids.shape == (1, 7, 64) and fit.centroids.dtype == torch.bfloat16
    assert torch.equal(fit.a[0].long(), a)
    assert fit.counts[0].tolist() == counts.tolist()
    assert torch.equal(fit.a[0].long(), y)  # one seed row per planted cluster recovers the classes
    assert fit.changed.shape == (1, 6) and int(fit.changed[0, 0]) == 600
    assert km.iterations(fit.changed)[0] < 6 and fit.best == 0
    assert abs(float(fit.objective[0]) - float(fit.s.double().sum())) < 1e-9


# ------------------------------------------------------------------------------ scores

def _brute_acc(t):
    """Best one-to-one matching by exhaustive search (K, C <= 6)."""
    t = np.asarray(t)
    K, C = t.shape
    best = 0
    if K <= C:
        for cols in itertools.permutations(range(C), K):
            best = max(best, sum(t[k, c] for k, c in enumerate(cols)))
    else:
        for rows in itertools.permutations(range(K), C):
            best = max(best, sum(t[k, c] for c, k in enumerate(rows)))
    return best / t.sum()


@pytest.mark.parametrize("K,C", [(4, 4), (3, 6), (6, 3), (5, 5), (2, 5), (6, 2)])
def test_matching_against_brute_force(K, C):
    rng = np.random.default_rng(K * 10 + C)
    for _ in range(5):
        t = rng.integers(0, 30, size=(K, C))
        sc = km.cluster_scores(t)
        assert sc["acc"] == pytest.approx(_brute_acc(t), abs=1e-12)
        m = km.cluster_matching(t)
        used = [c for c in m if c >= 0]
        assert len(used) == min(K, C) == len(set(used))  # one-to-one, unmatched clusters are -1
        assert sc["purity"] == pytest.approx(t.max(1).sum() / t.sum())


@pytest.mark.parametrize("K,C", [(10, 10), (7, 12), (15, 6)])
def test_scores_against_sklearn_and_scipy(K, C):
    metrics = pytest.importorskip("sklearn.metrics")
    opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(K + C)
    a = rng.integers(0, K, size=500)
    y = np.where(rng.random(500) < 0.6, a % C, rng.integers(0, C, size=500))
    t = km.contingency(torch.from_numpy(a), torch.from_numpy(y), K, C)
    assert t.sum() == 500 and t[a[0], y[0]] >= 1
    sc = km.cluster_scores(t)
    assert sc["nmi"] == pytest.approx(metrics.normalized_mutual_info_score(y, a), abs=1e-10)
    assert sc["ari"] == pytest.approx(metrics.adjusted_rand_score(y, a), abs=1e-10)
    r, c = opt.linear_sum_assignment(t, maximize=True)
    assert sc["acc"] == pytest.approx(t[r, c].sum() / 500, abs=1e-12)


def test_scores_perfect_single_cluster_and_val_with_train_matching():
    perfect = np.array([[0, 9, 0], [7, 0, 0], [0, 0, 5]])
    assert km.cluster_scores(perfect) == {"acc": 1.0, "nmi": 1.0, "ari": 1.0, "purity": 1.0}
    single = np.array([[5, 6, 7], [0, 0, 0]])  # every row in cluster 0
    sc = km.cluster_scores(single)
    assert sc["nmi"] == 0.0 and sc["ari"] == 0.0 and sc["acc"] == pytest.approx(7 / 18)
    assert km.cluster_scores(np.array([[9], [0]]))["nmi"] == 1.0  # one block on both sides
    # K > C: the unmatched cluster counts as wrong, purity does not mind
    t = np.array([[10, 0], [0, 10], [6, 0]])
    sc = km.cluster_scores(t)
    assert sc["acc"] == pytest.approx(20 / 26) and sc["purity"] == 1.0
    # val is scored with the matching found on train, not its own
    m = km.cluster_matching(np.array([[8, 1], [2, 9]]))
    assert m.tolist() == [0, 1]
    assert km.cluster_scores(np.array([[0, 5], [5, 0]]), m)["acc"] == 0.0
    # purity ties: the value does not depend on the tie rule; clusters map to the majority class
    assert km.cluster_scores(np.array([[3, 3], [1, 5]]))["purity"] == pytest.approx(8 / 12)


# ------------------------------------------------------------------------------ contract rules

def test_exact_ties_go_to_the_lowest_k():
    torch.manual_seed(1)
    base = normalize_bf16(torch.randn(5, 64))
    C = torch.cat([base, base])[None]  # centroids k and k + 5 tie exactly
    Xn = normalize_bf16(torch.randn(40, 64))
    a, s = km.assign_step(Xn, C)
    assert bool((a < 5).all())
    assert torch.equal(s[0], (Xn.float() @ base.float().t()).max(1).values)


def test_nan_rows_take_zero_and_nan_never_wins():
    torch.manual_seed(2)
    x = torch.randn(30, 32)
    x[3] = float("nan")
    C = normalize_bf16(torch.randn(6, 32))[None].clone()
    a, s = km.kmeans_assign(x, C)
    assert int(a[0, 3]) == 0 and bool(torch.isnan(s[0, 3]))
    assert not bool(torch.isnan(s[0, [i for i in range(30) if i != 3]]).any())
    C[0, 0] = float("nan")  # a NaN centroid is never chosen by a finite row
    a, _ = km.kmeans_assign(x, C)
    assert not bool((a[0, [i for i in range(30) if i != 3]] == 0).any())


def test_padding_columns_never_win_when_every_similarity_is_negative():
    torch.manual_seed(3)
    K = 37  # padded to 48: a zero padding column would score 0 > every real similarity
    c = normalize_bf16(torch.randn(1, 64))
    C = c.repeat(K, 1)[None]
    a, s = km.assign_step((-c.float()).to(torch.bfloat16).repeat(9, 1), C)
    assert bool((a == 0).all()) and bool((s < -0.9).all())


def test_empty_cluster_keeps_its_bits():
    x, _, rows = planted(200, 32, 4, 0.2, 4)
    Xn = normalize_bf16(x)
    C = Xn[[0, 1, 2, 3]][None].clone()
    a = torch.zeros(1, 200, dtype=torch.int32)  # nobody in clusters 1..3
    S, counts, new = km.update_step(Xn, a, C)
    assert counts.tolist() == [[200, 0, 0, 0]] and bool((S[0, 1:] == 0).all())
    assert torch.equal(new[0, 1:].view(torch.int16), C[0, 1:].view(torch.int16))
    ref = torch.nn.functional.normalize(Xn.double().sum(0), dim=0)
    assert torch.allclose(new[0, 0].double(), ref, atol=2.0 ** -8)


def test_fixed_point_bits_after_convergence():
    x, _, rows = planted(400, 32, 5, 0.3, 5)
    f1 = km.kmeans_fit(x, 5, restarts=1, iters=8, init=[rows.tolist()])
    assert km.iterations(f1.changed)[0] < 8
    f2 = km.kmeans_fit(x, 5, restarts=1, iters=13, init=[rows.tolist()])
    assert torch.equal(f1.centroids.view(torch.int16), f2.centroids.view(torch.int16))
    assert torch.equal(f1.a, f2.a) and torch.equal(f1.s, f2.s)
    assert bool((f2.changed[0, km.iterations(f2.changed)[0]:] == 0).all())


def test_restart_independence_and_repeatability():
    torch.manual_seed(6)
    x = torch.randn(300, 40)
    state = torch.get_rng_state()
    f8 = km.kmeans_fit(x, 6, restarts=8, iters=5, seed=11)
    assert torch.equal(torch.get_rng_state(), state)  # the global generator is not touched
    init = km.draw_init(300, 6, 8, 11)
    assert init[3].tolist() == torch.randperm(300, generator=torch.Generator().manual_seed(14))[:6].tolist()
    for r in (0, 3, 7):
        f1 = km.kmeans_fit(x, 6, restarts=1, iters=5, init=[init[r].tolist()])
        assert torch.equal(f1.a[0], f8.a[r]) and torch.equal(f1.s[0], f8.s[r])
        assert torch.equal(f1.centroids[0].view(torch.int16), f8.centroids[r].view(torch.int16))
        assert torch.equal(f1.changed[0], f8.changed[r])
        assert float(f1.objective[0]) == float(f8.objective[r])
    g8 = km.kmeans_fit(x, 6, restarts=8, iters=5, seed=11)
    assert torch.equal(g8.a, f8.a) and torch.equal(g8.s, f8.s) and g8.best == f8.best
    assert f8.best == int(f8.objective.argmax())


# ------------------------------------------------------------------------------ configuration

BASE = {"parameter": {"epochs": 1, "momentum": 0.9, "warmup_epochs": 0, "classifier": "kmeans"},
        "experiment": {"batches": 8, "base_cnn": "resnet18", "lr": 0.1, "decay": 0.0,
                       "name": "cifar10"}}


@pytest.mark.parametrize("key,bad", [("kmeans_k", 1), ("kmeans_k", 0), ("kmeans_k", 2.5),
                                     ("kmeans_k", 1025), ("kmeans_restarts", 0),
                                     ("kmeans_restarts", 17), ("kmeans_restarts", 1.5),
                                     ("kmeans_iters", 0), ("kmeans_iters", 1001)])
def test_validate_rejects_bad_values_and_names_the_key(key, bad):
    from simclr_amd.config import check_eval_conf
    check_eval_conf(BASE)  # configs without the keys keep working
    cfg = {"parameter": dict(BASE["parameter"], **{key: bad}), "experiment": BASE["experiment"]}
    with pytest.raises(AssertionError, match="parameter." + key):
        check_eval_conf(cfg)
    for other in ("centroid", "knn", "linear", "nonlinear"):  # ignored for the other classifiers
        cfg["parameter"]["classifier"] = other
        check_eval_conf(cfg)


def test_limits():
    from simclr_amd.config import check_eval_conf
    ok = {"parameter": dict(BASE["parameter"], kmeans_k=100, kmeans_restarts=9, kmeans_iters=1000),
          "experiment": BASE["experiment"]}
    check_eval_conf(ok)  # 9 x 112 = 1008 <= 1024
    ok["parameter"]["kmeans_restarts"] = 10  # 1120
    with pytest.raises(AssertionError, match="kmeans_restarts"):
        check_eval_conf(ok)
    with pytest.raises(AssertionError, match="sweep"):
        check_eval_conf({"parameter": dict(BASE["parameter"], sweep_lr=[0.1]),
                         "experiment": BASE["experiment"]})
    x = torch.randn(20, 16)
    with pytest.raises(ValueError, match="kmeans_k"):
        km.kmeans_fit(x, 21, restarts=1, iters=1)  # K <= N
    km.kmeans_fit(x, 20, restarts=1, iters=1)
    with pytest.raises(ValueError, match="kmeans_restarts"):
        km.kmeans_fit(x, 17, restarts=17, iters=1)  # 16 x 32 would be fine, 17 restarts are not
    km.kmeans_fit(x, 17, restarts=16, iters=1)
    with pytest.raises(ValueError, match="kmeans_restarts"):
        km.check_limits(65, 13, 1)  # 13 x 80 = 1040
    km.check_limits(65, 12, 1)
    with pytest.raises(ValueError, match="kmeans_iters"):
        km.kmeans_fit(x, 4, restarts=1, iters=0)
    with pytest.raises(ValueError, match="4096"):
        km.check_limits(4, 1, 1, 100, 4160)
    with pytest.raises(ValueError, match="2\\^31"):
        km.check_limits(4, 1, 1, 2 ** 20, 2048)
    with pytest.raises(ValueError, match="init"):
        km.kmeans_fit(x, 4, restarts=2, iters=1, init=[[0, 1, 2, 3]])


# ------------------------------------------------------------------------------ probe and CLI

def test_run_probe_kmeans_schema():
    from simclr_amd.evaluation.probes import DownstreamDataset, run_probe
    x, y, _ = planted(240, 32, 4, 0.3, 7)
    tr, va = DownstreamDataset(x[:200], y[:200]), DownstreamDataset(x[200:], y[200:])
    cfg = {"parameter": {"kmeans_restarts": 3, "kmeans_iters": 10, "seed": 0, "top_k": 5}}
    res = run_probe(cfg, "kmeans", tr, va, 4, 5, torch.device("cpu"))
    assert set(res) == SCORE_KEYS | RUN_KEYS
    assert res["kmeans_k"] == 4 and res["kmeans_restarts"] == 3 and res["kmeans_iters"] == 10
    assert len(res["objective"]) == len(res["iterations"]) == 3 and len(res["cluster_sizes"]) == 4
    assert sum(res["cluster_sizes"]) == 200 and 0 <= res["best"] < 3
    assert res["objective"][res["best"]] == max(res["objective"]) <= 1.0
    assert all(1 <= t <= 10 for t in res["iterations"])
    for k in SCORE_KEYS:
        assert -1.0 <= res[k] <= 1.0
    assert res["train_purity"] >= res["train_acc"] > 0.7  # planted clusters are found
    # the defaults, and K other than the class count
    r2 = run_probe({"parameter": {"kmeans_k": 6, "kmeans_iters": 3}}, "kmeans", tr, va, 4, 5,
                   torch.device("cpu"))
    assert r2["kmeans_k"] == 6 and r2["kmeans_restarts"] == 8 and len(r2["cluster_sizes"]) == 6
    with pytest.raises(ValueError, match="sweep"):
        run_probe({"parameter": {"sweep_lr": [0.1]}, "experiment": {"lr": 0.1, "decay": 0.0}},
                  "kmeans", tr, va, 4, 5, torch.device("cpu"))
    with pytest.raises(ValueError, match="kmeans"):
        run_probe(cfg, "bogus", tr, va, 4, 5, torch.device("cpu"))


@pytest.mark.timeout(600)
def test_eval_cli_kmeans(tmp_path):
    from simclr_amd.models.contrastive import ContrastiveModel
    torch.manual_seed(5)
    run = tmp_path / "run"
    run.mkdir()
    model = ContrastiveModel(base_cnn="resnet18", d=128)
    torch.save({"module." + k: v for k, v in model.state_dict().items()}, run / "epoch=1-cifar10.pt")
    ev = tmp_path / "ev"
    r = subprocess.run([sys.executable, str(ROOT / "eval.py"), "data.synthetic=true",
                        "data.synthetic_size=32", "experiment.batches=8",
                        "experiment.base_cnn=resnet18", "parameter.classifier=kmeans",
                        "parameter.kmeans_restarts=2", "parameter.kmeans_iters=4",
                        f"experiment.target_dir={run}", f"hydra.run.dir={ev}"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads((ev / "results.json").read_text())["epoch=1-cifar10.pt"]
    assert set(res) == SCORE_KEYS | RUN_KEYS
    assert res["kmeans_k"] == 10 and res["kmeans_restarts"] == 2 and res["kmeans_iters"] == 4
    assert all(0.0 <= res[m] <= 1.0 for m in SCORE_KEYS if "ari" not in m)
    assert -1.0 <= res["train_ari"] <= 1.0 and -1.0 <= res["val_ari"] <= 1.0
