"""HIP kernels of csrc/kmeans.hip (fused similarity / top-1 assignment, one-hot GEMM update, slab
merge + normalise) against fp64 torch on the kernels' own bf16 operands and against the torch twin
of ops/kmeans.py.

Assignment: a row may disagree with the fp64 arg-max only when its fp64 gap between the best and
the second best similarity is below delta = 2 · Fp · 2^-24, the accumulation bound of two fp32 sums
of Fp products of unit rows; at most 1 % of a shape's rows may be that close (asserted first), and
``s`` agrees to delta on every row.  Update: |S - S64| <= n_k · 2^-24 · Σ_i |x_id| per element (n_k
fp32 additions of exactly represented bf16 values), counts exact, a centroid element within the
larger of one bf16 ulp and that bound divided by the norm of the twin's value."""
import json
import subprocess
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = Path(__file__).resolve().parents[1]


def _km():
    from simclr_amd.ops import _ext
    _ext.require()
    from simclr_amd.ops import kmeans
    return kmeans


def _operands(N, F, K, R, seed):
    from simclr_amd.ops.knn import normalize_bf16
    g = torch.Generator().manual_seed(seed)
    Xn = normalize_bf16(torch.randn(N, F, generator=g).to(DEV))
    C = normalize_bf16(torch.randn(R * K, F, generator=g).to(DEV)).view(R, K, -1).contiguous()
    return Xn, C


def _check_assign(Xn, C, a, s, tag=""):
    """(a, s) of the kernel against the fp64 similarities of the same bf16 operands."""
    R, K, Fp = C.shape
    N = Xn.shape[0]
    delta = 2.0 * Fp * 2.0 ** -24
    assert a.shape == s.shape == (R, N) and a.dtype == torch.int32 and s.dtype == torch.float32
    assert bool((a >= 0).all()) and bool((a < K).all())
    for r in range(R):
        ref = Xn.double() @ C[r].double().t()
        top = ref.topk(2, dim=1)
        close = (top.values[:, 0] - top.values[:, 1]) < delta
        share = float(close.double().mean())
        gap = float((top.values[:, 0] - top.values[:, 1]).min())
        bad = (a[r].long() != top.indices[:, 0]) & ~close
        err = float((s[r].double() - top.values[:, 0]).abs().max())
        print(f"{tag} r={r} close {share:.4%} min gap {gap:.2e} mismatches {int(bad.sum())} "
              f"s err {err:.2e} (delta {delta:.2e})")
        assert share <= 0.01, (share, tag)
        assert not bool(bad.any()), (int(bad.sum()), tag)
        assert err <= delta, (err, delta, tag)


def _check_update(Xn, a, C, S, counts, new, tag=""):
    """(S, counts, centroids) of the kernels against the fp64 sums of the given assignments."""
    km = _km()
    R, K, Fp = C.shape
    X64, Xabs = Xn.double(), Xn.double().abs()
    St, ct, newt = km.update_step(Xn, a, C, hip=False)
    assert torch.equal(counts, ct), tag
    for r in range(R):
        ar = a[r].long()
        S64 = torch.zeros(K, Fp, device=DEV, dtype=torch.float64).index_add_(0, ar, X64)
        bound = ct[r].double()[:, None] * 2.0 ** -24 * \
            torch.zeros(K, Fp, device=DEV, dtype=torch.float64).index_add_(0, ar, Xabs)
        err = (S[r].double() - S64).abs()
        print(f"{tag} r={r} S err max {float(err.max()):.2e} bound max {float(bound.max()):.2e}")
        assert bool((err <= bound).all()), (float((err - bound).max()), tag)
        den = St[r].double().pow(2).sum(1).sqrt().clamp_min(1e-12)[:, None]
        ref = newt[r].double()
        ulp = 2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 7)
        cerr = (new[r].double() - ref).abs()
        assert bool((cerr <= torch.maximum(ulp, bound / den)).all()), (float(cerr.max()), tag)
        empty = ct[r] == 0
        assert torch.equal(new[r][empty].view(torch.int16), C[r][empty].view(torch.int16)), tag


# (1008, 200, 37, 3): ragged rows, F padded to 256, K padded to 48; (4096, 128, 100, 8): 896
# centroid rows = 7 column tiles, restarts crossing tile borders; (130, 64, 2, 16): 16 restarts
@pytest.mark.parametrize("N,F,K,R", [(512, 64, 16, 1), (1008, 200, 37, 3), (4096, 128, 100, 8),
                                     (130, 64, 2, 16)])
def test_assign_matches_fp64_reference(N, F, K, R):
    km = _km()
    Xn, C = _operands(N, F, K, R, seed=N + K)
    a, s = km.assign_step(Xn, C)
    _check_assign(Xn, C, a, s, f"assign {N}x{F} K{K} R{R}")
    a2, s2 = km.assign_step(Xn, C)
    assert torch.equal(a, a2) and torch.equal(s, s2), "not repeatable"
    # the counts and the changed rows of the same launch
    _, _, counts, changed = km._assign_hip(Xn, C, prev=a)
    assert changed.tolist() == [0] * R
    for r in range(R):
        assert counts[r].tolist() == torch.bincount(a[r].long(), minlength=K).tolist()
    prev = a.clone()
    prev[:, ::3] = (prev[:, ::3] + 1) % K
    assert km._assign_hip(Xn, C, prev=prev)[3].tolist() == [(N + 2) // 3] * R


def test_ties_nan_and_padding_columns():
    km = _km()
    from simclr_amd.ops.knn import normalize_bf16
    torch.manual_seed(1)
    base = normalize_bf16(torch.randn(5, 64, device=DEV))
    Xn = normalize_bf16(torch.randn(300, 64, device=DEV))
    a, s = km.assign_step(Xn, torch.cat([base, base])[None].contiguous())
    assert bool((a < 5).all())  # centroids k and k + 5 tie exactly: the lowest k
    ref = (Xn.double() @ base.double().t()).max(1).values
    assert float((s[0].double() - ref).abs().max()) <= 2 * 64 * 2.0 ** -24
    # NaN: a NaN row takes 0, a NaN centroid never wins
    x = torch.randn(200, 64, device=DEV)
    x[3] = float("nan")
    C = normalize_bf16(torch.randn(6, 64, device=DEV))[None].clone()
    a, s = km.kmeans_assign(x, C)
    ok = torch.arange(200, device=DEV) != 3
    assert int(a[0, 3]) == 0 and bool(torch.isnan(s[0, 3])) and not bool(torch.isnan(s[0, ok]).any())
    C[0, 0] = float("nan")
    a, _ = km.kmeans_assign(x, C)
    assert int(a[0, 3]) == 0 and not bool((a[0, ok] == 0).any())
    # every real similarity negative: the zero padding columns (K = 37 -> 48) must not win
    c = normalize_bf16(torch.randn(1, 64, device=DEV))
    a, s = km.assign_step((-c.float()).to(torch.bfloat16).repeat(130, 1), c.repeat(37, 1)[None])
    assert bool((a == 0).all()) and bool((s < -0.9).all())


def test_update_matches_fp64_sums():
    km = _km()
    N, F, K, R = 1003, 200, 37, 3  # ragged N: the last K-step of a split and the last split are short
    Xn, C = _operands(N, F, K, R, seed=9)
    g = torch.Generator().manual_seed(10)
    a = torch.randint(0, K, (R, N), generator=g).to(torch.int32)
    a[1][a[1] == 5] = 6    # restart 1: cluster 5 is empty
    a[2][:] = 36           # restart 2: everything in the last cluster
    a = a.to(DEV)
    S, counts, new = km.update_step(Xn, a, C)
    assert int(counts[1, 5]) == 0 and counts[2].tolist() == [0] * 36 + [N]
    _check_update(Xn, a, C, S, counts, new, "update")
    S2, _, new2 = km.update_step(Xn, a, C)
    assert torch.equal(S, S2) and torch.equal(new.view(torch.int16), new2.view(torch.int16))


def test_teacher_forced_iterations():
    """Five Lloyd iterations; the kernel's own centroids go into both paths every iteration."""
    km = _km()
    N, F, K, R = 1008, 200, 37, 3
    Xn, _ = _operands(N, F, K, R, seed=11)
    init = km.draw_init(N, K, R, 3)
    C = Xn[init.view(-1).to(DEV)].view(R, K, -1).contiguous()
    for t in range(5):
        a, s = km.assign_step(Xn, C)
        _check_assign(Xn, C, a, s, f"iter {t}")
        S, counts, new = km.update_step(Xn, a, C)
        _check_update(Xn, a, C, S, counts, new, f"iter {t}")
        C = new


def _planted(N, F, K, noise, seed):
    g = torch.Generator().manual_seed(seed)
    centres = torch.linalg.qr(torch.randn(F, K, generator=g))[0].t().contiguous()
    y = torch.arange(N) % K
    return centres[y] + noise * torch.randn(N, F, generator=g) / F ** 0.5, y


def _planted_case(N, F, K, T):
    km = _km()
    x, y = _planted(N, F, K, 0.3, seed=F + K)
    Nv = 256
    # restart 0: one row per cluster; restart 1: all its rows from class 0 where that has K rows
    bad = torch.arange(K) * K if K * K <= N - Nv else km.draw_init(N - Nv, K, 1, 0)[0]
    init = torch.stack([torch.arange(K), bad])
    twin = km.kmeans_fit(x[:-Nv], K, 2, T, init=init)
    sim = km.normalize_bf16(x[:-Nv]).double() @ twin.centroids[0].double().t()
    top = sim.topk(2, dim=1).values
    assert float((top[:, 0] - top[:, 1]).min()) > 0.4
    fit = km.kmeans_fit(x[:-Nv].to(DEV), K, 2, T, init=init)
    table = km.contingency(fit.a[0], y[:-Nv], K, K)
    assert km.cluster_scores(table)["ari"] == 1.0 and fit.best == 0 == twin.best
    assert (table == km.contingency(twin.a[0], y[:-Nv], K, K)).all()
    assert fit.counts.cpu().tolist() == [torch.bincount(fit.a[r].long().cpu(), minlength=K).tolist()
                                         for r in range(2)]
    assert torch.equal(fit.changed[0], twin.changed[0]) and int(fit.changed[0, 0]) == N - Nv
    va, _ = km.kmeans_assign(x[-Nv:].to(DEV), fit.centroids[0])
    vt, _ = km.kmeans_assign(x[-Nv:], twin.centroids[0])
    assert (km.contingency(va, y[-Nv:], K, K) == km.contingency(vt, y[-Nv:], K, K)).all()
    assert float(fit.objective[0]) == pytest.approx(float(twin.objective[0]), rel=1e-5)
    return fit


def test_planted_clusters_are_recovered():
    _planted_case(2048 + 256, 64, 10, 8)


def test_planted_clusters_wide_features():
    _planted_case(4096 + 256, 2048, 100, 3)


def test_fixed_point_independence_and_repeatability():
    km = _km()
    x, _ = _planted(2048, 64, 10, 0.3, seed=5)
    x = x.to(DEV)
    init = torch.arange(10)[None]
    f1 = km.kmeans_fit(x, 10, 1, 6, init=init)
    assert km.iterations(f1.changed)[0] < 6
    f2 = km.kmeans_fit(x, 10, 1, 11, init=init)  # a converged restart is a fixed point
    assert torch.equal(f1.centroids.view(torch.int16), f2.centroids.view(torch.int16))
    assert torch.equal(f1.a, f2.a) and torch.equal(f1.s, f2.s)
    assert bool((f2.changed[0, km.iterations(f2.changed)[0]:] == 0).all())
    # restart r of an R = 8 run is the R = 1 run with the same initial rows, bit for bit
    g = torch.Generator().manual_seed(6)
    z = torch.randn(1008, 200, generator=g).to(DEV)
    f8 = km.kmeans_fit(z, 37, 8, 4, seed=21)
    init8 = km.draw_init(1008, 37, 8, 21)
    for r in (0, 2, 7):
        f = km.kmeans_fit(z, 37, 1, 4, init=init8[r][None])
        assert torch.equal(f.a[0], f8.a[r]) and torch.equal(f.s[0], f8.s[r]), r
        assert torch.equal(f.centroids[0].view(torch.int16), f8.centroids[r].view(torch.int16)), r
        assert torch.equal(f.changed[0], f8.changed[r]) and torch.equal(f.counts[0], f8.counts[r])
        assert float(f.objective[0]) == float(f8.objective[r])
    g8 = km.kmeans_fit(z, 37, 8, 4, seed=21)  # two runs
    assert torch.equal(g8.a, f8.a) and torch.equal(g8.s, f8.s) and g8.best == f8.best
    assert torch.equal(g8.centroids.view(torch.int16), f8.centroids.view(torch.int16))
    assert torch.equal(g8.objective, f8.objective) and torch.equal(g8.changed, f8.changed)


def test_bindings_reject_out_of_limit_sizes():
    km = _km()
    from simclr_amd.ops import _ext
    ops = _ext.ops()

    def call(N=64, Fp=64, K=4, R=1, T=2, xn=None, cm_rows=None, a_rows=None, t_cols=None):
        Kp = km.padded_k(max(K, 1))
        i32 = dict(device=DEV, dtype=torch.int32)
        xn = torch.zeros(N, Fp, device=DEV, dtype=torch.bfloat16) if xn is None else xn
        cm = torch.zeros(R * Kp if cm_rows is None else cm_rows, Fp, device=DEV, dtype=torch.bfloat16)
        ops.kmeans_fit(xn, cm, K, R, T, torch.zeros(R if a_rows is None else a_rows, N, **i32),
                       torch.zeros(R, N, device=DEV), torch.zeros(R * Kp, **i32),
                       torch.zeros(R, T + 1 if t_cols is None else t_cols, **i32),
                       torch.zeros(R, device=DEV, dtype=torch.float64))

    call()  # the base case is accepted
    big = torch.zeros(1, 64, device=DEV, dtype=torch.bfloat16).expand(2 ** 25, 64)
    for kw, name in ((dict(Fp=96), "Fp must"), (dict(Fp=4160), "Fp must"), (dict(R=0), "R must"),
                     (dict(R=17), "R must"), (dict(K=1), "K must"), (dict(K=65, N=64), "K must be <= N"),
                     (dict(K=100, R=10, N=128), r"R \* Kp"), (dict(T=0), "T must"),
                     (dict(T=1001), "T must"), (dict(cm_rows=8), "cmat must"),
                     (dict(a_rows=2), "a must"), (dict(t_cols=2), "changed must"),
                     (dict(xn=big, N=2 ** 25), "N must")):
        with pytest.raises(RuntimeError, match=name):
            call(**kw)
    Xn, C = _operands(64, 64, 4, 1, 0)
    with pytest.raises(RuntimeError, match="cmat must"):
        ops.kmeans_assign(Xn, C.view(4, 64), 4, 1, torch.zeros(1, 64, device=DEV, dtype=torch.int32),
                          torch.zeros(1, 64, device=DEV), torch.zeros(16, device=DEV, dtype=torch.int32),
                          torch.zeros(1, 1, device=DEV, dtype=torch.int32),
                          torch.zeros(1, device=DEV, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="S must"):
        ops.kmeans_update(Xn, torch.zeros(1, 64, device=DEV, dtype=torch.int32), 4, 1,
                          torch.zeros(16, device=DEV, dtype=torch.int32), km._pack(C),
                          torch.zeros(4, 64, device=DEV), torch.zeros(1, device=DEV, dtype=torch.int32))


def test_run_probe_matches_the_cpu_twin():
    _km()
    from simclr_amd.evaluation.probes import DownstreamDataset, run_probe
    x, y = _planted(2048 + 512, 64, 10, 0.3, seed=8)
    cfg = {"parameter": {"kmeans_restarts": 3, "kmeans_iters": 10, "seed": 4}}
    out = []
    for dev in ("cpu", DEV):
        tr = DownstreamDataset(x[:2048].to(dev), y[:2048].to(dev))
        va = DownstreamDataset(x[2048:].to(dev), y[2048:].to(dev))
        out.append(run_probe(cfg, "kmeans", tr, va, 10, 5, torch.device(dev)))
    cpu, gpu = out
    assert set(cpu) == set(gpu)
    for k in cpu:
        if k == "objective":
            assert gpu[k] == pytest.approx(cpu[k], rel=1e-5)
        else:
            assert gpu[k] == cpu[k], k


@pytest.mark.timeout(900)
def test_cli_pretrains_and_kmeans_reads_the_checkpoint(tmp_path):
    run = tmp_path / "run"
    common = ["data.synthetic=true", "data.synthetic_size=256", "experiment.batches=32",
              "experiment.base_cnn=resnet18"]
    r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, str(ROOT / "main.py"), *common,
                        "parameter.epochs=1", "experiment.save_model_epoch=1",
                        f"hydra.run.dir={run}"], cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert (run / "epoch=1-cifar10.pt").exists()
    ev = tmp_path / "ev"
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, str(ROOT / "eval.py"), *common,
                        "parameter.classifier=kmeans", "parameter.kmeans_restarts=4",
                        "parameter.kmeans_iters=10", f"experiment.target_dir={run}",
                        f"hydra.run.dir={ev}"], cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads((ev / "results.json").read_text())["epoch=1-cifar10.pt"]
    scores = {"train_acc", "val_acc", "train_nmi", "val_nmi", "train_ari", "val_ari",
              "train_purity", "val_purity"}
    assert set(res) == scores | {"kmeans_k", "kmeans_restarts", "kmeans_iters", "best", "objective",
                                 "iterations", "cluster_sizes"}
    assert all(0.0 <= res[m] <= 1.0 for m in scores if "ari" not in m)
    assert -1.0 <= res["train_ari"] <= 1.0 and -1.0 <= res["val_ari"] <= 1.0
    assert res["kmeans_k"] == 10 and len(res["objective"]) == 4 and sum(res["cluster_sizes"]) == 256
