"""Weighted k-NN probe on the CPU: the torch implementation of the contract in ops/knn.py against
a brute-force fp64 computation on the same bf16-rounded operands, a hand-built vote, the probe's
result schema and the ``eval.py parameter.classifier=knn`` command line."""
import json
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from simclr_amd.ops.knn import K_STEP, knn_topk, knn_vote, normalize_bf16

ROOT = Path(__file__).resolve().parents[1]


def _brute(query, bank, k, self_offset=None):
    """Reference neighbours: fp64 similarities of the bf16 operands, python sort by (-sim, idx)."""
    qn, bn = normalize_bf16(query).double(), normalize_bf16(bank).double()
    sim = qn @ bn.t()
    out_v, out_i = [], []
    for i in range(sim.shape[0]):
        cand = [(-float(sim[i, j]), j) for j in range(sim.shape[1])
                if not (self_offset is not None and j == self_offset + i)
                and float(sim[i, j]) == float(sim[i, j])]
        cand.sort()
        out_v.append([-v for v, _ in cand[:k]])
        out_i.append([j for _, j in cand[:k]])
    return out_v, out_i, sim


def test_normalize_rounds_once_and_pads():
    torch.manual_seed(0)
    x = torch.randn(5, 96)
    xn = normalize_bf16(x)
    assert xn.dtype == torch.bfloat16 and xn.shape == (5, 2 * K_STEP)
    ref = torch.nn.functional.normalize(x.double(), dim=1)
    assert torch.allclose(xn[:, :96].double(), ref, rtol=2.0 ** -8, atol=0)  # one bf16 rounding
    assert bool((xn[:, 96:] == 0).all())


@pytest.mark.parametrize("Q,N,D,k,off", [(7, 50, 24, 5, None), (9, 40, 70, 8, 3),
                                         (4, 6, 16, 200, None), (4, 6, 16, 200, 1)])
def test_topk_matches_brute_force(Q, N, D, k, off):
    torch.manual_seed(1)
    bank = torch.randn(N, D)
    query = torch.randn(Q, D) if off is None else bank[off:off + Q].clone()
    vals, idx = knn_topk(query, bank, k, self_offset=off)
    k_eff = min(k, N - (off is not None))  # k > N is clipped
    assert vals.shape == idx.shape == (Q, k_eff)
    assert vals.dtype == torch.float32 and idx.dtype == torch.int32
    rv, ri, sim = _brute(query, bank, k, off)
    assert idx.tolist() == ri  # randn similarities are spaced far above the fp32 error
    assert torch.allclose(vals.double(), torch.tensor(rv, dtype=torch.float64), atol=D * 2.0 ** -24)
    if off is not None:
        assert not bool((idx.long() == (torch.arange(Q) + off)[:, None]).any())
    else:
        q2 = bank[:3].clone()  # without self_offset a bank row finds itself first
        assert knn_topk(q2, bank, 1)[1].view(-1).tolist() == [0, 1, 2]


def test_topk_exact_ties_go_to_the_lower_index():
    torch.manual_seed(2)
    base = torch.randn(12, 32)
    bank = torch.cat([base, base])  # every row twice: rows j and j + 12 tie exactly
    vals, idx = knn_topk(torch.randn(5, 32), bank, 10)
    for r in range(5):
        i, v = idx[r].tolist(), vals[r].tolist()
        for a in range(0, 10, 2):
            assert v[a] == v[a + 1] and i[a + 1] == i[a] + 12 and i[a] < 12
        assert v == sorted(v, reverse=True)


def test_vote_hand_built():
    C, T = 4, 0.5
    #        bank rows:  0  1  2  3  4
    labels = torch.tensor([0, 1, 1, 2, 0])
    vals = torch.tensor([[0.9, 0.5, 0.5, 0.1],
                         [0.8, 0.2, float("-inf"), float("-inf")],
                         [float("-inf")] * 4])
    idx = torch.tensor([[3, 1, 2, 0], [4, 3, -1, -1], [-1] * 4], dtype=torch.int32)
    targets = torch.tensor([1, 3, 0])
    scores, rank = knn_vote(vals, idx, labels, C, T, targets)
    e = lambda s: float(torch.exp(torch.tensor((s - 1.0) / T)))
    want = torch.tensor([[e(0.1), 2 * e(0.5), e(0.9), 0.0], [e(0.8), 0.0, e(0.2), 0.0], [0.0] * 4])
    assert torch.allclose(scores, want, rtol=1e-6)
    # row 0: class 1 (2·e^-1 = 0.736) is below class 2 (e^-0.2 = 0.819): rank 1; row 1: the target
    # class 3 has no neighbour: rank C; row 2: no neighbour at all: rank C
    assert rank.tolist() == [1, C, C] and rank.dtype == torch.int32
    # a tie between two classes goes to the lower class index
    s2, r2 = knn_vote(torch.tensor([[0.5, 0.5]]), torch.tensor([[0, 1]], dtype=torch.int32),
                      labels, C, T, torch.tensor([1]))
    assert r2.tolist() == [1] and float(s2[0, 0]) == float(s2[0, 1])


def test_nan_rows_are_never_selected_and_never_correct():
    torch.manual_seed(3)
    bank = torch.randn(20, 16)
    bank[4] = float("nan")
    labels = torch.arange(20) % 3
    query = torch.randn(6, 16)
    query[2] = float("nan")
    vals, idx = knn_topk(query, bank, 20)
    ok = [r for r in range(6) if r != 2]
    assert not bool((idx[ok] == 4).any())                 # the NaN bank row is never a neighbour
    assert bool((idx[ok, :19] >= 0).all()) and bool((idx[ok, 19] == -1).all())
    assert bool((idx[2] == -1).all())                     # the NaN query has no neighbours
    targets = torch.zeros(6, dtype=torch.long)
    scores, rank = knn_vote(vals, idx, labels, 3, 0.1, targets)
    assert int(rank[2]) == 3 and bool((scores[2] == 0).all())
    assert bool((rank[ok] < 3).all()) and bool(torch.isfinite(scores).all())


def test_run_probe_knn_schema_and_leave_one_out():
    from simclr_amd.evaluation.probes import DownstreamDataset, run_probe
    torch.manual_seed(4)
    C = 4
    ytr, yva = torch.arange(64) % C, torch.arange(24) % C
    centres = torch.randn(C, 32) * 3
    tr = DownstreamDataset(centres[ytr] + torch.randn(64, 32), ytr)
    va = DownstreamDataset(centres[yva] + torch.randn(24, 32), yva)
    cfg = {"parameter": {"knn_k": 5, "knn_t": 0.2, "seed": 0}}
    res = run_probe(cfg, "knn", tr, va, C, 3, torch.device("cpu"))
    assert set(res) == {"train_acc", "train_top_3_acc", "val_acc", "val_top_3_acc", "knn_k", "knn_t"}
    assert res["knn_k"] == 5 and res["knn_t"] == 0.2
    assert res["val_acc"] > 0.9 and res["train_top_3_acc"] >= res["train_acc"] > 0.9
    # leave-one-out: with every label unique to its row, self is the only correct neighbour
    uniq = DownstreamDataset(tr.data, torch.arange(64))
    r1 = run_probe({"parameter": {"knn_k": 1}}, "knn", uniq, uniq, 64, 1, torch.device("cpu"))
    assert r1["train_acc"] == 0.0 and r1["val_acc"] == 1.0 and r1["knn_t"] == 0.1
    with pytest.raises(ValueError, match="knn"):
        run_probe(cfg, "bogus", tr, va, C, 3, torch.device("cpu"))


def test_validate_checks_knn_keys_only_for_knn():
    from simclr_amd.config import check_eval_conf
    base = {"parameter": {"epochs": 1, "momentum": 0.9, "warmup_epochs": 0, "classifier": "knn"},
            "experiment": {"batches": 8, "base_cnn": "resnet18", "lr": 0.1, "decay": 0.0}}
    check_eval_conf(base)  # configs without the keys keep working
    for key, bad in (("knn_k", 0), ("knn_t", 0.0)):
        cfg = {"parameter": dict(base["parameter"], **{key: bad}), "experiment": base["experiment"]}
        with pytest.raises(AssertionError, match=key):
            check_eval_conf(cfg)
        cfg["parameter"]["classifier"] = "centroid"
        check_eval_conf(cfg)


@pytest.mark.timeout(600)
def test_eval_cli_knn(tmp_path):
    from simclr_amd.models.contrastive import ContrastiveModel
    torch.manual_seed(5)
    run = tmp_path / "run"
    run.mkdir()
    model = ContrastiveModel(base_cnn="resnet18", d=128)
    torch.save({"module." + k: v for k, v in model.state_dict().items()}, run / "epoch=1-cifar10.pt")
    ev = tmp_path / "ev"
    r = subprocess.run([sys.executable, str(ROOT / "eval.py"), "data.synthetic=true",
                        "data.synthetic_size=32", "experiment.batches=8",
                        "experiment.base_cnn=resnet18", "parameter.classifier=knn",
                        "parameter.knn_k=3", f"experiment.target_dir={run}",
                        f"hydra.run.dir={ev}"], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads((ev / "results.json").read_text())["epoch=1-cifar10.pt"]
    assert set(res) == {"train_acc", "train_top_5_acc", "val_acc", "val_top_5_acc", "knn_k",
                        "knn_t"}
    assert res["knn_k"] == 3 and res["knn_t"] == 0.1
    assert all(0.0 <= res[m] <= 1.0 for m in ("train_acc", "train_top_5_acc", "val_acc",
                                              "val_top_5_acc"))
