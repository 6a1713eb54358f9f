"""HIP kernels of csrc/knn.hip (normalise + round, fused similarity / top-k, weighted vote) against
fp64 torch on the kernels' own bf16 operands, and the k-NN probe against the torch fallback.

Similarity tolerance: eps = Dp · 2^-24, the worst-case fp32 accumulation error of a dot product
of Dp terms of unit-norm operands.  The four top-k assertions together are equality with the
reference up to eps-ties, for every query row."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from simclr_amd.ops import _ext
    _ext.require()
    return _ext.ops()


def _check_topk(query, bank, k, self_offset=None):
    """Runs knn_topk twice (bitwise equal) and asserts (a)-(d) against the fp64 reference."""
    from simclr_amd.ops.knn import knn_topk, normalize_bf16
    _ops()
    Q, N = query.shape[0], bank.shape[0]
    vals, idx = knn_topk(query, bank, k, self_offset=self_offset)
    vals2, idx2 = knn_topk(query, bank, k, self_offset=self_offset)
    assert torch.equal(vals, vals2) and torch.equal(idx, idx2), "not repeatable"
    k_eff = min(k, N - (self_offset is not None))
    assert vals.shape == idx.shape == (Q, k_eff)
    qn, bn = normalize_bf16(query), normalize_bf16(bank)
    eps = qn.shape[1] * 2.0 ** -24
    ref = qn.double() @ bn.double().t()
    rows = torch.arange(Q, device=DEV)
    i64 = idx.long()
    # (b) in range, distinct, not self
    assert bool((i64 >= 0).all()) and bool((i64 < N).all())
    srt = i64.sort(dim=1)[0]
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), "duplicate neighbours"
    if self_offset is not None:
        assert not bool((i64 == (rows + self_offset)[:, None]).any()), "self selected"
    # (a) values are the similarities at the returned indices
    err = (vals.double() - ref.gather(1, i64)).abs().max().item()
    assert err <= eps, (err, eps)
    # (c) (val descending, idx ascending)
    dv = vals[:, 1:] - vals[:, :-1]
    assert bool(((dv < 0) | ((dv == 0) & (i64[:, 1:] > i64[:, :-1]))).all()), "order"
    # (d) nothing clearly above the k-th was left out
    chosen = torch.zeros(Q, N, dtype=torch.bool, device=DEV)
    chosen[rows[:, None], i64] = True
    if self_offset is not None:
        s = rows + self_offset
        ok = (s >= 0) & (s < N)
        chosen[rows[ok], s[ok]] = True  # self is excused
    missed = (~chosen) & (ref > (vals[:, -1].double() + eps)[:, None])
    assert not bool(missed.any()), f"{int(missed.sum())} neighbours above the k-th left out"
    return vals, idx


def test_normalize_matches_torch():
    from simclr_amd.ops.knn import normalize_bf16
    _ops()
    torch.manual_seed(0)
    for dt in (torch.float32, torch.bfloat16):
        x = (torch.randn(37, 96, device=DEV) * 3).to(dt)
        xn = normalize_bf16(x)
        assert xn.shape == (37, 128) and xn.dtype == torch.bfloat16
        assert bool((xn[:, 96:] == 0).all())
        ref = torch.nn.functional.normalize(x.double(), dim=1)
        # one rounding to bf16 (2^-9 relative) of an fp32 quotient
        assert torch.allclose(xn[:, :96].double(), ref, rtol=2.0 ** -8, atol=0)
    z = normalize_bf16(torch.zeros(3, 64, device=DEV))
    assert bool((z == 0).all())  # eps: no division by zero


# (130, 3001, 128, 200): ragged Q and N, compactions; (64, 517, 2048, 5): long K loop;
# (257, 8192, 512, 256): maximum k, 8 bank splits, merge; (32, 150, 96, 200): D padding, k > N
@pytest.mark.parametrize("Q,N,D,k", [(130, 3001, 128, 200), (64, 517, 2048, 5),
                                     (257, 8192, 512, 256), (16, 100, 128, 1),
                                     (32, 150, 96, 200)])
def test_topk_matches_fp64_reference(Q, N, D, k):
    torch.manual_seed(10)
    query = torch.randn(Q, D, device=DEV)
    bank = torch.randn(N, D, device=DEV)
    vals, idx = _check_topk(query, bank, k)
    assert vals.shape[1] == min(k, N)


def test_topk_adversarial_ascending_bank():
    """Bank sorted by ascending similarity to the queries' common direction: every tile beats the
    threshold, so the block compacts every few tiles."""
    from simclr_amd.ops.knn import normalize_bf16
    torch.manual_seed(11)
    D = 128
    u = torch.randn(D, device=DEV)
    bank = torch.randn(3001, D, device=DEV)
    order = (normalize_bf16(bank).float() @ u).argsort()
    bank = bank[order].contiguous()
    query = u[None, :] + 0.05 * torch.randn(130, D, device=DEV)
    vals, idx = _check_topk(query, bank, 200)
    assert float(idx.float().mean()) > 2500  # the neighbours sit at the end of the bank


def test_topk_exact_ties_index_ascending():
    torch.manual_seed(12)
    base = torch.randn(700, 128, device=DEV)
    bank = torch.cat([base, base])  # rows j and j + 700 tie exactly
    vals, idx = _check_topk(torch.randn(70, 128, device=DEV), bank, 100)
    assert torch.equal(vals[:, 0::2], vals[:, 1::2])
    assert torch.equal(idx[:, 1::2], idx[:, 0::2] + 700)


def test_topk_self_offset():
    from simclr_amd.ops.knn import knn_topk
    torch.manual_seed(13)
    bank = torch.randn(1000, 128, device=DEV)
    off, Q = 300, 200
    query = bank[off:off + Q].clone()
    _check_topk(query, bank, 50, self_offset=off)
    _, idx = knn_topk(query, bank, 50)
    assert torch.equal(idx[:, 0].long(), torch.arange(off, off + Q, device=DEV))


def test_topk_nan_rows():
    from simclr_amd.ops.knn import knn_topk
    _ops()
    torch.manual_seed(14)
    bank = torch.randn(300, 64, device=DEV)
    bank[7] = float("nan")
    query = torch.randn(20, 64, device=DEV)
    query[5] = float("nan")
    vals, idx = knn_topk(query, bank, 256)
    ok = torch.arange(20, device=DEV) != 5
    assert not bool((idx[ok] == 7).any())
    assert bool((idx[ok, :255] >= 0).all())
    assert bool((idx[5] == -1).all()) and bool((vals[5] == float("-inf")).all())


@pytest.fixture(scope="module")
def neighbours():
    from simclr_amd.ops.knn import knn_topk
    _ops()
    torch.manual_seed(20)
    return knn_topk(torch.randn(130, 128, device=DEV), torch.randn(3001, 128, device=DEV), 200)


@pytest.mark.parametrize("C", [10, 100, 1000])
def test_vote_matches_fp64_scatter_add(neighbours, C):
    from simclr_amd.ops.knn import knn_vote
    vals, idx = neighbours
    Q, T = vals.shape[0], 0.1
    g = torch.Generator().manual_seed(21 + C)
    labels = torch.randint(0, C, (3001,), generator=g).to(DEV)
    targets = torch.randint(0, C, (Q,), generator=g).to(DEV)
    scores, rank = knn_vote(vals, idx, labels, C, T, targets)
    scores2, rank2 = knn_vote(vals, idx, labels, C, T, targets)
    assert torch.equal(scores, scores2) and torch.equal(rank, rank2)
    lab = labels[idx.long()]
    ref = torch.zeros(Q, C, dtype=torch.float64, device=DEV)
    ref.scatter_add_(1, lab, torch.exp((vals.double() - 1.0) / T))
    assert torch.allclose(scores.double(), ref, rtol=1e-5, atol=0)
    t = targets.view(-1, 1)
    st = scores.gather(1, t)
    cls = torch.arange(C, device=DEV).view(1, -1)
    above = ((scores > st) | ((scores == st) & (cls < t))).sum(1)
    hit = (lab == t).any(1)
    want = torch.where(hit, above, torch.full_like(above, C)).to(torch.int32)
    assert torch.equal(rank, want)
    if C == 1000:
        assert bool((~hit).any())  # the rank-C rule is exercised


def test_probe_matches_torch_fallback():
    """knn_eval on the kernels against the torch fallback on the CPU.  Clustered features: seed 30,
    10 centres randn(512), rows centre[y] + 6.0 · randn (fallback top-1 accuracy 0.795, measured
    on the CPU).  k = 20: the k-th neighbour then sits in the sparse upper tail of the
    similarities, where a tie within the two paths' fp32 accumulation difference (~1e-7) is least
    likely; such a tie is the only way the neighbour sets can differ."""
    from simclr_amd.evaluation.probes import DownstreamDataset, knn_eval
    _ops()
    g = torch.Generator().manual_seed(30)
    C, D, noise, k, T = 10, 512, 6.0, 20, 0.1
    centres = torch.randn(C, D, generator=g)
    ytr = torch.randint(0, C, (2048,), generator=g)
    yva = torch.randint(0, C, (512,), generator=g)
    Xtr = centres[ytr] + noise * torch.randn(2048, D, generator=g)
    Xva = centres[yva] + noise * torch.randn(512, D, generator=g)
    cpu_tr, cpu_va = DownstreamDataset(Xtr, ytr), DownstreamDataset(Xva, yva)
    gpu_tr = DownstreamDataset(Xtr.to(DEV), ytr.to(DEV))
    gpu_va = DownstreamDataset(Xva.to(DEV), yva.to(DEV))
    a1, ak, s_cpu = knn_eval(cpu_tr, cpu_va, C, k, T, 5, return_scores=True)
    assert 0.60 < a1 < 0.95, a1
    b1, bk, s_gpu = knn_eval(gpu_tr, gpu_va, C, k, T, 5, return_scores=True)
    assert torch.allclose(s_gpu.cpu(), s_cpu, rtol=1e-4, atol=0)
    assert (a1, ak) == (b1, bk)
