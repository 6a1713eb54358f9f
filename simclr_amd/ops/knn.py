"""Weighted k-nearest-neighbour probe ops (Wu et al., InstDisc): exact top-k cosine neighbours of
every query in a feature bank and the temperature-weighted class vote, on the HIP kernels of
csrc/knn.hip on the GPU and as torch ops of the same contract elsewhere.

Contract (both paths):

* rows are L2-normalised in fp32 (``F.normalize``, eps 1e-12; the norm itself is accumulated in
  fp64 so that it does not depend on the summation order) and rounded once to bf16; everything
  below is exact on those bf16 operands, so the paths differ only by fp32 accumulation order;
* ``sim = q·b`` with fp32 accumulation; the ``k_eff = min(k, N - [self excluded])`` largest per
  query, ordered by (sim descending, bank index ascending); with ``self_offset = s`` bank row
  ``s + i`` is never a neighbour of query ``i``; a NaN similarity is never selected (a slot that
  could not be filled holds ``-inf`` / index ``-1``);
* ``score[c] = Σ_{j in top-k, label_j = c} exp((sim_j - 1) / T)``; the target's rank is the number
  of classes with a larger score, or an equal score and a lower index; a target class without a
  neighbour among the k gets rank C (never correct).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import registry

K_STEP = 64        # the kernels' K-step: operand rows are zero-padded to a multiple of it
MAX_K = 256
MAX_DP = 4096
MAX_CLASSES = 1024
QUERY_CHUNK = 8192  # queries per kernel call: bounds the scratch and the outputs in flight


def _hip_ok(t: torch.Tensor) -> bool:
    return t.is_cuda and registry.use_hip(t)


def normalize_bf16(x: torch.Tensor) -> torch.Tensor:
    """[R][D] fp32 / bf16 -> [R][Dp] bf16: rows L2-normalised in fp32, rounded once, zero-padded."""
    assert x.dim() == 2, "expected [rows][features]"
    R, D = x.shape
    Dp = (D + K_STEP - 1) // K_STEP * K_STEP
    if _hip_ok(x):
        from . import _ext
        if x.dtype not in (torch.float32, torch.bfloat16):
            x = x.float()
        out = torch.empty(R, Dp, device=x.device, dtype=torch.bfloat16)
        if R:
            _ext.ops().knn_normalize(x.contiguous(), out)
        return out
    out = torch.zeros(R, Dp, device=x.device, dtype=torch.bfloat16)
    # the kernel's arithmetic: norm accumulated in fp64 and rounded to fp32 (independent of the
    # summation order), fp32 quotient, one rounding to bf16
    xf = x.float()
    den = xf.double().pow(2).sum(1).sqrt().float().clamp_min(1e-12)
    out[:, :D] = (xf / den[:, None]).to(torch.bfloat16)
    return out


def _topk_torch(qn: torch.Tensor, bn: torch.Tensor, k: int, self_offset: Optional[int],
                chunk: int = 1024) -> Tuple[torch.Tensor, torch.Tensor]:
    Q, N = qn.shape[0], bn.shape[0]
    vals = torch.empty(Q, k, device=qn.device, dtype=torch.float32)
    idx = torch.empty(Q, k, device=qn.device, dtype=torch.int32)
    bt = bn.float().t()
    for s in range(0, Q, chunk):
        sim = qn[s:s + chunk].float() @ bt + 0.0  # -0 -> +0: equal floats tie
        n = sim.shape[0]
        if self_offset is not None:
            col = torch.arange(s, s + n, device=sim.device) + self_offset
            ok = (col >= 0) & (col < N)
            sim[torch.arange(n, device=sim.device)[ok], col[ok]] = float("nan")
        sim = torch.where(torch.isnan(sim), torch.full_like(sim, float("-inf")), sim)
        # a stable descending sort keeps equal similarities in ascending index order
        v, i = torch.sort(sim, dim=1, descending=True, stable=True)
        v, i = v[:, :k], i[:, :k]
        vals[s:s + n] = v
        idx[s:s + n] = torch.where(v == float("-inf"), torch.full_like(i, -1), i).to(torch.int32)
    return vals, idx


def knn_topk(query: torch.Tensor, bank: torch.Tensor, k: int,
             self_offset: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(vals [Q][k_eff] fp32, idx [Q][k_eff] int32): the k_eff most similar bank rows of every
    query row, (sim descending, index ascending).  ``self_offset = s`` excludes bank row ``s + i``
    for query row ``i`` (leave-one-out when the queries are ``bank[s:s + Q]``)."""
    assert query.dim() == 2 and bank.dim() == 2 and query.shape[1] == bank.shape[1], \
        "query [Q][D] and bank [N][D] must share D"
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k must be in [1, {MAX_K}], got {k}")
    Q, N = query.shape[0], bank.shape[0]
    k_eff = max(0, min(k, N - (1 if self_offset is not None else 0)))
    if Q == 0 or k_eff == 0:
        return (torch.empty(Q, k_eff, device=query.device, dtype=torch.float32),
                torch.empty(Q, k_eff, device=query.device, dtype=torch.int32))
    bank = bank.to(query.device)
    bn = normalize_bf16(bank)
    if bn.shape[1] > MAX_DP:
        raise ValueError(f"feature width {query.shape[1]} exceeds {MAX_DP}")
    if not _hip_ok(query):
        return _topk_torch(normalize_bf16(query), bn, k_eff, self_offset)
    from . import _ext
    vals = torch.empty(Q, k_eff, device=query.device, dtype=torch.float32)
    idx = torch.empty(Q, k_eff, device=query.device, dtype=torch.int32)
    for s in range(0, Q, QUERY_CHUNK):
        qn = normalize_bf16(query[s:s + QUERY_CHUNK])
        _ext.ops().knn_topk(qn, bn, k_eff, self_offset is not None, (self_offset or 0) + s,
                            vals[s:s + QUERY_CHUNK], idx[s:s + QUERY_CHUNK])
    return vals, idx


def knn_vote(vals: torch.Tensor, idx: torch.Tensor, bank_labels: torch.Tensor, num_classes: int,
             temperature: float, targets: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(scores [Q][C] fp32, rank [Q] int32) from the sorted neighbours of ``knn_topk``."""
    assert vals.shape == idx.shape and vals.dim() == 2
    if not temperature > 0:
        raise ValueError(f"temperature must be > 0, got {temperature}")
    if not 1 <= num_classes <= MAX_CLASSES:
        raise ValueError(f"num_classes must be in [1, {MAX_CLASSES}], got {num_classes}")
    Q, k = vals.shape
    C = num_classes
    dev = vals.device
    labels = bank_labels.to(device=dev, dtype=torch.long).contiguous()
    targets = targets.to(device=dev, dtype=torch.long).contiguous()
    assert targets.numel() == Q
    scores = torch.zeros(Q, C, device=dev, dtype=torch.float32)
    if Q == 0 or k == 0:
        return scores, torch.full((Q,), C, device=dev, dtype=torch.int32)
    if _hip_ok(vals):
        from . import _ext
        rank = torch.empty(Q, device=dev, dtype=torch.int32)
        _ext.ops().knn_vote(vals.float().contiguous(), idx.to(torch.int32).contiguous(), labels, C,
                            float(temperature), targets, scores, rank)
        return scores, rank
    i64 = idx.long()
    lab = labels[i64.clamp(0, labels.numel() - 1)]
    ok = (i64 >= 0) & (i64 < labels.numel()) & (lab >= 0) & (lab < C)
    lab = lab.clamp(0, C - 1)
    inv_t = torch.tensor(1.0 / temperature, dtype=torch.float32, device=dev)
    w = torch.where(ok, torch.exp((vals.float() - 1.0) * inv_t), torch.zeros_like(vals))
    scores.scatter_add_(1, lab, w)  # sequential along k: the neighbours' sorted order
    hits = torch.zeros(Q, C, device=dev, dtype=torch.float32).scatter_add_(1, lab, ok.float())
    t_ok = (targets >= 0) & (targets < C)
    t = targets.clamp(0, C - 1).view(-1, 1)
    st = scores.gather(1, t)
    cls = torch.arange(C, device=dev).view(1, -1)
    above = ((scores > st) | ((scores == st) & (cls < t))).sum(1)
    hit = t_ok & (hits.gather(1, t).view(-1) > 0)
    rank = torch.where(hit, above, torch.full_like(above, C)).to(torch.int32)
    return scores, rank
