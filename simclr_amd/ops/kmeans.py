"""Spherical k-means probe ops (Lloyd's algorithm on L2-normalised features, R restarts trained in
one pass) and the label-based scores of a partition, on the HIP kernels of csrc/kmeans.hip on the
GPU and as torch ops of the same contract elsewhere.

Contract (both paths):

1. Operands.  ``X = normalize_bf16(features)`` (the k-NN contract of ``ops/knn.py``: rows
   L2-normalised in fp32 with an fp64 norm, rounded once to bf16, zero-padded to ``Fp``).
   Everything below is exact on those operands up to the fp32 summation order.
2. Initialisation.  Restart r takes the rows
   ``torch.randperm(N, generator=torch.Generator().manual_seed(seed + r))[:K]`` of X as its
   centroids; the permutation is drawn on the CPU on both paths and the global generator is not
   touched.  ``init`` ([R][K] row indices) replaces the draw.
3. Assign.  ``sim_ik = x_i·c_k`` with fp32 accumulation; ``a_i`` is the arg-max under the total
   order (sim descending, k ascending): exact ties go to the lowest k.  A NaN never wins; a row
   with only NaN similarities takes 0 (its ``s_i`` is NaN).  Padding columns ``k >= K`` never win,
   also when every real similarity is negative.  The best similarity ``s_i`` is kept in fp32.
4. Update.  ``S_k = Σ_{i: a_i = k} x_i`` in fp32, in a fixed order (row chunks in order, then the
   chunks merged in order; no floating-point atomics; this path forms S in fp64 and rounds it to
   fp32, which makes it the oracle).  The integer counts ``n_k`` are exact.
   ``c_k <- bf16(S_k / max(|S_k|, 1e-12))`` with the norm in fp64, as ``normalize_bf16`` does.  A
   cluster with ``n_k = 0`` keeps its previous centroid bit for bit.
5. Schedule.  T iterations of assign then update, then one final assign, which gives ``a``, ``s``
   and the final ``n_k``.  ``changed[r][t]`` is the number of rows whose assignment differs from
   iteration t - 1 (``changed[r][0] = N``); on the device it is an int32 array read once at the
   end, and no host value that changes per iteration reaches a launch.  ``iterations`` of a restart
   is the first t with ``changed == 0``, else T.  A converged restart is a fixed point (further
   iterations reproduce its centroids and assignments bit for bit), so nothing stops early.
6. Objective.  ``J_r = Σ_i s_i`` in fp64 in a fixed order; ``best`` is the arg-max of J, ties to
   the lowest r.
7. Independence and repeatability.  A restart's trajectory is bitwise independent of R and of the
   other restarts; two runs on one device give the same bits.
8. Val rows are assigned by one more assign pass against the best restart's final centroids.
9. Scores are computed on the host in fp64 from the integer contingency tables ``n[k][c]``: NMI
   (natural logs, arithmetic-mean normalisation, 1.0 when both partitions are a single block), ARI,
   purity (every cluster maps to its majority class, ties to the lower class) and ``acc``, the
   maximum-weight one-to-one matching of clusters to classes (rectangular when K != C; unmatched
   clusters count as wrong; val is scored with the train matching).

Limits: ``2 <= K <= N``, ``1 <= R <= 16``, ``1 <= T <= 1000``, ``Kp = 16·ceil(K/16)``,
``R·Kp <= 1024``, ``Fp <= 4096`` and ``N·Fp < 2^31`` (the kernels' 32-bit offsets).
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import registry
from .knn import K_STEP, normalize_bf16

MAX_RESTARTS = 16
MAX_ITERS = 1000
MAX_COLS = 1024    # R * Kp
MAX_FP = 4096
CHUNK = 8192       # rows per similarity block of the torch path


class KMeansFit(NamedTuple):
    centroids: torch.Tensor   # [R][K][Fp] bf16
    a: torch.Tensor           # [R][N] int32, the final assignment
    s: torch.Tensor           # [R][N] fp32, the similarity to the assigned centroid
    objective: torch.Tensor   # [R] fp64 (CPU): J_r
    changed: torch.Tensor     # [R][T] int32 (CPU)
    best: int
    counts: torch.Tensor      # [R][K] int32: the final cluster sizes


def _hip_ok(t: torch.Tensor) -> bool:
    return t.is_cuda and registry.use_hip(t)


def padded_k(K: int) -> int:
    return (K + 15) // 16 * 16


def check_limits(K, restarts, iters, N: Optional[int] = None, Fp: Optional[int] = None) -> None:
    """Raises ValueError naming the failing ``parameter.`` key.  ``None`` skips a check."""
    def is_int(v):
        return isinstance(v, int) and not isinstance(v, bool)
    if restarts is not None and not (is_int(restarts) and 1 <= restarts <= MAX_RESTARTS):
        raise ValueError(f"kmeans_restarts must be an integer in [1, {MAX_RESTARTS}], got {restarts!r}")
    if iters is not None and not (is_int(iters) and 1 <= iters <= MAX_ITERS):
        raise ValueError(f"kmeans_iters must be an integer in [1, {MAX_ITERS}], got {iters!r}")
    if K is not None:
        if not (is_int(K) and K >= 2):
            raise ValueError(f"kmeans_k must be an integer >= 2, got {K!r}")
        if N is not None and K > N:
            raise ValueError(f"kmeans_k must be <= the number of train rows {N}, got {K}")
        if padded_k(K) > MAX_COLS:
            raise ValueError(f"kmeans_k padded to {padded_k(K)} exceeds {MAX_COLS}")
        if restarts is not None and restarts * padded_k(K) > MAX_COLS:
            raise ValueError(f"kmeans_restarts x kmeans_k padded to 16 must be <= {MAX_COLS}, got "
                             f"{restarts} x {padded_k(K)}")
    if Fp is not None and Fp > MAX_FP:
        raise ValueError(f"feature width padded to {Fp} exceeds {MAX_FP}")
    if N is not None and Fp is not None and N * Fp >= 2 ** 31:
        raise ValueError(f"rows x padded feature width must be < 2^31, got {N} x {Fp}")


# ------------------------------------------------------------------------------ torch path

def _assign_torch(Xn: torch.Tensor, C: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    R, K, _ = C.shape
    N = Xn.shape[0]
    a = torch.empty(R, N, device=Xn.device, dtype=torch.int32)
    s = torch.empty(R, N, device=Xn.device, dtype=torch.float32)
    cols = torch.arange(K, device=Xn.device).view(1, -1)
    for r in range(R):
        ct = C[r].float().t()
        for b in range(0, N, CHUNK):
            sim = Xn[b:b + CHUNK].float() @ ct + 0.0  # -0 -> +0: equal floats tie
            nan = torch.isnan(sim)
            sim = torch.where(nan, torch.full_like(sim, float("-inf")), sim)
            m = sim.max(1).values
            first = torch.where(sim == m[:, None], cols, torch.full_like(cols, K)).min(1).values
            a[r, b:b + CHUNK] = first.to(torch.int32)
            s[r, b:b + CHUNK] = torch.where(nan.all(1), torch.full_like(m, float("nan")), m)
    return a, s


def _update_torch(Xn: torch.Tensor, a: torch.Tensor, C: torch.Tensor
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    R, K, Fp = C.shape
    X64 = Xn.double()
    S = torch.empty(R, K, Fp, device=Xn.device, dtype=torch.float32)
    counts = torch.empty(R, K, device=Xn.device, dtype=torch.int32)
    for r in range(R):
        ar = a[r].long()
        S[r] = torch.zeros(K, Fp, device=Xn.device, dtype=torch.float64).index_add_(0, ar, X64).float()
        counts[r] = torch.bincount(ar, minlength=K)[:K].to(torch.int32)
    den = S.double().pow(2).sum(2).sqrt().float().clamp_min(1e-12)
    new = (S / den[:, :, None]).to(torch.bfloat16)
    return S, counts, torch.where((counts > 0)[:, :, None], new, C)


# ------------------------------------------------------------------------------ HIP path

def _pack(C: torch.Tensor) -> torch.Tensor:
    """[R][K][Fp] -> the kernels' [R * Kp][Fp] matrix (padding rows zero)."""
    R, K, Fp = C.shape
    cm = torch.zeros(R, padded_k(K), Fp, device=C.device, dtype=torch.bfloat16)
    cm[:, :K] = C
    return cm.view(-1, Fp)


def _unpack(cm: torch.Tensor, R: int, K: int) -> torch.Tensor:
    return cm.view(R, padded_k(K), -1)[:, :K].contiguous()


def _assign_hip(Xn, C, prev=None):
    from . import _ext
    R, K, _ = C.shape
    N, dev = Xn.shape[0], Xn.device
    a = (torch.full((R, N), -1, device=dev, dtype=torch.int32) if prev is None
         else prev.to(torch.int32).clone().contiguous())
    s = torch.empty(R, N, device=dev, dtype=torch.float32)
    counts = torch.zeros(R * padded_k(K), device=dev, dtype=torch.int32)
    changed = torch.zeros(R, 1, device=dev, dtype=torch.int32)
    it = torch.zeros(1, device=dev, dtype=torch.int32)
    _ext.ops().kmeans_assign(Xn, _pack(C), K, R, a, s, counts, changed, it)
    return a, s, counts.view(R, -1)[:, :K].contiguous(), changed.view(R)


def _update_hip(Xn, a, C):
    from . import _ext
    R, K, Fp = C.shape
    Kp, dev = padded_k(K), Xn.device
    a = a.to(torch.int32).contiguous()
    cnt = torch.zeros(R, Kp, device=dev, dtype=torch.int32)
    for r in range(R):  # exact integer counts of the given assignments
        cnt[r, :K] = torch.bincount(a[r].long().clamp(0, K - 1), minlength=K)[:K]
    counts = cnt[:, :K].contiguous()
    cm = _pack(C)
    S = torch.empty(R * Kp, Fp, device=dev, dtype=torch.float32)
    it = torch.zeros(1, device=dev, dtype=torch.int32)
    _ext.ops().kmeans_update(Xn, a, K, R, cnt.view(-1), cm, S, it)
    return S.view(R, Kp, Fp)[:, :K].contiguous(), counts, _unpack(cm, R, K)


def assign_step(Xn: torch.Tensor, C: torch.Tensor, hip: Optional[bool] = None):
    """One assign pass on prepared operands: Xn [N][Fp] bf16, C [R][K][Fp] bf16 -> (a, s) [R][N]."""
    if _hip_ok(Xn) if hip is None else hip:
        return _assign_hip(Xn, C)[:2]
    return _assign_torch(Xn, C)


def update_step(Xn: torch.Tensor, a: torch.Tensor, C: torch.Tensor, hip: Optional[bool] = None):
    """One update on prepared operands -> (S [R][K][Fp] fp32, counts [R][K] int32, new centroids)."""
    if _hip_ok(Xn) if hip is None else hip:
        return _update_hip(Xn, a, C)
    return _update_torch(Xn, a, C)


# ------------------------------------------------------------------------------ public ops

def draw_init(N: int, K: int, restarts: int, seed: int) -> torch.Tensor:
    """[R][K] row indices: restart r takes the first K of a CPU permutation seeded ``seed + r``."""
    return torch.stack([torch.randperm(N, generator=torch.Generator().manual_seed(seed + r))[:K]
                        for r in range(restarts)])


def kmeans_fit(features: torch.Tensor, K: int, restarts: int = 8, iters: int = 50, seed: int = 0,
               init: Optional[Sequence[Sequence[int]]] = None, hip: Optional[bool] = None) -> KMeansFit:
    """Spherical k-means of ``features`` [N][F]: ``restarts`` runs of ``iters`` Lloyd iterations in
    one pass.  ``init`` ([R][K] row indices) replaces the seeded draw of the initial centroids."""
    assert features.dim() == 2, "expected [rows][features]"
    N, F = features.shape
    Fp = (F + K_STEP - 1) // K_STEP * K_STEP
    check_limits(K, restarts, iters, N, Fp)
    if init is None:
        init = draw_init(N, K, restarts, seed)
    init = torch.as_tensor(init, dtype=torch.long)
    if tuple(init.shape) != (restarts, K) or bool((init < 0).any()) or bool((init >= N).any()):
        raise ValueError(f"init must be [restarts][K] = [{restarts}][{K}] row indices in [0, {N})")
    Xn = normalize_bf16(features)
    dev = Xn.device
    C = Xn[init.to(dev).view(-1)].view(restarts, K, Fp).contiguous()
    R, T = restarts, iters
    if _hip_ok(Xn) if hip is None else hip:
        from . import _ext
        cm = _pack(C)
        a = torch.empty(R, N, device=dev, dtype=torch.int32)
        s = torch.empty(R, N, device=dev, dtype=torch.float32)
        counts = torch.empty(R * padded_k(K), device=dev, dtype=torch.int32)
        changed = torch.empty(R, T + 1, device=dev, dtype=torch.int32)
        J = torch.empty(R, device=dev, dtype=torch.float64)
        _ext.ops().kmeans_fit(Xn, cm, K, R, T, a, s, counts, changed, J)
        C = _unpack(cm, R, K)
        counts = counts.view(R, -1)[:, :K].contiguous()
        changed, J = changed[:, :T].cpu(), J.cpu()  # the one read-back
    else:
        prev = torch.full((R, N), -1, device=dev, dtype=torch.int32)
        changed = torch.zeros(R, T, dtype=torch.int32)
        for t in range(T):
            a, _ = _assign_torch(Xn, C)
            changed[:, t] = (a != prev).sum(1).cpu().to(torch.int32)
            prev = a
            _, _, C = _update_torch(Xn, a, C)
        a, s = _assign_torch(Xn, C)
        counts = torch.stack([torch.bincount(a[r].long(), minlength=K)[:K] for r in range(R)]
                             ).to(torch.int32)
        J = s.double().sum(1).cpu()
    order = torch.where(torch.isnan(J), torch.full_like(J, float("-inf")), J)
    best = int(torch.where(order == order.max())[0][0])
    return KMeansFit(C, a, s, J, changed, best, counts)


def iterations(changed: torch.Tensor) -> List[int]:
    """Per restart: the first t with ``changed[r][t] == 0``, else T."""
    out = []
    for row in changed.tolist():
        out.append(next((t for t, c in enumerate(row) if c == 0), len(row)))
    return out


def kmeans_assign(features: torch.Tensor, centroids: torch.Tensor, hip: Optional[bool] = None
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(a int32, s fp32): one assign pass of ``features`` [N][F] against ``centroids`` ([K][Fp]
    -> [N] outputs, or [R][K][Fp] -> [R][N]), the bf16 centroids of ``kmeans_fit``."""
    single = centroids.dim() == 2
    C = (centroids[None] if single else centroids).to(device=features.device, dtype=torch.bfloat16)
    Xn = normalize_bf16(features)
    if C.dim() != 3 or C.shape[2] != Xn.shape[1]:
        raise ValueError(f"centroids must be [K][{Xn.shape[1]}] or [R][K][{Xn.shape[1]}]")
    check_limits(C.shape[1], C.shape[0], None, None, Xn.shape[1])
    if Xn.shape[0] == 0:
        a = torch.empty(C.shape[0], 0, device=Xn.device, dtype=torch.int32)
        s = torch.empty(C.shape[0], 0, device=Xn.device, dtype=torch.float32)
    else:
        a, s = assign_step(Xn, C.contiguous(), hip)
    return (a[0], s[0]) if single else (a, s)


# ------------------------------------------------------------------------------ scores (host, fp64)

def contingency(a: torch.Tensor, y: torch.Tensor, K: int, C: int) -> np.ndarray:
    """n[k][c]: the number of rows in cluster k with label c, int64."""
    a64 = a.detach().to("cpu", torch.long).view(-1)
    y64 = y.detach().to("cpu", torch.long).view(-1)
    assert a64.numel() == y64.numel()
    ok = (a64 >= 0) & (a64 < K) & (y64 >= 0) & (y64 < C)
    flat = torch.bincount(a64[ok] * C + y64[ok], minlength=K * C)
    return flat.view(K, C).numpy().astype(np.int64)


def linear_assignment_max(weights) -> List[Tuple[int, int]]:
    """Maximum-weight one-to-one matching of the rows and columns of a rectangular table: the
    min(rows, cols) pairs (row, col), by the Hungarian algorithm with potentials, O(n^2 m)."""
    w = np.asarray(weights, dtype=np.float64)
    flip = w.shape[0] > w.shape[1]
    if flip:
        w = w.T
    n, m = w.shape
    if n == 0:
        return []
    cost = w.max() - w
    u, v = np.zeros(n + 1), np.zeros(m + 1)
    p, way = np.zeros(m + 1, dtype=np.int64), np.zeros(m + 1, dtype=np.int64)
    for i in range(1, n + 1):
        p[0] = i
        j0 = 0
        minv = np.full(m + 1, np.inf)
        used = np.zeros(m + 1, dtype=bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            cur = cost[i0 - 1] - u[i0] - v[1:]
            free = ~used[1:]
            better = free & (cur < minv[1:])
            minv[1:][better] = cur[better]
            way[1:][better] = j0
            cand = np.where(free, minv[1:], np.inf)
            j1 = int(np.argmin(cand)) + 1
            delta = cand[j1 - 1]
            u[p[used]] += delta
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    pairs = [(int(p[j]) - 1, j - 1) for j in range(1, m + 1) if p[j]]
    if flip:
        pairs = [(c, r) for r, c in pairs]
    return sorted(pairs)


def cluster_matching(table) -> np.ndarray:
    """map[k]: the class matched to cluster k by the maximum-weight matching, -1 if unmatched."""
    t = np.asarray(table, dtype=np.int64)
    out = np.full(t.shape[0], -1, dtype=np.int64)
    for k, c in linear_assignment_max(t):
        out[k] = c
    return out


def _entropy(counts: np.ndarray, n: float) -> float:
    c = counts[counts > 0].astype(np.float64)
    return float(-(c / n * np.log(c / n)).sum())


def cluster_scores(table, matching: Optional[np.ndarray] = None) -> Dict[str, float]:
    """acc / nmi / ari / purity of the contingency table n[k][c].  ``matching`` (``map[k]``, as
    ``cluster_matching`` returns) scores ``acc`` with a matching found elsewhere (val with train's)."""
    t = np.asarray(table, dtype=np.int64)
    n = float(t.sum())
    if n == 0:
        return {"acc": 0.0, "nmi": 0.0, "ari": 0.0, "purity": 0.0}
    rows, cols = t.sum(1), t.sum(0)
    if matching is None:
        matching = cluster_matching(t)
    acc = sum(int(t[k, c]) for k, c in enumerate(matching) if c >= 0) / n
    purity = float(t.max(1).sum()) / n
    comb = lambda x: (x.astype(np.float64) * (x.astype(np.float64) - 1.0) / 2.0).sum()
    sij, sa, sb, tot = comb(t), comb(rows), comb(cols), n * (n - 1.0) / 2.0
    same = (np.count_nonzero(t, axis=1) <= 1).all() and (np.count_nonzero(t, axis=0) <= 1).all()
    hk, hc = _entropy(rows, n), _entropy(cols, n)
    if same:  # the same partition up to the names (also: one block on both sides): exactly 1
        nmi = 1.0
    else:
        kk, cc = np.nonzero(t)
        nij = t[kk, cc].astype(np.float64)
        mi = float((nij / n * (np.log(nij * n) - np.log(rows[kk].astype(np.float64) * cols[cc]))).sum())
        nmi = min(1.0, max(0.0, mi / (0.5 * (hk + hc))))
    if same:
        ari = 1.0
    else:
        exp = sa * sb / tot
        ari = float((sij - exp) / (0.5 * (sa + sb) - exp))
    return {"acc": float(acc), "nmi": float(nmi), "ari": ari, "purity": purity}
