"""Geometry probe ops: label-free and label-aware numbers on how frozen features fill their space
(uniformity and alignment, Wang & Isola 2020; effective rank, RankMe of Garrido et al. 2023 and
the participation ratio of the covariance spectrum), on the HIP kernels of csrc/geometry.hip on
the GPU and as torch ops of the same contract elsewhere.

Contract, pair part (``pair_stats``; both paths):

1. Operands.  ``u = normalize_bf16(features)`` (the k-NN contract of ``ops/knn.py``: rows
   L2-normalised in fp32 with an fp64 norm, rounded once to bf16, zero-padded to ``Dp``).
   Everything below is exact on those operands up to the fp32 summation order.
2. Terms.  ``s_ij = u_i·u_j`` with fp32 accumulation, for the unordered pairs ``i < j`` only;
   ``e_ij = exp(c (s_ij - 1))`` in fp32 with ``c = fp32(2 t)`` (``exp(-t |u_i - u_j|^2)`` for unit
   rows) and ``d_ij = 2 - 2 s_ij`` (one rounding).
3. Raw sums.  ``E = Σ e_ij``, ``A = Σ d_ij``, ``A_same = Σ_{y_i = y_j} d_ij`` and the exact integer
   counts ``pairs`` and ``same_pairs``, counted where the terms are summed (a self pair or a pair
   visited twice shows in them).  Labels are int32 and only compared for equality; without labels
   ``A_same`` and ``same_pairs`` are ``None``.
4. Summation order.  An fp32 sum never spans more than one 128 x 128 tile of the Gram matrix (a
   chain of at most ``PAIR_CHAIN`` = 72 roundings); the tile partials are added in fp64 in tile
   order on the host after one read-back.  No atomics: two runs give the same bits.  This path
   forms the terms in fp32 and adds them in fp64, which makes it the oracle.
5. No N x N buffer exists; scratch is the tile partials (20 bytes per tile).  Only the tiles on or
   above the diagonal are visited; rows past N are masked by index.

Contract, spectrum part (``spectrum``; the operands are the raw features, not the normalised):

6. Mean.  ``μ_d`` is the column mean accumulated in fp64 in a fixed order (rows in chunks of
   ``CHUNK`` = 2048; in a chunk row group g of 16 adds its rows g, g + 16, ... in order, then the
   groups in order; then the chunks in order), divided by N in fp64 and rounded to fp32.  Both
   paths use that order, so ``μ`` and ``c`` have the same bits on every device.
7. ``c = bf16(x - μ)`` (fp32 difference, rounded once), ``[N][Dp]``, padding columns zero.
8. ``S = cᵀc``, ``[Dp][Dp]`` fp64: fp32 accumulation over one chunk of at most 2048 rows; the
   chunk results are added in fp64, the chunks of a split in chunk order and then the splits in
   split order (``syrk_splits``: one split from Dp 2048 on, where the triangle's 528 tiles of
   64 x 64 fill the device; below that about 512 blocks).  Only the tiles on or above the diagonal
   are computed and the other triangle is the mirror, so S is bitwise symmetric.
9. ``Cov = S / N`` in fp64; eigenvalues by ``torch.linalg.eigvalsh`` in fp64 on the host, clamped
   at 0, sorted descending.  A non-finite S gives NaN eigenvalues (nothing is decomposed).

Host metrics (fp64; ``pair_metrics``, ``spectrum_metrics``): ``uniformity = log(E / pairs)``,
``mean_sq_dist = A / pairs``, ``class_alignment = A_same / same_pairs``, ``class_separation =
(A - A_same) / (pairs - same_pairs)``; with ``p = λ / Σλ`` and ``σ = sqrt(λ)``:
``effective_rank = exp(-Σ p log p)``, ``rankme = exp(-Σ q log q)`` with ``q = σ / Σσ + 1e-7``,
``participation_ratio = (Σλ)² / Σλ²``, ``top_eig_share = p_0``, ``dims_90`` / ``dims_99`` the
fewest leading eigenvalues whose sum reaches that share of Σλ (to 1e-12 relative, so that k equal
eigenvalues give ``ceil(0.9 k)``), ``dim_std_*`` from ``sqrt(diag Cov)`` (the median is the lower
middle), ``eig_shares`` the 32 largest ``p``.  A zero denominator gives ``None``.

Limits (``check_limits``; the bindings check them again before any launch): ``N >= 2``,
``Dp <= 4096``, ``N·Dp < 2^31``, ``t > 0`` and finite; the pair part also needs
``N <= 128·65535`` (the triangle's tile count stays below 2^31).  The number of distinct labels is
not limited.
"""
from __future__ import annotations

import math
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch

from . import registry
from .knn import K_STEP, normalize_bf16

MAX_DP = 4096
PAIR_TILE = 128
PAIR_CHAIN = 72          # roundings in a tile's fp32 sums: 63 in a thread, 6 over lanes, 3 over waves
MAX_PAIR_ROWS = PAIR_TILE * 65535
CHUNK = 2048             # rows per fp32 accumulation chunk of S, and per column-sum chunk
ROW_GROUPS = 16
S_TILE = 64
EIG_SHARES = 32
ROW_BLOCK = 512          # rows per similarity block of the torch path


class PairSums(NamedTuple):
    E: float
    A: float
    A_same: Optional[float]
    pairs: int
    same_pairs: Optional[int]


class Spectrum(NamedTuple):
    eig: torch.Tensor              # [D] fp64 (CPU): eigenvalues of Cov, clamped at 0, descending
    cov_diag: torch.Tensor         # [D] fp64 (CPU)
    S: torch.Tensor                # [Dp][Dp] fp64 (CPU)
    mean: torch.Tensor             # [Dp] fp32
    c: Optional[torch.Tensor]      # [N][Dp] bf16 with ``return_centered``


def _hip_ok(t: torch.Tensor) -> bool:
    return t.is_cuda and registry.use_hip(t)


def padded_d(D: int) -> int:
    return (D + K_STEP - 1) // K_STEP * K_STEP


def check_limits(N: Optional[int] = None, Dp: Optional[int] = None, t=None, pairs: bool = True) -> None:
    """Raises ValueError naming the failing argument (``geometry_t`` is also the name of the
    ``parameter.`` key).  ``None`` skips a check; ``pairs`` adds the pair part's row limit."""
    if t is not None:
        ok = isinstance(t, (int, float)) and not isinstance(t, bool)
        if not (ok and t > 0 and math.isfinite(t)):
            raise ValueError(f"geometry_t must be a finite number > 0, got {t!r}")
    if N is not None and N < 2:
        raise ValueError(f"features: rows N must be >= 2, got {N}")
    if N is not None and pairs and N > MAX_PAIR_ROWS:
        raise ValueError(f"features: rows N must be <= {MAX_PAIR_ROWS} for the pair statistics, got {N}")
    if Dp is not None and Dp > MAX_DP:
        raise ValueError(f"features: width padded to Dp {Dp} exceeds {MAX_DP}")
    if N is not None and Dp is not None and N * Dp >= 2 ** 31:
        raise ValueError(f"features: N x Dp must be < 2^31, got {N} x {Dp}")


def pair_tiles(N: int) -> int:
    T = (N + PAIR_TILE - 1) // PAIR_TILE
    return T * (T + 1) // 2


def syrk_splits(N: int, Dp: int) -> int:
    """Splits of the chunks of S over blocks (csrc/geometry.hip ``geo_syrk_splits``)."""
    Td = Dp // S_TILE
    tiles, chunks = Td * (Td + 1) // 2, (N + CHUNK - 1) // CHUNK
    want = min((512 + tiles - 1) // tiles, chunks)
    per = (chunks + want - 1) // want
    return (chunks + per - 1) // per


# ------------------------------------------------------------------------------ pair part

def _ordered_sum(col: np.ndarray) -> float:
    return float(np.cumsum(col, dtype=np.float64)[-1])


def _pair_torch(Xn: torch.Tensor, labels: Optional[torch.Tensor], t: float) -> PairSums:
    N = Xn.shape[0]
    xt = Xn.float().t()
    c = torch.tensor(2.0 * t, dtype=torch.float32, device=Xn.device)
    cols = torch.arange(N, device=Xn.device).view(1, -1)
    E = A = A_same = 0.0
    pairs = same = 0
    for b in range(0, N, ROW_BLOCK):
        s = Xn[b:b + ROW_BLOCK].float() @ xt
        upper = cols > torch.arange(b, b + s.shape[0], device=Xn.device).view(-1, 1)
        e = torch.exp((s - 1.0) * c).double()
        d = (2.0 - 2.0 * s).double()
        E += float(e[upper].sum())
        A += float(d[upper].sum())
        pairs += int(upper.sum())
        if labels is not None:
            eq = upper & (labels[b:b + ROW_BLOCK].view(-1, 1) == labels.view(1, -1))
            A_same += float(d[eq].sum())
            same += int(eq.sum())
    if labels is None:
        return PairSums(E, A, None, pairs, None)
    return PairSums(E, A, A_same, pairs, same)


def _pair_hip(Xn: torch.Tensor, labels: Optional[torch.Tensor], t: float) -> PairSums:
    from . import _ext
    tiles = pair_tiles(Xn.shape[0])
    fpart = torch.empty(tiles, 3, device=Xn.device, dtype=torch.float32)
    ipart = torch.empty(tiles, 2, device=Xn.device, dtype=torch.int32)
    _ext.ops().geometry_pair(Xn, labels, float(t), fpart, ipart)
    fp, ip = fpart.cpu().numpy(), ipart.cpu().numpy().astype(np.int64)  # the one read-back
    E, A = _ordered_sum(fp[:, 0]), _ordered_sum(fp[:, 1])
    pairs = int(ip[:, 0].sum())
    if labels is None:
        return PairSums(E, A, None, pairs, None)
    return PairSums(E, A, _ordered_sum(fp[:, 2]), pairs, int(ip[:, 1].sum()))


def pair_stats(features: torch.Tensor, labels: Optional[torch.Tensor] = None, t: float = 2.0,
               hip: Optional[bool] = None) -> PairSums:
    """The raw pair sums of ``features`` [N][D] (fp32 / bf16) over the pairs i < j."""
    assert features.dim() == 2, "expected [rows][features]"
    N, D = features.shape
    check_limits(N, padded_d(D), t)
    if labels is not None:
        if labels.numel() != N:
            raise ValueError(f"labels must hold one entry per row ({N}), got {labels.numel()}")
        labels = labels.to(device=features.device, dtype=torch.int32).contiguous().view(-1)
    Xn = normalize_bf16(features)
    if _hip_ok(Xn) if hip is None else hip:
        return _pair_hip(Xn, labels, t)
    return _pair_torch(Xn, labels, t)


def _ratio(num: Optional[float], den: Optional[int]) -> Optional[float]:
    if num is None or den is None or den == 0:
        return None
    return float(num) / float(den)


def pair_metrics(sums: PairSums) -> Dict:
    """The pair metrics of the module docstring from the raw sums, in fp64."""
    mean_e = _ratio(sums.E, sums.pairs)
    if mean_e is None:
        uni = None
    elif mean_e > 0:
        uni = math.log(mean_e)
    else:
        uni = float("-inf") if mean_e == 0 else float("nan")
    other = None if sums.A_same is None else sums.A - sums.A_same
    rest = None if sums.same_pairs is None else sums.pairs - sums.same_pairs
    return {
        "uniformity": uni,
        "mean_sq_dist": _ratio(sums.A, sums.pairs),
        "class_alignment": _ratio(sums.A_same, sums.same_pairs),
        "class_separation": _ratio(other, rest),
        "pairs": int(sums.pairs),
        "same_class_pairs": None if sums.same_pairs is None else int(sums.same_pairs),
    }


# ------------------------------------------------------------------------------ spectrum part

def _center_torch(x: torch.Tensor, Dp: int):
    """(μ [Dp] fp32, c [N][Dp] bf16) in the summation order of item 6."""
    N, D = x.shape
    f64 = dict(device=x.device, dtype=torch.float64)
    tot = torch.zeros(D, **f64)
    for r0 in range(0, N, CHUNK):
        xc = x[r0:r0 + CHUNK].double()
        pad = -xc.shape[0] % ROW_GROUPS
        if pad:  # (+0.0 rows change no bit of the group sums)
            xc = torch.cat([xc, torch.zeros(pad, D, **f64)])
        xg = xc.view(-1, ROW_GROUPS, D)
        acc = torch.zeros(ROW_GROUPS, D, **f64)
        for k in range(xg.shape[0]):
            acc = acc + xg[k]
        t = torch.zeros(D, **f64)
        for g in range(ROW_GROUPS):
            t = t + acc[g]
        tot = tot + t
    mu = torch.zeros(Dp, device=x.device, dtype=torch.float32)
    mu[:D] = (tot / float(N)).float()
    c = torch.zeros(N, Dp, device=x.device, dtype=torch.bfloat16)
    c[:, :D] = (x - mu[:D]).to(torch.bfloat16)
    return mu, c


def _syrk_torch(c: torch.Tensor) -> torch.Tensor:
    N, Dp = c.shape
    chunks, splits = (N + CHUNK - 1) // CHUNK, syrk_splits(N, Dp)
    cps = (chunks + splits - 1) // splits
    S = None
    for z in range(splits):
        part = torch.zeros(Dp, Dp, device=c.device, dtype=torch.float64)
        for ch in range(z * cps, min(chunks, (z + 1) * cps)):
            cc = c[ch * CHUNK:(ch + 1) * CHUNK].float()
            part = part + (cc.t() @ cc).double()
        S = part if S is None else S + part
    return S


def spectrum(features: torch.Tensor, return_centered: bool = False,
             hip: Optional[bool] = None) -> Spectrum:
    """The covariance spectrum of ``features`` [N][D]."""
    assert features.dim() == 2, "expected [rows][features]"
    N, D = features.shape
    Dp = padded_d(D)
    check_limits(N, Dp, pairs=False)
    x = features.float().contiguous()
    if _hip_ok(x) if hip is None else hip:
        from . import _ext
        Np = (N + 63) // 64 * 64
        mu = torch.empty(Dp, device=x.device, dtype=torch.float32)
        cT = torch.empty(Dp, Np, device=x.device, dtype=torch.bfloat16)
        _ext.ops().geometry_center(x, mu, cT)
        S = torch.empty(Dp, Dp, device=x.device, dtype=torch.float64)
        _ext.ops().geometry_syrk(cT, N, S)
        c = cT[:, :N].t().contiguous() if return_centered else None
        S = S.cpu()  # the one read-back
    else:
        mu, c = _center_torch(x, Dp)
        S = _syrk_torch(c).cpu()
        c = c if return_centered else None
    cov = S[:D, :D] / float(N)
    if bool(torch.isfinite(cov).all()):
        eig = torch.linalg.eigvalsh(cov).clamp_min(0.0).flip(0).contiguous()
    else:
        eig = torch.full((D,), float("nan"), dtype=torch.float64)
    return Spectrum(eig, cov.diagonal().clone(), S, mu, c)


def _entropy_rank(p: np.ndarray) -> float:
    nz = p[p > 0]
    return float(np.exp(-(nz * np.log(nz)).sum())) if not np.isnan(p).any() else float("nan")


def effective_rank(eig) -> Optional[float]:
    lam = np.asarray(eig, dtype=np.float64)
    tot = lam.sum()
    if tot == 0:
        return None
    return _entropy_rank(lam / tot)


def rankme(eig, eps: float = 1e-7) -> Optional[float]:
    sv = np.sqrt(np.asarray(eig, dtype=np.float64))
    tot = sv.sum()
    if tot == 0:
        return None
    return _entropy_rank(sv / tot + eps)


def participation_ratio(eig) -> Optional[float]:
    lam = np.asarray(eig, dtype=np.float64)
    sq = (lam * lam).sum()
    if sq == 0:
        return None
    return float(lam.sum() ** 2 / sq)


def dims_for_share(eig, share: float) -> Optional[int]:
    lam = np.asarray(eig, dtype=np.float64)
    tot = lam.sum()
    if tot == 0 or np.isnan(tot):
        return None
    reach = np.cumsum(lam) >= share * tot * (1.0 - 1e-12)
    return int(np.argmax(reach)) + 1 if reach.any() else int(lam.size)


def spectrum_metrics(eig, cov_diag) -> Dict:
    """The spectrum metrics of the module docstring from the eigenvalues (descending, >= 0) and the
    diagonal of Cov, in fp64."""
    lam = np.asarray(eig, dtype=np.float64)
    sd = np.sqrt(np.clip(np.asarray(cov_diag, dtype=np.float64), 0.0, None))
    tot = lam.sum()
    shares = None if tot == 0 else [float(v) for v in (lam / tot)[:EIG_SHARES]]
    srt = np.sort(sd)
    return {
        "effective_rank": effective_rank(lam),
        "rankme": rankme(lam),
        "participation_ratio": participation_ratio(lam),
        "top_eig_share": None if shares is None else shares[0],
        "dims_90": dims_for_share(lam, 0.90),
        "dims_99": dims_for_share(lam, 0.99),
        "dim_std_min": float(sd.min()),
        "dim_std_median": float(srt[(srt.size - 1) // 2]),
        "dim_std_max": float(sd.max()),
        "eig_shares": shares,
    }
