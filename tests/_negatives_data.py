"""Inputs and fp64 references shared by tests/test_ntxent_negatives.py and
tests/test_gpu_ntxent_negatives.py (the weighted-negatives NT-Xent, loss/ntxent.py).

Recipe: ``z0 = randn(n, D)``, ``z1 = z0 + σ·randn(n, D)`` from a seeded CPU generator,
``z = [z0; z1]`` rounded to bf16 (the kernels score bf16 z, so every path sees the same values),
returned in fp64.  The clamp ``Ng = max(raw, floor)`` is a kink of the loss, so a comparison is
only meaningful where no row sits on it: :func:`clamp_flags` asserts that no row has raw/floor
within [0.98, 1.02] and returns k_i = [raw_i >= floor_i] from fp64; the seeds in ``SEED`` were
picked so that this holds for every setting in ``SETTINGS`` at that shape and regime (and, in
the mixed regime, so that the settings with τ⁺ > 0 have rows on both sides).
"""
import math

import torch
import torch.nn.functional as F

SHAPES = [(8, 32), (24, 64), (64, 128), (40, 256)]  # (n, D): one 16-row tile, a ragged tile
#                                       count, several splits; every D instantiation
SETTINGS = [(0.0, 0.0, True), (0.0, 0.1, False), (1.0, 0.1, False), (0.5, 0.05, True),
            (2.0, 0.0, False)]  # (β, τ⁺, decoupled)
# clamp regimes (τ, σ): no clamped row / clamped and unclamped rows / (nearly) all rows clamped
REGIMES = {"free": (0.5, 3.0), "mixed": (0.1, 3.0), "clamped": (0.1, 1.0)}
SEED = {}  # (n, D, regime) -> seed, filled below


def make_z(n, D, sigma, seed):
    g = torch.Generator().manual_seed(seed)
    z0 = torch.randn(n, D, generator=g)
    z1 = z0 + sigma * torch.randn(n, D, generator=g)
    return torch.cat([z0, z1]).to(torch.bfloat16).double()


def case(n, D, regime):
    """(z fp64 of bf16 values, τ) of a shape in a clamp regime."""
    tau, sigma = REGIMES[regime]
    return make_z(n, D, sigma, SEED[(n, D, regime)]), tau


def sims(z, cols, col_offset, n, tau):
    """s [R][Ccols], the positive's column per row and the mask of Neg(i), from fp64 z."""
    zn = F.normalize(z, dim=1)
    cn = zn if cols is None else F.normalize(cols, dim=1)
    s = zn @ cn.t() / tau
    R = z.shape[0]
    idx = torch.arange(R)
    pcol = col_offset + torch.where(idx < n, idx + n, idx - n)
    neg = torch.ones_like(s, dtype=torch.bool)
    neg[idx, col_offset + idx] = False
    neg[idx, pcol] = False
    return s, pcol, neg


def clamp_ratio(z, n, tau, beta, tau_plus, cols=None, col_offset=0):
    """raw_i / floor_i per row, fp64 (independent of the shift c)."""
    s, pcol, neg = sims(z, cols, col_offset, n, tau)
    sn = s.masked_fill(~neg, float("-inf"))
    L0 = torch.logsumexp(beta * sn, 1) if beta > 0 else math.log(s.shape[1] - 2)
    u = torch.logsumexp((1 + beta) * sn, 1) - L0
    sp = s[torch.arange(z.shape[0]), pcol]
    return (torch.exp(u) - tau_plus * torch.exp(sp)) / (1 - tau_plus) / math.exp(-1 / tau)


def clamp_flags(z, n, tau, beta, tau_plus, cols=None, col_offset=0):
    """k_i from fp64, after asserting that no row is within 2 % of the kink."""
    ratio = clamp_ratio(z, n, tau, beta, tau_plus, cols, col_offset)
    near = (ratio >= 0.98) & (ratio <= 1.02)
    assert not bool(near.any()), ratio[near]
    return ratio >= 1.0


def hcl_rows(z, n, tau, beta, tau_plus, decoupled):
    """The published hard-negative / debiased objective, one anchor and one column at a time in
    fp64 python floats: neg = exp(s) over the N = R − 2 negatives, pos = exp(s_p),
    imp = exp(β·log neg), reweight = Σ imp·neg / mean(imp),
    Ng = max((−τ⁺·N·pos + reweight) / (1 − τ⁺), N·e^{−1/τ}),
    loss = −log(pos / (pos + Ng)); decoupled: −log(pos / Ng)."""
    R = z.shape[0]
    zn = F.normalize(z, dim=1).tolist()
    N = R - 2
    rows = []
    for i in range(R):
        p = i + n if i < n else i - n
        pos, neg = None, []
        for c in range(R):
            if c == i:
                continue
            e = math.exp(sum(a * b for a, b in zip(zn[i], zn[c])) / tau)
            if c == p:
                pos = e
            else:
                neg.append(e)
        imp = [math.exp(beta * math.log(v)) for v in neg]
        reweight = sum(w * v for w, v in zip(imp, neg)) / (sum(imp) / N)
        Ng = max((-tau_plus * N * pos + reweight) / (1 - tau_plus), N * math.exp(-1 / tau))
        rows.append(-math.log(pos / ((0.0 if decoupled else pos) + Ng)))
    return torch.tensor(rows, dtype=torch.float64)


SEED.update({  # (rows with k = 1 per setting, in SETTINGS' order)
    (8, 32, "free"): 0,  # 16, 16, 16, 16, 16 of 16
    (8, 32, "mixed"): 1,  # 16, 8, 12, 14, 16 of 16
    (8, 32, "clamped"): 0,  # 16, 0, 1, 1, 16 of 16
    (24, 64, "free"): 0,  # 48, 48, 48, 48, 48 of 48
    (24, 64, "mixed"): 0,  # 48, 19, 39, 42, 48 of 48
    (24, 64, "clamped"): 0,  # 48, 0, 2, 2, 48 of 48
    (64, 128, "free"): 0,  # all 128
    (64, 128, "mixed"): 0,  # 128, 40, 84, 97, 128 of 128
    (64, 128, "clamped"): 0,  # 128, 0, 0, 0, 128 of 128
    (40, 256, "free"): 0,  # all 80
    (40, 256, "mixed"): 0,  # 80, 6, 25, 50, 80 of 80
    (40, 256, "clamped"): 0,  # 80, 0, 0, 0, 80 of 80
})


def check_regime(k, regime, tau_plus):
    """The clamp flags are what the regime promises (τ⁺ = 0 never clamps)."""
    if tau_plus == 0 or regime == "free":
        assert bool(k.all())
    elif regime == "mixed":
        assert bool(k.any()) and not bool(k.all())
    else:
        assert int(k.sum()) <= len(k) // 4
