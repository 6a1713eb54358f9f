"""Barlow Twins loss (Zbontar et al., 2021): redundancy reduction on the D x D cross-correlation
of the two views' embeddings.  No negatives and no temperature, so the loss does not depend on
the batch size the way NT-Xent does (``loss.kind=barlow``).

The contract, identical in the kernels of ``csrc/barlow.hip`` and in :func:`barlow_twins_torch`:

* Rows are ``z = [view0; view1]``, ``[2n][D]``.  On the HIP path z is the head's bf16 output; an
  fp32 z is read as given.  dz comes back in z's dtype.
* Standardisation per view v and column d, in fp32 and a fixed row order:
  ``μ = (1/n) Σ_b z``, then ``σ² = (1/n) Σ_b (z − μ)²`` (biased, two passes),
  ``ẑ = (z − μ) · rsqrt(σ² + eps)`` — the paper's ``BatchNorm1d(affine=False)``.  The row order
  is :func:`_row_sum`'s in the kernel and in the twin, and rsqrt is the correctly rounded
  ``1 / sqrt``, so both round the same ẑ to bf16.  A constant
  column gives ẑ = 0, never NaN.  With ``round_operands`` (the HIP path always) ẑ is rounded once
  to bf16; everything below is exact on those operands up to the fp32 summation order.
* ``C = ẑ0ᵀ ẑ1 / n`` (fp32 accumulation over the whole batch; the kernels split the batch over
  blocks and merge the partial slabs in split order, no atomics).
* ``loss = Σ_i (1 − C_ii)² + λ Σ_{i≠j} C_ij²``, a fixed-order fp32 sum.  No reduction modes.
* Backward, g the upstream scalar: ``G_ii = −2g(1 − C_ii)``, ``G_ij = 2gλ C_ij``, rounded once to
  bf16 with ``round_operands`` (it is the operand of the next GEMMs); ``dẑ0 = ẑ1 · Gᵀ / n``,
  ``dẑ1 = ẑ0 · G / n`` (fp32 accumulation, K = D); per view and column, on the ẑ the forward kept,
  ``dz = rsqrt(σ²+eps) · (dẑ − mean_b(dẑ) − ẑ · mean_b(dẑ·ẑ))`` with fp32 means.
* Bitwise repeatable.  No host value that changes per step reaches a launch (g is read on the
  device), and the allocations are ``torch.empty`` calls as in ``_NTXentHipFn``, so a step with
  this loss captures as one with NT-Xent does.
* HIP path: ``n % 32 == 0``, ``D % 64 == 0``, ``64 <= D <= 2048`` and ``registry.use_hip(z)``;
  anything else takes the twin (unrounded, in fp32; fp64 for a ``double`` z).
* Data-parallel runs: by default the loss is per rank (each rank correlates its own n images)
  and the gradients are averaged by the flat store's buckets.

``global_batch`` (``loss.barlow_global``): the loss of the global batch, as the paper defines it.
W ranks hold z_r ``[2n][D]`` with the same n, N = W·n; three collectives per step:

1. Local statistics per rank, view and column, in fp32 and :func:`_row_sum`'s order:
   ``μ_r = (1/n) Σ_b z`` (quotient through fp64), then ``M2_r = Σ_b (z − μ_r)²``, not divided.
2. One all-gather of ``[2][2][D]`` (μ_r, M2_r) gives ``[W][2][2][D]``; every rank merges it in
   rank order in fp32: ``μ = (Σ_r μ_r) / W``, ``M2 = Σ_r (M2_r + n·(μ_r − μ)²)``, ``σ² = M2 / N``,
   quotients and ``rstd = 1 / sqrt(σ² + eps)`` through fp64; ``ẑ = (z − μ)·rstd``, rounded once to
   bf16 on the HIP path and by the rounded twin.  A column constant over the global batch gives
   ẑ = 0 (exactly when W·μ_r is representable: always for W a power of two), never NaN; one
   constant within each rank but not between them has ``M2_r = 0`` and σ² from the mean term.
3. ``S_r = ẑ0ᵀ ẑ1`` over the rank's n rows (slabs merged in split order, not divided), one fp32
   SUM all-reduce of ``[D][D]``, ``C = S / N``, the loss as above.  Every rank has the same value.
4. Backward: a rank returns ``dz_r = W · ∂L/∂z_r``, so that the gradient buckets' mean over the
   ranks is the gradient of the global loss (the true gradient, not the authors' DDP code's,
   which is off by W).  G from C as above; ``dẑ0 = ẑ1·Gᵀ / n``, ``dẑ1 = ẑ0·G / n`` with the LOCAL n
   (= W/N); the per-view column sums of dẑ and dẑ·ẑ, ``[2][2][D]`` in tile order, are all-gathered
   and added in rank order; ``dz = rstd·(dẑ − Σ/N − ẑ·Σ/N)``.
5. W = 1 (a forced 1-rank group): loss, C and dz are bit for bit the per-rank path's, in the
   kernels, in the rounded twin and in the unrounded one (which, for autograd's dz to keep its
   bits, forms ẑ as ``(c_r − (μ − μ_r))·rstd`` from the rank's centred rows ``c_r = z − μ_r``).
6. No atomics, no per-step host value in a launch; every collective is a ``torch.distributed``
   call on ``pstate``'s group, issued on the current stream (the chain is serial).  Repeatable
   up to the all-reduce's own order.  The one-shot IPC exchange is not used.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.distributed as dist
from torch import nn

from ..ops import registry
from ..parallel import state as pstate


def _bf16_round(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(x.dtype)


ROW_GROUPS = 16  # of the fixed row order (k_bt_standardize's 16 row groups)


def _row_sum(x: torch.Tensor) -> torch.Tensor:
    """x [2][n][D] -> [2][1][D], the rows added in the contract's fixed order: group r of 16 adds
    rows r, r + 16, r + 32, ... in order, then the 16 groups are added in order (the order of
    ``k_bt_standardize``, so the statistics have the same bits on every device).  n that is no
    multiple of 16 (never the kernels' case) takes ``sum``."""
    v, n, D = x.shape
    if n % ROW_GROUPS:
        return x.sum(dim=1, keepdim=True)
    xg = x.view(v, n // ROW_GROUPS, ROW_GROUPS, D)
    acc = xg[:, 0]
    for k in range(1, n // ROW_GROUPS):
        acc = acc + xg[:, k]
    tot = acc[:, 0]
    for k in range(1, ROW_GROUPS):
        tot = tot + acc[:, k]
    return tot.unsqueeze(1)


def _standardize(zf: torch.Tensor, n: int, eps: float):
    """zf [2n][D] -> ẑ [2][n][D], rstd [2][1][D] (biased, two passes; rsqrt as the correctly
    rounded 1 / sqrt)."""
    zv = zf.view(2, n, zf.shape[1])
    dt = zf.dtype
    # quotients and the root through fp64, rounded once to z's precision: correctly rounded on
    # every device (torch's fp32 division and sqrt on the GPU are not), as in k_bt_standardize
    mu = (_row_sum(zv).double() / n).to(dt)
    c = zv - mu
    var = (_row_sum(c * c).double() / n).to(dt)
    rstd = (1.0 / torch.sqrt((var + eps).double()).to(dt).double()).to(dt)
    return c * rstd, rstd


def _local_stats(zf: torch.Tensor, n: int) -> torch.Tensor:
    """zf [2n][D] -> [2][2][D]: [0] = μ_r, [1] = M2_r = Σ_b (z − μ_r)² per view (not divided), the
    values ``_standardize`` forms before its division (``k_bt_stats``)."""
    zv = zf.view(2, n, zf.shape[1])
    mu = (_row_sum(zv).double() / n).to(zf.dtype)
    c = zv - mu
    return torch.stack([mu.squeeze(1), _row_sum(c * c).squeeze(1)])


def _merge_moments(gst: torch.Tensor, n: int):
    """gst [W][2][2][D], every rank's (μ_r, M2_r) in rank order -> μ, σ² [2][D] of the W·n rows:
    the rank-order merge of the contract (``k_bt_merge_standardize``)."""
    W, dt = gst.shape[0], gst.dtype
    sm = gst[0, 0]
    for r in range(1, W):
        sm = sm + gst[r, 0]
    mu = (sm.double() / W).to(dt)
    m2 = None
    for r in range(W):
        d = gst[r, 0] - mu
        t = gst[r, 1] + n * (d * d)
        m2 = t if m2 is None else m2 + t
    return mu, (m2.double() / (W * n)).to(dt)


def _merge_stats(gst: torch.Tensor, n: int, eps: float):
    """:func:`_merge_moments`, then rstd as ``_standardize``'s -> μ, rstd [2][1][D]."""
    mu, var = _merge_moments(gst, n)
    rstd = (1.0 / torch.sqrt((var + eps).double()).to(gst.dtype).double()).to(gst.dtype)
    return mu.unsqueeze(1), rstd.unsqueeze(1)


def _rank_sum(g: torch.Tensor) -> torch.Tensor:
    """g [W][...] -> the W blocks added in rank order."""
    tot = g[0]
    for r in range(1, g.shape[0]):
        tot = tot + g[r]
    return tot


def _gather(x: torch.Tensor, world_size: int, group) -> torch.Tensor:
    """x -> [W][*x.shape], every rank's x in rank order (not differentiable)."""
    out = torch.empty((world_size, *x.shape), device=x.device, dtype=x.dtype)
    dist.all_gather_into_tensor(out.view(-1), x.contiguous().view(-1), group=group)  # (flat: gloo)
    return out


def _loss_terms(C: torch.Tensor, lambd: float) -> torch.Tensor:
    eye = torch.eye(C.shape[0], dtype=torch.bool, device=C.device)
    om = 1.0 - C
    return torch.where(eye, om * om, (lambd * C) * C).sum()


class _BarlowTwinFn(torch.autograd.Function):
    """The twin with ``round_operands``: ẑ and G rounded to bf16 at the kernels' points, with the
    three exchanges of the contract (statistics, the slab, the column sums) where the kernels
    have them.  With no group and ``W`` = 1 (the per-rank loss) the exchanges are the identity:
    μ = μ_0 / 1 and M2 = M2_0 + n · 0, a gather of one block, no all-reduce."""

    @staticmethod
    def _exchange(x, W, group):
        """[W][*x.shape] in rank order; the per-rank loss (no group, W = 1) has the one block."""
        return x.unsqueeze(0) if group is None and W == 1 else _gather(x, W, group)

    @staticmethod
    def forward(ctx, z, n, lambd, eps, group, W):
        zf = z.float()
        gst = _BarlowTwinFn._exchange(_local_stats(zf, n), W, group)
        mu, rstd = _merge_stats(gst, n, eps)
        zh = _bf16_round((zf.view(2, n, -1) - mu) * rstd)
        S = zh[0].t() @ zh[1]
        if group is not None or W > 1:
            S = S.contiguous()
            dist.all_reduce(S, group=group)
        C = S / (W * n)
        ctx.save_for_backward(zh, rstd, C)
        ctx.cfg = (n, lambd, z.dtype, group, W)
        ctx.mark_non_differentiable(C)
        return _loss_terms(C, lambd), C

    @staticmethod
    def backward(ctx, gout, _gc):
        zh, rstd, C = ctx.saved_tensors
        n, lambd, zdtype, group, W = ctx.cfg
        g = gout.float()
        eye = torch.eye(C.shape[0], dtype=torch.bool, device=C.device)
        G = _bf16_round(torch.where(eye, (-2.0 * g) * (1.0 - C), (2.0 * g * lambd) * C))
        dzh = torch.stack([zh[1] @ G.t(), zh[0] @ G]) / n
        csum = torch.stack([dzh.sum(dim=1), (dzh * zh).sum(dim=1)], dim=1)  # [2 views][2][D]
        tot = _rank_sum(_BarlowTwinFn._exchange(csum, W, group))
        m1 = tot[:, 0:1] / (W * n)
        m2 = tot[:, 1:2] / (W * n)
        dz = rstd * ((dzh - m1) - zh * m2)
        return dz.reshape(2 * n, -1).to(zdtype), None, None, None, None, None


def _global_plain(z: torch.Tensor, n: int, lambd: float, eps: float, group, W: int):
    """The unrounded loss over all ranks on differentiable ops and differentiable collectives:
    every rank backpropagates its identical loss, so their backward yields W · ∂L/∂z_r.
    ẑ is formed from the rank's own centred rows, ``(c_r − (μ − μ_r))·rstd`` with
    ``c_r = z − μ_r`` (the c_r that M2_r is summed from): the same value as ``(z − μ)·rstd`` up to
    one rounding, and on a 1-rank group (μ − μ_r = 0) the per-rank path's graph, so that the
    loss, C and autograd's dz have its bits."""
    from torch.distributed.nn.functional import all_gather, all_reduce
    zf = z if z.dtype == torch.float64 else z.float()
    zv = zf.view(2, n, -1)
    mu_r = (_row_sum(zv).double() / n).to(zf.dtype)
    c = zv - mu_r
    stats = torch.stack([mu_r.squeeze(1), _row_sum(c * c).squeeze(1)])  # as _local_stats
    gst = torch.stack(all_gather(stats, group=group))
    mu, rstd = _merge_stats(gst, n, eps)
    zh = (c - (mu - mu_r)) * rstd
    S = all_reduce((zh[0].t() @ zh[1]).contiguous(), group=group)
    C = S / (W * n)
    return _loss_terms(C, lambd), C


def barlow_twins_torch(z: torch.Tensor, n: int, lambd: float, eps: float = 1e-5,
                       round_operands: bool = False, return_c: bool = False, group=None,
                       world_size: int = 1, rank: int = 0):
    """The loss on torch ops; ``z`` = [view0; view1] of shape [2n, D].  Without
    ``round_operands`` these are plain differentiable ops (a ``double`` z gives the fp64 oracle);
    with it, an explicit function that rounds ẑ and G to bf16 where the kernels do.
    ``return_c``: also return C (not differentiable with ``round_operands``).
    ``group`` / ``world_size`` / ``rank`` (as ``nt_xent_torch``): with a group or more than one
    rank, the loss of the global batch of ``world_size`` · n images (module docstring); every
    rank passes its own z and gets the same loss, and dz = world_size · ∂loss/∂z.  ``rank`` is
    accepted for the signature of ``nt_xent_torch`` only: every exchange is symmetric in the
    ranks (all-gather, all-reduce), so nothing here depends on it."""
    if z.dim() != 2 or z.shape[0] != 2 * n:
        raise ValueError(f"z must be [2n][D] with n = {n}, got {tuple(z.shape)}")
    if round_operands:
        loss, C = _BarlowTwinFn.apply(z, n, float(lambd), float(eps), group, int(world_size))
    elif group is not None or world_size > 1:
        loss, C = _global_plain(z, n, float(lambd), float(eps), group, int(world_size))
    else:
        zh, _ = _standardize(z if z.dtype == torch.float64 else z.float(), n, eps)
        C = zh[0].t() @ zh[1] / n
        loss = _loss_terms(C, float(lambd))
    return (loss, C) if return_c else loss


class _BarlowHipFn(torch.autograd.Function):
    """``st`` None, the per-rank loss: seven launches (standardise, correlate, loss partials,
    their sum; G, dẑ, dz).  ``st`` a parallel state, the loss over all ranks: ten launches (nine
    with a single slab: stats + merge replace standardise, the slab merge is new, colsum + the
    global std backward replace the std backward) and three collectives on the current stream
    (statistics all-gather, slab all-reduce, column-sum all-gather); ``bt_corr``, ``bt_loss``
    (one slab, n = N), ``bt_grad`` and ``bt_backward`` are the per-rank path's."""

    @staticmethod
    def forward(ctx, z, n, lambd, eps, st):
        from ..ops import _ext
        ops = _ext.ops()
        D = z.shape[1]
        dev = z.device
        zc = z.contiguous()
        if st is not None:
            W = st.world_size
            stats = torch.empty((2, 2, D), device=dev, dtype=torch.float32)
            ops.bt_stats(zc, stats)
            gstats = torch.empty((W, 2, 2, D), device=dev, dtype=torch.float32)
            dist.all_gather_into_tensor(gstats.view(-1), stats.view(-1), group=st.group)
        rstd = torch.empty((2, D), device=dev, dtype=torch.float32)
        zh = torch.empty((2 * n, D), device=dev, dtype=torch.bfloat16)
        zhT = torch.empty((2, D, n), device=dev, dtype=torch.bfloat16)
        if st is None:
            ops.bt_standardize(zc, eps, rstd, zh, zhT)
        else:
            ops.bt_merge_standardize(zc, gstats, eps, rstd, zh, zhT)
        splits = ops.bt_corr_splits(n, D)
        part = torch.empty((splits, D, D), device=dev, dtype=torch.float32)
        ops.bt_corr(zhT, n, splits, part)
        rows = n
        if st is not None:
            if splits > 1:
                S = torch.empty((D, D), device=dev, dtype=torch.float32)
                ops.bt_slab_merge(part, splits, S)
            else:
                S = part.view(D, D)  # (the single slab is S_r already)
            dist.all_reduce(S, group=st.group)
            part, splits, rows = S, 1, W * n
        C = torch.empty((D, D), device=dev, dtype=torch.float32)
        lpart = torch.empty((ops.bt_loss_blocks(D),), device=dev, dtype=torch.float32)
        ops.bt_loss(part, splits, rows, lambd, C, lpart)
        out = torch.empty((1,), device=dev, dtype=torch.float32)
        ops.nt_reduce_loss(lpart, 1.0, out)
        ctx.save_for_backward(zh, rstd, C)
        ctx.cfg = (n, lambd, z.dtype, st)
        ctx.mark_non_differentiable(C)
        return out.view(()), C

    @staticmethod
    def backward(ctx, gout, _gc):
        from ..ops import _ext
        ops = _ext.ops()
        zh, rstd, C = ctx.saved_tensors
        n, lambd, zdtype, st = ctx.cfg
        D = zh.shape[1]
        dev = zh.device
        g = gout.reshape(1).float().contiguous()
        G = torch.empty((D, D), device=dev, dtype=torch.bfloat16)
        GT = torch.empty((D, D), device=dev, dtype=torch.bfloat16)
        ops.bt_grad(C, lambd, g, G, GT)
        dzh = torch.empty((2 * n, D), device=dev, dtype=torch.float32)
        colpart = torch.empty((2, n // 32, 2, D), device=dev, dtype=torch.float32)
        ops.bt_backward(zh, G, GT, dzh, colpart)
        sums, std_backward = colpart, ops.bt_std_backward
        if st is not None:
            csum = torch.empty((2, 2, D), device=dev, dtype=torch.float32)
            ops.bt_colsum(colpart, csum)
            gsum = torch.empty((st.world_size, 2, 2, D), device=dev, dtype=torch.float32)
            dist.all_gather_into_tensor(gsum.view(-1), csum.view(-1), group=st.group)
            sums, std_backward = gsum, ops.bt_std_backward_global
        bf16 = zdtype == torch.bfloat16
        dz = torch.empty((2 * n, D), device=dev, dtype=torch.bfloat16 if bf16 else torch.float32)
        std_backward(zh, rstd, dzh, sums, *((dz, None) if bf16 else (None, dz)))
        return dz, None, None, None, None


def hip_path(z: torch.Tensor, n: int) -> bool:
    """Whether ``z`` = [2n][D] takes the kernels (the limits in the module docstring)."""
    D = z.shape[1]
    return (z.is_cuda and z.dtype in (torch.bfloat16, torch.float32) and n >= 32 and n % 32 == 0
            and D % 64 == 0 and 64 <= D <= 2048 and registry.use_hip(z))


class BarlowTwins(nn.Module):
    def __init__(self, lambd: float = 0.0051, eps: float = 1e-5, global_batch: bool = False):
        """``lambd``: the weight of the off-diagonal (redundancy) term, the paper's 0.0051;
        ``eps``: the standardisation's, BatchNorm1d's 1e-5; ``global_batch``
        (``loss.barlow_global``): with a data-parallel group, the loss of all ranks' images
        (module docstring) instead of the per-rank one."""
        if not lambd > 0.0:
            raise ValueError(f"loss.barlow_lambda must be > 0, got {lambd}")
        if not eps > 0.0:
            raise ValueError(f"eps must be > 0, got {eps}")
        super().__init__()
        self.lambd = float(lambd)
        self.eps = float(eps)
        self.global_batch = bool(global_batch)

    def forward(self, view0: torch.Tensor, view1: Optional[torch.Tensor] = None,
                return_c: bool = False):
        """``forward(view0, view1)`` or ``forward(z)`` with z = [view0; view1], as ``NTXent``;
        returns the scalar loss (``return_c``: and C, for inspection)."""
        if view1 is not None:
            z = torch.cat([view0, view1], dim=0)
            n = view0.shape[0]
        else:
            z = view0
            n = z.shape[0] // 2
        if z.dim() != 2 or z.shape[0] != 2 * n:
            raise ValueError(f"z must be [2n][D], got {tuple(z.shape)}")
        st = pstate.get()
        st = st if self.global_batch and st.comm else None  # the all-rank loss or the per-rank one
        if hip_path(z, n):
            loss, C = _BarlowHipFn.apply(z, n, self.lambd, self.eps, st)
            return (loss, C) if return_c else loss
        group, W, rank = (None, 1, 0) if st is None else (st.group, st.world_size, st.rank)
        return barlow_twins_torch(z, n, self.lambd, self.eps, return_c=return_c, group=group,
                                  world_size=W, rank=rank)
