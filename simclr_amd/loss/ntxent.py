"""NT-Xent loss (normalised temperature-scaled cross entropy).

Reference API: ``NT_Xent(temperature, reduction, device)(view0, view1)``
(``/root/reference/loss.py:4-65``).  Semantics: anchors are the 2N rows of both
views; for each, the logits are cosine similarities / τ to every other row (self excluded), the
target is the same image's other view; ``reduction="mean"`` averages over the 2N anchors,
``"sum"`` sums, ``"none"`` returns a (2, N) tensor [view0 anchors; view1 anchors].

Extension (north star): ``gather=True`` all-gathers the bf16 embeddings z of every
rank over RCCL on a side stream, overlapped with this rank's normalisation and the scoring of
its own columns (the peers' columns are scored into further online-LSE partials once they
arrive), so each anchor sees 2·N·W − 1 candidates instead of 2N − 1 (negatives from the global
batch).  The gradient w.r.t. the gathered columns returns through a reduce-scatter on a side
stream, overlapped with the row-gradient kernel.
Parity default is ``gather=False`` (the reference's loss is per-GPU local).

GPU path: the fused exact-fp32 MFMA kernels of ``csrc/ntxent.hip`` (no N×N logits, no mask or
concat copies, no host→device target upload per call).  CPU / fp32 path: torch ops.

Extension: the supervised contrastive loss ("SupCon", Khosla et al., L_out^sup without its
τ/τ_base factor), ``NTXent(..., supervised=True)(z, labels=y)`` or ``SupCon(...)(z, y)``
(``loss.supervised``).  The contract, identical on the GPU and in :func:`sup_con_torch`:

* Rows are ``z = [view0; view1]``, R = 2n per rank; labels are one integer per image, ``y[n]``;
  row r has label ``y[r mod n]``.  Labels are compared for equality only (any int32 value).
* With ``gather=True`` the columns are the all-gathered rows of every rank (Ccols = W·R) and the
  column labels the all-gathered view-expanded labels, in the same rank-major order.
* For anchor i (a local row): A(i) = every column except i's own; P(i) = {c ∈ A(i): y_c = y_i}
  (the other view is always in it, |P(i)| ≥ 1);
  ``loss_i = LSE_{a∈A(i)} s_ia − (1/|P(i)|) Σ_{p∈P(i)} s_ip`` with ``s = ẑ_i·ẑ_c / τ`` and the
  NT-Xent normalisation (bf16 z, fp32, eps 1e-12).
* ``mean`` = Σ_i loss_i / R, ``sum`` the plain sum, ``none`` (2, n) on the torch path only.
* Gradient in normalised space: ``dS_ia = g·(softmax_ia − [a∈P(i)]/|P(i)|)`` (zero at a = i),
  contracted by the same row and column passes; the normalisation backward is unchanged.
* All labels distinct: the loss and dz are bitwise those of NT-Xent on the same device, locally
  and gathered (the positive sum is a plain fp32 sum in tile, lane-group and split order — one
  match is that one value —, |P| an exact fp32 count, 1/|P| = 1).
* Bitwise repeatable: no atomics, a fixed merge order across lane groups and splits.
* ``gather="ring"`` with ``supervised`` is a ``ValueError``; limits as NT-Xent (R % 16 == 0,
  D in {32, 64, 128, 256} for the HIP path).

Extension: weighted negatives, ``NTXent(..., hard_beta=β, tau_plus=τ⁺, decoupled=bool)``
(``loss.hard_beta``, ``loss.tau_plus``, ``loss.decoupled``): hard-negative sampling (Robinson et
al. 2021, negatives importance-weighted by exp(β·s)), the debiased loss (Chuang et al. 2020, the
expected share τ⁺ of false negatives subtracted) and decoupled contrastive learning (Yeh et al.
2022, the positive leaves the denominator).  The loss is "weighted" when any of the three
differs from its default (0, 0, False); otherwise it is NT-Xent, by the same ops in the same
order.  The contract, identical on the GPU and in :func:`nt_xent_weighted_torch`:

* Rows, columns (local or all-gathered), ẑ, ``s``, ``col_offset``, the own column and the
  positive p(i) are NT-Xent's.  Neg(i) = every column but i's own and its positive,
  N = Ccols − 2.
* ``L1_i = LSE_{a∈Neg(i)} (1+β)·s_ia``, ``L0_i = LSE_{a∈Neg(i)} β·s_ia`` (β = 0: L0 = log N
  exactly, no second sum), ``u_i = L1_i − L0_i``.
* With ``c_i = max(u_i, s_ip)``: ``raw_i = N·(exp(u_i − c_i) − τ⁺·exp(s_ip − c_i)) / (1 − τ⁺)``,
  ``floor_i = N·exp(−1/τ − c_i)`` (the published clamp at N·e^{−1/τ}),
  ``Ng_i = max(raw_i, floor_i)``, ``T_i = κ·exp(s_ip − c_i) + Ng_i`` with κ = 0 if decoupled,
  else 1; ``loss_i = −s_ip + c_i + log T_i``.  Every exp argument is <= 0.
* ``mean`` = Σ_i loss_i / R, ``sum`` the plain sum, ``none`` (2, n) on the torch path only.
* Gradient in normalised space, ``k_i = [raw_i >= floor_i]``:
  ``A_i = k_i·N/(1−τ⁺)·exp(u_i − c_i)/T_i``,
  ``B_i = −1 + (κ − k_i·τ⁺·N/(1−τ⁺))·exp(s_ip − c_i)/T_i``,
  ``dS_ia = g·A_i·((1+β)·exp((1+β)s_ia − L1_i) − β·exp(β·s_ia − L0_i))`` for a ∈ Neg(i),
  ``dS_ip = g·B_i``, ``dS_ii = 0``; a clamped row (k = 0) has no gradient through its
  negatives, as published.
* Bitwise repeatable, the plain kernels' merge order; ``gather=True`` is supported,
  ``gather="ring"``, ``supervised`` and the other ``loss.kind`` values are not (``ValueError``);
  limits as NT-Xent, anything else and ``reduction="none"`` take the twin.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.distributed as dist
import torch.nn.functional as F
from torch import nn

from ..ops import registry
from ..parallel import state as pstate


def nt_xent_torch(z: torch.Tensor, n: int, temperature: float, reduction: str = "mean",
                  gather: bool = False, group=None, world_size: int = 1, rank: int = 0):
    """Oracle implementation on torch ops; ``z`` = [view0; view1] of shape [2n, d]."""
    zn = F.normalize(z if z.dtype == torch.float64 else z.float(), p=2, dim=1)
    R = zn.shape[0]
    if gather and world_size > 1:
        from torch.distributed.nn.functional import all_gather
        cols = torch.cat(all_gather(zn, group=group), dim=0)
        col_offset = rank * R
    else:
        cols = zn
        col_offset = 0
    sim = zn @ cols.t() / temperature
    idx = torch.arange(R, device=z.device)
    self_mask = torch.zeros_like(sim, dtype=torch.bool)
    self_mask[idx, col_offset + idx] = True
    sim = sim.masked_fill(self_mask, float("-inf"))
    targets = col_offset + torch.where(idx < n, idx + n, idx - n)
    rows = F.cross_entropy(sim, targets, reduction="none")
    if reduction == "none":
        return rows.view(2, n)
    if reduction == "sum":
        return rows.sum()
    return rows.sum() / n * 0.5


def check_negatives(hard_beta, tau_plus, decoupled) -> bool:
    """The three weighted-negatives arguments; returns whether the loss is "weighted" (any of
    them differs from its default).  ``ValueError`` names the failing key."""
    for key, v in (("loss.hard_beta", hard_beta), ("loss.tau_plus", tau_plus)):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError(f"{key} must be a number, got {v!r}")
        if not math.isfinite(v):
            raise ValueError(f"{key} must be finite, got {v!r}")
    if hard_beta < 0:
        raise ValueError(f"loss.hard_beta must be >= 0, got {hard_beta!r}")
    if not 0 <= tau_plus < 1:
        raise ValueError(f"loss.tau_plus must be in [0, 1), got {tau_plus!r}")
    if not isinstance(decoupled, bool):
        raise ValueError(f"loss.decoupled must be a boolean, got {decoupled!r}")
    return hard_beta > 0 or tau_plus > 0 or decoupled


def nt_xent_weighted_torch(z: torch.Tensor, n: int, temperature: float, hard_beta: float,
                           tau_plus: float, decoupled: bool, reduction: str = "mean",
                           gather: bool = False, group=None, world_size: int = 1, rank: int = 0):
    """NT-Xent with weighted negatives on torch ops (the contract in the module docstring);
    ``z`` = [view0; view1] of shape [2n, d].  All three arguments at their defaults: NT-Xent
    itself, :func:`nt_xent_torch`."""
    if not check_negatives(hard_beta, tau_plus, decoupled):
        return nt_xent_torch(z, n, temperature, reduction, gather, group, world_size, rank)
    zn = F.normalize(z if z.dtype == torch.float64 else z.float(), p=2, dim=1)
    R = zn.shape[0]
    if gather and world_size > 1:
        from torch.distributed.nn.functional import all_gather
        cols = torch.cat(all_gather(zn, group=group), dim=0)
        col_offset = rank * R
    else:
        cols = zn
        col_offset = 0
    sim = zn @ cols.t() / temperature
    rows = weighted_rows(sim, n, col_offset, temperature, hard_beta, tau_plus, decoupled)
    if reduction == "none":
        return rows.view(2, n)
    if reduction == "sum":
        return rows.sum()
    return rows.sum() / n * 0.5


def weighted_rows(sim: torch.Tensor, n: int, col_offset: int, temperature: float,
                  hard_beta: float, tau_plus: float, decoupled: bool) -> torch.Tensor:
    """loss_i of the weighted-negatives contract from the similarities ``sim`` [2n][Ccols]
    (= s, already divided by τ); row i's own column is ``col_offset + i``."""
    R = sim.shape[0]
    idx = torch.arange(R, device=sim.device)
    pcol = col_offset + torch.where(idx < n, idx + n, idx - n)
    s_p = sim[idx, pcol]
    out = torch.zeros_like(sim, dtype=torch.bool)  # not in Neg(i): the own column, the positive
    out[idx, col_offset + idx] = True
    out[idx, pcol] = True
    neg = sim.masked_fill(out, float("-inf"))
    N = sim.shape[1] - 2
    L1 = torch.logsumexp((1.0 + hard_beta) * neg, dim=1)
    u = L1 - (torch.logsumexp(hard_beta * neg, dim=1) if hard_beta > 0 else math.log(N))
    # the loss does not depend on the shift c (the floor moves with it), so c carries no gradient
    c = torch.maximum(u, s_p).detach()
    e_p = torch.exp(s_p - c)
    raw = N * (torch.exp(u - c) - tau_plus * e_p) / (1.0 - tau_plus)
    floor = N * torch.exp(-1.0 / temperature - c)
    if decoupled:
        # log max(raw, floor): a clamped row has c = s_ip, and at a small temperature its floor
        # N·exp(−1/τ − c) underflows fp32 while its logarithm is known
        k = raw >= floor
        log_T = torch.where(k, torch.log(torch.where(k, raw, torch.ones_like(raw))),
                            math.log(N) - 1.0 / temperature - c)
    else:
        log_T = torch.log(e_p + torch.maximum(raw, floor))
    return -s_p + c + log_T


def _check_labels(labels, n: int, device) -> torch.Tensor:
    """``labels``: one integer per image, ``y[n]`` (int32 or int64), on z's device."""
    if not isinstance(labels, torch.Tensor):
        raise TypeError("labels must be a tensor of n integer class labels")
    if labels.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"labels must be int32 or int64, not {labels.dtype}")
    if labels.dim() != 1 or labels.numel() != n:
        raise ValueError(f"labels must hold one label per image ({n}), got shape "
                         f"{tuple(labels.shape)}")
    if labels.device != device:
        raise ValueError(f"labels must be on z's device ({device}), not {labels.device}")
    return labels.contiguous()


def sup_con_torch(z: torch.Tensor, n: int, labels: torch.Tensor, temperature: float,
                  reduction: str = "mean", gather: bool = False, group=None,
                  world_size: int = 1, rank: int = 0):
    """SupCon oracle on torch ops (the contract in the module docstring); ``z`` = [view0; view1]
    of shape [2n, d], ``labels`` = y[n].  The same operations as :func:`nt_xent_torch` around
    the positive term, so that distinct labels give its result bit for bit."""
    zn = F.normalize(z if z.dtype == torch.float64 else z.float(), p=2, dim=1)
    R = zn.shape[0]
    y = _check_labels(labels, n, z.device).to(torch.int64)
    yrow = torch.cat([y, y])
    if gather and world_size > 1:
        from torch.distributed.nn.functional import all_gather
        cols = torch.cat(all_gather(zn, group=group), dim=0)
        ys = [torch.empty_like(yrow) for _ in range(world_size)]
        dist.all_gather(ys, yrow, group=group)
        ycol = torch.cat(ys)
        col_offset = rank * R
    else:
        cols = zn
        ycol = yrow
        col_offset = 0
    sim = zn @ cols.t() / temperature
    idx = torch.arange(R, device=z.device)
    self_mask = torch.zeros_like(sim, dtype=torch.bool)
    self_mask[idx, col_offset + idx] = True
    sim = sim.masked_fill(self_mask, float("-inf"))
    pos = (yrow[:, None] == ycol[None, :]) & ~self_mask  # P(i); the other view is always in it
    logp = F.log_softmax(sim, dim=1)  # s_ia - LSE_i
    rows = -(logp.masked_fill(~pos, 0.0).sum(dim=1) / pos.sum(dim=1).to(logp.dtype))
    if reduction == "none":
        return rows.view(2, n)
    if reduction == "sum":
        return rows.sum()
    return rows.sum() / n * 0.5


_SIDE: dict = {}


def _side_stream(dev: torch.device) -> "torch.cuda.Stream":
    """Per-device side stream of the gathered loss's collectives."""
    if dev not in _SIDE:
        _SIDE[dev] = torch.cuda.Stream(device=dev)
    return _SIDE[dev]


# z all-gathers the fused projection head already issued on the side stream, one per view, each
# under the next view's GEMM 2 (models/head_fused.py): (device, z.data_ptr()) -> (zb_all,
# tensors the side stream still uses).  The loss takes the gathered rows from here instead of
# issuing its own all-gather.
_PREGATHER: dict = {}


def register_pregather(z: torch.Tensor, zb_all: torch.Tensor, keep) -> None:
    _PREGATHER.clear()  # one step in flight per process
    _PREGATHER[(z.device, z.data_ptr())] = (zb_all, keep)


def take_pregather(z: torch.Tensor):
    return _PREGATHER.pop((z.device, z.data_ptr()), None)


class _NTXentHipFn(torch.autograd.Function):
    """NT-Xent (``y`` None) or, with the labels ``y[n]``, SupCon on the label-mode kernels
    (``nt_sup_*``): the rank's view-expanded int32 label block is built on the device
    (``nt_expand_labels``) and, for the gathered loss, all-gathered on the side stream right
    behind z.  The order of the ``torch.empty`` calls, launches, collectives and stream waits
    of each mode is part of the contract: the step is captured into a graph and replayed.

    ``neg`` = (β, τ⁺, decoupled) selects the weighted-negatives kernels (``nt_w_*``, ``y`` None):
    the row buffer ``lse`` then holds (L1, A, B, L0) per row and the forward partials 5 floats
    per row if β > 0; everything else, the order included, is the plain mode's."""

    @staticmethod
    def forward(ctx, z, y, n, temperature, reduction, gather, st, neg=None):
        from ..ops import _ext
        ops = _ext.ops()
        R, D = z.shape
        dev = z.device
        zb = z.contiguous() if z.dtype == torch.bfloat16 else z.to(torch.bfloat16).contiguous()
        inv_t = 1.0 / temperature
        labelled = y is not None
        npart = 4 if labelled else 3  # floats per row of a forward partial
        if neg is not None:
            beta, tau_plus, decoupled = neg
            npart = 5 if beta > 0 else 3
        lse = torch.empty((R, 4) if neg is not None else (R,), device=dev, dtype=torch.float32)
        inv_cnt = torch.empty((R,), device=dev, dtype=torch.float32) if labelled else None
        rows = torch.empty((R,), device=dev, dtype=torch.float32)
        y_loc = ycol = None
        if labelled:
            y_loc = torch.empty((R,), device=dev, dtype=torch.int32)
            ops.nt_expand_labels(y, None, 2, y_loc)

        def score(labels, y0, lo, hi, splits, base):
            # columns [lo, hi) into the partials [base, base + splits); labels cover [y0, ...)
            if labelled:
                ops.nt_sup_forward_range(znT, labels, y0, R, col_offset, n, inv_t, part, lo, hi,
                                         splits, base)
            elif neg is not None:
                ops.nt_w_forward_range(znT, R, col_offset, n, inv_t, beta, part, lo, hi, splits,
                                       base)
            else:
                ops.nt_forward_range(znT, R, col_offset, n, inv_t, part, lo, hi, splits, base)

        def finish(splits):
            if labelled:
                ops.nt_sup_finish(part, R, splits, lse, inv_cnt, rows)
            elif neg is not None:
                ops.nt_w_finish(part, R, splits, Ccols, inv_t, beta, tau_plus, decoupled, lse,
                                rows)
            else:
                ops.nt_finish(part, R, splits, lse, rows)

        if gather and st.comm:
            # global negatives: the ranks exchange bf16 z (half the bytes of gathering fp32 ẑ) on
            # a side stream.  Meanwhile this rank normalises its own rows and scores them against
            # its OWN columns (their online log-sum-exp partials, the positive included); after
            # the exchange every rank normalises the peers' rows with the same row-wise kernel
            # (its copy of a peer's ẑ is bitwise the peer's own) and scores the remaining
            # columns into further split partials; one merge gives lse and the loss.
            W = st.world_size
            col_offset = st.rank * R
            Ccols = W * R
            cur = torch.cuda.current_stream(dev)
            side = _side_stream(dev)
            side.wait_stream(cur)
            pre = take_pregather(zb)
            ipc = getattr(st, "ipc", None)  # one-shot stores over xGMI (comm/ipc.py, csrc/comm.hip)
            if labelled:
                ycol = torch.empty((Ccols,), device=dev, dtype=torch.int32)
            if pre is not None and tuple(pre[0].shape) == (Ccols, D):
                # the head gathered z view by view on this side stream, under its GEMM 2
                zb_all, pre_keep = pre
            else:
                pre_keep = pre  # (a mismatched pre-gather's buffers: still in use on the side stream)
                zb_all = torch.empty((Ccols, D), device=dev, dtype=torch.bfloat16)
                with torch.cuda.stream(side):
                    if ipc is not None:
                        ipc.all_gather(("ntxent", "z"), zb, zb_all)
                    else:
                        dist.all_gather_into_tensor(zb_all, zb, group=st.group)
            if labelled:
                with torch.cuda.stream(side):  # the labels: one more small collective, same wait
                    if ipc is not None:
                        ipc.all_gather(("ntxent", "y"), y_loc, ycol)
                    else:
                        dist.all_gather_into_tensor(ycol, y_loc, group=st.group)
            zall = torch.empty((Ccols, D), device=dev, dtype=torch.float32)
            inv_all = torch.empty((Ccols,), device=dev, dtype=torch.float32)
            zn = zall[col_offset:col_offset + R]
            inv = inv_all[col_offset:col_offset + R]
            znT = torch.empty((D, Ccols), device=dev, dtype=torch.float32)
            ops.nt_normalize(zb, zn, inv)
            ops.nt_transpose_cols(zn, znT, col_offset)
            s_loc = ops.nt_fwd_splits(R, R)
            s_rem = ops.nt_fwd_splits(R, Ccols - R)
            part = torch.empty(((s_loc + 2 * s_rem) * R * npart,), device=dev,
                               dtype=torch.float32)
            # the rank's own block first, with its own labels (overlaps the exchange)
            score(y_loc, col_offset, col_offset, col_offset + R, s_loc, 0)
            cur.wait_stream(side)
            zb_all.record_stream(cur)
            if labelled:
                ycol.record_stream(cur)
            del pre_keep  # (the head's per-view gather buffers: the side stream is joined)
            # every row in one launch each (this rank's block is rewritten with identical
            # values, after the local scoring read it: same stream)
            ops.nt_normalize(zb_all, zall, inv_all)
            ops.nt_transpose(zall, znT)
            nsp = s_loc
            for lo, hi in ((0, col_offset), (col_offset + R, Ccols)):
                if hi > lo:
                    sp = max(1, (s_rem * (hi - lo) + (Ccols - R) - 1) // (Ccols - R))
                    score(ycol, 0, lo, hi, sp, nsp)
                    nsp += sp
            finish(nsp)
        else:
            zn = torch.empty((R, D), device=dev, dtype=torch.float32)
            inv = torch.empty((R,), device=dev, dtype=torch.float32)
            ops.nt_normalize(zb, zn, inv)
            zall = zn
            ycol = y_loc
            col_offset = 0
            Ccols = R
            znT = torch.empty((D, Ccols), device=dev, dtype=torch.float32)
            ops.nt_transpose(zall, znT)
            splits = ops.nt_fwd_splits(R, Ccols)
            part = torch.empty((splits * R * npart,), device=dev, dtype=torch.float32)
            score(ycol, 0, 0, Ccols, splits, 0)
            finish(splits)
        out = torch.empty((1,), device=dev, dtype=torch.float32)
        scale = 1.0 / R if reduction == "mean" else 1.0
        ops.nt_reduce_loss(rows, scale, out)
        ctx.save_for_backward(zn, zall, znT, lse, inv, inv_cnt, ycol)
        ctx.cfg = (n, inv_t, scale, col_offset, gather, st, z.dtype, neg)
        return out.view(())

    @staticmethod
    def backward(ctx, gout):
        from ..ops import _ext
        ops = _ext.ops()
        zn, zall, znT, lse, inv, inv_cnt, ycol = ctx.saved_tensors
        n, inv_t, scale, col_offset, gather, st, zdtype, neg = ctx.cfg
        R, D = zn.shape
        Ccols = zall.shape[0]
        dev = zn.device
        g = gout.reshape(1).float().contiguous()

        def grad_pass(row_mode, part, splits, out):
            if ycol is not None:
                ops.nt_sup_backward_part(row_mode, zall, znT, lse, inv_cnt, ycol, R, col_offset,
                                         n, inv_t, scale, g, part, splits, out)
            elif neg is not None:
                ops.nt_w_backward_part(row_mode, zall, znT, lse, R, col_offset, n, inv_t, neg[0],
                                       scale, g, part, splits, out)
            else:
                ops.nt_backward_part(row_mode, zall, znT, lse, R, col_offset, n, inv_t, scale, g,
                                     part, splits, out)

        s_col = ops.nt_bwd_splits(Ccols, R)
        part2 = torch.empty((s_col * Ccols * D,), device=dev, dtype=torch.float32)
        d_cols = torch.empty((Ccols, D), device=dev, dtype=torch.float32)
        grad_pass(False, part2, s_col, d_cols)
        overlap = gather and st.comm
        if overlap:
            # global negatives: only this rank's slice of the column gradient is needed, so a
            # reduce-scatter (1/W of an all-reduce's bytes over xGMI) — issued on a side stream
            # so it runs under the row-gradient kernel below
            cur = torch.cuda.current_stream(dev)
            side = _side_stream(dev)
            side.wait_stream(cur)
            mine = torch.empty((R, D), device=dev, dtype=torch.float32)
            with torch.cuda.stream(side):
                ipc = getattr(st, "ipc", None)
                if ipc is not None:
                    ipc.reduce_scatter(("ntxent", "dcols"), d_cols, mine)
                else:
                    dist.reduce_scatter_tensor(mine, d_cols, group=st.group)
            # (d_cols / mine stay referenced until the join below, which orders every later
            # allocation on this stream after the side stream's use)
        s_row = ops.nt_bwd_splits(R, Ccols)
        part = torch.empty((s_row * R * D,), device=dev, dtype=torch.float32)
        d_rows = torch.empty((R, D), device=dev, dtype=torch.float32)
        grad_pass(True, part, s_row, d_rows)
        if overlap:
            cur.wait_stream(side)
            d_rows += mine
        else:
            d_rows += d_cols[col_offset:col_offset + R]
        if zdtype == torch.bfloat16:
            dz = torch.empty((R, D), device=dev, dtype=torch.bfloat16)
            ops.nt_normalize_backward(zn, inv, d_rows, dz, None)
        else:
            dz = torch.empty((R, D), device=dev, dtype=torch.float32)
            ops.nt_normalize_backward(zn, inv, d_rows, None, dz)
        return dz, None, None, None, None, None, None, None


class NTXent(nn.Module):
    def __init__(self, temperature: float = 0.1, reduction: str = "mean",
                 device: Optional[torch.device] = None, gather=False, supervised: bool = False,
                 hard_beta: float = 0.0, tau_plus: float = 0.0, decoupled: bool = False):
        """``gather``: False (reference, per-GPU negatives), True (all-gathered global
        negatives, fused kernel) or ``"ring"`` (global negatives circulated around the ranks,
        loss/ring.py).  ``supervised``: the SupCon loss (module docstring); ``forward`` then
        needs ``labels``.  ``hard_beta`` >= 0, ``tau_plus`` in [0, 1), ``decoupled``: weighted
        negatives (module docstring); not with ``supervised`` or the ring."""
        assert temperature > 0.0
        assert reduction in {"none", "mean", "sum"}
        super().__init__()
        self.temperature = temperature
        self.reduction = reduction
        self.gather = "ring" if str(gather).lower() == "ring" else bool(gather)
        self.supervised = bool(supervised)
        if self.supervised and self.gather == "ring":
            raise ValueError("loss.supervised=true is not available with loss.gather=ring "
                             "(use loss.gather=true for global columns)")
        self.weighted = check_negatives(hard_beta, tau_plus, decoupled)
        self.hard_beta, self.tau_plus, self.decoupled = float(hard_beta), float(tau_plus), decoupled
        if self.weighted:
            keys = "loss.hard_beta / loss.tau_plus / loss.decoupled"
            if self.supervised:
                raise ValueError(f"{keys} are not available with loss.supervised=true")
            if self.gather == "ring":
                raise ValueError(f"{keys} are not available with loss.gather=ring "
                                 "(use loss.gather=true for global columns)")
        # (β, τ⁺, decoupled) of the weighted kernels; None: plain NT-Xent / SupCon
        self._neg = (self.hard_beta, self.tau_plus, self.decoupled) if self.weighted else None

    def forward(self, view0: torch.Tensor, view1: Optional[torch.Tensor] = None,
                labels: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``forward(view0, view1)`` as the reference, or ``forward(z)`` with z = [view0; view1];
        ``labels`` = y[n], one integer per image, with ``supervised`` (and only then)."""
        if view1 is not None:
            z = torch.cat([view0, view1], dim=0)
            n = view0.shape[0]
        else:
            z = view0
            n = z.shape[0] // 2
        st = pstate.get()
        R, D = z.shape
        if self.supervised and labels is None:
            raise ValueError("the supervised loss (loss.supervised) needs labels")
        if labels is not None and not self.supervised:
            raise ValueError("labels were given but the loss is not supervised "
                             "(loss.supervised)")
        y = _check_labels(labels, n, z.device) if self.supervised else None
        if self.gather == "ring" and st.comm and st.world_size > 1:
            # global negatives with the column blocks circulating around the ranks (loss/ring.py)
            from .ring import nt_xent_ring
            if self.reduction != "mean":
                raise ValueError("ring NT-Xent supports reduction='mean'")
            return nt_xent_ring(z, n, self.temperature, st.group, st.world_size, st.rank)
        if (z.is_cuda and self.reduction != "none" and registry.use_hip(z) and R % 16 == 0
                and D in (32, 64, 128, 256)):
            return _NTXentHipFn.apply(z, y, n, self.temperature, self.reduction, self.gather, st,
                                      self._neg)
        if self.weighted:
            return nt_xent_weighted_torch(z, n, self.temperature, self.hard_beta, self.tau_plus,
                                          self.decoupled, self.reduction, self.gather, st.group,
                                          st.world_size, st.rank)
        if self.supervised:
            return sup_con_torch(z, n, y, self.temperature, self.reduction, self.gather,
                                 st.group, st.world_size, st.rank)
        return nt_xent_torch(z, n, self.temperature, self.reduction, self.gather, st.group,
                             st.world_size, st.rank)


class SupCon(NTXent):
    """``NTXent(..., supervised=True)`` with the labels as a positional argument."""

    def __init__(self, temperature: float = 0.1, reduction: str = "mean",
                 device: Optional[torch.device] = None, gather=False):
        super().__init__(temperature, reduction, device, gather, supervised=True)

    def forward(self, z: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:  # noqa: D102
        return super().forward(z, None, labels=labels)


# reference class name
NT_Xent = NTXent
