"""NNCLR loss (Dwibedi et al., 2021, "With a Little Help from My Friends"): every embedding is
replaced by its nearest neighbour in a FIFO support set of past embeddings, and that neighbour
is contrasted against the other view of the image (``loss.kind=nnclr``).  The paper's predictor
MLP is not part of it.

The contract, identical in the kernels of ``csrc/nnclr.hip`` and in :func:`nnclr_torch`:

1. Rows are ``z = [view0; view1]``, ``[2n][D]``.  On the HIP path z is the head's bf16 output; an
   fp32 z is read as given.  dz comes back in z's dtype.  ``ẑ = z / max(‖z‖, 1e-12)`` in fp32
   (the norm accumulated in fp64 and rounded once, the quotient correctly rounded, so the
   kernel and the twin form the same bits).  The rounding point: the NT-Xent kernels never round
   ẑ (their only bf16 value is z itself; ``k_normalize`` writes ẑ in fp32 and the similarity runs
   on the fp32 MFMA).  Here the support set holds bf16 rows and the search runs on the bf16 MFMA,
   so ẑ is rounded to bf16 ONCE, right after the normalisation, and that ``ẑb`` is the operand
   of the lookup, of the loss and of the enqueue; the fp32 ẑ is kept for the normalisation
   backward alone, as NT-Xent keeps it.  With ``round_operands`` the twin rounds at that point;
   everything below is then exact on those operands up to the fp32 summation order.
2. Support set ``Qm [Q][D]``, bf16 unit rows, and a device int32 cursor, both allocated when the
   module is built: ``torch.randn`` from a generator seeded with the run's seed, L2-normalised,
   rounded to bf16.  The set is always full; there is no "filled" count.
3. Lookup, for each of the 2n rows: ``j(r) = argmax_k ẑb_r·Qm_k`` (fp32 accumulation over bf16
   operands), ordered by (similarity descending, index ascending): exact ties go to the lowest
   k; a NaN similarity never wins, and a row whose similarities are all NaN (or −inf) takes
   index 0.  ``a_r = Qm[j(r)]`` is copied into a saved ``[2n][D]`` bf16 buffer in the forward;
   the backward reads that buffer, never the queue.  No gradient flows through the lookup or a.
4. Loss (the paper's pseudo-code, symmetrised): row ``r = v·n + i`` against the n embeddings of
   the other view, ``s_rc = a_r·ẑb_{(1−v)n+c} / τ``, ``loss_r = LSE_c s_rc − s_ri``,
   ``loss = (1/2n) Σ_r loss_r`` in a fixed order.  The mean is the only reduction.
5. Backward, g the upstream scalar (read on the device), ``p_rc = softmax_c s_rc``:
   ``dẑ_{(1−v)n+c} = (g / (2nτ)) Σ_i (p_{(vn+i),c} − [i = c]) · a_{vn+i}`` (S recomputed from the
   saved operands; the rounding of ẑ passes the gradient straight through), then the NT-Xent
   normalisation backward ``dz = (dẑ − ẑ (ẑ·dẑ)) / max(‖z‖, 1e-12)`` on the fp32 ẑ.
6. Enqueue, after both lookups and the loss forward of the step: the n rows ẑb of view 0 go to
   positions ``(cursor + b) mod Q``, ``b = 0..n−1`` (a write may wrap in the middle of a batch),
   then ``cursor ← (cursor + n) mod Q``; one launch (one block: no block may read the cursor
   after it was advanced), the cursor never visits the host.  Both lookups of a step see the
   queue as it was when the step began.  ``NNCLR.forward(z, update=False)`` leaves queue and
   cursor alone.
7. Bitwise repeatable, no atomics: candidates are merged across lane groups and queue splits by
   the total order of 3.  No per-step host value reaches a launch and the allocations are
   ``torch.empty`` calls as in ``_NTXentHipFn``, so the step captures and replays as before; the
   enqueue is the last launch of the loss's forward, on its stream, behind the lookup.
8. HIP path: ``n % 16 == 0``, ``D ∈ {32, 64, 128, 256}``, ``Q % 256 == 0``, ``n ≤ Q`` and
   ``registry.use_hip(z)``; anything else takes the unrounded twin (fp32; fp64 for a ``double``
   z), whose enqueue still writes bf16 rows.
9. Data-parallel runs: loss and support set are per rank; the gradients are averaged by the flat
   store's buckets.  The resume file carries ``nn_queue`` (queue, cursor) of rank 0.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from ..ops import registry


def _bf16_round(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(x.dtype)


def _normalize_exact(zf: torch.Tensor):
    """zf [R][D] fp32 -> ẑ fp32, 1 / max(‖z‖, 1e-12) [R]: ``k_nc_normalize``'s values (the norm
    in fp64, rounded once; quotients through fp64, whose second rounding to fp32 is innocuous, so
    they are the correctly rounded fp32 quotients on every device)."""
    zd = zf.double()
    den = zd.pow(2).sum(dim=1, keepdim=True).sqrt().float().clamp_min(1e-12).double()
    return (zd / den).float(), (1.0 / den).float().squeeze(1)


def nn_lookup_torch(zq: torch.Tensor, queue: torch.Tensor) -> torch.Tensor:
    """``argmax_k zq_r·queue_k`` by (similarity descending, index ascending); a NaN never wins,
    a row without a finite or +inf similarity takes index 0.  Returns int64 ``[R]``."""
    sim = zq @ queue.to(zq.dtype).t()
    sim = torch.where(torch.isnan(sim), torch.full_like(sim, float("-inf")), sim)
    best = sim.max(dim=1, keepdim=True).values
    Q = queue.shape[0]
    ar = torch.arange(Q, device=sim.device).expand_as(sim)
    return torch.where(sim == best, ar, torch.full_like(ar, Q)).min(dim=1).values


def _cross_logits(a: torch.Tensor, zop: torch.Tensor, n: int, inv_t: float) -> torch.Tensor:
    """S [2][n][n]: S[v][i][c] = a_{vn+i}·zop_{(1−v)n+c} / τ."""
    av, zv = a.view(2, n, -1), zop.view(2, n, -1)
    return torch.stack([av[0] @ zv[1].t(), av[1] @ zv[0].t()]) * inv_t


def _loss_from_logits(S: torch.Tensor) -> torch.Tensor:
    n = S.shape[1]
    rows = torch.logsumexp(S, dim=2) - torch.diagonal(S, dim1=1, dim2=2)
    return rows.sum() / (2 * n)


def nnclr_backward_torch(zn: torch.Tensor, inv_norm: torch.Tensor, zop: torch.Tensor,
                         a: torch.Tensor, n: int, temperature: float, g) -> torch.Tensor:
    """The explicit backward of the contract (5): ``zn`` the unrounded ẑ, ``inv_norm`` =
    1 / max(‖z‖, 1e-12), ``zop`` the loss's operand (ẑb, or ẑ for the unrounded twin), ``a`` the
    neighbours, ``g`` the upstream scalar.  Returns dz ``[2n][D]`` in zn's dtype."""
    inv_t = 1.0 / temperature
    S = _cross_logits(a, zop, n, inv_t)
    P = torch.softmax(S, dim=2)
    W = (g / (2 * n)) * (P - torch.eye(n, dtype=S.dtype, device=S.device))
    av = a.view(2, n, -1)
    # dẑ of view 1 from the anchors of view 0, and the reverse
    dzh = torch.cat([W[1].t() @ av[1], W[0].t() @ av[0]]) * inv_t
    dot = (zn * dzh).sum(dim=1, keepdim=True)
    return (dzh - zn * dot) * inv_norm.unsqueeze(1)


class _NNCLRTwinFn(torch.autograd.Function):
    """The twin with ``round_operands``: ẑ rounded to bf16 where ``k_nc_normalize`` rounds it."""

    @staticmethod
    def forward(ctx, z, queue, n, temperature, nn_idx):
        zn, inv = _normalize_exact(z.float())
        zb = _bf16_round(zn)
        idx = nn_lookup_torch(zb, queue) if nn_idx is None else nn_idx.to(torch.int64)
        a = queue[idx]
        af = a.float()
        ctx.save_for_backward(zn, inv, zb, af)
        ctx.cfg = (n, temperature, z.dtype)
        ctx.mark_non_differentiable(idx, a)
        return _loss_from_logits(_cross_logits(af, zb, n, 1.0 / temperature)), idx, a

    @staticmethod
    def backward(ctx, gout, _gi, _ga):
        zn, inv, zb, af = ctx.saved_tensors
        n, temperature, zdtype = ctx.cfg
        dz = nnclr_backward_torch(zn, inv, zb, af, n, temperature, gout.float())
        return dz.to(zdtype), None, None, None, None


def nnclr_torch(z: torch.Tensor, queue: torch.Tensor, n: int, temperature: float,
                round_operands: bool = False, nn_idx: Optional[torch.Tensor] = None,
                return_nn: bool = False):
    """The loss on torch ops; ``z`` = [view0; view1] of shape [2n, D], ``queue`` the support set
    ``[Q][D]`` (read, never written).  Without ``round_operands`` these are plain differentiable
    ops on the unrounded ẑ (a ``double`` z gives the fp64 oracle); with it, an explicit function
    that rounds ẑ to bf16 where the kernels do.  ``nn_idx`` ``[2n]``: take these neighbours
    instead of searching (the tests pass the kernel's own choice, so that a near-tie cannot move
    a comparison).  ``return_nn``: also return idx (int64 ``[2n]``) and ``a = queue[idx]``."""
    if z.dim() != 2 or z.shape[0] != 2 * n:
        raise ValueError(f"z must be [2n][D] with n = {n}, got {tuple(z.shape)}")
    if queue.dim() != 2 or queue.shape[1] != z.shape[1]:
        raise ValueError(f"the support set must be [Q][{z.shape[1]}], got {tuple(queue.shape)}")
    if round_operands:
        loss, idx, a = _NNCLRTwinFn.apply(z, queue, n, float(temperature), nn_idx)
    else:
        zf = z if z.dtype == torch.float64 else z.float()
        zh = zf / zf.norm(dim=1, keepdim=True).clamp_min(1e-12)
        idx = (nn_lookup_torch(zh.detach(), queue) if nn_idx is None
               else nn_idx.to(torch.int64))
        a = queue[idx]
        loss = _loss_from_logits(_cross_logits(a.to(zh.dtype), zh, n, 1.0 / temperature))
    return (loss, idx, a) if return_nn else loss


def enqueue_torch(queue: torch.Tensor, cursor: torch.Tensor, rows: torch.Tensor) -> None:
    """The contract's enqueue (6) on torch ops, in place and without a host read: ``rows``
    ``[n][D]`` go to ``(cursor + b) mod Q``, then the cursor advances by n.  More rows than the
    set holds: the last Q of them remain, as writing them one after another would leave."""
    Q, n = queue.shape[0], rows.shape[0]
    b = torch.arange(max(0, n - Q), n, device=queue.device)
    pos = (cursor.to(torch.int64) + b) % Q
    queue.index_copy_(0, pos, rows[b].to(queue.dtype))
    cursor.copy_((cursor.to(torch.int64) + n) % Q)


class _NNCLRHipFn(torch.autograd.Function):
    """Seven launches forward (normalise, top-1 per split, select + gather, loss partials, their
    merge, the mean, enqueue; six with ``update=False``), two backward (column pass, split sum +
    normalisation backward)."""

    @staticmethod
    def forward(ctx, z, queue, cursor, n, temperature, update):
        from ..ops import _ext
        ops = _ext.ops()
        R, D = z.shape
        Q = queue.shape[0]
        dev = z.device
        zc = z.contiguous()
        inv_t = 1.0 / temperature
        zn = torch.empty((R, D), device=dev, dtype=torch.float32)
        zb = torch.empty((R, D), device=dev, dtype=torch.bfloat16)
        inv = torch.empty((R,), device=dev, dtype=torch.float32)
        ops.nc_normalize(zc, zn, zb, inv)
        qs = ops.nc_top1_splits(R, Q)
        candv = torch.empty((qs, R), device=dev, dtype=torch.float32)
        candi = torch.empty((qs, R), device=dev, dtype=torch.int32)
        idx = torch.empty((R,), device=dev, dtype=torch.int32)
        a = torch.empty((R, D), device=dev, dtype=torch.bfloat16)
        ops.nc_lookup(zb, queue, qs, candv, candi, idx, a)
        ls = ops.nc_loss_splits(n)
        part = torch.empty((ls * R * 3,), device=dev, dtype=torch.float32)
        ops.nc_forward(a, zb, inv_t, ls, part)
        lse = torch.empty((R,), device=dev, dtype=torch.float32)
        rows = torch.empty((R,), device=dev, dtype=torch.float32)
        ops.nt_finish(part, R, ls, lse, rows)
        out = torch.empty((1,), device=dev, dtype=torch.float32)
        ops.nt_reduce_loss(rows, 1.0 / R, out)
        if update:  # behind every launch that reads the queue
            ops.nc_enqueue(zb, queue, cursor)
        ctx.save_for_backward(zn, zb, inv, a, lse)
        ctx.cfg = (n, inv_t, ls, z.dtype)
        ctx.mark_non_differentiable(idx, a)
        return out.view(()), idx, a

    @staticmethod
    def backward(ctx, gout, _gi, _ga):
        from ..ops import _ext
        ops = _ext.ops()
        zn, zb, inv, a, lse = ctx.saved_tensors
        n, inv_t, ls, zdtype = ctx.cfg
        R, D = zn.shape
        dev = zn.device
        g = gout.reshape(1).float().contiguous()
        part = torch.empty((ls * R * D,), device=dev, dtype=torch.float32)
        if zdtype == torch.bfloat16:
            dz = torch.empty((R, D), device=dev, dtype=torch.bfloat16)
            ops.nc_backward(a, zb, zn, inv, lse, inv_t, g, ls, part, dz, None)
        else:
            dz = torch.empty((R, D), device=dev, dtype=torch.float32)
            ops.nc_backward(a, zb, zn, inv, lse, inv_t, g, ls, part, None, dz)
        return dz, None, None, None, None, None


def hip_path(z: torch.Tensor, n: int, Q: int) -> bool:
    """Whether ``z`` = [2n][D] with a support set of Q rows takes the kernels (limits: module
    docstring, 8)."""
    D = z.shape[1]
    return (z.is_cuda and z.dtype in (torch.bfloat16, torch.float32) and n >= 16 and n % 16 == 0
            and D in (32, 64, 128, 256) and Q >= 256 and Q % 256 == 0 and n <= Q
            and registry.use_hip(z))


class NNCLR(nn.Module):
    def __init__(self, temperature: float = 0.1, queue_size: int = 16384, dim: int = 128,
                 device: Optional[torch.device] = None, seed: Optional[int] = None):
        """``temperature``: τ; ``queue_size``: Q, the support set's rows (``loss.nn_queue``);
        ``dim``: D (``parameter.d``); ``seed``: of the generator the initial rows are drawn from
        (None: torch's global one)."""
        if not temperature > 0.0:
            raise ValueError(f"parameter.temperature must be > 0, got {temperature}")
        if int(queue_size) < 1 or int(dim) < 1:
            raise ValueError(f"loss.nn_queue and the embedding size must be >= 1, got "
                             f"{queue_size}, {dim}")
        super().__init__()
        self.temperature = float(temperature)
        gen = None
        if seed is not None:
            gen = torch.Generator()
            gen.manual_seed(int(seed))
        rows = torch.randn((int(queue_size), int(dim)), generator=gen, dtype=torch.float32)
        rows = torch.nn.functional.normalize(rows, p=2, dim=1).to(torch.bfloat16)
        self.register_buffer("queue", rows.to(device) if device is not None else rows)
        self.register_buffer("cursor", torch.zeros((1,), dtype=torch.int32, device=device))

    @property
    def queue_size(self) -> int:
        return self.queue.shape[0]

    def queue_state(self) -> dict:
        """The resume file's ``nn_queue`` entry: the support set and the cursor, on the host."""
        return {"queue": self.queue.detach().cpu().clone(),
                "cursor": self.cursor.detach().cpu().clone()}

    def load_queue_state(self, state: dict) -> None:
        q, c = state["queue"], state["cursor"]
        if tuple(q.shape) != tuple(self.queue.shape) or q.dtype != self.queue.dtype:
            raise ValueError(f"nn_queue: the file's support set is {tuple(q.shape)} {q.dtype}, "
                             f"this run's (loss.nn_queue, parameter.d) "
                             f"{tuple(self.queue.shape)} {self.queue.dtype}")
        self.queue.copy_(q)
        self.cursor.copy_(c.reshape(1).to(torch.int32))

    def forward(self, view0: torch.Tensor, view1: Optional[torch.Tensor] = None,
                update: bool = True, return_nn: bool = False):
        """``forward(view0, view1)`` or ``forward(z)`` with z = [view0; view1], as ``NTXent``;
        returns the scalar loss (``return_nn``: and idx ``[2n]``, a ``[2n][D]``).  ``update``:
        enqueue view 0's ẑb behind the lookups and advance the cursor."""
        if view1 is not None:
            z = torch.cat([view0, view1], dim=0)
            n = view0.shape[0]
        else:
            z = view0
            n = z.shape[0] // 2
        if z.dim() != 2 or z.shape[0] != 2 * n or n < 1:
            raise ValueError(f"z must be [2n][D], got {tuple(z.shape)}")
        if z.shape[1] != self.queue.shape[1]:
            raise ValueError(f"z has D = {z.shape[1]}, the support set D = "
                             f"{self.queue.shape[1]} (parameter.d)")
        if hip_path(z, n, self.queue_size):
            loss, idx, a = _NNCLRHipFn.apply(z, self.queue, self.cursor, n, self.temperature,
                                             bool(update))
        else:
            loss, idx, a = nnclr_torch(z, self.queue, n, self.temperature, return_nn=True)
            if update:
                with torch.no_grad():
                    zn, _ = _normalize_exact(z[:n].detach().float())
                    enqueue_torch(self.queue, self.cursor, zn)
        return (loss, idx, a) if return_nn else loss
