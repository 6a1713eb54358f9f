"""Linear-probe sweep: G = |lrs| x |decays| linear classifiers trained on the same shuffled
feature batches, on the HIP kernels of csrc/probe.hip on the GPU and as torch ops of the same
contract (the twin) elsewhere.  The twin is the CPU path and the tests' oracle.

Contract (both paths):

* features are rounded once to bf16 and zero-padded to a multiple of ``K_STEP`` columns
  (``prepare_features``); they are frozen data;
* every configuration starts from the same ``nn.Linear(F, C)`` initialisation and owns the columns
  ``[g · Cp, g · Cp + C)`` of ``G · Cp``, ``Cp = 16 · ceil(C / 16)``; padding columns take no part
  in the softmax, get zero gradient and never move;
* forward: ``logits = X[idx] · Wshᵀ + b`` on a bf16 shadow of the fp32 master weights, fp32
  accumulation, fp32 bias; softmax, CE and ``dlogits = (softmax - onehot) / rows`` in fp32 per
  configuration (``rows`` is the rows present: the last batch of an epoch is ragged);
* ``db`` is the fp32 column sum of ``dlogits``; ``dW = bf16(dlogits)ᵀ · X[idx]`` with fp32
  accumulation over the whole batch (no split-K);
* update: ``torch.optim.SGD(nesterov=True)`` in fp32 on weights and bias alike — ``g += wd · p``,
  ``buf = g`` on step 0 else ``m · buf + g``, ``p -= lr · (g + m · buf)`` — then the shadow is
  refreshed; ``lr = lr0_g · f[step]`` as an fp32 product with ``f`` tabulated once on the host in
  fp64 and rounded to fp32 (``cosine_table``), so device and twin use the same bits;
* evaluation: per configuration mean CE, top-1 and top-k with ``ops.classify.ce_rank``'s rules
  (ties to the lower class, a NaN logit of another class ranks above the target, a NaN target
  logit is never correct);
* a configuration's trajectory is bitwise independent of the other configurations and of G: the
  kernels compute a configuration from its own columns in an order fixed by (rows, F, C), the
  twin runs the configurations one after the other on identical shapes.

Limits: ``G <= 16``, ``G · Cp <= 1024``, padded feature width ``<= 4096``, batch ``<= 4096``.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import registry

K_STEP = 64          # feature columns are zero-padded to a multiple of it
MAX_CONFIGS = 16
MAX_COLS = 1024      # G · Cp
MAX_FP = 4096
MAX_ROWS = 4096      # rows of one kernel call: the batch size, and the evaluation chunk


def padded_classes(num_classes: int) -> int:
    return (num_classes + 15) // 16 * 16


def padded_features(num_features: int) -> int:
    return (num_features + K_STEP - 1) // K_STEP * K_STEP


def grid(lrs: Sequence[float], decays: Sequence[float]) -> List[Tuple[float, float]]:
    """The sweep's (lr, decay) configurations: decay-major, lr-minor."""
    return [(float(lr), float(d)) for d in decays for lr in lrs]


def check_limits(num_configs: int, num_classes: Optional[int] = None,
                 num_features: Optional[int] = None, batch: Optional[int] = None) -> None:
    """``ValueError`` naming the failing key for anything outside the kernels' limits."""
    if not 1 <= num_configs <= MAX_CONFIGS:
        raise ValueError(f"parameter.sweep_lr x parameter.sweep_decay: {num_configs} "
                         f"configurations, must be in [1, {MAX_CONFIGS}]")
    if num_classes is not None:
        if num_classes < 1:
            raise ValueError(f"num_classes must be >= 1, got {num_classes}")
        cols = num_configs * padded_classes(num_classes)
        if cols > MAX_COLS:
            raise ValueError(
                f"parameter.sweep_lr x parameter.sweep_decay: {num_configs} configurations x "
                f"{padded_classes(num_classes)} padded classes = {cols} columns, must be <= "
                f"{MAX_COLS}")
    if num_features is not None and not 1 <= padded_features(num_features) <= MAX_FP:
        raise ValueError(f"feature width {num_features} (padded {padded_features(num_features)}) "
                         f"must be in [1, {MAX_FP}]")
    if batch is not None and not 1 <= batch <= MAX_ROWS:
        raise ValueError(f"experiment.batches must be in [1, {MAX_ROWS}] for a sweep, got {batch}")


def cosine_table(total_steps: int) -> torch.Tensor:
    """f[step] = ½ (1 + cos(π · step / total)) for step in [0, total), fp64 rounded to fp32."""
    f = [0.5 * (1.0 + math.cos(math.pi * s / total_steps)) for s in range(max(1, total_steps))]
    return torch.tensor(f, dtype=torch.float64).to(torch.float32)


def initial_lrs(lrs: Sequence[float], batch: int, linear_schedule: bool) -> List[float]:
    if linear_schedule:
        return [lr * batch / 256.0 for lr in lrs]
    return [lr * math.sqrt(batch) for lr in lrs]


def prepare_features(X: torch.Tensor, round_operands: bool = True) -> torch.Tensor:
    """[N][F] -> [N][Fp] zero-padded, rounded once to bf16 (fp32 with the rounding off)."""
    assert X.dim() == 2, "expected [rows][features]"
    N, F = X.shape
    Fp = padded_features(F)
    if Fp > MAX_FP:
        raise ValueError(f"feature width {F} (padded {Fp}) exceeds {MAX_FP}")
    out = torch.zeros(N, Fp, device=X.device, dtype=torch.bfloat16 if round_operands else torch.float32)
    out[:, :F] = X.float()
    return out


def _rank(z: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """The target's rank by ``ce_rank``'s rules on [rows][C] logits."""
    C = z.shape[1]
    ok = (t >= 0) & (t < C)
    tc = t.clamp(0, C - 1).view(-1, 1)
    zt = z.gather(1, tc)
    cls = torch.arange(C, device=z.device).view(1, -1)
    above = (z > zt) | ((z == zt) & (cls < tc)) | (torch.isnan(z) & (cls != tc))
    never = torch.isnan(zt.view(-1)) | ~ok
    return torch.where(never, torch.full_like(tc.view(-1), C), above.sum(1)).to(torch.int32)


def _ce_twin(z: torch.Tensor, t: torch.Tensor, grad: bool = True):
    """The twins' softmax / CE block on fp32 logits ``z`` [rows][C] and targets ``t`` [rows]:
    per-row loss (NaN for a target outside [0, C)), the target's rank and, with ``grad``,
    ``(softmax - onehot) / rows`` (a row without a valid target has no one-hot entry)."""
    rows, C = z.shape
    ok = (t >= 0) & (t < C)
    tc = t.clamp(0, C - 1)
    m = z.max(1).values
    e = torch.exp(z - m[:, None])
    s = e.sum(1)
    nan = torch.full((rows,), float("nan"), device=z.device)
    zt = torch.where(ok, z.gather(1, tc.view(-1, 1)).view(-1), nan)
    loss = torch.log(s) + m - zt
    rank = _rank(z, t)
    if not grad:
        return loss, rank, None
    onehot = torch.zeros(rows, C, device=z.device, dtype=torch.float32)
    onehot[torch.arange(rows, device=z.device)[ok], tc[ok]] = 1.0
    return loss, rank, (e / s[:, None] - onehot) / float(rows)


class LinearSweep:
    """State of a sweep: fp32 master weights and momentum, the bf16 shadow and the step counter.

    ``weight`` [C][F] / ``bias`` [C] are the one initialisation every configuration starts from;
    ``lr0`` / ``decay`` hold one value per configuration; ``ftab`` is ``cosine_table(total)``.
    ``round_operands=False`` and ``accumulate=torch.float64`` exist for the tests (the twin's
    semantics against ``learnable_eval``, and its own accumulation error); both select the twin,
    as does ``hip=False``."""

    def __init__(self, weight: torch.Tensor, bias: torch.Tensor, lr0: Sequence[float],
                 decay: Sequence[float], momentum: float, ftab: torch.Tensor, device=None,
                 round_operands: bool = True, accumulate: torch.dtype = torch.float32,
                 hip: Optional[bool] = None):
        assert weight.dim() == 2 and bias.dim() == 1 and bias.shape[0] == weight.shape[0]
        assert len(lr0) == len(decay), "one lr0 and one decay per configuration"
        dev = torch.device(device) if device is not None else weight.device
        self.device = dev
        self.G, self.C, self.F = len(lr0), weight.shape[0], weight.shape[1]
        self.Cp, self.Fp = padded_classes(self.C), padded_features(self.F)
        check_limits(self.G, self.C, self.F)
        for v in lr0:
            if not v > 0:
                raise ValueError(f"parameter.sweep_lr: every lr must be > 0, got {v}")
        for v in decay:
            if not v >= 0:
                raise ValueError(f"parameter.sweep_decay: every decay must be >= 0, got {v}")
        self.round_operands = bool(round_operands)
        self.accumulate = accumulate
        plain = self.round_operands and accumulate == torch.float32
        if hip is None:
            hip = plain and dev.type == "cuda" and registry.use_hip(torch.empty(0, device=dev))
        if hip and not plain:
            raise ValueError("the HIP path rounds its operands and accumulates in fp32")
        self.hip = bool(hip)
        NT = self.G * self.Cp
        self.W = torch.zeros(NT, self.Fp, device=dev, dtype=torch.float32)
        self.b = torch.zeros(NT, device=dev, dtype=torch.float32)
        Wv, bv = self.W.view(self.G, self.Cp, self.Fp), self.b.view(self.G, self.Cp)
        Wv[:, :self.C, :self.F] = weight.detach().to(device=dev, dtype=torch.float32)
        bv[:, :self.C] = bias.detach().to(device=dev, dtype=torch.float32)
        self.Mw = torch.zeros_like(self.W)
        self.Mb = torch.zeros_like(self.b)
        self.Wsh = self.W.to(torch.bfloat16) if self.round_operands else self.W
        self.lr0 = torch.tensor([float(v) for v in lr0], dtype=torch.float64).to(torch.float32).to(dev)
        self.wd = torch.tensor([float(v) for v in decay], dtype=torch.float64).to(torch.float32).to(dev)
        self.momentum = float(momentum)
        self.ftab = ftab.to(device=dev, dtype=torch.float32).contiguous()
        self.step = 0
        self._scratch: Dict[str, torch.Tensor] = {}

    # ------------------------------------------------------------------ accessors
    def weights(self, g: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(W [C][F], b [C]) fp32 master of configuration ``g``."""
        return (self.W.view(self.G, self.Cp, self.Fp)[g, :self.C, :self.F],
                self.b.view(self.G, self.Cp)[g, :self.C])

    def _check_batch(self, X: torch.Tensor, idx: torch.Tensor) -> int:
        rows = idx.numel()
        if X.dim() != 2 or X.shape[1] != self.Fp:
            raise ValueError(f"features must be prepare_features() output [N][{self.Fp}], got "
                             f"{tuple(X.shape)}")
        if not 1 <= rows <= MAX_ROWS:
            raise ValueError(f"experiment.batches: a call takes 1..{MAX_ROWS} rows, got {rows}")
        return rows

    def _buf(self, name: str, shape, dtype) -> torch.Tensor:
        t = self._scratch.get(name)  # the kernels' scratch: fixed shapes, allocated once
        if t is None:
            t = self._scratch[name] = torch.empty(*shape, device=self.device, dtype=dtype)
        return t

    # ------------------------------------------------------------------ forward
    def forward(self, X: torch.Tensor, y: torch.Tensor, idx: torch.Tensor, train: bool = True,
                loss_out: Optional[torch.Tensor] = None, loss_offset: int = 0,
                want_rank: bool = True) -> Dict[str, torch.Tensor]:
        """Forward / CE (and the gradients when ``train``) of the rows ``idx`` of ``X``.

        Returns ``loss`` [G][rows], ``rank`` [G][rows] int32, ``logits`` [rows][G][C] and, when
        training, ``dl`` [G][rows][C] (the rounded dlogits as fp32) and ``db`` [G][C].  With
        ``loss_out`` [G][n] the losses are written to its columns ``loss_offset ...`` instead."""
        rows = self._check_batch(X, idx)
        idx = idx.to(device=self.device, dtype=torch.long).contiguous()
        if loss_out is not None:
            assert loss_out.dim() == 2 and loss_out.shape[0] == self.G and loss_out.is_contiguous()
            assert 0 <= loss_offset and loss_offset + rows <= loss_out.shape[1]
        if self.hip:
            return self._forward_hip(X, y, idx, rows, train, loss_out, loss_offset, want_rank)
        return self._forward_twin(X, y, idx, rows, train, loss_out, loss_offset)

    def _forward_hip(self, X, y, idx, rows, train, loss_out, loss_offset, want_rank):
        from . import _ext
        G, C, Cp = self.G, self.C, self.Cp
        NT = G * Cp
        Z = self._buf("Z", (MAX_ROWS, NT), torch.float32)
        if loss_out is None:
            lbuf = self._buf("loss", (G, MAX_ROWS), torch.float32)
            lflat, stride, loss = lbuf.view(-1), MAX_ROWS, lbuf[:, :rows]
        else:
            lflat, stride = loss_out.view(-1)[loss_offset:], loss_out.shape[1]
            loss = loss_out[:, loss_offset:loss_offset + rows]
        rank = torch.empty(G, rows, device=self.device, dtype=torch.int32) if want_rank else None
        dlT = dbp = None
        if train:
            dlT = self._buf("dlT", (NT, MAX_ROWS), torch.bfloat16)
            dbp = self._buf("dbp", (MAX_ROWS // 16, NT), torch.float32)
        _ext.ops().probe_forward(X, y, idx, self.Wsh, self.b, G, C, Z, lflat, stride, rank, dlT, dbp)
        out = {"loss": loss, "rank": rank, "logits": Z[:rows].view(rows, G, Cp)[:, :, :C]}
        if train:
            out["dlT"], out["dbp"] = dlT, dbp
            out["dl"] = dlT.view(G, Cp, -1)[:, :C, :rows].permute(0, 2, 1)
            out["db"] = dbp[:(rows + 15) // 16].view(-1, G, Cp)[:, :, :C]
        return out

    def _forward_twin(self, X, y, idx, rows, train, loss_out, loss_offset):
        G, C, Cp = self.G, self.C, self.Cp
        acc = self.accumulate
        xa = X[idx].to(acc)
        t = y.to(device=self.device, dtype=torch.long)[idx]
        Wv, bv = self.Wsh.view(G, Cp, self.Fp), self.b.view(G, Cp)
        loss = torch.empty(G, rows, device=self.device, dtype=torch.float32)
        rank = torch.empty(G, rows, device=self.device, dtype=torch.int32)
        logits = torch.empty(rows, G, C, device=self.device, dtype=torch.float32)
        dl = torch.zeros(G, rows, C, device=self.device, dtype=torch.float32) if train else None
        db = torch.zeros(G, C, device=self.device, dtype=torch.float32) if train else None
        for g in range(G):  # one configuration at a time, identical shapes: bitwise independent
            z = (xa @ Wv[g, :C].to(acc).t()).float() + bv[g, :C]
            loss[g], rank[g], d = _ce_twin(z, t, train)
            logits[:, g] = z
            if train:
                db[g] = d.to(acc).sum(0).float()
                dl[g] = d.to(torch.bfloat16).float() if self.round_operands else d
        if loss_out is not None:
            loss_out[:, loss_offset:loss_offset + rows] = loss
        out = {"loss": loss, "rank": rank, "logits": logits}
        if train:
            out["dl"], out["db"], out["x"] = dl, db, xa
        return out

    # ------------------------------------------------------------------ update
    def update(self, X: torch.Tensor, idx: torch.Tensor, fwd: Dict[str, torch.Tensor]) -> None:
        """Weight gradient of ``fwd`` (a training ``forward`` of the same batch) and one SGD step."""
        rows = self._check_batch(X, idx)
        if not 0 <= self.step < self.ftab.numel():
            raise ValueError(f"step {self.step} outside the schedule table of {self.ftab.numel()}")
        idx = idx.to(device=self.device, dtype=torch.long).contiguous()
        if self.hip:
            from . import _ext
            _ext.ops().probe_update(X, idx, fwd["dlT"], fwd["dbp"], self.W, self.Mw, self.Wsh,
                                    self.b, self.Mb, self.lr0, self.wd, self.ftab, self.step,
                                    self.momentum, self.G, self.C)
            self.step += 1
            return
        G, C, Cp = self.G, self.C, self.Cp
        acc = self.accumulate
        xa = fwd["x"] if "x" in fwd else X[idx].to(acc)
        m = torch.tensor(self.momentum, dtype=torch.float32, device=self.device)
        Wv, Mv = self.W.view(G, Cp, self.Fp), self.Mw.view(G, Cp, self.Fp)
        bv, Mbv = self.b.view(G, Cp), self.Mb.view(G, Cp)
        for g in range(G):
            lr = self.lr0[g] * self.ftab[self.step]  # fp32 product
            dW = (fwd["dl"][g].to(acc).t() @ xa).float()
            for p, buf, grad in ((Wv[g, :C], Mv[g, :C], dW), (bv[g, :C], Mbv[g, :C], fwd["db"][g])):
                gr = grad + self.wd[g] * p
                nb = gr if self.step == 0 else m * buf + gr
                buf.copy_(nb)
                p.copy_(p - lr * (gr + m * nb))
        if self.round_operands:
            self.Wsh.copy_(self.W.to(torch.bfloat16))
        self.step += 1

    def train_step(self, X: torch.Tensor, y: torch.Tensor, idx: torch.Tensor,
                   loss_out: Optional[torch.Tensor] = None, loss_offset: int = 0) -> torch.Tensor:
        """One SGD step of every configuration on the rows ``idx``; returns the [G][rows] losses."""
        fwd = self.forward(X, y, idx, True, loss_out, loss_offset, want_rank=False)
        self.update(X, idx, fwd)
        return fwd["loss"]

    # ------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def evaluate(self, X: torch.Tensor, y: torch.Tensor, top_k: int = 5,
                 chunk: int = MAX_ROWS) -> Tuple[List[float], List[float], List[float]]:
        """Per configuration (mean CE, top-1, top-k accuracy) over all rows of ``X``."""
        n = X.shape[0]
        k = max(1, min(top_k, self.C))
        y = y.to(device=self.device, dtype=torch.long).contiguous()
        acc = torch.zeros(self.G, 3, dtype=torch.float64, device=self.device)
        for s in range(0, n, chunk):
            idx = torch.arange(s, min(n, s + chunk), device=self.device)
            out = self.forward(X, y, idx, train=False)
            acc[:, 0] += out["loss"].double().sum(1)
            acc[:, 1] += (out["rank"] == 0).sum(1)
            acc[:, 2] += (out["rank"] < k).sum(1)
        a = (acc / max(1, n)).cpu().tolist()
        return [r[0] for r in a], [r[1] for r in a], [r[2] for r in a]
