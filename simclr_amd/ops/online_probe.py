"""Online linear probe: one linear classifier trained on the stop-gradient encoder output of every
pre-training step ("linear eval while pre-training"), on the HIP kernels of csrc/probe.hip (the
sweep's forward and weight gradient under the online row policy) on the GPU and as torch ops of the
same contract (the twin) elsewhere.  The twin is the CPU / fp32 path and the tests' oracle.

Contract (both paths):

* input: the encoder output ``h`` of both views, ``[2n][F]``, detached; row ``r`` has the label
  ``y[r mod n]``; ``Cp = 16 · ceil(C / 16)`` and ``F`` is zero-padded to a multiple of ``K_STEP``;
  padding columns take no part in the softmax, get zero gradient and never move;
* forward: ``logits = h · Wshᵀ + b`` with ``h`` rounded once to bf16 (it already is on the HIP
  path), ``Wsh`` a bf16 shadow of the fp32 master, fp32 accumulation, fp32 bias; softmax, CE and
  ``dlogits = (softmax - onehot) / (2n)`` in fp32; per row the loss and the target's rank by
  ``ops.classify.ce_rank``'s rules (ties to the lower class, a NaN target logit is never correct);
* metrics are progressive: this step's rows, on the weights *before* this step's update, are
  added to device accumulators (loss sum fp64; top-1, top-k and row counts int64) in a fixed
  order, no atomics; ``reset_metrics`` zeroes them, ``metrics`` reads them;
* gradient: ``db`` is the fp32 column sum of ``dlogits``, ``dW = bf16(dlogits)ᵀ · h`` with fp32
  accumulation over all ``2n`` rows, both in one flat fp32 buffer ``[Cp · Fp + Cp]``; with a
  data-parallel group that buffer is all-reduced and scaled by ``1 / W``;
* update: ``torch.optim.SGD(nesterov=True)`` in fp32 on weights and bias alike — ``g += wd · p``,
  ``buf = m · buf + g`` (``buf`` starts at zero), ``p -= lr · (g + m · buf)`` — then the shadow
  is refreshed; ``lr`` is the pre-training's warmup + cosine shape (``optim.schedule.lr_at``),
  evaluated on the device by ``lr_step`` on a step counter and an LR cell the probe owns.

No host value that changes per step reaches a launch, so a captured step replays correctly.

Limits of the HIP path: ``C <= 1024``, padded ``F <= 4096``, ``2n % 16 == 0``; anything else takes
the twin.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
import torch.distributed as dist

from ..optim.schedule import MODE_WARMUP_COSINE, lr_at
from . import registry
from .probe_sweep import K_STEP, _ce_twin, padded_classes, padded_features  # noqa: F401

MAX_CLASSES = 1024
MAX_FP = 4096
MAX_ROWS = 8192   # rows of one kernel call (2n)
ROW_TILE = 16     # the HIP path needs 2n % ROW_TILE == 0


def initial_lr(lr: float, batch: int, linear_schedule: bool) -> float:
    """``calculate_initial_lr`` on the probe's own base rate."""
    return lr * batch / 256.0 if linear_schedule else lr * math.sqrt(batch)


def hip_shape_ok(num_classes: int, num_features: int) -> bool:
    return 1 <= num_classes <= MAX_CLASSES and 1 <= padded_features(num_features) <= MAX_FP


class OnlineProbe:
    """State of the probe: flat fp32 master / momentum / gradient (``[Cp · Fp]`` weights then
    ``[Cp]`` bias), the bf16 shadow, the device step counter and LR cell, the metric accumulators.

    ``weight`` [C][F] / ``bias`` [C] are the initialisation.  ``group`` / ``world_size``: the
    data-parallel group whose ranks average the gradient (``comm`` forces the collective on a
    1-rank group).  ``round_operands=False`` and ``accumulate=torch.float64`` exist for the tests;
    both select the twin, as does ``hip=False``."""

    def __init__(self, weight: torch.Tensor, bias: torch.Tensor, lr0: float, decay: float = 0.0,
                 momentum: float = 0.9, top_k: int = 5, warmup_steps: int = 0,
                 total_steps: int = 0, device=None, round_operands: bool = True,
                 accumulate: torch.dtype = torch.float32, hip: Optional[bool] = None,
                 group=None, world_size: int = 1, comm: Optional[bool] = None):
        assert weight.dim() == 2 and bias.dim() == 1 and bias.shape[0] == weight.shape[0]
        dev = torch.device(device) if device is not None else weight.device
        self.device = dev
        self.C, self.F = int(weight.shape[0]), int(weight.shape[1])
        self.Cp, self.Fp = padded_classes(self.C), padded_features(self.F)
        if not lr0 > 0:
            raise ValueError(f"online_probe.lr must be > 0, got lr0 {lr0}")
        if not decay >= 0:
            raise ValueError(f"online_probe.decay must be >= 0, got {decay}")
        if not 0 <= momentum < 1:
            raise ValueError(f"online_probe.momentum must be in [0, 1), got {momentum}")
        if int(top_k) < 1:
            raise ValueError(f"online_probe.top_k must be >= 1, got {top_k}")
        self.lr0, self.decay, self.momentum = float(lr0), float(decay), float(momentum)
        self.top_k = max(1, min(int(top_k), self.C))
        self.warmup, self.total = int(warmup_steps), int(total_steps)
        self.round_operands = bool(round_operands)
        self.accumulate = accumulate
        plain = self.round_operands and accumulate == torch.float32
        if hip is None:
            hip = (plain and dev.type == "cuda" and hip_shape_ok(self.C, self.F)
                   and registry.use_hip(torch.empty(0, device=dev)))
        if hip and not (plain and hip_shape_ok(self.C, self.F)):
            raise ValueError("the HIP path rounds its operands, accumulates in fp32 and needs "
                             f"C <= {MAX_CLASSES}, padded F <= {MAX_FP}")
        self.hip = bool(hip)
        self.group, self.world_size = group, int(world_size)
        self.comm = bool(comm) if comm is not None else self.world_size > 1
        self.gscale = 1.0 / self.world_size
        nw = self.Cp * self.Fp
        self.master = torch.zeros(nw + self.Cp, device=dev, dtype=torch.float32)
        self.W, self.b = self.master[:nw].view(self.Cp, self.Fp), self.master[nw:]
        self.W[:self.C, :self.F] = weight.detach().to(device=dev, dtype=torch.float32)
        self.b[:self.C] = bias.detach().to(device=dev, dtype=torch.float32)
        self.mom = torch.zeros_like(self.master)
        self.grad = torch.zeros_like(self.master)
        self.Wsh = self.W.to(torch.bfloat16) if self.round_operands else self.W
        self.step_t = torch.zeros(1, device=dev, dtype=torch.int64)
        self.lr_t = torch.zeros(1, device=dev, dtype=torch.float32)
        self.acc_loss = torch.zeros(1, device=dev, dtype=torch.float64)
        self.acc_cnt = torch.zeros(3, device=dev, dtype=torch.int64)  # top-1, top-k, rows
        self.host_step = 0
        self.hip_steps = 0  # steps issued on the kernels (tests / accounting)
        self._scratch: Dict[str, torch.Tensor] = {}

    # ------------------------------------------------------------------ accessors
    def weights(self):
        """(W [C][F], b [C]) fp32 master."""
        return self.W[:self.C, :self.F], self.b[:self.C]

    def broadcast_from(self, src: int = 0) -> None:
        """Every rank starts from rank ``src``'s probe (as the model's parameters do)."""
        if self.comm and self.group is not None and self.world_size > 1:
            dist.broadcast(self.master, src=src, group=self.group)
            self._refresh_shadow()

    def _refresh_shadow(self) -> None:
        if self.round_operands:
            self.Wsh.copy_(self.W)

    def _buf(self, name: str, shape, dtype, zero: bool = False) -> torch.Tensor:
        key = f"{name}{tuple(shape)}"
        t = self._scratch.get(key)  # the kernels' scratch: fixed shapes, allocated once
        if t is None:
            make = torch.zeros if zero else torch.empty
            t = self._scratch[key] = make(*shape, device=self.device, dtype=dtype)
        return t

    def _check(self, h: torch.Tensor, y: torch.Tensor) -> int:
        if h.dim() != 2 or h.shape[1] != self.F:
            raise ValueError(f"h must be [2n][{self.F}], got {tuple(h.shape)}")
        if y.dim() != 1 or y.numel() < 1 or h.shape[0] % y.numel() != 0:
            raise ValueError(f"labels must be [n] with the {h.shape[0]} rows of h a multiple of "
                             f"n, got shape {tuple(y.shape)}")
        if y.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"labels must be int32 or int64, not {y.dtype}")
        return h.shape[0]

    # ------------------------------------------------------------------ one step
    @torch.no_grad()
    def step(self, h: torch.Tensor, y: torch.Tensor) -> Dict[str, torch.Tensor]:
        """Forward, metrics, gradient and update on ``h`` [2n][F] with labels ``y`` [n]; returns
        the step's intermediates (the tests read them)."""
        rows = self._check(h, y)
        h = h.detach()
        if self.hip and h.is_cuda and rows % ROW_TILE == 0 and rows <= MAX_ROWS:
            out = self._forward_hip(h, y, rows)
            if self.comm:
                dist.all_reduce(self.grad, group=self.group)
            ops = torch.ops.simclr_amd
            ops.lr_step(self.step_t, self.lr_t, self.lr0, self.warmup, self.total,
                        MODE_WARMUP_COSINE)
            ops.online_probe_update(self.master, self.grad, self.mom, self.Wsh, self.lr_t,
                                    self.decay, self.momentum, self.gscale, self.C, self.F,
                                    self.Fp)
            self.hip_steps += 1
        else:
            out = self._forward_twin(h, y, rows)
            if self.comm:
                dist.all_reduce(self.grad, group=self.group)
            self._update_twin()
        self.host_step += 1
        return out

    def _forward_hip(self, h, y, rows):
        ops = torch.ops.simclr_amd
        C, Cp, Fp = self.C, self.Cp, self.Fp
        Rp = (rows + 31) // 32 * 32
        if h.dtype == torch.bfloat16 and self.F == Fp and h.is_contiguous():
            X = h
        else:  # pad (and round once) into a buffer of the probe's own
            X = self._buf("X", (rows, Fp), torch.bfloat16, zero=True)
            X[:, :self.F].copy_(h)
        y32 = y if y.dtype == torch.int32 else y.to(torch.int32)
        y32 = y32.to(self.device).contiguous()
        Z = self._buf("Z", (rows, Cp), torch.float32)
        loss = self._buf("loss", (rows,), torch.float32)
        rank = self._buf("rank", (rows,), torch.int32)
        dlT = self._buf("dlT", (Cp, Rp), torch.bfloat16)
        dbp = self._buf("dbp", (rows // 16, Cp), torch.float32)
        ops.online_probe_forward(X, y32, self.Wsh, self.b, C, Z, loss, rank, dlT, dbp)
        ops.online_probe_metrics(loss, rank, self.top_k, self.acc_loss, self.acc_cnt)
        ops.online_probe_wgrad(X, dlT, dbp, self.grad, C)
        return {"loss": loss, "rank": rank, "logits": Z[:, :C], "dl": dlT[:C, :rows].t(),
                "dbp": dbp[:, :C], "x": X}

    def _forward_twin(self, h, y, rows):
        C, F = self.C, self.F
        acc = self.accumulate
        x = h.to(self.device)
        x = x.to(torch.bfloat16) if self.round_operands else x.float()
        xa = x.to(acc)
        t = y.to(device=self.device, dtype=torch.long).repeat(rows // y.numel())
        z = (xa @ self.Wsh[:C, :F].to(acc).t()).float() + self.b[:C]
        loss, rank, d = _ce_twin(z, t)
        dl = d.to(torch.bfloat16).float() if self.round_operands else d
        self.acc_loss += loss.double().sum()
        self.acc_cnt += torch.stack([(rank == 0).sum(), (rank < self.top_k).sum(),
                                     torch.tensor(rows, device=self.device)]).to(torch.int64)
        gW = self.grad[:self.Cp * self.Fp].view(self.Cp, self.Fp)
        gW[:C, :F] = (dl.to(acc).t() @ xa).float()
        self.grad[self.Cp * self.Fp:][:C] = d.to(acc).sum(0).float()
        return {"loss": loss, "rank": rank, "logits": z, "dl": dl, "x": x}

    def _update_twin(self):
        C, F = self.C, self.F
        lr = lr_at(MODE_WARMUP_COSINE, self.host_step, self.lr0, self.warmup, self.total)
        self.step_t += 1
        self.lr_t.fill_(lr)  # rounded to fp32, as lr_step's cell
        f32 = dict(dtype=torch.float32, device=self.device)
        m, wd = torch.tensor(self.momentum, **f32), torch.tensor(self.decay, **f32)
        gs = torch.tensor(self.gscale, **f32)
        nw = self.Cp * self.Fp
        for lo, shape, sel in ((0, (self.Cp, self.Fp), (slice(0, C), slice(0, F))),
                               (nw, (self.Cp,), (slice(0, C),))):
            n = math.prod(shape)
            p = self.master[lo:lo + n].view(shape)[sel]
            buf = self.mom[lo:lo + n].view(shape)[sel]
            g = self.grad[lo:lo + n].view(shape)[sel] * gs + wd * p
            nb = m * buf + g
            buf.copy_(nb)
            p.copy_(p - self.lr_t * (g + m * nb))
        self._refresh_shadow()

    # ------------------------------------------------------------------ metrics
    def reset_metrics(self) -> None:
        self.acc_loss.zero_()
        self.acc_cnt.zero_()

    def metrics(self, group=None) -> Dict[str, float]:
        """The accumulators since ``reset_metrics`` (one device read): mean loss, top-1 and top-k
        accuracy, rows.  ``group``: the sums are all-reduced over its ranks first (collective)."""
        loss, cnt = self.acc_loss.clone(), self.acc_cnt.clone()
        if group is not None:
            dist.all_reduce(loss, group=group)
            dist.all_reduce(cnt, group=group)
        ls = float(loss.item())
        top1, topk, rows = (int(v) for v in cnt.tolist())
        d = max(1, rows)
        return {"loss": ls / d, "acc": top1 / d, "top_k_acc": topk / d, "rows": rows,
                "top_k": self.top_k}

    # ------------------------------------------------------------------ checkpoint
    def state_dict(self) -> dict:
        return {"master": self.master.detach().cpu().clone(),
                "momentum": self.mom.detach().cpu().clone(), "step": int(self.host_step)}

    def load_state_dict(self, sd: dict) -> None:
        if tuple(sd["master"].shape) != tuple(self.master.shape):
            raise ValueError(f"online_probe state of {tuple(sd['master'].shape)} does not fit a "
                             f"probe of {tuple(self.master.shape)} (classes / features differ)")
        self.master.copy_(sd["master"].to(self.device))
        self.mom.copy_(sd["momentum"].to(self.device))
        self.host_step = int(sd["step"])
        self.step_t.fill_(self.host_step)
        self._refresh_shadow()


def validate(conf: dict) -> None:
    """``ValueError`` naming the bad ``online_probe`` key."""
    en = conf.get("enabled", False)
    if not isinstance(en, bool):
        raise ValueError("online_probe.enabled must be a boolean")

    def num(key):
        v = conf.get(key)
        return v is None or (isinstance(v, (int, float)) and not isinstance(v, bool))
    for key in ("lr", "decay", "momentum"):
        if not num(key):
            raise ValueError(f"online_probe.{key} must be a number")
    lr, decay, mom, k = conf.get("lr"), conf.get("decay"), conf.get("momentum"), conf.get("top_k")
    if lr is not None and not lr > 0.0:
        raise ValueError("online_probe.lr must be > 0")
    if decay is not None and not decay >= 0.0:
        raise ValueError("online_probe.decay must be >= 0")
    if mom is not None and not 0.0 <= mom < 1.0:
        raise ValueError("online_probe.momentum must be in [0, 1)")
    if k is not None and (not isinstance(k, int) or isinstance(k, bool) or k < 1):
        raise ValueError("online_probe.top_k must be an integer >= 1")
