"""Fused residual-stage executor: the ResNet body (layer1..layer4) as ONE hand-scheduled
forward/backward on the HIP kernels, instead of a chain of per-op autograd nodes.

Reference semantics: torchvision BasicBlock / Bottleneck (v1.5) inside the reference's
``ContrastiveModel.f`` (``/root/reference/model.py:76-114``) with every BatchNorm converted to
SyncBatchNorm (main.py:176) and the two views run as separate forwards (main.py:112-113, so BN
statistics are per view: SURVEY Q17).  The math is unchanged; what changes is where the
BatchNorm work happens:

forward, per block (S = 2 view segments, stats per segment, all-reduced across ranks)::

    a1 = conv1(x)                      epilogue: Σ, Σ² partials of a1        (BN1 stats)
    a2 = conv2(relu(bn1(a1)))          prologue applies BN1+ReLU on the gathered operand, so
                                       the BN1 output is never written to HBM; epilogue: BN2 stats
    a3 = conv3(relu(bn2(a2)))          (bottleneck only) same
    ad = convd(x)                      (downsample) epilogue: BNd stats
    out = relu(bn3(a3) + [bnd(ad) | x])  one elementwise pass (two affines + add + ReLU)

backward, per block, given g = dL/d out::

    BN3 (and BNd) backward reduce/apply with the ReLU mask of ``out`` → da3 (, dad, or the
    identity-path gradient g3 = g·[out > 0])
    db2 = dgrad3(da3): the epilogue applies the BN2-ReLU mask (recomputed from a2) and emits the
          BN2 backward partials Σg, Σg·x̂ (no separate reduce pass) → finalize → da2 (one pass)
    dW3 = wgrad(da3, relu(bn2(a2)))   prologue recomputes the BN2 output on the fly
    ... same for conv2 / BN1 ...
    dx  = dgrad1(da1) + [dgrad_d(dad) | g3]  accumulated in the dgrad epilogue (no extra add)

Compared with the module path this removes the BN1/BN2 apply passes, both backward reduce
passes of BN1/BN2, every autograd gradient-accumulation add at the residual branches, and the
materialised BN outputs (less HBM traffic and memory).  Weight / BN-parameter gradients go
straight into the flat fp32 gradient buffer and notify the bucketed all-reducer as soon as
they are final (overlap with the rest of the backward).
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import List, NamedTuple, Optional, Tuple, Union

import torch
import torch.distributed as dist

from ..ops import _ext
from ..ops.conv_hip import (BlockOut, BnApply, BnBackward, Epilogue, Igemm, StatsOut, WgradDY,
                            WgradX, DgradLaunch, dgrad_plan, fwd_geom, run_wgrad, shadow_ohwi,
                            wt_shape)
from ..parallel import state as pstate
from ..parallel.state import site_key


# attribution experiment (never for training): SIMCLR_SKIP_WGRAD=1 drops the backbone's weight-
# gradient kernels, exposing how much of the step the dgrad / BatchNorm chain alone takes
_SKIP_WGRAD = os.environ.get("SIMCLR_SKIP_WGRAD", "0") == "1"
# attribution experiment: SIMCLR_EXPERIMENT_SKIP_BNREDUCE=fwd|bwd|all drops the BatchNorm
# reduce/finalize launches (garbage statistics): the upper bound of folding them into the convs
_SKIP_BNRED = os.environ.get("SIMCLR_EXPERIMENT_SKIP_BNREDUCE", "")


def _empty_nhwc(n, h, w, c, dev, dtype=torch.bfloat16):
    return torch.empty((n, h, w, c), device=dev, dtype=dtype)


def _allreduce(t: torch.Tensor, st, branch: bool = False) -> None:
    if st.comm:
        g = st.branch_stat_group if branch and st.branch_stat_group is not None else st.stats_group
        dist.all_reduce(t, group=g)


def _stage_of(b: "_BlockSpec") -> int:
    """ResNet stage (1-4) of a block named ``layer<s>.<i>``."""
    return int(b.name[5]) if b.name.startswith("layer") else 0


def _deliver_grad(param: torch.Tensor, compute) -> None:
    """Run ``compute(out)`` writing the fp32 gradient of ``param`` into its flat-store slot
    (and notify the reducer); unbound parameters accumulate into ``param.grad``."""
    slot = getattr(param, "_slot", None)
    if slot is not None:
        compute(slot.grad)
        slot.store.mark_ready(slot.index)
        return
    g = torch.empty(param.shape if param.dim() != 4 else
                    (param.shape[0], param.shape[2], param.shape[3], param.shape[1]),
                    device=param.device, dtype=torch.float32)
    compute(g)
    if param.dim() == 4:
        g = g.permute(0, 3, 1, 2)
    if param.grad is None:
        param.grad = g.contiguous() if param.dim() != 4 else g
    else:
        param.grad.add_(g)


def _out_hw(h: int, k: int, stride: int, pad: int) -> int:
    """Output extent of a k-tap window over ``h`` positions."""
    return (h + 2 * pad - k) // stride + 1


def _nhwc(t: torch.Tensor, bf16: bool = False) -> torch.Tensor:
    """Contiguous [N, H, W, C] view of an NCHW tensor (a channels_last copy if it is not one
    already); ``bf16``: cast first."""
    if bf16 and t.dtype != torch.bfloat16:
        t = t.to(torch.bfloat16)
    tn = t.permute(0, 2, 3, 1)
    if not tn.is_contiguous():
        tn = t.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
    return tn


@dataclass
class _ConvSpec:
    conv: torch.nn.Module
    bn: torch.nn.Module
    stride: int
    k: int
    pad: int

    @classmethod
    def of(cls, conv, bn) -> "_ConvSpec":
        """Kernel, stride and padding as the (square) conv module states them."""
        k, stride, pad = (v[0] if isinstance(v, tuple) else v
                          for v in (conv.kernel_size, conv.stride, conv.padding))
        return cls(conv, bn, stride, k, pad)

    def out_hw(self, h: int) -> int:
        return _out_hw(h, self.k, self.stride, self.pad)


@dataclass
class _BlockSpec:
    convs: List[_ConvSpec]
    down: Optional[_ConvSpec]
    name: str = ""


@dataclass
class _BNState:
    mi: torch.Tensor        # [2][S][C] mean / invstd
    ss: torch.Tensor        # [2][S][C] scale / shift
    count: float


@dataclass
class _BlockTape:
    x: torch.Tensor                     # block input, NHWC bf16
    acts: List[torch.Tensor] = field(default_factory=list)   # pre-BN conv outputs (NHWC)
    bns: List[_BNState] = field(default_factory=list)
    # what conv i actually consumed: (tensor, prologue scale/shift or None)
    ins: List[Tuple[torch.Tensor, Optional[torch.Tensor]]] = field(default_factory=list)
    ad: Optional[torch.Tensor] = None
    bnd: Optional[_BNState] = None
    out: Optional[torch.Tensor] = None
    mask: Optional[torch.Tensor] = None  # uint8 ReLU bitmask of ``out`` (bit per channel)
    # pooled stem only: (window argmax bytes, pre-BN value at the argmax) of the max-pool
    pool: Optional[Tuple[torch.Tensor, torch.Tensor]] = None


class LazyBN(NamedTuple):
    """A BatchNorm backward left to its consumers' operand prologues: dy = coef.A·g +
    coef.B·a + coef.D is computed on the fly and never written to HBM."""
    a: torch.Tensor                     # the BN's input (pre-BN conv output)
    coef: torch.Tensor                  # [3][S][C] (_bn_bwd_finish)


class BlockOutput(NamedTuple):
    """A block output not formed yet: out = relu(bn(aL) + res'), mask = its ReLU bitmask."""
    aL: torch.Tensor                    # the block's last pre-BN activation
    ss: torch.Tensor                    # its BN scale / shift [2][S][C]
    res: torch.Tensor                   # residual: block input, or the downsample's pre-BN output
    rss: Optional[torch.Tensor]         # the downsample BN's scale / shift (None: identity)
    out: torch.Tensor
    mask: torch.Tensor


# The records below keep a leading ``kind`` tag and the field order of the plain tuples they
# name, so a caller may pass either and positional readers (tests' recorders) keep working.

class MaskEpi(NamedTuple):
    """dgrad epilogue of a BN + ReLU producer (mode 3): g = dx·[bn(a_prev) > 0]."""
    kind: str                           # "mask"
    a_prev: torch.Tensor
    bs: _BNState


class ResEpi(NamedTuple):
    """dgrad epilogue of a residual-block producer (mode 4): g = (dx + resid)·[y > 0].
    ``mask``: the ReLU bitmask of its output y, ``a_prev`` / ``mi`` its last pre-BN activation
    and BN mean / invstd; ``resid`` may alias dx.  With ``ad`` / ``mid`` (its downsample's
    pre-BN activation and mean / invstd) the partials of the downsample BN too."""
    kind: str                           # "res"
    resid: torch.Tensor
    mask: torch.Tensor
    a_prev: torch.Tensor
    mi: torch.Tensor
    ad: Optional[torch.Tensor] = None
    mid: Optional[torch.Tensor] = None


class BnBwdLocal(NamedTuple):
    """A started BN backward that one fused launch finishes (single GPU / IPC exchange)."""
    kind: str                           # "local"
    bn: torch.nn.Module
    partial: torch.Tensor
    nblk_seg: int
    bs: _BNState
    ipc: object


class BnBwdDist(NamedTuple):
    """A started BN backward whose local sums are being all-reduced (``work``)."""
    kind: str                           # "dist"
    bn: torch.nn.Module
    sums: torch.Tensor
    work: object
    bs: _BNState


# persistent blocks per view segment of the fused 1x1 backward (2 segments: 2x this many blocks)
_BWD1X1_BPS = 128


def bn_fwd(ops, bn, partial, nblk_seg: int, rows_seg: int, S: int, st, slot: int = 0) -> _BNState:
    """The BatchNorm state of ``bn`` from a conv epilogue's Σ, Σ² partials: one reduce /
    finalize launch.  ``slot``: ticket array of the last-arriver reduce (1 on the downsample
    stream, so a concurrent reduce on the main stream never shares its counters)."""
    C = bn.num_features
    dev = partial.device
    count = float(rows_seg * st.world_size)
    mi = torch.empty((2 * S * C,), device=dev, dtype=torch.float32)
    ss = torch.empty((2 * S * C,), device=dev, dtype=torch.float32)
    ipc = st.ipc
    if _SKIP_BNRED in ("fwd", "all"):
        return _BNState(mi, ss.view(2, S * C), count)
    if not st.comm or ipc is not None:
        # one launch: reduce + finalize (last-arriver); at world > 1 the IPC statistics
        # exchange runs inside it (comm/ipc.py)
        ops.bn_reduce_fused(partial, nblk_seg, S, C, 1, count=count, eps=bn.eps,
                            momentum=bn.momentum, rm=bn.running_mean, rv=bn.running_var,
                            mi=mi, nbt=bn.num_batches_tracked, gamma=bn.weight.detach(),
                            beta=bn.bias.detach(), ss=ss, ticket_slot=slot,
                            **(ipc.kwargs(site_key(bn, "fwd"), S, C) if ipc is not None else {}))
    else:
        stats = torch.empty((2 * S * C,), device=dev, dtype=torch.float32)
        ops.bn_reduce_fused(partial, nblk_seg, S, C, 0, stats=stats, ticket_slot=slot)
        _allreduce(stats, st, branch=slot == 1)
        ops.bn_finalize(stats, S, C, count, bn.eps, bn.momentum, bn.running_mean,
                        bn.running_var, mi, bn.num_batches_tracked,
                        gamma=bn.weight.detach(), beta=bn.bias.detach(), ss=ss)
    return _BNState(mi, ss.view(2, S * C), count)


def deliver_bn_grads(bn, run) -> None:
    """``run(dgamma_out, dbeta_out)`` writes dγ, dβ; route them into the flat store."""
    gslot = getattr(bn.weight, "_slot", None)
    bslot = getattr(bn.bias, "_slot", None)
    if gslot is not None and bslot is not None:
        run(gslot.grad, bslot.grad)
        gslot.store.mark_ready(gslot.index)
        bslot.store.mark_ready(bslot.index)
        return
    C = bn.num_features
    dg = torch.empty((C,), device=bn.weight.device, dtype=torch.float32)
    db = torch.empty((C,), device=bn.weight.device, dtype=torch.float32)
    run(dg, db)
    _deliver_grad(bn.weight, lambda o: o.copy_(dg))
    _deliver_grad(bn.bias, lambda o: o.copy_(db))


def bn_bwd_start(ops, bn, partial, nblk_seg: int, bs: _BNState, S: int, st):
    """Phase 1 of a BN backward from Σg, Σg·x̂ partials.

    Distributed: reduce to the LOCAL [2][S][C] sums, write dγ, dβ from them (SyncBN
    semantics: parameter gradients are per-rank and summed by the data-parallel reducer
    like every other gradient — using the all-reduced sums here would count them W
    times), then start the all-reduce of the sums asynchronously; the caller schedules
    independent work (a weight gradient) before ``bn_bwd_finish``.  Single GPU: nothing
    to wait for (one fused launch in the finish)."""
    C = bn.num_features
    if not st.comm or st.ipc is not None:
        return BnBwdLocal("local", bn, partial, nblk_seg, bs, st.ipc)
    dev = partial.device
    sums = torch.empty((2 * S * C,), device=dev, dtype=torch.float32)
    # one launch: the local sums (all-reduced below) and dγ, dβ from them
    deliver_bn_grads(bn, lambda dg, db: ops.bn_reduce_fused(
        partial, nblk_seg, S, C, 0, stats=sums, dgamma=dg, dbeta=db))
    work = dist.all_reduce(sums, group=st.stats_group, async_op=True)
    return BnBwdDist("dist", bn, sums, work, bs)


def bn_bwd_finish(ops, h: Union[BnBwdLocal, BnBwdDist], S: int) -> torch.Tensor:
    """Phase 2: coef [3][S][C] for the input gradient (from the global sums)."""
    bn, bs = h.bn, h.bs
    C = bn.num_features
    dev = bs.mi.device
    coef = torch.empty((3 * S * C,), device=dev, dtype=torch.float32)
    if _SKIP_BNRED in ("bwd", "all"):
        return coef
    if isinstance(h, BnBwdLocal):
        # single launch; with the IPC exchange dγ, dβ come from the local sums and coef
        # from the global ones (SyncBN semantics, see bn_bwd_start)
        kw = h.ipc.kwargs(site_key(bn, "bwd"), S, C) if h.ipc is not None else {}
        deliver_bn_grads(bn, lambda dg, db: ops.bn_reduce_fused(
            h.partial, h.nblk_seg, S, C, 2, count=bs.count, eps=0.0, momentum=0.0, mi=bs.mi,
            gamma=bn.weight.detach(), dgamma=dg, dbeta=db, coef=coef, **kw))
    else:
        h.work.wait()
        ops.bn_bwd_finalize(h.sums, bs.mi, bn.weight.detach(), S, C, bs.count, None, None,
                            coef)
    return coef


class _OutGrad(NamedTuple):
    """What the backward of a block's output (BN_L + shortcut + ReLU) hands to its convs."""
    g3: torch.Tensor                    # g·[out > 0]
    da: torch.Tensor                    # BN_L's input gradient (not written when ``lazy``)
    lazy: Optional[LazyBN]              # BN_L's backward left to conv L's operand prologues
    dad: Optional[torch.Tensor]         # the downsample BN's input gradient, materialised, or
    ds_dual: Optional[tuple]            # (g3, coefd) for the fused pass that never writes it


class FusedStages:
    """Executor over ``resnet.layer1..layer4`` (modules stay the parameter / state owners).

    The fusion switches are class-level defaults, so an executor made without the constructor
    (tests of the launch helpers) reads the same values; tests and A/B tools flip them on an
    instance.  ``BLOCK_OUT_PROLOGUE`` / ``STEM_FUSED`` are copied at construction."""

    BLOCK_OUT_PROLOGUE = True
    # SIMCLR_FUSED_STEM=0: the stem stays on the per-module path (A/B attribution)
    STEM_FUSED = os.environ.get("SIMCLR_FUSED_STEM", "1") != "0"

    # BN backward of a bottleneck's conv3 inside conv3's dgrad/wgrad operand prologues
    # (only up to 128 input channels: measured net loss or break-even above, r2 log)
    bnb_prologue = True
    _bnb_max_cin = 128
    # BN1's backward in conv1's operand prologues as well: measured +0.85 ms/step (r4 log)
    lazy_bn1 = False
    # expansion convs from this many input channels on read a materialised BN2+ReLU input
    # (_mat_expand)
    mat_expand_min_cin = 128
    # a downsample block's output gradient: BN3's backward in conv3's operand prologues and
    # only the downsample BN's gradient materialised (one-output apply instead of the
    # two-output bn_bwd_apply2) where conv3's backward is the fused 1x1 kernel (layer1.0):
    # -0.12 ms/step (3 of 3 A/B rounds); also on the other prologue-eligible conv3s
    # (layer2.0, register-staged weight gradient) neutral to worse (r4 optimisation log)
    lazy_bn3_ds = True
    _lazy_bn3_ds_dual_only = True
    # a 3x3 stride-1 conv2's output-gradient BatchNorm backward (BN2) in its patch-kernel
    # dgrad prologue, which also stores it for the weight gradient: one pass instead of a
    # bn_bwd_apply pass plus the dgrad's re-read (layer1 / layer2; _patch_bnb_ok)
    patch_bnb = os.environ.get("SIMCLR_PATCH_BNB", "1") != "0"
    # weight gradients on a second stream (forked after each conv's dY is final, joined at
    # the end of the backward): they only feed the flat gradient buffer, so they overlap the
    # dgrad / BatchNorm chain that the next layer's gradient depends on
    wgrad_stream = os.environ.get("SIMCLR_WGRAD_STREAM", "1") != "0"
    # the downsample branch of a stage's first block (forward conv + BN, backward dgrad) on
    # its own stream, concurrent with the main branch until the block output / conv1 dgrad
    branch_stream = os.environ.get("SIMCLR_BRANCH_STREAM", "1") != "0"
    # a stride-2 1x1 downsample's dgrad is kept compact ([N, H/2, W/2, C]: it only reaches
    # the even positions) and added by conv1's dgrad epilogue through the subsampled-residual
    # mode — instead of zero-filling a full-resolution tensor (0.9 GB/step of fills at
    # ResNet-50 CIFAR) and re-reading it whole
    compact_ds = True
    # a block's output (BN3 + shortcut + ReLU) formed inside the next block's conv1 prologue
    # instead of a separate pass that conv1 re-reads, at every stage (the prologue kernels
    # keep their DMA pipelined: 24.06 -> 23.80 ms/step A/B, r2 optimisation log)
    block_out_min_hw = 1
    block_out_prologue = BLOCK_OUT_PROLOGUE
    # a bottleneck's conv3 backward at Ci = 64 / Co = 256 (ResNet-50 layer1) as ONE fused
    # pass (conv.hip conv1x1_bwd_dual): dgrad + BN2 mask / partials + weight gradient, so the
    # 0.5-1 GB output gradient is read once instead of once per pass
    fused_bwd1x1 = True
    # ... and the wide form at Ci = 128 / Co = 512 (ResNet-50 layer2 conv3; conv.hip
    # conv1x1_bwd_dual_w: the Ci slices of a row range share each dY tile through L2), which
    # also takes the forward's materialised BN2+ReLU input (_mat_expand) as its X operand
    fused_bwd1x1_wide = True
    # the narrow fused 1x1 backward (Co 256 / Ci 64) as the 8-wave kernel
    # (conv1x1_bwd_dual_w, 64-row tiles) instead of the 4-wave one: -0.03..-0.08 ms/step,
    # 3 of 3 rounds (r6 log)
    dual8 = True
    # the fused 1x1 backward kernels' weight-gradient slab reduction on the main stream
    # (serial, ~10 µs at the full chip) instead of the weight-gradient stream
    dual_reduce_main = False
    # a stride-1 1x1 downsample of the narrow shape (layer1.0, Co 256 / Ci 64) whose BatchNorm
    # backward is lazy: its dgrad and weight gradient from one pass over g and its pre-BN
    # activation (the plain form of conv1x1_bwd_dual) instead of a BN-apply pass writing
    # its input gradient, a dgrad and a weight gradient each reading it; on the main stream
    # ("main") or the downsample branch stream ("branch")
    fused_ds_dual = True
    ds_dual_stream = "main"
    # ... and layer2.0's stride-2 downsample (Co 512 / Ci 256, dY materialised): measured
    # neutral to +0.06 ms (r6 log), so off by default
    fused_ds_dual_s2 = False
    # persistent blocks per view segment of the fused 1x1 backward kernels (A/B knobs):
    # narrow form / layer1.0 downsample, and the wide form (x 2 Ci slices)
    bwd1x1_bps = _BWD1X1_BPS
    bwd1x1_bps_wide = 64
    # the ImageNet stem (7x7 / stride 2 / pad 3 over the 3 image channels) as a 4x4 / stride-1
    # conv over the 2x2 space-to-depth of the padded image (csrc/eval.hip k_stem_s2d):
    # K 256 instead of 392 gathered columns, 32-byte instead of 16-byte gathers
    stem_s2d = True

    # created on first use: the weight-gradient and downsample-branch streams, the batched
    # dgrad-weight transform of the whole backbone (one launch per backward) and the event of
    # its prefetch, the space-to-depth image of the current step
    _side = _branch = _wt_event = _s2d_cache = _wt_sig = _wt_table = None
    _wt_ready = False
    # the stem conv + BN where the executor can run it, and the ImageNet stem's max-pool (k,
    # stride, pad), fused around (stem_forward / backward): BN + ReLU + max-pool in one pass,
    # the max-pool / ReLU / BN backward in one pass
    stem = _stem_block = stem_pool = None

    def __init__(self, resnet: torch.nn.Module, segments: int = 2):
        from .resnet import BasicBlock, Bottleneck
        self.resnet = resnet
        self.S = segments
        self.calls = 0
        # launch accounting (tests): block outputs formed in a conv1 prologue / as their own pass
        self.dual_launches = 0
        self.out_apply_calls = 0
        self._side_keep: List[torch.Tensor] = []
        self._wt_cache = {}
        self._dual_cache = {}
        self._patch_bnb_cache = {}
        self.block_out_prologue = type(self).BLOCK_OUT_PROLOGUE
        # A/B of the fusion switches above without code edits (tools/envab.sh):
        # SIMCLR_FUSED_ATTRS="attr=value,..." (ints / true / false / strings), applied at
        # construction
        for kv in filter(None, os.environ.get("SIMCLR_FUSED_ATTRS", "").split(",")):
            k, v = kv.split("=", 1)
            if not hasattr(self, k):
                raise ValueError(f"SIMCLR_FUSED_ATTRS: FusedStages has no switch {k!r}")
            if v.lower() in ("true", "false"):
                setattr(self, k, v.lower() == "true")
            else:
                try:
                    setattr(self, k, int(v))
                except ValueError:
                    setattr(self, k, v)
        self.stem_fused = type(self).STEM_FUSED
        from .resnet import _Identity
        from ..ops.pooling import MaxPool2d
        mp = getattr(resnet, "maxpool", None)
        if isinstance(mp, (_Identity, MaxPool2d)):
            self.stem = _ConvSpec.of(resnet.conv1, resnet.bn1)
            self._stem_block = _BlockSpec([self.stem], None, "stem")
            if isinstance(mp, MaxPool2d):
                self.stem_pool = (int(mp.kernel_size), int(mp.stride), int(mp.padding))
        self.blocks: List[_BlockSpec] = []
        for li, layer in enumerate((resnet.layer1, resnet.layer2, resnet.layer3, resnet.layer4)):
            for bi, blk in enumerate(layer):
                if not isinstance(blk, (Bottleneck, BasicBlock)):
                    raise TypeError(f"unsupported block {type(blk).__name__}")
                convs = [_ConvSpec.of(getattr(blk, f"conv{i}"), getattr(blk, f"bn{i}"))
                         for i in range(1, 4 if isinstance(blk, Bottleneck) else 3)]
                down = _ConvSpec.of(*blk.downsample) if blk.downsample is not None else None
                self.blocks.append(_BlockSpec(convs, down, f"layer{li + 1}.{bi}"))

    # ------------------------------------------------------------------ feasibility
    def supported(self, x: torch.Tensor) -> bool:
        """Every fused launch needs view segments aligned to the smallest tile (64 rows)."""
        if x.dtype != torch.bfloat16 or not x.is_cuda or x.dim() != 4:
            return False
        Nb, C, H, W = x.shape
        return self._shape_ok(Nb, H, W)

    def stem_supported(self, img: torch.Tensor) -> bool:
        """The image batch can enter at the stem: a stem conv without max-pool, an input that
        needs no gradient, and stem-output rows per view that tile (256-row BatchNorm-backward
        prologue splits of the stem weight gradient)."""
        if not (self.stem_fused and self.stem is not None):
            return False
        if (img.requires_grad or img.dtype != torch.bfloat16 or not img.is_cuda
                or img.dim() != 4 or img.shape[1] % 8 or img.shape[1] < self.stem.conv.in_channels):
            return False
        Nb, _, H, W = img.shape
        OH, OW = self.stem.out_hw(H), self.stem.out_hw(W)
        if self.stem_pool is not None:
            # the stem weight gradient reads a materialised BN input gradient (no 256-row
            # BN-backward prologue splits); the blocks see the pooled map
            if Nb % self.S or ((Nb // self.S) * OH * OW) % 64 or self.stem.conv.out_channels % 8:
                return False
            return self._shape_ok(Nb, _out_hw(OH, *self.stem_pool), _out_hw(OW, *self.stem_pool))
        if Nb % self.S or ((Nb // self.S) * OH * OW) % 256:
            return False
        return self._shape_ok(Nb, OH, OW)

    def _shape_ok(self, Nb: int, H: int, W: int) -> bool:
        if Nb % self.S or H != W:
            return False
        n = Nb // self.S
        for b in self.blocks:
            hin = H
            for i, cs in enumerate(b.convs):
                oh = cs.out_hw(hin)
                if (n * oh * oh) % 64:
                    return False
                if cs.stride == 2:  # BN-epilogue dgrad: per parity-class segments
                    for r in (0, 1):
                        if (n * ((hin - r + 1) // 2) ** 2) % 64:
                            return False
                hin = oh
            H = hin
        return True

    # ------------------------------------------------------------------ building blocks
    def _conv_bn_fwd(self, ops, xn, cs: _ConvSpec, pro_ss: Optional[torch.Tensor], S: int, st,
                     dual: Optional[BlockOutput] = None, slot: int = 0):
        """a = conv(pro(x)) and the BatchNorm state of ``cs.bn`` over it (statistics partials
        from the conv epilogue, one reduce / finalize launch)."""
        a, partial, nblk = self._conv_fwd(ops, xn, cs, pro_ss, S, dual=dual)
        rows_seg = a.shape[0] * a.shape[1] * a.shape[2] // S
        return a, self._bn_fwd(ops, cs.bn, partial, nblk, rows_seg, S, st, slot=slot)

    def _s2d_ok(self, cs: _ConvSpec, xn: torch.Tensor) -> bool:
        """The stem conv runs in its space-to-depth form (``stem_s2d``)."""
        if not (self.stem_s2d and cs is self.stem and xn.is_cuda):
            return False
        Nb, H, W, C = xn.shape
        return (cs.k == 7 and cs.stride == 2 and cs.pad == 3 and cs.conv.in_channels <= 4
                and C % 4 == 0 and (H + 6) % 2 == 0 and (W + 6) % 2 == 0)

    def _s2d_input(self, ops, xn: torch.Tensor) -> torch.Tensor:
        """[Nb, (H+6)/2, (W+6)/2, 16]: the padded image, 2x2 space-to-depth (kept for the
        weight gradient of the same step)."""
        c = self._s2d_cache
        if c is not None and c[0] is xn:
            return c[1]
        Nb, H, W, _ = xn.shape
        xs = _empty_nhwc(Nb, (H + 6) // 2, (W + 6) // 2, 16, xn.device)
        ops.stem_s2d(xn, self.stem.conv.in_channels, 3, xs)
        self._s2d_cache = (xn, xs)
        return xs

    @staticmethod
    def _s2d_weight(weight: torch.Tensor) -> torch.Tensor:
        """7x7 kernel [Co][Ci<=4][7][7] -> the 4x4 kernel over the space-to-depth input,
        OHWI [Co][4][4][16]: w'[co][bh][bw][(dy * 2 + dx) * 4 + c] = w[co][c][2bh + dy][2bw + dx]
        (zero at 2bh + dy = 7 or 2bw + dx = 7 and for c >= Ci)."""
        w = shadow_ohwi(weight, weight.shape[1])  # [Co][7][7][Ci] bf16
        Co, Ci = w.shape[0], w.shape[-1]
        w8 = torch.nn.functional.pad(w, (0, 4 - Ci, 0, 1, 0, 1))  # [Co][8][8][4]
        return w8.view(Co, 4, 2, 4, 2, 4).permute(0, 1, 3, 2, 4, 5).reshape(Co, 4, 4, 16)

    @staticmethod
    def _s2d_unfold_grad(gs: torch.Tensor, out: torch.Tensor) -> None:
        """Weight gradient of the 4x4 form [Co][4][4][16] -> the 7x7 kernel's, OHWI
        [Co][7][7][Ci] (``out``, fp32)."""
        Co, Ci = out.shape[0], out.numel() // (out.shape[0] * 49)
        g8 = gs.view(Co, 4, 4, 2, 2, 4).permute(0, 1, 3, 2, 4, 5).reshape(Co, 8, 8, 4)
        out.view(Co, 7, 7, Ci).copy_(g8[:, :7, :7, :Ci])

    def _conv_fwd(self, ops, xn, cs: _ConvSpec, pro_ss: Optional[torch.Tensor], S: int,
                  dual: Optional[BlockOutput] = None):
        """a = conv(pro(x)) with BN statistics partials in the epilogue.

        ``dual``: the input is the previous block's output, formed in this conv's prologue from
        that block's last activation ``aL`` and residual ``res`` and written to ``out`` /
        ``mask`` by the same kernel (``xn`` is ``out``).
        Returns (a, partials, blocks per segment); the caller reduces the partials
        (``_bn_fwd``)."""
        Nb, H, W, C = xn.shape
        Co = cs.conv.out_channels
        OH, OW = cs.out_hw(H), cs.out_hw(W)
        a = _empty_nhwc(Nb, OH, OW, Co, xn.device)
        if dual is None and pro_ss is None and self._s2d_ok(cs, xn):
            xn = self._s2d_input(ops, xn)
            w = self._s2d_weight(cs.conv.weight)
            g = fwd_geom(Nb, xn.shape[1], xn.shape[2], 16, OH, OW, 4, 4, 1, 0, Co)
        else:
            w = shadow_ohwi(cs.conv.weight, C)
            g = fwd_geom(Nb, H, W, C, OH, OW, cs.k, cs.k, cs.stride, cs.pad, Co)
        M = Nb * OH * OW
        pro, A = None, xn
        if dual is not None:
            pro = BlockOut(dual.ss[0], dual.ss[1], M // S, dual.res,
                           None if dual.rss is None else dual.rss.view(-1), dual.out, dual.mask)
            A = dual.aL
        elif pro_ss is not None:
            pro = BnApply(pro_ss[0], pro_ss[1], M // S)
        job = Igemm(A, w, a, g, want_stats=True, pro=pro, seg_rows=M // S)
        v = job.choose(ops)
        bm = ops.igemm_variant_bm(v)
        stats = torch.empty(((M // bm) * 2 * Co,), device=xn.device, dtype=torch.float32)
        job.launch(ops, v, StatsOut(stats))
        return a, stats, M // bm // S

    def _dual_ok(self, ops, xn, cs: _ConvSpec, S: int) -> bool:
        """Can ``cs`` (a block's conv1) form its input — the previous block's output — in its
        prologue (1x1 / stride 1 / unpadded, an LDS-DMA tile that fits the doubled staging)?"""
        if not (self.block_out_prologue and xn.is_cuda and cs.k == 1
                and cs.stride == 1 and cs.pad == 0):
            return False
        Nb, H, W, C = xn.shape
        if H < self.block_out_min_hw:
            return False
        key = (Nb, H, W, C, cs.conv.out_channels, S)
        cache = self._memo("_dual_cache")
        if key not in cache:  # host-side admissibility, once per shape
            g = fwd_geom(Nb, H, W, C, H, W, 1, 1, 1, 0, cs.conv.out_channels)
            M = Nb * H * W
            cache[key] = any(ops.igemm_dual_ok(v, g) and (M // S) % ops.igemm_variant_bm(v) == 0
                             for v in range(ops.igemm_nvariants()))
        return cache[key]

    def _bn_fwd(self, ops, bn, partial, nblk_seg: int, rows_seg: int, S: int, st,
                slot: int = 0) -> _BNState:
        return bn_fwd(ops, bn, partial, nblk_seg, rows_seg, S, st, slot)

    # the BatchNorm backward of the module-level functions, as methods: the executor calls
    # these (tests wrap them on the class to see every BatchNorm the executor runs)
    def _bn_bwd_start(self, ops, bn, partial, nblk_seg: int, bs: _BNState, S: int, st):
        return bn_bwd_start(ops, bn, partial, nblk_seg, bs, S, st)

    def _bn_bwd_finish(self, ops, h: Union[BnBwdLocal, BnBwdDist], S: int) -> torch.Tensor:
        return bn_bwd_finish(ops, h, S)

    def _bn_bwd(self, ops, bn, partial, nblk_seg: int, bs: _BNState, S: int, st) -> torch.Tensor:
        return self._bn_bwd_finish(ops, self._bn_bwd_start(ops, bn, partial, nblk_seg, bs, S, st),
                                   S)

    def _memo(self, name: str) -> dict:
        """A per-instance cache of host-side admissibility answers; an executor made without
        the constructor creates it on first use."""
        if name not in vars(self):
            setattr(self, name, {})
        return vars(self)[name]

    def _side_stream(self, dev) -> "torch.cuda.Stream":
        """The weight-gradient stream of ``dev``, created on first use."""
        if self._side is None or self._side.device != dev:
            self._side = torch.cuda.Stream(device=dev)
        return self._side

    def _issue_wgrad(self, cs: _ConvSpec, keep, compute, main: bool = False) -> None:
        """Deliver the weight gradient of ``cs`` (``compute(out)`` writes it) on the
        weight-gradient stream, forked here — or in line.  ``keep``: what ``compute`` reads,
        referenced until the join (the caching allocator must not hand that memory to a
        main-stream allocation while the side stream still reads it)."""
        if _SKIP_WGRAD:  # attribution experiment only: the step without weight gradients
            compute = lambda out: None  # noqa: E731
        side = self._side if self.wgrad_stream and not main else None
        if side is None:
            _deliver_grad(cs.conv.weight, compute)
            return
        self._side_keep.extend(keep)
        side.wait_stream(torch.cuda.current_stream(keep[0].device))
        with torch.cuda.stream(side):
            _deliver_grad(cs.conv.weight, compute)

    def _reduce_slabs(self, ops, cs: _ConvSpec, wpart: torch.Tensor, nslab: int) -> None:
        """The weight gradient of ``cs`` from the per-block slabs of a fused 1x1 backward."""
        self._issue_wgrad(cs, (wpart,), lambda out: ops.wgrad_reduce_slabs(wpart, nslab, out),
                          main=self.dual_reduce_main)

    def _wgrad(self, ops, dyn, xn, cs: _ConvSpec, pro_ss: Optional[torch.Tensor], S: int,
               bnb: Optional[LazyBN] = None, main: bool = False):
        """``bnb``: dy = coef.A·dyn + coef.B·a + coef.D, the BatchNorm backward of the conv's
        own BN, computed in the dY operand's prologue (never written to HBM)."""
        Nb, H, W, C = xn.shape
        Co = cs.conv.out_channels
        OH, OW = dyn.shape[1], dyn.shape[2]
        s2d = pro_ss is None and self._s2d_ok(cs, xn)
        if s2d:
            xn = self._s2d_input(ops, xn)
            g = fwd_geom(Nb, xn.shape[1], xn.shape[2], 16, OH, OW, 4, 4, 1, 0, Co)
        else:
            g = fwd_geom(Nb, H, W, C, OH, OW, cs.k, cs.k, cs.stride, cs.pad, Co)
        M = Nb * OH * OW
        pro = WgradX(pro_ss[0], pro_ss[1], M // S, True, S) if pro_ss is not None else None
        dpro = WgradDY(*bnb, M // S, S) if bnb is not None else None

        concurrent = bool(self.wgrad_stream) and self._side is not None and not main

        def compute(out):
            if s2d:  # the 4x4 form's gradient, folded back onto the 7x7 kernel
                gs = torch.empty((Co, 4, 4, 16), device=dyn.device, dtype=torch.float32)
                run_wgrad(ops, dyn, xn, gs, g, 16, pro=pro, dpro=dpro, concurrent=concurrent)
                self._s2d_unfold_grad(gs, out)
            else:  # creal: the stem's 3 image channels are gathered as 8 (zero-padded)
                run_wgrad(ops, dyn, xn, out, g, cs.conv.in_channels, pro=pro, dpro=dpro,
                          concurrent=concurrent)

        self._issue_wgrad(cs, [t for t in (dyn, xn, pro_ss, *(bnb or ())) if t is not None],
                          compute, main)

    @staticmethod
    def _bwd1x1_bps(rows_seg: int, cap: int = _BWD1X1_BPS) -> int:
        """Persistent blocks per view segment of conv1x1_bwd_dual (64-row tiles, equal shares)."""
        tiles = rows_seg // 64
        b = min(cap, tiles)
        while b > 1 and tiles % b:
            b -= 1
        return b

    def _bwd1x1_ok(self, cs: _ConvSpec, dyn: torch.Tensor, xin: torch.Tensor, pro_ss, a_prev,
                   S: int) -> bool:
        M = dyn.numel() // dyn.shape[-1]
        if not (self.fused_bwd1x1 and cs.k == 1 and cs.stride == 1
                and M % S == 0 and (M // S) % 64 == 0):
            return False
        co, ci = cs.conv.out_channels, cs.conv.in_channels
        if (co, ci) == (256, 64):
            return xin is a_prev and pro_ss is not None and M * 256 * 2 < (1 << 31)
        if (co, ci) == (512, 128) and self.fused_bwd1x1_wide:
            # X: a2 with the BN2 prologue, or the forward's materialised relu(bn2(a2))
            return ((xin is a_prev and pro_ss is not None)
                    or (pro_ss is None and xin.shape == a_prev.shape)) and M * 512 * 2 < (1 << 31)
        return False

    def _bwd1x1_fused(self, ops, dyn, bnb, cs: _ConvSpec, a_prev, bs_prev: _BNState, S: int,
                      xin: Optional[torch.Tensor] = None):
        """conv3 dgrad (mode-3 epilogue of BN2) + weight gradient in one launch; the weight
        gradient's split reduction runs on the side stream.  Returns (gm, partials, blocks per
        segment) like ``_dgrad`` with a ``MaskEpi``.  ``xin``: the conv's forward
        input when it was materialised (relu(bn2(a2)); wide form only)."""
        Nb, H, W, Ci = a_prev.shape
        Co = cs.conv.out_channels
        M = Nb * H * W
        wide = (Co, Ci) == (512, 128)
        # the wide kernel launches 2 blocks (Ci slices) per row block: 64 row blocks per view
        # segment fill the chip's 256 CUs once at S = 2
        bps = self._bwd1x1_bps(M // S, self.bwd1x1_bps_wide if wide else self.bwd1x1_bps)
        xraw = xin if (wide and xin is not None and xin is not a_prev) else None
        wt = self._dgrad_weight1x1(ops, cs, a_prev.shape, H, W)
        dev = dyn.device
        gm = _empty_nhwc(Nb, H, W, Ci, dev)
        stats = torch.empty((S * bps * 2 * Ci,), device=dev, dtype=torch.float32)
        wpart = torch.empty((S * bps * Co * Ci,), device=dev, dtype=torch.float32)
        a3, coef = bnb if bnb is not None else (None, None)
        if xraw is not None:  # X = the materialised relu(bn2(a2)); a2 for the epilogue
            ops.conv1x1_bwd_dual(dyn, a3, coef, xraw, bs_prev.ss.view(-1), bs_prev.mi.view(-1),
                                 wt, gm, stats, wpart, S, bps, a_prev)
        else:
            ops.conv1x1_bwd_dual(dyn, a3, coef, a_prev, bs_prev.ss.view(-1),
                                 bs_prev.mi.view(-1), wt, gm, stats, wpart, S, bps,
                                 dual8=bool(self.dual8))
        self._reduce_slabs(ops, cs, wpart, S * bps)
        return gm, stats, bps

    def _ds_dual_ok(self, b: _BlockSpec, tp: _BlockTape, S: int) -> bool:
        """A 1x1 downsample whose input needs no transform (the block input): stride 1 at the
        narrow dual shape (Co 256 / Ci 64, lazy BN backward), or stride 2 at Co 512 / Ci 256
        (layer2.0; dY materialised: ``_ds_dual_s2``)."""
        cs = b.down
        if not (self.fused_ds_dual and self.fused_bwd1x1 and tp.x.is_cuda and cs.k == 1
                and cs.pad == 0 and b.convs[0].stride == 1):
            return False
        Nb, H, W, Ci = tp.x.shape
        shape = (cs.conv.out_channels, cs.conv.in_channels)
        if cs.stride == 1:
            M = Nb * H * W
            return (shape == (256, 64) and Ci == 64 and M % S == 0 and (M // S) % 64 == 0
                    and M * 256 * 2 < (1 << 31))
        if cs.stride == 2 and self.fused_ds_dual_s2:
            Mo = Nb * cs.out_hw(H) * cs.out_hw(W)
            return (shape == (512, 256) and Ci == 256 and Nb % S == 0 and (Mo // S) % 64 == 0
                    and Mo * 512 * 2 < (1 << 31) and tp.x.numel() * 2 < (1 << 31))
        return False

    def _ds_dual(self, ops, b: _BlockSpec, tp: _BlockTape, lazy_d, S: int) -> torch.Tensor:
        """The downsample's input gradient (the residual of conv1's dgrad) and weight gradient
        from one pass over g3 and the pre-BN activation ad, the downsample BN's backward applied
        in registers (conv1x1_bwd_dual, plain form).  The weight gradient's split reduction runs
        on the weight-gradient stream."""
        cs = b.down
        g3, coefd = lazy_d
        Nb, H, W, Ci = tp.x.shape
        Co = cs.conv.out_channels
        dev = g3.device
        _ext.TAG = f"{b.name} ds dgrad+wgrad"
        s2 = cs.stride == 2
        OH, OW = cs.out_hw(H), cs.out_hw(W)
        if s2:
            # layer2.0: dY materialised (the lazy form of the wide kernel spills), then ONE pass
            # for the compact input gradient and the weight gradient (strided X)
            dad = torch.empty_like(tp.ad)
            ops.bn_bwd_apply(g3, None, tp.ad, coefd, S, False, dad, None)
        bps = self._bwd1x1_bps(Nb * OH * OW // S, 32 if s2 else self.bwd1x1_bps)
        wt = self._dgrad_weight1x1(ops, cs, tp.x.shape, OH, OW, compact=s2)
        resid = _empty_nhwc(Nb, OH, OW, Ci, dev)
        wpart = torch.empty((S * bps * Co * Ci,), device=dev, dtype=torch.float32)
        if s2:
            ops.conv1x1_bwd_dual_s2(dad, None, None, tp.x, wt, resid, wpart, S, bps)
        else:
            nostats = torch.empty((1,), device=dev, dtype=torch.float32)
            ops.conv1x1_bwd_dual(g3, tp.ad, coefd, tp.x, None, None, wt, resid, nostats, wpart,
                                 S, bps, dual8=bool(self.dual8))
        self._reduce_slabs(ops, cs, wpart, S * bps)
        return resid

    def _bnb_ok(self, cs: _ConvSpec, a: torch.Tensor, S: int) -> bool:
        """The BN-backward operand prologue applies to a 1x1 stride-1 conv whose per-segment
        rows tile evenly (64-row wgrad splits, 64..256-row dgrad tiles), and pays off only
        while each dy element is loaded about once: the dgrad re-reads its A operand per
        output-channel tile and the wgrad its dY operand per input-channel tile, so with
        ≥ 256 input channels the repeated prologue work outweighs the saved HBM pass
        (measured on layer3/layer4 of ResNet-50: net loss or break-even)."""
        M = a.numel() // a.shape[-1]
        return (self.bnb_prologue and cs.k == 1 and cs.stride == 1 and M % S == 0
                and (M // S) % 256 == 0 and cs.conv.in_channels <= self._bnb_max_cin)

    def _mat_expand(self, cs: _ConvSpec) -> bool:
        """A bottleneck's expansion 1x1 conv (conv3, Co = 4 Ci) takes its input BN2+ReLU as a
        materialised tensor instead of in its operand prologue from ``mat_expand_min_cin`` input
        channels on: the short-K GEMM re-reads and re-transforms its A tile once per output
        column tile (34-46 % of its roofline, r4 per-op table), and the backward's weight gradient
        then reads the stored input with the LDS-DMA tiles instead of an X-operand prologue.
        Below that (layer1, Ci = 64) conv3's backward is the fused 1x1 kernel, which applies
        BN2 itself.  -0.3 ms/step (r4 optimisation log)."""
        cin, cout = cs.conv.in_channels, cs.conv.out_channels
        return cs.k == 1 and cout >= 4 * cin and cin >= self.mat_expand_min_cin

    def _lazy_bn3_ds_ok(self, b: _BlockSpec, tp: _BlockTape, aL: torch.Tensor, S: int) -> bool:
        L = len(b.convs) - 1
        if not (self.lazy_bn3_ds and L > 0 and self._bnb_ok(b.convs[L], aL, S)):
            return False
        if not self._lazy_bn3_ds_dual_only:
            return True
        xin, pro_ss = tp.ins[L]
        return self._bwd1x1_ok(b.convs[L], aL, xin, pro_ss, tp.acts[L - 1], S)

    def _patch_bnb_ok(self, ops, cs: _ConvSpec, a: torch.Tensor, S: int) -> bool:
        """Can conv ``cs`` (output ``a``) take its output gradient's BatchNorm backward in the
        dgrad prologue of the LDS-resident-patch kernel (3x3 / stride 1 / pad 1, the second
        operand fits the kernel's register stage) and store it for the weight gradient?"""
        if not (self.patch_bnb and a.is_cuda and cs.k == 3 and cs.stride == 1 and cs.pad == 1):
            return False
        Nb, H, W, C = a.shape
        M = Nb * H * W
        if M % S or (M // S) % 256:
            return False
        Ci = cs.conv.in_channels
        key = (Nb, H, W, C, Ci)
        cache = self._memo("_patch_bnb_cache")
        if key not in cache:
            g = dgrad_plan(Nb, H, W, Ci, H, W, C, 3, 1, 1).launches[0].geom
            cache[key] = any(ops.igemm_variant_patch(v) and ops.igemm_variant_ok(v, g, True, True)
                             for v in range(ops.igemm_nvariants()))
        return cache[key]

    def _lazy_bn1_ok(self, b: _BlockSpec, a1: torch.Tensor, S: int) -> bool:
        """BN1's backward applied in conv1's dgrad / weight-gradient operand prologues instead
        of a materialising pass (a bottleneck's 1x1 stride-1 conv1)."""
        cs0 = b.convs[0]
        M = a1.numel() // a1.shape[-1]
        return (self.lazy_bn1 and cs0.k == 1 and cs0.stride == 1
                and M % S == 0 and (M // S) % 256 == 0)

    def _dgrad(self, ops, dyn, cs: _ConvSpec, in_shape, S: int, accumulate: bool = False,
               dx: Optional[torch.Tensor] = None,
               bn_epi: Union[None, MaskEpi, ResEpi] = None, bnb: Optional[LazyBN] = None,
               compact: bool = False, sub_resid: bool = False,
               bnb_out: Optional[torch.Tensor] = None):
        """dx (NHWC) = conv-transpose(dy).  ``accumulate``: dx += result (dx must be given).

        ``bn_epi`` (``MaskEpi`` / ``ResEpi``) selects a BatchNorm-backward epilogue that also
        returns Σg, Σg·x̂ partials (segment-major across stride-2 parity classes) → (dx,
        partial, blocks_per_segment); a ``ResEpi`` with ``ad`` → (p3, pd), the partials of the
        producer's downsample BN too.
        ``bnb`` (1x1 stride-1; 3x3 stride-1 on the patch kernel with ``bnb_out``): the A operand
        is the BatchNorm backward coef.A·dyn + coef.B·a + coef.D computed in the prologue;
        ``bnb_out`` receives that operand (the weight gradient's dY).
        ``compact`` (stride-2 1x1, pad 0): return the dgrad only at the even input positions, as
        a dense [N, ceil(H/2), ceil(W/2), Ci] tensor (one stride-1 GEMM, no zero fill).
        ``sub_resid``: the residual (``dx`` with ``accumulate``, or bn_epi's resid) is such a
        compact tensor; the epilogue adds it at the even positions and dx is a new tensor.
        """
        Nb, H, W, Ci = in_shape
        _, OH, OW, Co = dyn.shape
        dev = dyn.device
        if bn_epi is not None:  # (a plain tuple of either layout is taken too)
            bn_epi = (MaskEpi if bn_epi[0] == "mask" else ResEpi)._make(bn_epi)
        w = shadow_ohwi(cs.conv.weight, Ci)
        plan = dgrad_plan(Nb, H, W, Ci, OH, OW, Co, cs.k, cs.stride, cs.pad, compact)
        launches = [(self._dgrad_weight(ops, cs, w, ln), ln) for ln in plan.launches]
        if compact:
            assert bn_epi is None and not accumulate
            dc = _empty_nhwc(Nb, OH, OW, Ci, dev)
            (wt, ln), = launches
            job = Igemm(dyn, wt, dc, ln.geom)
            job.launch(ops, job.choose(ops))
            return dc, None, 0
        resid_c = None
        if sub_resid:
            assert cs.stride == 1 and (accumulate or bn_epi is not None)
            resid_c = dx if bn_epi is None else bn_epi.resid
            dx = None  # the full-resolution result is a new tensor
        if dx is None:
            dx = _empty_nhwc(Nb, H, W, Ci, dev)
        if plan.zero_fill:
            assert bn_epi is None, "BN-epilogue dgrad needs every output position covered"
            if not accumulate:
                dx.zero_()
        if bn_epi is None:
            epi = Epilogue(1, dx) if accumulate else None
            if resid_c is not None:
                epi = Epilogue(1, resid_c, sub=True)
            for wt, ln in launches:
                job = Igemm(dyn, wt, dx, ln.geom, epi=epi)
                job.launch(ops, job.choose(ops))
            return dx, None, 0
        assert not accumulate
        if bn_epi.kind == "mask":
            bs = bn_epi.bs
            epi = Epilogue(3, b=bn_epi.a_prev, ss=bs.ss.view(-1), mi=bs.mi)
        else:
            epi = Epilogue(4, bn_epi.resid, c=bn_epi.a_prev, mask=bn_epi.mask,
                           sub=resid_c is not None, mi=bn_epi.mi, c2=bn_epi.ad, mi2=bn_epi.mid)
        bpro = None
        if bnb is not None:
            assert cs.stride == 1 and len(launches) == 1 and (cs.k == 1 or bnb_out is not None)
            a_b, coef_b = bnb
            bpro = BnBackward.of(coef_b, S * Co, launches[0][1].M // S, a_b, bnb_out)
        chosen = []
        for wt, ln in launches:
            job = Igemm(dyn, wt, dx, ln.geom, want_stats=True, pro=bpro, epi=epi,
                        seg_rows=ln.M // S)
            v = job.choose(ops)
            chosen.append((job, v, job.seg_rows // ops.igemm_variant_bm(v)))
        seg_blocks = sum(nb for _, _, nb in chosen)
        partial = torch.empty((S * seg_blocks * 2 * Ci,), device=dev, dtype=torch.float32)
        partial2 = torch.empty_like(partial) if epi.c2 is not None else None
        base = 0
        for job, v, nb in chosen:
            job.launch(ops, v, StatsOut(partial, seg_blocks, base, partial2))
            base += nb
        if partial2 is not None:
            return dx, (partial, partial2), seg_blocks
        return dx, partial, seg_blocks

    # ------------------------------------------------------------------ dgrad weights
    @staticmethod
    def _wt_params(cs: _ConvSpec):
        """[(parity class, weight_transform params)] of a conv's dgrad: the (key, wt) projection
        of its plan (``conv_hip.dgrad_plan``).  The parameters depend on the conv alone, not on
        the image: any extent with all four parity classes (2 x 2 on) gives them."""
        conv = cs.conv
        OH = cs.out_hw(2)
        plan = dgrad_plan(1, 2, 2, conv.in_channels, OH, OH, conv.out_channels, cs.k, cs.stride,
                          cs.pad)
        return [(ln.key, ln.wt) for ln in plan.launches]

    def prepare_backward(self, ops) -> None:
        """Transform every conv's dgrad weights in ONE launch (weights change only at the
        optimizer step).  Needs flat-store-bound bf16 shadows (stable addresses); the plan is
        built eagerly once and rebuilt if the shadows move — never during graph capture."""
        convs = [cs for b in self.blocks for cs in (b.convs + ([b.down] if b.down else []))]
        shadows = []
        for cs in convs:
            slot = getattr(cs.conv.weight, "_slot", None)
            if slot is None or slot.shadow is None:
                self._wt_ready = False
                return
            shadows.append(slot.shadow)
        sig = tuple(t.data_ptr() for t in shadows)
        if sig != self._wt_sig:
            if torch.cuda.is_current_stream_capturing():
                self._wt_ready = False
                return
            Ws, Wts, params, cache = [], [], [], {}
            for cs, w in zip(convs, shadows):
                for key, p in self._wt_params(cs):
                    wt = torch.empty(wt_shape(p), device=w.device, dtype=torch.bfloat16)
                    Ws.append(w)
                    Wts.append(wt)
                    params.extend(p)
                    cache[(id(cs.conv), key)] = wt
            plan = ops.weight_transform_plan(Ws, Wts, params)
            self._wt_table = (plan[:-1].to(shadows[0].device), int(plan[-1]), Ws)
            self._wt_cache = cache
            self._wt_sig = sig
        ops.weight_transform_batch(self._wt_table[0], self._wt_table[1])
        self._wt_ready = True

    def _prefetch_dgrad_weights(self, ops, xn: torch.Tensor) -> None:
        """The batched dgrad-weight transform (prepare_backward) depends only on the weights, which
        are final once the previous optimizer step ran: issue it on the (idle during the forward)
        weight-gradient stream at the start of the forward, so it is off the critical path of
        the backward, which waits on its event."""
        self._wt_event = None
        if not (self.wgrad_stream and xn.is_cuda):
            return
        side = self._side_stream(xn.device)
        side.wait_stream(torch.cuda.current_stream(xn.device))
        with torch.cuda.stream(side):
            self.prepare_backward(ops)
        if self._wt_ready:
            ev = torch.cuda.Event()
            ev.record(side)
            self._wt_event = ev

    def _dgrad_weight(self, ops, cs: _ConvSpec, w, ln: DgradLaunch):
        """The transformed weight of one dgrad launch: from the batched transform
        (prepare_backward) when it ran, else transformed here."""
        shape = ln.wt_shape
        if self._wt_ready:
            wt = self._wt_cache.get((id(cs.conv), ln.key))
            if wt is not None and wt.shape[0] == shape[0]:
                return wt
        wt = torch.empty(shape, device=w.device, dtype=torch.bfloat16)
        ops.weight_transform(w, wt, ln.wt)
        return wt

    def _dgrad_weight1x1(self, ops, cs: _ConvSpec, in_shape, OH: int, OW: int,
                         compact: bool = False):
        """The transformed weight of a 1x1 conv's dgrad (its first / only launch)."""
        Nb, H, W, Ci = in_shape
        plan = dgrad_plan(Nb, H, W, Ci, OH, OW, cs.conv.out_channels, 1, cs.stride, 0, compact)
        return self._dgrad_weight(ops, cs, shadow_ohwi(cs.conv.weight, Ci), plan.launches[0])

    # ------------------------------------------------------------------ forward / backward
    def forward(self, xn: torch.Tensor) -> Tuple[torch.Tensor, List[_BlockTape]]:
        ops = _ext.ops()
        st = pstate.get()
        S = self.S
        self.calls += 1
        tapes: List[_BlockTape] = []
        x = xn
        self._prefetch_dgrad_weights(ops, xn)
        br = self._branch_stream(xn)
        pend = None  # the previous block's output, not yet formed (BlockOutput)
        for b in self.blocks:
            tp = _BlockTape(x=x)
            pro_ss = None
            cur = x
            dual = None
            if pend is not None:
                if self._dual_ok(ops, x, b.convs[0], S):
                    dual = pend  # formed (and written to x) by this block's conv1 prologue
                else:
                    self._out_apply(ops, pend, S)
                pend = None
            forked = False

            def fork_down():
                # the downsample conv + BN only meet the main branch at the block output; their
                # statistics all-reduce uses its own communicator (no ordering with the main's)
                br.wait_stream(torch.cuda.current_stream(x.device))
                with torch.cuda.stream(br):
                    self._down_fwd(ops, b, tp, x, S, st, slot=1)

            if b.down is not None and br is not None and dual is None:
                fork_down()
                forked = True
            for ci_, cs in enumerate(b.convs):
                _ext.TAG = f"{b.name} conv{ci_ + 1} fwd"
                if pro_ss is not None and (cs.k > 1 or self._mat_expand(cs)):
                    # a k x k conv re-gathers every input pixel k² times: applying BN+ReLU in
                    # its prologue costs more VALU work than one materialising pass (measured,
                    # also for the LDS-resident patch kernels: r3 optimisation log); likewise
                    # the short-K expansion convs (_mat_expand)
                    bmat = torch.empty_like(cur)
                    ops.bn_apply_ss(cur, pro_ss, None, None, bmat, S, True)
                    cur, pro_ss = bmat, None
                tp.ins.append((cur, pro_ss))
                if ci_ == 0 and dual is not None:
                    a, bs = self._conv_bn_fwd(ops, cur, cs, None, S, st, dual=dual)
                    self.dual_launches += 1
                    if b.down is not None and br is not None:
                        fork_down()  # after the launch that writes its input x
                        forked = True
                else:
                    a, bs = self._conv_bn_fwd(ops, cur, cs, pro_ss, S, st)
                tp.acts.append(a)
                tp.bns.append(bs)
                cur, pro_ss = a, bs.ss
            aL, bsL = tp.acts[-1], tp.bns[-1]
            out = torch.empty_like(aL)
            # the next block's input-gradient epilogue only needs [out > 0]: 1 bit per element
            mask = torch.empty((aL.numel() // 8,), device=aL.device, dtype=torch.uint8)
            _ext.TAG = f"{b.name} ds fwd"
            if b.down is not None:
                if forked:
                    torch.cuda.current_stream(x.device).wait_stream(br)  # join
                else:
                    self._down_fwd(ops, b, tp, x, S, st)
                pend = BlockOutput(aL, bsL.ss, tp.ad, tp.bnd.ss, out, mask)
            else:
                pend = BlockOutput(aL, bsL.ss, x, None, out, mask)
            tp.out = out
            tp.mask = mask
            tapes.append(tp)
            x = out
        if pend is not None:
            self._out_apply(ops, pend, S)
        _ext.TAG = ""
        return x, tapes

    def stem_forward(self, img: torch.Tensor):
        """Stem conv (statistics epilogue) → BatchNorm finalize → BN + ReLU apply with the
        ReLU bitmask (the stem is the producer of layer1.0 like one block of another), then the
        blocks.  Returns (output, tapes, stem tape)."""
        ops = _ext.ops()
        st = pstate.get()
        S = self.S
        cs = self.stem
        _ext.TAG = "stem fwd"
        a, bs = self._conv_bn_fwd(ops, img, cs, None, S, st)
        if self.stem_pool is not None:
            # maxpool(relu(bn(a))) in one pass; the full-resolution BN output is never written
            K, Sd, P = self.stem_pool
            Nb, OH, OW, C = a.shape
            x0 = _empty_nhwc(Nb, _out_hw(OH, K, Sd, P), _out_hw(OW, K, Sd, P), C, a.device)
            arg = torch.empty(x0.shape, device=a.device, dtype=torch.uint8)
            asel = torch.empty_like(x0)
            _ext.TAG = "stem bn+relu+maxpool"
            ops.bn_relu_maxpool(a, bs.ss.view(-1), S, x0, arg, asel, K, Sd, P)
            tp = _BlockTape(x=img, acts=[a], bns=[bs], out=x0, pool=(arg, asel))
        else:
            x0 = torch.empty_like(a)
            mask = torch.empty((a.numel() // 8,), device=a.device, dtype=torch.uint8)
            ops.bn_apply_ss(a, bs.ss, None, None, x0, S, True, mask)
            tp = _BlockTape(x=img, acts=[a], bns=[bs], out=x0, mask=mask)
        out, tapes = self.forward(x0)
        return out, tapes, tp

    def _out_apply(self, ops, pend: BlockOutput, S: int) -> None:
        """Block output = relu(bn3(aL) + shortcut) and its ReLU bitmask, as its own pass."""
        self.out_apply_calls += 1
        ops.bn_apply_ss(pend.aL, pend.ss, pend.res, pend.rss, pend.out, S, True, pend.mask)

    def _branch_stream(self, t: torch.Tensor):
        if not (self.branch_stream and t.is_cuda):
            return None
        if self._branch is None or self._branch.device != t.device:
            self._branch = torch.cuda.Stream(device=t.device)
        return self._branch

    def _down_fwd(self, ops, b: _BlockSpec, tp: _BlockTape, x, S: int, st, slot: int = 0):
        tp.ad, tp.bnd = self._conv_bn_fwd(ops, x, b.down, None, S, st, slot=slot)

    def backward(self, gout: torch.Tensor, tapes: List[_BlockTape],
                 stem_tape: Optional[_BlockTape] = None) -> Optional[torch.Tensor]:
        """Gradient w.r.t. the executor input, or None with ``stem_tape`` (the stem's
        parameter gradients are delivered and the image needs none)."""
        ops = _ext.ops()
        st = pstate.get()
        S = self.S
        if self._wt_event is not None and self._wt_ready:
            # transposed during the forward
            torch.cuda.current_stream(gout.device).wait_event(self._wt_event)
        else:
            self.prepare_backward(ops)
        self._wt_event = None
        main = None
        if self.wgrad_stream and gout.is_cuda:
            main = torch.cuda.current_stream(gout.device)
            side = self._side_stream(gout.device)
            store = self._flat_store()
            if store is not None:
                store.producer_streams = [main, side]
        g, pre = gout, None
        pooled = stem_tape is not None and stem_tape.pool is not None
        # a pooled stem is not a block-boundary producer (the max-pool sits between its BN and
        # layer1.0): layer1.0 returns the raw gradient of the pooled map
        stem_prev = (self._stem_block, stem_tape) if (stem_tape is not None and not pooled) \
            else None
        hook = self.resnet.stage_grads_ready if main is not None else None
        for idx in range(len(self.blocks) - 1, -1, -1):
            prev = (self.blocks[idx - 1], tapes[idx - 1]) if idx > 0 else stem_prev
            g, pre = self._block_backward(ops, st, S, self.blocks[idx], tapes[idx], g, pre, prev)
            stage = _stage_of(self.blocks[idx])
            if hook is not None and stage >= 2 and _stage_of(self.blocks[idx - 1]) != stage:
                # the stage's first block is done: every weight gradient of the stage is queued
                # on the side stream and every BN parameter gradient written on this one (its
                # last BN backward finished at the start of this block): its optimizer update
                # can run beside the rest of the backward instead of in the step's tail
                self._side.wait_stream(main)
                with torch.cuda.stream(self._side):
                    hook(stage)
        if pooled:
            # g = dL/d(pooled map).  BatchNorm partials from pooled-size tensors (g is zero off
            # the window argmaxes; relu'(y[argmax]) = [pooled > 0]), then ONE full-resolution
            # pass: max-pool backward + ReLU mask + BN input gradient (k_maxpool_bwd_bn)
            _ext.TAG = "stem bwd"
            arg, asel = stem_tape.pool
            a0, bs0, x0 = stem_tape.acts[0], stem_tape.bns[0], stem_tape.out
            C = a0.shape[-1]
            nblk = ops.bn_blocks(x0.numel() // C, C, S)
            partial = torch.empty((S * nblk * 2 * C,), device=a0.device, dtype=torch.float32)
            ops.bn_bwd_reduce(g, x0, asel, bs0.mi, S, True, partial)
            coef = self._bn_bwd(ops, self.stem.bn, partial, nblk, bs0, S, st)
            da = torch.empty_like(a0)
            K, Sd, P = self.stem_pool
            ops.maxpool_bwd_bn(g, arg, x0, a0, coef, S, da, K, Sd, P)
            _ext.TAG = "stem wgrad"
            self._wgrad(ops, da, stem_tape.x, self.stem, None, S, main=True)
        elif stem_tape is not None:
            # g = dL/d(stem output)·[y > 0] with the stem BatchNorm's partials from layer1.0's
            # conv1 dgrad epilogue: finish its backward, weight gradient with the BN backward in
            # the dY prologue (da never materialised)
            _ext.TAG = "stem bwd"
            coef = self._bn_bwd_finish(ops, pre[0], S)
            _ext.TAG = "stem wgrad"
            # on the main stream: nothing else is left for it, while the weight-gradient stream
            # still works through layer1.0's (the tail of the step runs both side by side)
            self._wgrad(ops, g, stem_tape.x, self.stem, None, S,
                        bnb=LazyBN(stem_tape.acts[0], coef), main=True)
        if stem_tape is not None:
            _ext.TAG = ""
            g = None  # the image needs no gradient
        if main is not None:
            if store is not None and getattr(store, "defer_side_join", False):
                # joined in store.finish(), after the stem's backward
                keep, self._side_keep = self._side_keep, []
                store.defer_join(self._side, keep)
            else:
                main.wait_stream(self._side)  # join: every weight gradient is in the flat buffer
                self._side_keep.clear()
        self._wt_ready = False  # the optimizer step changes the weights
        return g

    def _flat_store(self):
        for b in self.blocks:
            slot = getattr(b.convs[0].conv.weight, "_slot", None)
            if slot is not None:
                return slot.store
        return None

    def _block_backward(self, ops, st, S, b: _BlockSpec, tp: _BlockTape, g: torch.Tensor,
                        pre, prev):
        """``g`` = dL/d(block output).  ``pre = None``: g is the raw gradient; otherwise g is
        already ReLU-masked and ``pre`` is the started BN backward (``_bn_bwd_start``) of this
        block's last BN, whose Σg, Σg·x̂ partials the following block's dgrad epilogue
        produced.  Returns the same pair for the block input: masked + started when the
        producer is another block of this executor (``prev``), raw otherwise.

        Every BN all-reduce (distributed) is started before an independent weight-gradient
        kernel and finished after it, so its latency hides behind the wgrad."""
        o = self._out_bn_bwd(ops, st, S, b, tp, g, pre)
        # (bottleneck blocks: conv1 is 1x1 stride 1, so its dgrad epilogue covers every input
        # position; a BasicBlock's conv1 carries the stride itself)
        compact = (b.down is not None and self.compact_ds and b.down.stride == 2 and b.down.k == 1
                   and b.down.pad == 0 and b.convs[0].stride == 1)
        resid, join = self._ds_dgrad_start(ops, S, b, tp, o, compact)
        da, lazy0 = self._chain_bwd(ops, st, S, b, tp, o, prev)
        dx, h = self._conv1_dgrad(ops, st, S, b, tp, o, da, lazy0, resid, join, compact, prev)
        _ext.TAG = f"{b.name} conv1 wgrad"
        self._wgrad(ops, da, tp.x, b.convs[0], None, S, bnb=lazy0)
        if o.dad is not None:
            _ext.TAG = f"{b.name} ds wgrad"
            self._wgrad(ops, o.dad, tp.x, b.down, None, S)
        _ext.TAG = ""
        return dx, h

    def _out_bn_bwd(self, ops, st, S, b: _BlockSpec, tp: _BlockTape, g, pre) -> _OutGrad:
        """Backward of the block output: BN_L from the raw gradient (reduce, apply with the
        ReLU mask of ``out``) or finished from its started handle (``pre``), then the downsample
        BN's — both from one pass, or one of them left to its consumer (``_OutGrad``)."""
        out = tp.out
        L = len(b.convs) - 1
        _ext.TAG = f"{b.name} bn{L + 1} bwd"
        aL, bsL = tp.acts[L], tp.bns[L]
        C = aL.shape[-1]
        R = aL.numel() // C
        dev = aL.device
        da = torch.empty_like(aL)
        lazy = None
        if pre is None:
            nblk = ops.bn_blocks(R, C, S)
            partial = torch.empty((S * nblk * 2 * C,), device=dev, dtype=torch.float32)
            ops.bn_bwd_reduce(g, out, aL, bsL.mi, S, True, partial)
            coefL = self._bn_bwd(ops, b.convs[L].bn, partial, nblk, bsL, S, st)
            g3 = torch.empty_like(out)
            ops.bn_bwd_apply(g, out, aL, coefL, S, True, da, g3)  # g3 = g·[out > 0]
        else:
            g3 = g
            h3, hd = pre
            coefL = self._bn_bwd_finish(ops, h3, S)
            if hd is None:
                if L > 0 and self._bnb_ok(b.convs[L], aL, S):
                    lazy = LazyBN(aL, coefL)  # da never materialised: conv L's operand prologues
                else:
                    ops.bn_bwd_apply(g3, None, aL, coefL, S, False, da, None)
        dad = None
        ds_dual = None  # (g3, coefd): the downsample's backward as one fused pass (_ds_dual)
        if b.down is not None:
            _ext.TAG = f"{b.name} bnds bwd"
            if pre is not None and hd is not None:
                # both BNs of the block output from one pass over g3 (their partials came
                # from the following block's dgrad epilogue) — or only the downsample BN's,
                # with BN3's backward left to conv3's operand prologues
                coefd = self._bn_bwd_finish(ops, hd, S)
                if self._lazy_bn3_ds_ok(b, tp, aL, S):
                    lazy = LazyBN(aL, coefL)
                    if self._ds_dual_ok(b, tp, S):
                        ds_dual = (g3, coefd)  # dad never materialised
                    else:
                        dad = torch.empty_like(tp.ad)
                        ops.bn_bwd_apply(g3, None, tp.ad, coefd, S, False, dad, None)
                else:
                    dad = torch.empty_like(tp.ad)
                    ops.bn_bwd_apply2(g3, aL, coefL, da, tp.ad, coefd, dad, S)
            else:
                dad = torch.empty_like(tp.ad)
                nblk_d = ops.bn_blocks(R, C, S)
                partial_d = torch.empty((S * nblk_d * 2 * C,), device=dev, dtype=torch.float32)
                ops.bn_bwd_reduce(g3, None, tp.ad, tp.bnd.mi, S, False, partial_d)
                coefd = self._bn_bwd(ops, b.down.bn, partial_d, nblk_d, tp.bnd, S, st)
                if pre is not None:
                    ops.bn_bwd_apply2(g3, aL, coefL, da, tp.ad, coefd, dad, S)
                else:
                    ops.bn_bwd_apply(g3, None, tp.ad, coefd, S, False, dad, None)
        return _OutGrad(g3, da, lazy, dad, ds_dual)

    def _ds_dgrad_start(self, ops, S, b: _BlockSpec, tp: _BlockTape, o: _OutGrad, compact: bool):
        """The downsample's input gradient where it can run beside the conv chain: the fused
        pass (``_ds_dual``) or the dgrad on the branch stream → (it, the stream to join or
        None); (None, None) leaves the dgrad to ``_conv1_dgrad``."""
        if b.down is None:
            return None, None
        br = self._branch_stream(tp.ad)
        if o.ds_dual is not None:
            if br is not None and self.ds_dual_stream == "branch":
                br.wait_stream(torch.cuda.current_stream(tp.ad.device))
                with torch.cuda.stream(br):
                    return self._ds_dual(ops, b, tp, o.ds_dual, S), br
            return self._ds_dual(ops, b, tp, o.ds_dual, S), None
        if br is None:
            return None, None
        # the downsample dgrad only meets the conv chain at conv1's dgrad epilogue
        br.wait_stream(torch.cuda.current_stream(o.dad.device))
        with torch.cuda.stream(br):
            _ext.TAG = f"{b.name} ds dgrad"
            return self._dgrad(ops, o.dad, b.down, tp.x.shape, S, compact=compact)[0], br

    def _chain_bwd(self, ops, st, S, b: _BlockSpec, tp: _BlockTape, o: _OutGrad, prev):
        """Convs L..2, last to first: dgrad (+ BN-bwd partials) → start BN all-reduce → wgrad →
        finish BN → apply.  Returns (da, lazy0): conv1's output gradient, or with ``lazy0``
        the masked gradient whose BN1 backward is left to conv1's operand prologues."""
        L = len(b.convs) - 1
        g3, da, lazy = o.g3, o.da, o.lazy
        lazy0 = None
        pend = None  # (g, LazyBN): the BN backward feeding conv i, left to its patch dgrad
        for i in range(L, 0, -1):
            cs = b.convs[i]
            xin, pro_ss = tp.ins[i]
            a_prev, bs_prev = tp.acts[i - 1], tp.bns[i - 1]
            _ext.TAG = f"{b.name} conv{i + 1} dgrad"
            dyn, bnb = (g3, lazy) if (i == L and lazy is not None) else (da, None)
            if pend is not None:
                # dgrad with the BN backward in its patch prologue; that operand is stored as
                # the weight gradient's dY on the way (no separate bn_bwd_apply pass)
                gsrc, lazy_b = pend
                pend = None
                dy_m = torch.empty_like(lazy_b.a)
                gm, part, nb = self._dgrad(ops, gsrc, cs, a_prev.shape, S,
                                           bn_epi=MaskEpi("mask", a_prev, bs_prev),
                                           bnb=lazy_b, bnb_out=dy_m)
                wdy, wbnb = dy_m, None
            elif self._bwd1x1_ok(cs, dyn, xin, pro_ss, a_prev, S):
                _ext.TAG = f"{b.name} conv{i + 1} dgrad+wgrad"
                gm, part, nb = self._bwd1x1_fused(ops, dyn, bnb, cs, a_prev, bs_prev, S, xin)
                wdy = None  # the weight gradient came from the same launch
            else:
                gm, part, nb = self._dgrad(ops, dyn, cs, a_prev.shape, S,
                                           bn_epi=MaskEpi("mask", a_prev, bs_prev), bnb=bnb)
                wdy, wbnb = dyn, bnb
            h = self._bn_bwd_start(ops, b.convs[i - 1].bn, part, nb, bs_prev, S, st)
            if wdy is not None:
                _ext.TAG = f"{b.name} conv{i + 1} wgrad"
                self._wgrad(ops, wdy, xin, cs, pro_ss, S, bnb=wbnb)
            _ext.TAG = f"{b.name} bn{i} bwd"
            coef = self._bn_bwd_finish(ops, h, S)
            if i == 1 and prev is not None and self._lazy_bn1_ok(b, a_prev, S):
                lazy0 = LazyBN(a_prev, coef)  # da1 never materialised: conv1's prologues
                da = gm
                continue
            if i - 1 >= 1 and self._patch_bnb_ok(ops, b.convs[i - 1], a_prev, S):
                pend = (gm, LazyBN(a_prev, coef))
                continue
            da_next = torch.empty_like(a_prev)
            ops.bn_bwd_apply(gm, None, a_prev, coef, S, False, da_next, None)
            da = da_next
        return da, lazy0

    def _conv1_dgrad(self, ops, st, S, b: _BlockSpec, tp: _BlockTape, o: _OutGrad, da, lazy0,
                     resid, join, compact: bool, prev):
        """The block's input gradient: conv1's dgrad plus the residual — the identity path's g3
        or the downsample's input gradient (joined from ``join``, or its dgrad issued here).
        With a producer inside the executor (``prev``) the epilogue applies its ReLU mask and
        emits the partials of its block-output BatchNorm(s), whose backward is started here →
        (dx, (h3, hd)); otherwise (raw dx, None)."""
        cs0 = b.convs[0]
        if b.down is None:
            resid = o.g3
        elif join is not None:
            torch.cuda.current_stream(tp.ad.device).wait_stream(join)
        elif resid is None:
            _ext.TAG = f"{b.name} ds dgrad"
            resid, _, _ = self._dgrad(ops, o.dad, b.down, tp.x.shape, S, compact=compact)
        _ext.TAG = f"{b.name} conv1 dgrad"
        if prev is None:
            dx, _, _ = self._dgrad(ops, da, cs0, tp.x.shape, S, accumulate=True, dx=resid,
                                   sub_resid=compact)
            return dx, None
        pb, ptp = prev
        pds = pb.down is not None
        dx, part, nb = self._dgrad(ops, da, cs0, tp.x.shape, S, bnb=lazy0,
                                   dx=resid if b.down is not None and not compact else None,
                                   sub_resid=compact,
                                   bn_epi=ResEpi("res", resid, ptp.mask, ptp.acts[-1],
                                                 ptp.bns[-1].mi, ptp.ad if pds else None,
                                                 ptp.bnd.mi if pds else None))
        p3, pd = part if pds else (part, None)
        return dx, (self._bn_bwd_start(ops, pb.convs[-1].bn, p3, nb, ptp.bns[-1], S, st),
                    self._bn_bwd_start(ops, pb.down.bn, pd, nb, ptp.bnd, S, st) if pds else None)


class FusedStemStagesFn(torch.autograd.Function):
    """Autograd boundary around stem + executor: input = the image batch (channels_last bf16,
    no gradient), output = last block output; every parameter gradient bypasses autograd (flat
    store).  ``anchor`` (the stem weight) makes autograd call the backward."""

    @staticmethod
    def forward(ctx, img, anchor, ex: FusedStages):
        out, ctx.tapes, ctx.stem_tape = ex.stem_forward(_nhwc(img))
        ctx.ex = ex
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gout):
        ctx.ex.backward(_nhwc(gout, bf16=True), ctx.tapes, ctx.stem_tape)
        ctx.tapes = None
        ctx.stem_tape = None
        return None, None, None


class FusedStagesFn(torch.autograd.Function):
    """Autograd boundary around the executor: input = stem output (channels_last bf16),
    output = last block output; parameter gradients bypass autograd (flat store)."""

    @staticmethod
    def forward(ctx, x, anchor, ex: FusedStages):
        out, ctx.tapes = ex.forward(_nhwc(x))
        ctx.ex = ex
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gout):
        dx = ctx.ex.backward(_nhwc(gout, bf16=True), ctx.tapes)
        ctx.tapes = None
        return dx.permute(0, 3, 1, 2), None, None
