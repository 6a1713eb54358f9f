"""Autograd wrapper of the implicit-GEMM conv kernels (``csrc/conv.hip``).

Tensors: activations are logical NCHW / physical NHWC (``channels_last``) bf16; weights are
consumed as OHWI bf16 (the flat store's shadow) and their gradients are produced as OHWI fp32
directly into the flat gradient buffer.

Pass decomposition (every pass is an implicit GEMM or a weight-gradient launch; which kernel
family and tile runs it — register-staged ``igemm_nt`` / ``wgrad_tn``, LDS-DMA ``igemm_glds`` /
``wgrad_glds`` / ``wgrad_pipe`` / ``wgrad_xp``, or the patch kernels — is the autotuned variant,
one row of the descriptor tables in ``csrc/conv.hip``):

* forward   : gather x with (stride s, pad p); epilogue also emits per-channel Σy, Σy² block
              partials that the following BatchNorm consumes instead of re-reading y.
* dgrad s=1 : dx = conv(dy, flip(W)ᵀ) — gather dy with offset −(K−1−p), B = weight_transform
              (W[co][K−1−kh][K−1−kw][ci] → [ci][kh][kw][co]).
* dgrad s=2 : per output parity class (r, c) ∈ {0,1}²: the taps kh ≡ r+p (mod 2) form a
              stride-1 sub-convolution with negative tap step (dh = −1) whose outputs land on
              rows 2i+r, cols 2j+c (strided epilogue).  No zero-inserted MACs.
* wgrad     : dW[co][kh][kw][ci] = Σ_m dy[m][co] · im2col(x)[m][(kh,kw,ci)], split over m.

How a launch is described (the fused executor and the fused head build the same records):

* ``Geom``: the kernels' ``ConvGeom`` by field name (``fwd_geom``, ``gemm_geom``, and the dgrad
  geometries of ``dgrad_plan``); the ops take it as their ``int[] geom``.
* ``dgrad_plan``: the dgrad decomposition above, once — per launch the parity class, the
  ``weight_transform`` parameters of its B operand, the ``Geom`` and the row count, plus whether
  dx needs a zero fill; also the compact stride-2 1x1 form.
* ``Igemm``: one implicit GEMM — operands, ``Geom``, at most one A-operand prologue (``BnApply``,
  ``BnBackward``, ``BlockOut``), an ``Epilogue``, the segment rows.  ``choose`` (tuning key,
  admissibility, trials on scratch outputs) and ``launch`` (with a ``StatsOut``) read the same
  fields and share the one ``ops.igemm`` call.
* ``run_wgrad``: the one ``ops.wgrad`` call, with the ``WgradX`` / ``WgradDY`` operand prologues;
  split over M, or ``one_split`` straight into the output.
"""
from __future__ import annotations

import functools
from typing import NamedTuple, Optional, Tuple, Union

import torch

from . import _ext, tuning


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


_GEOM_FIELDS = ("Nb IH IW C OH OW KH KW ish isw dh dw ih0 iw0 N OHp OWp osh osw ooh oow "
                "ldo").split()


class Geom(NamedTuple("Geom", [(f, int) for f in _GEOM_FIELDS])):
    """Geometry of one implicit-GEMM / weight-gradient launch: ``ConvGeom`` of
    ``csrc/kernels.h``, field for field.  It *is* the 22-int tuple the ops take as ``int[] geom``
    (and compares / hashes like it, so tuning keys built from it match recorded tables)."""
    __slots__ = ()

    @property
    def M(self) -> int:
        """GEMM rows: output positions gathered by this launch."""
        return self.Nb * self.OH * self.OW

    @property
    def K(self) -> int:
        return self.KH * self.KW * self.C


@functools.lru_cache(maxsize=None)
def _geom(Nb, IH, IW, C, OH, OW, KH, KW, N, ih0=0, iw0=0, stride=1, step=1, full=None,
          ostride=1, ooh=0, oow=0) -> Geom:
    """``stride``: input stride; ``step``: tap step (-1: taps walk backwards); the output
    rows land in a ``full`` = (OHp, OWp) image at ``ostride * i + (ooh, oow)``."""
    OHp, OWp = full if full is not None else (OH, OW)
    return Geom(Nb, IH, IW, C, OH, OW, KH, KW, stride, stride, step, step, ih0, iw0, N,
                OHp, OWp, ostride, ostride, ooh, oow, N)


def fwd_geom(N, H, W, C, OH, OW, KH, KW, stride, pad, Co) -> Geom:
    return _geom(N, H, W, C, OH, OW, KH, KW, Co, ih0=-pad, iw0=-pad, stride=stride)


def gemm_geom(M, K, N) -> Geom:
    """A dense [M, K] x [N, K]ᵀ GEMM: a 1x1 conv over an [M, 1, 1, K] "image"."""
    return _geom(M, 1, 1, K, 1, 1, 1, 1, N)


def wt_shape(p):
    """Shape [Ci][kh][kw][Co] of the weight that ``weight_transform`` parameters ``p`` give."""
    return (p[3], p[4], p[5], p[0])


class DgradLaunch(NamedTuple):
    key: Tuple[int, int]          # output parity class (r, c); (0, 0) for a one-launch dgrad
    wt: Tuple[int, ...]           # the 10 weight_transform parameters of its B operand
    geom: Geom
    M: int                        # its GEMM rows

    @property
    def wt_shape(self):
        return wt_shape(self.wt)


class DgradPlan(NamedTuple):
    launches: Tuple[DgradLaunch, ...]
    zero_fill: bool               # some input positions get no tap: dx must be zeroed first


@functools.lru_cache(maxsize=None)
def dgrad_plan(Nb, H, W, Ci, OH, OW, Co, k, stride, pad, compact: bool = False) -> DgradPlan:
    """The ordered launches of the input gradient dx [Nb, H, W, Ci] of a k x k conv from
    dy [Nb, OH, OW, Co] (the decomposition of the module docstring; ``k``: int or (KH, KW)).

    ``compact`` (stride-2 1x1 unpadded): only the even input positions, as a dense
    [Nb, OH, OW, Ci] tensor — the (0, 0) parity class as one stride-1 GEMM, no zero fill."""
    KH, KW = _pair(k)
    if compact:
        assert stride == 2 and KH == KW == 1 and pad == 0
        assert (OH, OW) == ((H + 1) // 2, (W + 1) // 2)
        return DgradPlan((DgradLaunch((0, 0), (Co, 1, 1, Ci, 1, 1, 0, 2, 0, 2),
                                      _geom(Nb, OH, OW, Co, OH, OW, 1, 1, Ci), Nb * OH * OW),),
                         False)
    if stride == 1:
        g = _geom(Nb, OH, OW, Co, H, W, KH, KW, Ci, ih0=-(KH - 1 - pad), iw0=-(KW - 1 - pad))
        return DgradPlan((DgradLaunch((0, 0), (Co, KH, KW, Ci, KH, KW, KH - 1, -1, KW - 1, -1),
                                      g, Nb * H * W),), False)
    assert stride == 2, "only stride 1/2 convolutions are supported"
    launches, zero_fill = [], False
    for r in (0, 1):
        for c in (0, 1):
            kh0, kw0 = (r + pad) % 2, (c + pad) % 2
            nkh = (KH - kh0 + 1) // 2 if kh0 < KH else 0
            nkw = (KW - kw0 + 1) // 2 if kw0 < KW else 0
            ohc, owc = (H - r + 1) // 2, (W - c + 1) // 2
            if ohc == 0 or owc == 0:
                continue
            if nkh == 0 or nkw == 0:
                zero_fill = True
                continue
            g = _geom(Nb, OH, OW, Co, ohc, owc, nkh, nkw, Ci, ih0=(r + pad - kh0) // 2,
                      iw0=(c + pad - kw0) // 2, step=-1, full=(H, W), ostride=2, ooh=r, oow=c)
            launches.append(DgradLaunch((r, c), (Co, KH, KW, Ci, nkh, nkw, kh0, 2, kw0, 2), g,
                                        Nb * ohc * owc))
    return DgradPlan(tuple(launches), zero_fill)


# ---------------------------------------------------------------------------- fusion operands
# A-operand prologues of the implicit GEMM.  The three kinds share the kernel's operand slots
# (sc, sh, d, seg_rows, relu, A2, rss, out, mask); each record names the ones it owns and
# leaves the others at the class-level None.

class BnApply(NamedTuple):
    """a = relu?(sc[seg]·A + sh[seg]): the previous BatchNorm (+ ReLU) applied on the gathered
    operand; ``sc`` / ``sh`` are [S][C], ``seg_rows`` the rows per view segment."""
    sc: Optional[torch.Tensor]
    sh: Optional[torch.Tensor]
    seg_rows: int
    relu: bool = True
    d = A2 = rss = out = mask = None


class BnBackward(NamedTuple):
    """a = sc[seg]·A + sh[seg]·A2 + d[seg]: the BatchNorm backward (coefficient rows A, B, D of
    ``coef`` [3][S][C]) of the output gradient A against the pre-BN activation ``A2``.  ``out``
    (patch variants only): the operand is also stored there — the weight gradient's dY."""
    sc: torch.Tensor
    sh: torch.Tensor
    d: torch.Tensor
    seg_rows: int
    A2: torch.Tensor
    out: Optional[torch.Tensor] = None
    relu = False
    rss = mask = None

    @classmethod
    def of(cls, coef, SC: int, seg_rows: int, A2, out=None) -> "BnBackward":
        """From the flat ``coef`` [3][S][C] of ``bn_bwd_finalize`` (``SC`` = S·C)."""
        return cls(coef[:SC], coef[SC:2 * SC], coef[2 * SC:], seg_rows, A2, out)


class BlockOut(NamedTuple):
    """a = relu(sc[seg]·A + sh[seg] + res'): A is a residual block's pre-BN last activation,
    ``res`` its residual (``rss``: the residual's BN [2][S][C] table, None for identity); the
    conv consumes the block output and also writes it to ``out`` with its ReLU bitmask
    ``mask``."""
    sc: torch.Tensor
    sh: torch.Tensor
    seg_rows: int
    res: torch.Tensor
    rss: Optional[torch.Tensor]
    out: torch.Tensor
    mask: torch.Tensor
    relu = True
    d = None
    A2 = property(lambda self: self.res)


_NO_PRO = BnApply(None, None, 0, False)


class Epilogue(NamedTuple):
    """Output epilogue ``mode`` (conv.hip): 1 / 2 accumulate ``a`` (, ``b``) into the output;
    3 masks with [bn(b) > 0] from the tables ``ss`` / ``mi``; 4 adds the residual ``a`` and
    masks with the bitmask ``mask``, statistics against ``c`` / ``mi``, and with ``c2`` /
    ``mi2`` a second BatchNorm's statistics too (``StatsOut.stats2``).  ``sub``: the residual
    ``a`` is stride-2 subsampled (added at the even positions)."""
    mode: int = 0
    a: Optional[torch.Tensor] = None
    b: Optional[torch.Tensor] = None
    c: Optional[torch.Tensor] = None
    mask: Optional[torch.Tensor] = None
    sub: bool = False
    ss: Optional[torch.Tensor] = None
    mi: Optional[torch.Tensor] = None
    c2: Optional[torch.Tensor] = None
    mi2: Optional[torch.Tensor] = None

    @property
    def kernel_mode(self) -> int:
        return self.mode | 256 if self.sub else self.mode  # bit 8: subsampled residual


_NO_EPI = Epilogue()


class StatsOut(NamedTuple):
    """Where a launch's per-block statistics partials go.  ``seg_blocks`` / ``base`` remap them
    segment-major when several launches (parity classes) share ``stats``: blocks per segment
    over all of them, and this launch's first block within a segment."""
    stats: Optional[torch.Tensor] = None
    seg_blocks: int = 0
    base: int = 0
    stats2: Optional[torch.Tensor] = None


_NO_STATS = StatsOut()


class Igemm(NamedTuple):
    """One implicit-GEMM launch: operands, geometry and fusions.  ``choose`` picks its tile
    variant (tuning key, admissibility, trials), ``launch`` issues it; both read these fields.
    ``seg_rows``: rows per view segment of the output — tiles must not straddle it (per-segment
    statistics, epilogue tables)."""
    A: torch.Tensor
    B: torch.Tensor
    out: torch.Tensor
    geom: Geom
    bias: Optional[torch.Tensor] = None
    want_stats: bool = False
    pro: Union[None, BnApply, BnBackward, BlockOut] = None
    epi: Optional[Epilogue] = None
    seg_rows: int = 0

    def _issue(self, ops, v, out, so: StatsOut, pro_out, pro_mask) -> None:
        pro, epi = self.pro or _NO_PRO, self.epi or _NO_EPI
        ops.igemm(self.A, self.B, out, self.bias, so.stats, self.geom,
                  pro_sc=pro.sc, pro_sh=pro.sh, pro_seg_rows=pro.seg_rows, pro_relu=pro.relu,
                  epi_mode=epi.kernel_mode, epi_a=epi.a, epi_b=epi.b, variant=v,
                  epi_ss=epi.ss, epi_mi=epi.mi,
                  # the kernel reads the segment only for the epilogue tables / stats remap
                  seg_rows=self.seg_rows if epi.mi is not None else 0,
                  stats_seg_blocks=so.seg_blocks, stats_base=so.base, epi_c=epi.c,
                  epi_mask=epi.mask, epi_c2=epi.c2 if so.stats2 is not None else None,
                  epi_mi2=epi.mi2 if so.stats2 is not None else None, stats2=so.stats2,
                  pro_d=pro.d, A2=pro.A2, pro_rss=pro.rss, pro_out=pro_out, pro_mask=pro_mask)

    def choose(self, ops) -> int:
        """Autotuned tile variant (admissible: BM divides the segment rows / M whenever a
        per-segment prologue, statistics or a per-segment epilogue need block-uniform
        segments)."""
        geom, pro = self.geom, self.pro
        bnb, dual = type(pro) is BnBackward, type(pro) is BlockOut
        patch_only = bnb and pro.out is not None  # (that store exists only in the patch kernel)
        emode = (self.epi or _NO_EPI).kernel_mode
        key = ("igemm", tuple(geom), self.want_stats, pro is not None, emode,
               self.bias is not None, self.seg_rows, bnb, dual, patch_only)
        hit = tuning.cached(key)
        if hit is not None:  # steady state: no per-launch walk over the variant table
            return hit
        M, N = geom.M, geom.N
        pseg = pro.seg_rows if pro is not None else 0
        cands = []
        for v in range(ops.igemm_nvariants()):
            bm = ops.igemm_variant_bm(v)
            if dual:
                if not ops.igemm_dual_ok(v, geom):
                    continue
            elif not ops.igemm_variant_ok(v, geom, pro is not None, bnb, emode):
                continue  # e.g. LDS-DMA variants: C % 64 == 0, BN-apply prologue only on 1x1
            if self.want_stats and M % bm:
                continue
            if pseg % bm or self.seg_rows % bm:
                continue
            if patch_only and not ops.igemm_variant_patch(v):
                continue
            cands.append(v)
        if not cands:
            raise ValueError(f"no igemm tile variant admissible for M={M} segment rows "
                             f"{self.seg_rows or pseg}")
        default = 1 if N <= 64 else 0
        if default not in cands:
            default = cands[0]

        def trial(v):
            # every output of a trial is scratch (tuning.py: trials touch no live tensor), the
            # block-output prologue's out / mask included; no second statistics stream, and
            # the BN-backward operand is not stored
            bm = ops.igemm_variant_bm(v)
            st = (torch.empty(((M + bm - 1) // bm) * 2 * N, device=self.out.device,
                              dtype=torch.float32) if self.want_stats else None)
            self._issue(ops, v, torch.empty_like(self.out), StatsOut(st),
                        torch.empty_like(pro.out) if dual else None,
                        torch.empty_like(pro.mask) if dual else None)

        return tuning.pick(key, cands, default, trial)

    def launch(self, ops, v: int, stats: StatsOut = _NO_STATS) -> None:
        pro = self.pro or _NO_PRO
        self._issue(ops, v, self.out, stats, pro.out, pro.mask)


def run_igemm(ops, A, B, out, geom, bias=None, want_stats=False, pro: Optional[BnApply] = None,
              epi: Optional[Epilogue] = None):
    """Launch the implicit GEMM with the autotuned tile variant for this problem; without an
    admissible variant for the statistics it runs without them.  Returns (stats, nblk) or
    None."""
    job = Igemm(A, B, out, geom, bias, want_stats, pro, epi)
    try:
        v = job.choose(ops)
    except ValueError:
        if pro is not None:
            raise ValueError("BN prologue fusion impossible for this shape")
        job = job._replace(want_stats=False)
        v = job.choose(ops)
    if not job.want_stats:
        job.launch(ops, v)
        return None
    nblk = geom.M // ops.igemm_variant_bm(v)
    stats = torch.empty((nblk * 2 * geom.N,), device=out.device, dtype=torch.float32)
    job.launch(ops, v, StatsOut(stats))
    return stats, nblk


# weight gradients issued beside the dgrad / BatchNorm chain (the fused executor's side stream)
# skip the 256 x 256 output tiles: the autotuner times candidates alone, where those tiles win,
# but their 128 KB of LDS per block keeps every chain block off the CU; under the concurrent
# step the best <= 256 x 128 tile is 0.17 ms/step faster (4 of 4 interleaved A/B rounds,
# profiles/r5_optimization_log.md)
CONCURRENT_MAX_TILE = 256 * 128


class WgradX(NamedTuple):
    """X-operand prologue of the weight gradient: x = relu?(sc[seg]·X + sh[seg]), the BatchNorm
    (+ ReLU) the forward applied on its input; ``S`` segments of ``seg_rows`` rows."""
    sc: Optional[torch.Tensor]
    sh: Optional[torch.Tensor]
    seg_rows: int
    relu: bool
    S: int


class WgradDY(NamedTuple):
    """dY-operand prologue: dy = A·dY + B·dY2 + D, the BatchNorm backward (``coef``
    [3][S][N]) computed on the fly; the splits are aligned to the ``S`` segments."""
    dY2: Optional[torch.Tensor]
    coef: Optional[torch.Tensor]
    seg_rows: int
    S: int


_NO_WX = WgradX(None, None, 0, False, 1)
_NO_WDY = WgradDY(None, None, 0, 1)


def run_wgrad(ops, dY, X, out, geom, creal, pro: Optional[WgradX] = None,
              dpro: Optional[WgradDY] = None, concurrent: bool = False,
              one_split: bool = False) -> None:
    """Weight gradient (fp32, written to ``out`` = OHWI) with the autotuned variant: split
    over M into partials that the op reduces, or with ``one_split`` (few rows: the output tiles
    alone fill the chip) as ONE split written straight into ``out``, no reduction.

    ``concurrent``: the kernel runs beside the critical chain (``CONCURRENT_MAX_TILE``)."""
    xp = WgradX._make(pro) if pro is not None else _NO_WX    # (plain tuples of that layout
    dp = WgradDY._make(dpro) if dpro is not None else _NO_WDY  # are taken too)
    if one_split:
        key = ("wgrad1split", tuple(geom), creal, pro is not None, dpro is not None)
    else:
        key = ("wgrad", tuple(geom), creal, pro is not None, dpro is not None, concurrent)

    def nsplit(v):
        splits = ops.wgrad_splits(geom, v)
        if dpro is None:
            return splits
        seg_iters = dp.seg_rows // 64
        sps = max(1, splits // dp.S)
        while seg_iters % sps:
            sps -= 1
        return dp.S * sps

    def launch(v, o):
        splits = 1 if one_split else nsplit(v)
        partial = o if one_split else torch.empty((splits * geom.N * geom.K,), device=dY.device,
                                                  dtype=torch.float32)
        ops.wgrad(dY, X, partial, o, geom, splits, creal, 0.0,
                  pro_sc=xp.sc, pro_sh=xp.sh, pro_seg_rows=xp.seg_rows, pro_relu=xp.relu,
                  pro_S=xp.S, variant=v, dY2=dp.dY2, dp_coef=dp.coef, dp_seg_rows=dp.seg_rows,
                  dp_S=dp.S)

    v = tuning.cached(key)
    if v is None:
        cands = [v for v in range(ops.wgrad_nvariants())
                 if ops.wgrad_variant_ok(v, geom, pro is not None, dpro is not None)]
        if one_split:  # the dY prologue of one split: register-staged variants (they take the
            # per-row view segment)
            cands = [c for c in cands if dpro is None or not ops.wgrad_variant_glds(c)]
        elif concurrent:
            cands = [c for c in cands
                     if ops.wgrad_variant_area(c) <= CONCURRENT_MAX_TILE] or cands
        default = 0 if one_split else (1 if geom.N <= 64 else 0)
        v = tuning.pick(key, cands, default, lambda vv: launch(vv, torch.empty_like(out)))
    launch(v, out)


def _nhwc(t: torch.Tensor) -> torch.Tensor:
    """Contiguous NHWC view of a channels_last 4-D tensor (copies only if needed)."""
    if t.dim() == 4:
        if not t.is_contiguous(memory_format=torch.channels_last):
            t = t.contiguous(memory_format=torch.channels_last)
        return t.permute(0, 2, 3, 1)
    return t.contiguous()


def _empty_cl(n, c, h, w, device, dtype=torch.bfloat16):
    return torch.empty((n, c, h, w), device=device, dtype=dtype,
                       memory_format=torch.channels_last)


def shadow_ohwi(weight: torch.Tensor, cpad: int) -> torch.Tensor:
    """bf16 OHWI weight for the kernels (flat-store shadow when bound; cast otherwise)."""
    slot = getattr(weight, "_slot", None)
    if slot is not None and slot.shadow is not None:
        w = slot.shadow  # [Co, KH, KW, Ci] bf16 contiguous
    else:
        w = weight.detach().permute(0, 2, 3, 1).to(torch.bfloat16).contiguous()
    ci = w.shape[-1]
    if cpad != ci:
        w = torch.nn.functional.pad(w, (0, cpad - ci)).contiguous()
    return w


class ConvHipFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, weight: torch.Tensor, stride: int, pad: int,
                emit_stats: bool):
        ops = _ext.ops()
        N, Cx, H, W = x.shape
        Co, Ci, KH, KW = weight.shape
        assert Cx >= Ci and Cx % 8 == 0, f"input channels {Cx} vs weight {Ci}"
        OH = (H + 2 * pad - KH) // stride + 1
        OW = (W + 2 * pad - KW) // stride + 1
        xn = _nhwc(x)
        w = shadow_ohwi(weight, Cx)
        y = _empty_cl(N, Co, OH, OW, x.device)
        g = fwd_geom(N, H, W, Cx, OH, OW, KH, KW, stride, pad, Co)
        res = run_igemm(ops, xn, w, y.permute(0, 2, 3, 1), g, want_stats=emit_stats)
        if res is not None:
            y._simclr_stats = res  # (partials, nblk): consumed by the next BatchNorm
        ctx.save_for_backward(x, weight)
        ctx.geom = (N, H, W, Cx, Ci, OH, OW, KH, KW, stride, pad, Co)
        return y

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        ops = _ext.ops()
        x, weight = ctx.saved_tensors
        N, H, W, Cx, Ci, OH, OW, KH, KW, stride, pad, Co = ctx.geom
        dyn = _nhwc(dy)
        if dyn.dtype != torch.bfloat16:
            dyn = dyn.to(torch.bfloat16)
        dx = None
        if ctx.needs_input_grad[0]:
            assert Cx == Ci, "dgrad through a channel-padded stem is not supported"
            w = shadow_ohwi(weight, Ci)
            dx = conv_dgrad(ops, dyn, w, N, H, W, Ci, OH, OW, KH, KW, stride, pad, Co)
        dw = None
        if ctx.needs_input_grad[1]:
            g = fwd_geom(N, H, W, Cx, OH, OW, KH, KW, stride, pad, Co)
            slot = getattr(weight, "_slot", None)
            if slot is not None:
                out = slot.grad  # [Co, KH, KW, Ci] fp32 contiguous view into the flat buffer
            else:
                out = torch.empty((Co, KH, KW, Ci), device=dy.device, dtype=torch.float32)
            run_wgrad(ops, dyn, _nhwc(x), out, g, Ci)
            if slot is not None:
                slot.store.mark_ready(slot.index)
            else:
                dw = out.permute(0, 3, 1, 2)
        return dx, dw, None, None, None


def conv_dgrad(ops, dyn, w_ohwi, N, H, W, Ci, OH, OW, KH, KW, stride, pad, Co):
    """dx [N, Ci, H, W] (channels_last) from dy (NHWC view) and the OHWI bf16 weight."""
    dx = _empty_cl(N, Ci, H, W, dyn.device)
    dxn = dx.permute(0, 2, 3, 1)
    plan = dgrad_plan(N, H, W, Ci, OH, OW, Co, (KH, KW), stride, pad)
    if plan.zero_fill:
        dx.zero_()
    for ln in plan.launches:
        wt = torch.empty(ln.wt_shape, device=dyn.device, dtype=torch.bfloat16)
        ops.weight_transform(w_ohwi, wt, ln.wt)
        run_igemm(ops, dyn, wt, dxn, ln.geom)
    return dx


def conv2d(x: torch.Tensor, w: torch.Tensor, stride, padding, weight_param=None,
           emit_stats: bool = True) -> Optional[torch.Tensor]:
    """HIP conv forward; returns None if this configuration is not supported by the kernels."""
    sh, sw = _pair(stride)
    ph, pw = _pair(padding)
    if sh != sw or ph != pw or sh not in (1, 2) or x.dtype != torch.bfloat16 or x.dim() != 4:
        return None
    if x.shape[1] % 8 != 0:
        return None
    param = weight_param if weight_param is not None else w
    return ConvHipFn.apply(x, param, sh, ph, emit_stats)
