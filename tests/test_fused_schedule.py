"""The fused executor's schedule, recorded on the CPU (models/fused.py): a constructed
``FusedStages`` is driven through ``stem_forward`` (so ``forward``) and ``backward`` on CPU
tensors with the recording stand-in of ``test_conv_calls.py``, and every op call (arguments as
(role, shape, dtype)), all-reduce / wait and every ``_ext.TAG`` value in force when one of them
is issued is compared, event for event, with ``tests/golden/fused_schedule_v1.json``.  The log
was recorded before ``_block_backward`` was split into phases (``python
tests/test_fused_schedule.py --write`` records it again after a deliberate change of the
schedule).

The cases are a bottleneck and a BasicBlock network of one or two blocks per stage at the smallest
input the executor supports (``_shape_ok``): 32 images (S = 2 views
of 16) entering layer1 at 16 x 16, so the per-view rows are 4096 / 1024 / 256 / 64 and every
stride-2 parity class tiles by 64.  Tensors the case made are named (input, output gradient, the
BatchNorm parameters and buffers), the tapes' tensors are named after the forward (so the
backward's log says which saved tensor each launch reads); everything else is ``new``.

Covered: the forward chain with its BN-apply materialisation (k x k convs, ``_mat_expand``) and
the separate block-output pass; the plain stem and the pooled stem, forward and backward; in
``_block_backward`` the raw-gradient and the started-handle form of the block-output BatchNorm
backward, the lazy BN3 (``_bnb_ok``, ``_lazy_bn3_ds_ok``), both BNs of a downsample block from
one pass (``bn_bwd_apply2``) and the downsample BN alone, the inline downsample dgrad (compact
and full), the conv chain through ``_dgrad`` + ``_wgrad`` and through the fused 1x1 backward
(``_bwd1x1_fused``, narrow and wide, with the materialised X), conv1 with the producer's
``ResEpi`` (with and without its downsample BN) and with the accumulate epilogue, and, with a
communicator, each BN all-reduce started before a weight gradient and waited for after it.

Not reachable on the CPU (every one is guarded by ``is_cuda``; the GPU suite and the benchmark's
output dump cover them): the block-output prologue (``_dual_ok``), ``_ds_dual``, the patch
BN-backward prologue (``_patch_bnb_ok``), the space-to-depth stem, and the weight-gradient and
branch streams (so every launch here is on the one implicit stream).
"""
import json
import sys
from types import SimpleNamespace

import pytest
import torch

from test_conv_calls import BF16, ROOT, Recorder, RecOps, _dump

GOLDEN = ROOT / "tests" / "golden" / "fused_schedule_v1.json"
S, NB, HW = 2, 32, 16

# (case, block type, blocks per stage, stem kind, communicator): each stage's first block
# (downsample) and an identity block wherever that takes another path than the stage before
# (a bottleneck's lazy BN3 and fused 1x1 backward depend on the width, a BasicBlock's nothing)
CASES = (("bottleneck, cifar stem, communicator", "Bottleneck", [2, 2, 2, 2], "cifar", True),
         ("basic block, pooled imagenet stem, single GPU", "BasicBlock", [2, 1, 1, 1], "imagenet",
          False))


class ScheduleOps(RecOps):
    def bn_blocks(self, R, C, S):
        """(a host-side query like the tile-variant ones: 256-row blocks per segment)"""
        return max(1, R // S // 256)


class ScheduleRecorder(Recorder):
    """... which also logs ``_ext.TAG`` whenever an event is issued under another value."""

    def __init__(self, monkeypatch):
        super().__init__(monkeypatch)
        self.ops = ScheduleOps(self)

    def case(self, name):
        super().case(name)
        self.tag = None

    def event(self, *ev):
        from simclr_amd.ops import _ext
        if ev[0] in ("cached", "pick"):  # the tuning lookups: test_conv_calls.py pins them
            return
        if _ext.TAG != self.tag:
            self.tag = _ext.TAG
            super().event("tag", self.tag)
        super().event(*ev)


def _name_tape(rec, tag, tp):
    def name(role, t):
        if t is not None and t.untyped_storage().data_ptr() not in rec.roles:
            rec.name(role, t)

    for i, (a, bs) in enumerate(zip(tp.acts, tp.bns)):
        name(f"{tag}.a{i + 1}", a)
        name(f"{tag}.bn{i + 1}.mi", bs.mi)
        name(f"{tag}.bn{i + 1}.ss", bs.ss)
    if tp.ad is not None:
        name(f"{tag}.ad", tp.ad)
        name(f"{tag}.bnd.mi", tp.bnd.mi)
        name(f"{tag}.bnd.ss", tp.bnd.ss)
    name(f"{tag}.out", tp.out)
    name(f"{tag}.mask", tp.mask)
    for i, t in enumerate(tp.pool or ()):
        name(f"{tag}.pool{i}", t)
    for i, (x, _) in enumerate(tp.ins):  # the materialised BN + ReLU inputs
        name(f"{tag}.in{i + 1}", x)


def _record(rec, monkeypatch):
    from simclr_amd.models import resnet
    from simclr_amd.models.fused import FusedStages
    from simclr_amd.ops import _ext
    from simclr_amd.parallel import state as pstate
    monkeypatch.setattr(_ext, "ops", lambda: rec.ops)
    monkeypatch.setattr(_ext, "TAG", "")
    for case, block, layers, stem, comm in CASES:
        torch.manual_seed(0)
        net = resnet.ResNet(getattr(resnet, block), layers, None, stem=stem)
        ex = FusedStages(net, S)
        monkeypatch.setattr(pstate, "_STATE", SimpleNamespace(
            comm=comm, ipc=None, world_size=2 if comm else 1, stats_group="stats",
            branch_stat_group="branch"))
        rec.case(case)
        for n, t in list(net.named_parameters()) + list(net.named_buffers()):
            rec.name(n, t)
        assert ex._shape_ok(NB, HW, HW) and not ex._shape_ok(NB // 2, HW, HW)
        hw = HW * ex.stem.stride * (ex.stem_pool[1] if ex.stem_pool else 1)
        out, tapes, stem_tape = ex.stem_forward(rec.T("img", NB, hw, hw, 8))
        assert tapes[0].x.shape == (NB, HW, HW, 64)
        _name_tape(rec, "stem", stem_tape)
        for b, tp in zip(ex.blocks, tapes):
            _name_tape(rec, b.name, tp)
        assert ex.backward(rec.T("gout", *out.shape), tapes, stem_tape) is None
        assert out.dtype == BF16 and _ext.TAG == ""
        assert ex.dual_launches == 0 and ex.out_apply_calls == len(ex.blocks)
        for n, p in net.named_parameters():
            assert p.grad is not None and p.grad.shape == p.shape, n


@pytest.fixture
def recorded(monkeypatch):
    rec = ScheduleRecorder(monkeypatch)
    _record(rec, monkeypatch)
    return rec.log


def test_schedule_matches_the_recorded_log(recorded):
    golden = json.loads(GOLDEN.read_text())
    assert list(recorded) == list(golden)
    for name, events in recorded.items():
        for i, (got, want) in enumerate(zip(events, golden[name])):
            assert got == want, f"{name}: event {i}"
        assert len(events) == len(golden[name]), name


if __name__ == "__main__" and sys.argv[1:] == ["--write"]:
    sys.path.insert(0, str(ROOT))
    mp = pytest.MonkeyPatch()
    try:
        r = ScheduleRecorder(mp)
        _record(r, mp)
    finally:
        mp.undo()
    GOLDEN.write_text(_dump(r.log))
    print(f"wrote {GOLDEN}")
