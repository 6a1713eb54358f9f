"""The conv wrapper's op calls, recorded on the CPU (ops/conv_hip.py, models/fused.py,
models/head_fused.py): which ``torch.ops.simclr_amd`` ops a dgrad, an implicit GEMM with each
fusion, a weight gradient and a BatchNorm reduce issue, in which order, with which arguments and
under which tuning keys.

``ops`` is a recording stand-in: every op takes the parameter names and defaults of its schema in
``csrc/bindings.cpp`` (so a positional and a keyword call give the same record), tensors are
recorded as (role, shape, dtype) — the role is the name the case gave the tensor, ``new`` for
one the code under test allocated — and the tile-variant queries answer from the small fixed
table below.  Tuning is off and the tensors live on the CPU, so ``tuning.pick`` takes its
default branch.  The log is compared call for call with ``tests/golden/conv_calls_v1.json``,
recorded before the launch descriptions became typed records (``python tests/test_conv_calls.py
--write`` records it again after a deliberate change of the launch sequence).
"""
import json
import re
import sys
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "conv_calls_v1.json"
BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8


def _schemas():
    """{op: [(parameter, default or ...)]} from the ``m.def("...")`` strings of bindings.cpp."""
    src = (ROOT / "simclr_amd" / "csrc" / "bindings.cpp").read_text()
    consts = {"None": None, "True": True, "False": False}
    out = {}
    for m in re.finditer(r'm\.def\(\s*((?:"[^"]*"\s*)+),', src):
        sig = "".join(re.findall(r'"([^"]*)"', m.group(1)))
        name, args = re.match(r"(\w+)\((.*)\)\s*->", sig).groups()
        params = []
        for a in filter(None, (s.strip() for s in args.split(","))):
            decl, eq, default = a.partition("=")
            params.append((decl.split()[-1],
                           ... if not eq else consts[default] if default in consts
                           else json.loads(default)))
        out[name] = params
    return out


class RecOps:
    """Recording stand-in of ``torch.ops.simclr_amd`` (see the module docstring)."""

    # the fixed tile-variant table: four implicit-GEMM variants (the last the patch kernel),
    # three weight-gradient variants
    IGEMM_BM = (128, 64, 256, 64)
    WGRAD_AREA = (256 * 256, 256 * 128, 128 * 128)
    WGRAD_GLDS = (True, False, True)
    WGRAD_SPLITS = (12, 8, 4)

    def __init__(self, rec):
        self._rec = rec
        self._schemas = _schemas()

    def igemm_nvariants(self):
        return 4

    def igemm_variant_bm(self, v):
        return self.IGEMM_BM[v]

    def igemm_variant_patch(self, v):
        return v == 3

    def igemm_variant_ok(self, v, geom, pro, bn_bwd_pro, epi_mode=0):
        assert len(geom) == 22 and isinstance(pro, bool) and isinstance(bn_bwd_pro, bool)
        if v == 0:
            return not bn_bwd_pro or geom[6] == 1
        if v == 2:
            return not pro and epi_mode < 256 and epi_mode != 2
        if v == 3:
            return geom[6] == 3 and geom[8] == 1
        return True

    def igemm_dual_ok(self, v, geom):
        assert len(geom) == 22
        return v in (0, 1) and geom[6] == 1

    def wgrad_nvariants(self):
        return 3

    def wgrad_variant_ok(self, v, geom, pro, dy_pro):
        assert len(geom) == 22 and isinstance(pro, bool) and isinstance(dy_pro, bool)
        return not dy_pro if v == 0 else not pro if v == 2 else True

    def wgrad_variant_area(self, v):
        return self.WGRAD_AREA[v]

    def wgrad_variant_glds(self, v):
        return self.WGRAD_GLDS[v]

    def wgrad_splits(self, geom, variant=-1):
        assert len(geom) == 22
        return self.WGRAD_SPLITS[variant]

    def __getattr__(self, name):
        params = self._schemas[name]

        def op(*args, **kw):
            assert len(args) <= len(params), name
            call = {p: d for p, d in params}
            call.update({p: a for (p, _), a in zip(params, args)})
            for k, a in kw.items():
                assert k in call and k not in [p for p, _ in params[:len(args)]], (name, k)
                call[k] = a
            missing = [p for p, a in call.items() if a is ...]
            assert not missing, (name, missing)
            self._rec.event("op", name, {p: self._rec.value(a) for p, a in call.items()})

        return op


class Recorder:
    def __init__(self, monkeypatch):
        from simclr_amd.models import fused
        from simclr_amd.ops import tuning
        self.log = {}
        self.events = None
        self.roles = {}
        self.keep = []
        self.ops = RecOps(self)
        monkeypatch.setattr(tuning, "ENABLED", False)
        monkeypatch.setattr(tuning, "_CACHE", {})
        monkeypatch.setattr(tuning, "_PINNED", {})
        self.tuning = tuning
        cached, pick = tuning.cached, tuning.pick

        def rec_cached(key):
            hit = cached(key)
            self.event("cached", key, hit)
            return hit

        def rec_pick(key, candidates, default, run, reps=3):
            v = pick(key, candidates, default, run, reps)
            self.event("pick", key, list(candidates), default, v)
            return v

        monkeypatch.setattr(tuning, "cached", rec_cached)
        monkeypatch.setattr(tuning, "pick", rec_pick)

        def all_reduce(t, group=None, async_op=False):
            self.event("all_reduce", self.value(t), group, async_op)
            return SimpleNamespace(wait=lambda: self.event("wait"))

        monkeypatch.setattr(fused, "dist", SimpleNamespace(all_reduce=all_reduce))

    def case(self, name):
        """Start a case: a cold tuning cache, no named tensors."""
        assert name not in self.log, name
        self.events = self.log[name] = []
        self.roles.clear()
        self.keep.clear()
        self.tuning._CACHE.clear()

    def event(self, *ev):
        self.events.append(json.loads(json.dumps(ev)))  # tuples -> lists, as the fixture holds

    def name(self, role, t):
        self.roles[t.untyped_storage().data_ptr()] = role
        self.keep.append(t)  # alive for the whole case: no other tensor gets its address
        return t

    def T(self, role, *shape, dtype=BF16):
        return self.name(role, torch.zeros(shape, dtype=dtype))

    def value(self, a):
        if isinstance(a, torch.Tensor):
            role = self.roles.get(a.untyped_storage().data_ptr(), "new")
            if a.storage_offset():
                role += f"+{a.storage_offset()}"
            return [role, list(a.shape), str(a.dtype).replace("torch.", "")]
        if isinstance(a, (list, tuple)):
            return [self.value(v) for v in a]
        assert a is None or isinstance(a, (bool, int, float, str)), type(a)
        return a


def _spec(rec, Ci, Co, k, stride, pad, tag="conv"):
    """A conv + BatchNorm spec of the fused executor with named parameters."""
    from simclr_amd.models.fused import _ConvSpec
    conv = torch.nn.Conv2d(Ci, Co, k, stride, pad, bias=False)
    bn = torch.nn.BatchNorm2d(Co)
    for n in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"):
        rec.name(f"{tag}.bn.{n}", getattr(bn, n))
    return _ConvSpec(conv, bn, stride, k, pad)


def _executor():
    from simclr_amd.models.fused import FusedStages
    return FusedStages.__new__(FusedStages)  # the launch helpers need no constructed state


def _bn_state(rec, S, C, tag="bs"):
    from simclr_amd.models.fused import _BNState
    return _BNState(rec.T(f"{tag}.mi", 2 * S * C, dtype=F32),
                    rec.T(f"{tag}.ss", 2 * S * C, dtype=F32).view(2, S * C), 128.0)


# the dgrad shapes: (input H = W, kernel, stride, pad); 5x5 gives unequal parity classes, the
# stride-2 1x1 has parity classes without taps (zero fill)
DGRADS = ((8, 3, 1, 1), (5, 3, 2, 1), (6, 1, 2, 0), (8, 7, 2, 3))


def _record(rec):
    from simclr_amd.models import head_fused
    from simclr_amd.models.fused import BlockOutput, LazyBN, MaskEpi, ResEpi
    from simclr_amd.ops import conv_hip
    from simclr_amd.ops.conv_hip import BnApply, Epilogue, WgradDY, WgradX
    ops, T = rec.ops, rec.T
    Nb, C, S = 2, 8, 2
    ex = _executor()

    for H, k, s, p in DGRADS:
        OH = (H + 2 * p - k) // s + 1
        rec.case(f"conv_dgrad k{k} s{s} p{p} {H}x{H}")
        conv_hip.conv_dgrad(ops, T("dy", Nb, OH, OH, C), T("w", C, k, k, C), Nb, H, H, C, OH, OH,
                            k, k, s, p, C)
        rec.case(f"fused dgrad k{k} s{s} p{p} {H}x{H}")
        ex._dgrad(ops, T("dy", Nb, OH, OH, C), _spec(rec, C, C, k, s, p), (Nb, H, H, C), S)
    rec.case("fused dgrad compact 6x6")
    ex._dgrad(ops, T("dy", Nb, 3, 3, C), _spec(rec, C, C, 1, 2, 0), (Nb, 6, 6, C), S,
              compact=True)

    # run_igemm: plain (twice: the second launch hits the tuning cache), with statistics, the
    # "no admissible variant with statistics" retry (50 rows tile with no variant), a BN-apply
    # prologue and epilogue modes 1 and 2
    g88 = conv_hip.fwd_geom(Nb, 8, 8, C, 8, 8, 3, 3, 1, 1, C)
    rec.case("run_igemm plain, cached")
    for _ in range(2):
        assert conv_hip.run_igemm(ops, T("x", Nb, 8, 8, C), T("w", C, 3, 3, C),
                                  T("y", Nb, 8, 8, C), g88) is None
    rec.case("run_igemm stats")
    st, nblk = conv_hip.run_igemm(ops, T("x", Nb, 8, 8, C), T("w", C, 3, 3, C),
                                  T("y", Nb, 8, 8, C), g88, bias=T("bias", C, dtype=F32),
                                  want_stats=True)
    assert nblk == 2 and st.numel() == 2 * 2 * C
    rec.case("run_igemm stats retry")
    g55 = conv_hip.fwd_geom(Nb, 5, 5, C, 5, 5, 3, 3, 1, 1, C)
    assert conv_hip.run_igemm(ops, T("x", Nb, 5, 5, C), T("w", C, 3, 3, C), T("y", Nb, 5, 5, C),
                              g55, want_stats=True) is None
    rec.case("run_igemm prologue, modes 1 and 2")
    pro = BnApply(T("sc", S * C, dtype=F32), T("sh", S * C, dtype=F32), 64, True)
    x, w, y = T("x", Nb, 8, 8, C), T("w", C, 3, 3, C), T("y", Nb, 8, 8, C)
    conv_hip.run_igemm(ops, x, w, y, g88, pro=pro)
    conv_hip.run_igemm(ops, x, w, y, g88, epi=Epilogue(1, T("ea", Nb, 8, 8, C)))
    conv_hip.run_igemm(ops, x, w, y, g88, want_stats=True,
                       epi=Epilogue(2, T("ea2", Nb, 8, 8, C), T("eb2", Nb, 8, 8, C)))
    with pytest.raises(ValueError, match="BN prologue fusion impossible"):
        conv_hip.run_igemm(ops, T("x5", Nb, 5, 5, C), w, T("y5", Nb, 5, 5, C), g55,
                           want_stats=True, pro=pro)

    # the executor's forward conv: plain, BN-apply prologue, block-output prologue (identity
    # residual and a downsample residual with its BN table)
    cs1 = _spec(rec, C, C, 1, 1, 0)
    rec.case("fused conv_fwd plain 3x3 s2")
    a, stats, nb = ex._conv_fwd(ops, T("x", Nb, 16, 16, C), _spec(rec, C, 16, 3, 2, 1), None, S)
    assert a.shape == (Nb, 8, 8, 16) and nb == 1 and stats.numel() == 2 * 2 * 16
    rec.case("fused conv_fwd BN-apply prologue")
    ex._conv_fwd(ops, T("x", Nb, 8, 8, C), cs1, T("ss", 2, S * C, dtype=F32), S)
    for rss in (None, "rss"):
        rec.case(f"fused conv_fwd block-output prologue, rss={rss}")
        out = T("out", Nb, 8, 8, C)
        dual = BlockOutput(T("aL", Nb, 8, 8, C), T("ss", 2, S * C, dtype=F32),
                           T("res", Nb, 8, 8, C), T("rss", 2, S * C, dtype=F32) if rss else None,
                           out, T("mask", Nb * 8 * 8 * C // 8, dtype=U8))
        ex._conv_fwd(ops, out, cs1, None, S, dual=dual)

    # the executor's dgrad with each epilogue: accumulate (mode 1), subsampled residual,
    # BN-backward mask epilogue (mode 3; stride 1, stride 2 with the statistics remap over the
    # parity classes), residual-block epilogue (mode 4) with and without the subsampled residual
    # and the second BatchNorm stream, the BN-backward prologue and its materialised operand
    cs3 = _spec(rec, C, C, 3, 1, 1)
    shape = (Nb, 8, 8, C)
    rec.case("fused dgrad accumulate")
    ex._dgrad(ops, T("dy", *shape), cs3, shape, S, accumulate=True, dx=T("dx", *shape))
    rec.case("fused dgrad accumulate, subsampled residual")
    ex._dgrad(ops, T("dy", *shape), cs3, shape, S, accumulate=True, dx=T("resid_c", Nb, 4, 4, C),
              sub_resid=True)
    rec.case("fused dgrad mask epilogue")
    _, part, nb = ex._dgrad(ops, T("dy", *shape), cs3, shape, S,
                            bn_epi=MaskEpi("mask", T("a_prev", *shape), _bn_state(rec, S, C)))
    assert nb == 1 and part.numel() == S * 1 * 2 * C
    rec.case("fused dgrad mask epilogue, stride 2")
    _, part, nb = ex._dgrad(ops, T("dy", Nb, 8, 8, C), _spec(rec, C, C, 3, 2, 1),
                            (Nb, 16, 16, C), S,
                            # (a plain tuple of the record's layout is taken too)
                            bn_epi=("mask", T("a_prev", Nb, 16, 16, C), _bn_state(rec, S, C)))
    assert nb == 4 and part.numel() == S * 4 * 2 * C
    for sub in (False, True):
        for second in (False, True):
            rec.case(f"fused dgrad residual epilogue, sub={sub} second={second}")
            resid = T("resid", Nb, 4, 4, C) if sub else T("resid", *shape)
            bn_epi = ResEpi("res", resid, T("mask", Nb * 8 * 8 * C // 8, dtype=U8),
                            T("a_prev", *shape), T("mi", 2 * S * C, dtype=F32),
                            T("ad", *shape) if second else None,
                            T("mid", 2 * S * C, dtype=F32) if second else None)
            _, part, nb = ex._dgrad(ops, T("dy", *shape), cs3, shape, S,
                                    dx=None if sub else resid, sub_resid=sub, bn_epi=bn_epi)
            assert isinstance(part, tuple) == second and nb == 1
    rec.case("fused dgrad BN-backward prologue 1x1")
    ex._dgrad(ops, T("g", *shape), cs1, shape, S,
              bn_epi=MaskEpi("mask", T("a_prev", *shape), _bn_state(rec, S, C)),
              bnb=LazyBN(T("a", *shape), T("coef", 3 * S * C, dtype=F32)))
    rec.case("fused dgrad BN-backward prologue 3x3, materialised operand")
    ex._dgrad(ops, T("g", *shape), cs3, shape, S,
              bn_epi=MaskEpi("mask", T("a_prev", *shape), _bn_state(rec, S, C)),
              bnb=LazyBN(T("a", *shape), T("coef", 3 * S * C, dtype=F32)),
              bnb_out=T("dy_m", *shape))

    # weight gradients: plain, X prologue, dY prologue at S = 2 and S = 4 (the splits are
    # aligned to the segments), beside the critical chain, the executor's wrapper, and the
    # head's one-split form
    g3 = conv_hip.fwd_geom(4, 8, 8, C, 8, 8, 3, 3, 1, 1, C)   # 256 rows
    g1 = conv_hip.fwd_geom(4, 8, 8, C, 8, 8, 1, 1, 1, 0, C)

    def wg_args():
        return T("dY", 4, 8, 8, C), T("X", 4, 8, 8, C), T("dW", C, 3, 3, C, dtype=F32)

    rec.case("run_wgrad plain, cached")
    for _ in range(2):
        conv_hip.run_wgrad(ops, *wg_args(), g3, C)
    rec.case("run_wgrad X prologue")
    conv_hip.run_wgrad(ops, *wg_args(), g3, 3,
                       pro=WgradX(T("sc", S * C, dtype=F32), T("sh", S * C, dtype=F32), 128,
                                  True, S))
    for Sd in (2, 4):
        rec.case(f"run_wgrad dY prologue S={Sd}")
        conv_hip.run_wgrad(ops, *wg_args(), g1, C,
                           dpro=WgradDY(T("dY2", 4, 8, 8, C), T("coef", 3 * Sd * C, dtype=F32),
                                        256 // Sd, Sd))
    rec.case("run_wgrad concurrent")
    conv_hip.run_wgrad(ops, *wg_args(), g3, C, concurrent=True)
    rec.case("fused wgrad X prologue + BN-backward dY prologue")
    ex._wgrad(ops, T("dy", *shape), T("x", *shape), cs1, T("ss", 2, S * C, dtype=F32), S,
              bnb=(T("a", *shape), T("coef", 3 * S * C, dtype=F32)))
    rec.case("head wgrad_direct")
    gg = conv_hip.gemm_geom(256, 64, 128)
    head_fused._wgrad_direct(ops, T("dz", 256, 128), T("y1", 256, 64),
                             T("dW2", 128, 1, 1, 64, dtype=F32), gg, 64,
                             pro=WgradX(T("sc", S * 64, dtype=F32), T("sh", S * 64, dtype=F32),
                                        128, True, S))
    head_fused._wgrad_direct(ops, T("gm", 256, 128), T("x", 256, 64),
                             T("dW1", 128, 1, 1, 64, dtype=F32), gg, 64,
                             dpro=(T("y1b", 256, 128), T("coef", 3 * S * 128, dtype=F32), 128, S))

    # BatchNorm reduce / finalize around the convs: single GPU, and the communicator branch
    # without the IPC exchange (statistics all-reduced between reduce and finalize)
    for comm in (False, True):
        st = SimpleNamespace(comm=comm, ipc=None, world_size=2 if comm else 1,
                             stats_group="stats", branch_stat_group="branch")
        for slot in (0, 1):
            rec.case(f"bn_fwd comm={comm} slot={slot}")
            cs = _spec(rec, C, C, 1, 1, 0)
            bs = ex._bn_fwd(ops, cs.bn, T("partial", 2 * 2 * C, dtype=F32), 1, 64, S, st,
                            slot=slot)
            assert bs.count == 64.0 * st.world_size and bs.ss.shape == (2, S * C)
        rec.case(f"bn_bwd comm={comm}")
        cs = _spec(rec, C, C, 1, 1, 0)
        coef = ex._bn_bwd(ops, cs.bn, T("partial", S * 2 * C, dtype=F32), 1,
                          _bn_state(rec, S, C), S, st)
        assert coef.numel() == 3 * S * C


def _wt_lists():
    """{model: [[conv, [[parity class, weight_transform parameters]]]]} of every conv."""
    from simclr_amd.models.fused import FusedStages
    from simclr_amd.models.resnet import resnet18, resnet50
    out = {}
    with torch.device("meta"):  # only the specs are read
        models = {"resnet50 cifar": resnet50(None, stem="cifar"),
                  "resnet50 imagenet": resnet50(None, stem="imagenet"),
                  "resnet18": resnet18(None, stem="reference_cifar")}
    for name, net in models.items():
        ex = FusedStages(net, 2)
        specs = [("stem", ex.stem)]
        for b in ex.blocks:
            specs += [(f"{b.name}.conv{i + 1}", cs) for i, cs in enumerate(b.convs)]
            if b.down is not None:
                specs.append((f"{b.name}.ds", b.down))
        out[name] = [[n, [[list(key), list(p)] for key, p in FusedStages._wt_params(cs)]]
                     for n, cs in specs]
        models[name] = [cs for _, cs in specs]
    return out, models


def _dump(log):
    lines = []
    for name, events in log.items():
        body = ",\n".join("  " + json.dumps(e) for e in events)
        lines.append(f"{json.dumps(name)}: [\n{body}\n]")
    return "{\n" + ",\n".join(lines) + "\n}\n"


@pytest.fixture
def recorded(monkeypatch):
    rec = Recorder(monkeypatch)
    _record(rec)
    return rec.log


def test_op_calls_match_the_recorded_log(recorded):
    golden = json.loads(GOLDEN.read_text())["calls"]
    assert list(recorded) == list(golden)
    for name, events in recorded.items():
        for i, (got, want) in enumerate(zip(events, golden[name])):
            assert got == want, f"{name}: event {i}"
        assert len(events) == len(golden[name]), name


def test_dgrad_weight_transform_lists_match_the_recorded_ones():
    """... and each is the (key, weight_transform parameters) projection of the conv's dgrad
    plan at a real extent (32 x 32 here), compact form included."""
    from simclr_amd.ops.conv_hip import dgrad_plan
    lists, specs = _wt_lists()
    assert lists == json.loads(GOLDEN.read_text())["wt_params"]
    for name, rows in lists.items():
        for (conv, got), cs in zip(rows, specs[name]):
            Ci, Co = cs.conv.in_channels, cs.conv.out_channels
            OH = (32 + 2 * cs.pad - cs.k) // cs.stride + 1
            plan = dgrad_plan(2, 32, 32, Ci, OH, OH, Co, cs.k, cs.stride, cs.pad)
            assert got == [[list(ln.key), list(ln.wt)] for ln in plan.launches], (name, conv)
            assert all(ln.geom.N == Ci and ln.geom.C == Co and ln.M == ln.geom.M
                       for ln in plan.launches)
            if cs.stride == 2 and cs.k == 1:
                compact, = dgrad_plan(2, 32, 32, Ci, OH, OH, Co, 1, 2, 0, compact=True).launches
                assert [list(compact.key), list(compact.wt)] == got[0] and not plan.launches[1:]


if __name__ == "__main__" and sys.argv[1:] == ["--write"]:
    sys.path.insert(0, str(ROOT))
    mp = pytest.MonkeyPatch()
    try:
        r = Recorder(mp)
        _record(r)
    finally:
        mp.undo()
    wt = _wt_lists()[0]
    wt_txt = ",\n".join(f"{json.dumps(k)}: [\n" + ",\n".join("  " + json.dumps(row) for row in v)
                        + "\n]" for k, v in wt.items())
    GOLDEN.write_text('{"calls": ' + _dump(r.log).rstrip("\n") + ',\n"wt_params": {\n'
                      + wt_txt + "\n}}\n")
    print(f"wrote {GOLDEN}")
