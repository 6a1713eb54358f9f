"""The kernels of ``loss.barlow_global`` (csrc/barlow.hip: k_bt_stats, k_bt_merge_standardize,
k_bt_slab_merge, k_bt_colsum around the per-rank k_bt_corr / k_bt_loss / k_bt_grad / k_bt_bwd /
k_bt_std_bwd) against the rounded torch twin over W ranks, in ONE process: the
collectives of loss/barlow.py are in-process fakes in the manner of
tests/test_gpu_ntxent_gather.py.  The peers' blocks of every exchange are filled from passes of
the twin over every rank's z (three exchanges: three passes, each making one more exchange right);
the rank under test then contributes its own kernel-made block, as it would on a real group.

Shapes (W, n, D): (2, 32, 64) one K step; (4, 32, 128) four ranks merged in order; (2, 96, 128)
three row tiles and three slabs; (8, 32, 64) eight ranks; (2, 64, 2048) the single 16 MiB slab,
all-reduced in place.

Tolerances are those tests/test_gpu_barlow.py puts on the per-rank kernels, with N = W·n rows
under C: the loss at 1e-4·max(1, |ref|), the relative L2 of dz below 1e-2, C within 2·N·2^-24 of
the twin's (one entry per 10,000 by 2^-8 / N more); rstd and the bf16 ẑ bit for bit the twin's.
A forced 1-rank RCCL group (tests/_barlow_global_steps.py) gives the per-rank path's bits."""
import copy
import importlib.util
import json
import os
import subprocess
import sys
import types
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = Path(__file__).resolve().parents[1]
LAMBD = 0.0051

_spec = importlib.util.spec_from_file_location("_barlow_cpu_tests",
                                               ROOT / "tests" / "test_barlow.py")
_cpu = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_cpu)
views, seed_for, check_c, c_bound = _cpu.views, _cpu.seed_for, _cpu.check_c, _cpu.c_bound

CASES = [(2, 32, 64, 0), (2, 32, 64, 1), (4, 32, 128, 0), (4, 32, 128, 3), (2, 96, 128, 0),
         (2, 96, 128, 1), (8, 32, 64, 5), (2, 64, 2048, 0), (2, 64, 2048, 1)]


def _rel(a, b):
    return float((a.float() - b.float()).norm() / (b.float().norm() + 1e-12))


def _slice(z, rank, n):
    N = z.shape[0] // 2
    return torch.cat([z[rank * n:(rank + 1) * n], z[N + rank * n:N + (rank + 1) * n]])


class World:
    """In-process collectives of W ranks that run one after another: exchange k of rank r records
    r's block and returns the blocks recorded so far (zeros for a rank not yet seen)."""

    def __init__(self, W):
        self.W, self.log, self.r, self.k = W, {}, 0, 0

    def enter(self, r):
        self.r, self.k = r, 0

    def _blocks(self, inp):
        slot = self.log.setdefault(self.k, {})
        self.k += 1
        slot[self.r] = inp.detach().cpu().clone()
        return [slot.get(j, torch.zeros_like(slot[self.r])) for j in range(self.W)]

    def all_gather(self, out, inp, group=None):
        out.copy_(torch.cat([b.reshape(-1) for b in self._blocks(inp)]).view_as(out))

    def all_reduce(self, t, group=None):
        blocks = self._blocks(t)
        tot = blocks[0]
        for b in blocks[1:]:
            tot = tot + b  # rank order
        t.copy_(tot)


def _patch(monkeypatch, world, r):
    from simclr_amd.loss import barlow as mod
    monkeypatch.setattr(mod.dist, "all_gather_into_tensor", world.all_gather)
    monkeypatch.setattr(mod.dist, "all_reduce", world.all_reduce)
    st = types.SimpleNamespace(comm=True, world_size=world.W, rank=r, group=None)
    monkeypatch.setattr(mod.pstate, "get", lambda: st)
    world.enter(r)
    return mod


def _twin(monkeypatch, world, z, n, r, lambd, g=None):
    mod = _patch(monkeypatch, world, r)
    zr = z.detach().cpu().clone().requires_grad_(True)  # (.cpu() alone would alias a host z)
    loss, C = mod.barlow_twins_torch(zr, n, lambd, round_operands=True, return_c=True,
                                     world_size=world.W, rank=r)
    (loss if g is None else loss * g).backward()
    return loss.detach(), zr.grad, C


def _hip(monkeypatch, world, z, n, r, lambd, g=None):
    from simclr_amd.ops import _ext
    _ext.require()
    mod = _patch(monkeypatch, copy.deepcopy(world), r)  # (the reference's blocks stay as they are)
    assert mod.hip_path(z, n)
    zh = z.detach().clone().requires_grad_(True)
    loss, C = mod.BarlowTwins(lambd, global_batch=True)(zh, return_c=True)
    (loss if g is None else loss * g).backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), zh.grad.cpu(), C.cpu()


def _make_reference(monkeypatch, zs, n, lambd, g=None):
    """-> (world with every exchange's blocks right, [(loss, dz, C) per rank]): three passes of
    the twin over every rank fill the three exchanges, the fourth is the reference."""
    world = World(len(zs))
    out = None
    for _ in range(4):
        out = [_twin(monkeypatch, world, z, n, r, lambd, g) for r, z in enumerate(zs)]
    assert sorted(world.log) == [0, 1, 2]
    return world, out


_REF = {}


def _reference(monkeypatch, W, n, D, lambd=LAMBD, dtype=torch.bfloat16):
    key = (W, n, D, lambd, dtype)
    if key not in _REF:
        N = W * n
        z = views(N, D, seed_for(N, D) + W)
        z = z.to(torch.bfloat16) if dtype == torch.bfloat16 else z * 1.0009765625
        zs = [_slice(z, r, n) for r in range(W)]
        _REF[key] = (z, zs, *_make_reference(monkeypatch, zs, n, lambd))
    return _REF[key]


def _check(got, ref, N, tag):
    loss, grad, C = got
    rl, rg, rC = ref
    dc = check_c(C, rC, N)
    print(f"{tag}: loss {float(loss):.6f} ref {float(rl):.6f} |dloss| "
          f"{abs(float(loss) - float(rl)):.3e} rel dz {_rel(grad, rg):.3e} max|dC| {dc:.3e} "
          f"(bound {c_bound(N):.3e})")
    assert grad.dtype == rg.dtype
    assert abs(float(loss) - float(rl)) <= 1e-4 * max(1.0, abs(float(rl))), (float(loss),
                                                                             float(rl))
    assert _rel(grad, rg) < 1e-2, _rel(grad, rg)


@pytest.mark.parametrize("W,n,D,r", CASES)
def test_kernels_match_rounded_twin(monkeypatch, W, n, D, r):
    """Measured on an MI355X: profiles/barlow.md."""
    _, zs, world, refs = _reference(monkeypatch, W, n, D)
    # every rank computes the same loss and C
    assert all(torch.equal(x[0], refs[0][0]) and torch.equal(x[2], refs[0][2]) for x in refs)
    got = _hip(monkeypatch, world, zs[r].to(DEV), n, r, LAMBD)
    _check(got, refs[r], W * n, f"W {W} n {n} D {D} rank {r}")


@pytest.mark.parametrize("W,n,D,r", [(2, 32, 64, 1), (4, 32, 128, 3), (2, 96, 128, 0),
                                     (8, 32, 64, 5), (2, 64, 2048, 1)])
def test_statistics_and_zhat_have_the_twins_bits(monkeypatch, W, n, D, r):
    from simclr_amd.loss import barlow as mod
    ops = torch.ops.simclr_amd
    _, zs, _, _ = _reference(monkeypatch, W, n, D)
    want = torch.stack([mod._local_stats(z.float(), n) for z in zs])  # [W][2][2][D], host
    z = zs[r].to(DEV)
    stats = torch.empty(2, 2, D, device=DEV)
    ops.bt_stats(z, stats)
    assert torch.equal(stats.cpu(), want[r])
    rstd = torch.empty(2, D, device=DEV)
    zh = torch.empty(2 * n, D, device=DEV, dtype=torch.bfloat16)
    zhT = torch.empty(2, D, n, device=DEV, dtype=torch.bfloat16)
    ops.bt_merge_standardize(z, want.to(DEV), 1e-5, rstd, zh, zhT)
    mu, rs = mod._merge_stats(want, n, 1e-5)
    zt = ((zs[r].float().view(2, n, D) - mu) * rs).to(torch.bfloat16)
    assert torch.equal(rstd.cpu(), rs.squeeze(1))
    assert torch.equal(zh.cpu().view(2, n, D), zt)
    assert torch.equal(zhT.cpu(), zt.transpose(1, 2))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n,D", [(32, 64), (96, 128)])
def test_standardize_is_stats_then_merge_of_one_rank(n, D, dtype):
    """``bt_standardize`` against ``bt_stats`` + ``bt_merge_standardize`` on the one rank's
    statistics: rstd, ẑ and ẑᵀ bit for bit (the kernels share the row passes and the write pass).
    (32, 64) is the smallest legal shape; n = 96 has 6 rows per row group and 3 chunks of the
    write pass.  Column 5 of view 0 is constant."""
    from simclr_amd.ops import _ext
    ops = _ext.ops()
    z = views(n, D, seed_for(n, D))
    z[:n, 5] = 1.25
    z = (z.to(torch.bfloat16) if dtype == torch.bfloat16 else z * 1.0009765625).to(DEV)

    def outputs():
        return (torch.empty(2, D, device=DEV),
                torch.empty(2 * n, D, device=DEV, dtype=torch.bfloat16),
                torch.empty(2, D, n, device=DEV, dtype=torch.bfloat16))

    one, two = outputs(), outputs()
    ops.bt_standardize(z, 1e-5, *one)
    stats = torch.empty(2, 2, D, device=DEV)
    ops.bt_stats(z, stats)
    ops.bt_merge_standardize(z, stats[None], 1e-5, *two)
    assert bool((one[1].view(2, n, D)[0, :, 5] == 0).all())
    for a, b, what in zip(one, two, ("rstd", "zh", "zhT")):
        assert torch.equal(a, b), what


def test_std_backward_reads_tiles_view_major_and_ranks_rank_major():
    """n = 64, D = 64, W = 2: ``colpart`` [2 views][2 tiles][2][D] and ``gsum`` [2 ranks][2 views]
    [2][D] have one shape and two meanings, and the two ops run one kernel with two sets of
    strides.  Both ops on the SAME buffer, each against dz = rstd·((dẑ − m1) − ẑ·m2) on the host
    with the parts added in ascending order in fp32 and m = Σ / 64 (tiles) or Σ / 128 (ranks).
    Bound per element: 8 · 2^-24 · rstd · (|dẑ| + |m1| + |ẑ·m2|): four fp32 roundings in the
    expression, fused product or not, and one ulp for each of the GPU's two divisions, doubled.
    A swapped stride moves m1 and m2 by about |Σ| / 64, some 1e-2: four orders above the bound."""
    from simclr_amd.ops import _ext
    ops = _ext.ops()
    n, D, W = 64, 64, 2
    g = torch.Generator().manual_seed(64064)
    dzh = torch.randn(2 * n, D, generator=g)
    rstd = torch.rand(2, D, generator=g) + 0.5
    zh = torch.randn(2 * n, D, generator=g).to(torch.bfloat16)
    sums = torch.randn(2, 2, 2, D, generator=g)
    assert sums.unique().numel() == sums.numel()

    def host(part, rows):
        """part(p, v) -> [2][D] = (Σ dẑ, Σ dẑ·ẑ) of part p for view v"""
        want, bound = [], []
        for v in range(2):
            tot = torch.zeros(2, D)
            for p in range(2):
                tot = tot + part(p, v)
            m1, m2 = (tot / rows).double()
            d, h = dzh[v * n:(v + 1) * n].double(), zh[v * n:(v + 1) * n].double()
            rs = rstd[v].double()
            want.append(rs * ((d - m1) - h * m2))
            bound.append(8 * 2.0 ** -24 * rs * (d.abs() + m1.abs() + (h * m2).abs()))
        return torch.cat(want), torch.cat(bound)

    got = []
    for op, part, rows in ((ops.bt_std_backward, lambda t, v: sums[v, t], n),
                           (ops.bt_std_backward_global, lambda r, v: sums[r, v], W * n)):
        dz = torch.empty(2 * n, D, device=DEV)
        op(zh.to(DEV), rstd.to(DEV), dzh.to(DEV), sums.to(DEV), None, dz)
        want, bound = host(part, float(rows))
        err = (dz.cpu().double() - want).abs()
        assert bool((err <= bound).all()), float((err / bound).max())
        got.append(dz.cpu())
    assert not torch.equal(got[0], got[1])  # (both ops reading one layout would pass the above)


@pytest.mark.parametrize("W,n,D", [(2, 32, 64), (4, 32, 128), (2, 96, 128), (2, 64, 2048)])
def test_ranks_sum_to_the_large_batch_gradient(monkeypatch, W, n, D):
    """z = x P with P fixed: the data-parallel mean Σ_r x_rᵀ dz_r / W of the kernels' dz against
    x ᵀ dz of the rounded twin on the whole batch in one process (x = z, P = I), within the dz
    bound; the loss within the loss bound."""
    from simclr_amd.loss.barlow import barlow_twins_torch
    z, zs, world, _ = _reference(monkeypatch, W, n, D)
    zr = z.clone().requires_grad_(True)
    big = barlow_twins_torch(zr, W * n, LAMBD, round_operands=True)
    big.backward()
    big = big.detach()
    want = z.float().t() @ zr.grad.float()
    got = torch.zeros(D, D)
    for r in range(W):
        loss, dz, _ = _hip(monkeypatch, world, zs[r].to(DEV), n, r, LAMBD)
        got += zs[r].float().t() @ dz.float() / W
        assert abs(float(loss) - float(big)) <= 1e-4 * max(1.0, abs(float(big)))
    print(W, n, D, "rel grad", _rel(got, want), float(big))
    assert _rel(got, want) < 1e-2, _rel(got, want)


def test_fp32_input_and_upstream_gradient(monkeypatch):
    W, n, D, r = 2, 32, 64, 1
    _, zs, world, refs = _reference(monkeypatch, W, n, D, dtype=torch.float32)
    got = _hip(monkeypatch, world, zs[r].to(DEV), n, r, LAMBD)
    assert got[1].dtype == torch.float32
    _check(got, refs[r], W * n, "fp32")
    # g != 1 is read on the device
    world_g, refs_g = _make_reference(monkeypatch, zs, n, 1.0, g=0.37)
    got = _hip(monkeypatch, world_g, zs[r].to(DEV), n, r, 1.0, g=0.37)
    _check(got, refs_g[r], W * n, "g 0.37")


def test_constant_columns(monkeypatch):
    """Column 7: constant over the global batch in view 0 (ẑ = 0, C's row 0).  Column 20:
    constant in both views everywhere (dz exactly 0).  Column 33: constant within each rank of
    view 0, another value per rank (M2_r = 0, σ² from the means: a live column)."""
    W, n, D = 2, 32, 64
    N = W * n
    z = views(N, D, 9)
    z[:N, 7] = 1.25
    z[:, 20] = -3.0
    for r in range(W):
        z[r * n:(r + 1) * n, 33] = r + 0.5
    z = z.to(torch.bfloat16)
    zs = [_slice(z, r, n) for r in range(W)]
    world, refs = _make_reference(monkeypatch, zs, n, LAMBD)
    for r in range(W):
        loss, grad, C = got = _hip(monkeypatch, world, zs[r].to(DEV), n, r, LAMBD)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad.float()).all())
        assert torch.equal(C[7], torch.zeros(D))
        assert torch.equal(grad[:, 20], torch.zeros(2 * n, dtype=grad.dtype))
        assert float(C[33].abs().max()) > 1e-3 and float(grad[:n, 33].float().abs().max()) > 0.0
        _check(got, refs[r], N, f"constant columns rank {r}")


@pytest.mark.parametrize("n,D", [(24, 64), (32, 96)])
def test_outside_the_limits_takes_the_twin(monkeypatch, n, D):
    """The module hands such a z to ``barlow_twins_torch`` with the group, world size and rank
    of the parallel state (the twin over real gloo ranks: tests/test_barlow_global.py)."""
    mod = _patch(monkeypatch, World(2), 1)
    z = views(n, D, 3, DEV).to(torch.bfloat16)
    assert not mod.hip_path(z, n)
    seen = {}

    def twin(zz, nn, lambd, eps, **kw):
        seen.update(kw, z=zz, n=nn)
        return torch.zeros((), device=zz.device)

    monkeypatch.setattr(mod, "barlow_twins_torch", twin)
    mod.BarlowTwins(global_batch=True)(z)
    assert seen["z"] is z and seen["n"] == n
    assert (seen["group"], seen["world_size"], seen["rank"]) == (None, 2, 1)


def test_repeatable(monkeypatch):
    W, n, D, r = 2, 96, 128, 1
    _, zs, world, _ = _reference(monkeypatch, W, n, D)
    a = _hip(monkeypatch, world, zs[r].to(DEV), n, r, LAMBD)
    b = _hip(monkeypatch, world, zs[r].to(DEV), n, r, LAMBD)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_ops_check_their_sizes():
    ops = torch.ops.simclr_amd
    bf = dict(device=DEV, dtype=torch.bfloat16)
    z = torch.zeros(64, 64, **bf)  # n 32
    with pytest.raises(RuntimeError, match="barlow"):
        ops.bt_stats(torch.zeros(48, 64, **bf), torch.zeros(2, 2, 64, device=DEV))  # n 24
    with pytest.raises(RuntimeError, match="bt_stats: stats"):
        ops.bt_stats(z, torch.zeros(2, 64, device=DEV))
    out = (torch.zeros(2, 64, device=DEV), torch.zeros(64, 64, **bf), torch.zeros(2, 64, 32, **bf))
    with pytest.raises(RuntimeError, match="bt_merge_standardize: gstats"):
        ops.bt_merge_standardize(z, torch.zeros(2, 2, 2, 128, device=DEV), 1e-5, *out)
    with pytest.raises(RuntimeError, match="bt_merge_standardize: gstats"):
        ops.bt_merge_standardize(z, torch.zeros(2 * 2 * 2 * 64, device=DEV), 1e-5, *out)
    with pytest.raises(RuntimeError, match="bt_merge_standardize sizes"):
        ops.bt_merge_standardize(z, torch.zeros(2, 2, 2, 64, device=DEV), 1e-5,
                                 torch.zeros(64, device=DEV), *out[1:])
    with pytest.raises(RuntimeError, match="bt_merge_standardize: W"):
        ops.bt_merge_standardize(z, torch.zeros(2048, 2, 2, 64, device=DEV), 1e-5, *out)
    with pytest.raises(RuntimeError, match="bt_slab_merge: part"):
        ops.bt_slab_merge(torch.zeros(2, 64, 64, device=DEV), 3, torch.zeros(64, 64, device=DEV))
    with pytest.raises(RuntimeError, match="bt_colsum: csum"):
        ops.bt_colsum(torch.zeros(2, 1, 2, 64, device=DEV), torch.zeros(2, 64, device=DEV))
    with pytest.raises(RuntimeError, match="bt_colsum: colpart"):
        ops.bt_colsum(torch.zeros(2, 2, 64, device=DEV), torch.zeros(2, 2, 64, device=DEV))
    args = (z, torch.zeros(2, 64, device=DEV), torch.zeros(64, 64, device=DEV))
    with pytest.raises(RuntimeError, match="bt_std_backward_global: gsum"):
        ops.bt_std_backward_global(*args, torch.zeros(2, 2, 64, device=DEV), torch.zeros_like(z),
                                   None)
    with pytest.raises(RuntimeError, match="bt_std_backward_global sizes"):
        ops.bt_std_backward_global(z, torch.zeros(64, device=DEV), args[2],
                                   torch.zeros(2, 2, 2, 64, device=DEV), torch.zeros_like(z),
                                   None)
    with pytest.raises(RuntimeError, match="bt_std_backward_global: dz size"):
        ops.bt_std_backward_global(*args, torch.zeros(2, 2, 2, 64, device=DEV),
                                   torch.zeros(32, 64, **bf), None)


# ------------------------------------------------------------------ a forced 1-rank RCCL group
def _worker(tmp_path, mode, key, port):
    out = tmp_path / f"{mode}-{key}.pt"
    env = dict(os.environ, SIMCLR_FORCE_COMM="1")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable,
                        str(ROOT / "tests" / "_barlow_global_steps.py"), mode, key, str(out),
                        str(port)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (mode, key, r.returncode, r.stdout[-2000:] + r.stderr[-3000:])
    return torch.load(out, weights_only=True)


@pytest.mark.timeout(300)
def test_one_rank_group_gives_the_per_rank_bits(tmp_path):
    """W = 1 on a forced-comm 1-rank RCCL group: loss, C and dz bitwise those of
    ``global_batch=False`` at (32, 64) and (512, 128), bf16 and fp32 z, with the three
    collectives issued (the worker counts them)."""
    res = _worker(tmp_path, "identity", "on", 29548)
    assert sorted(res) == ["bf16-32-64", "bf16-512-128", "fp32-32-64", "fp32-512-128"]
    for name, (local, glob) in res.items():
        for a, b, what in zip(local, glob, ("loss", "C", "dz")):
            assert a.dtype == b.dtype and torch.equal(a, b), (name, what)


@pytest.mark.timeout(1200)
def test_captured_steps_equal_eager_and_the_key_off(tmp_path):
    """Five steps with forced comm and the key on: eager, captured and replayed by
    hipGraphLaunch, and by the multi-stream executor (each in a process of its own, started only
    after the one before ended well): losses, master, momentum and BatchNorm buffers bit for bit,
    and equal to the same eager run with the key off (W = 1)."""
    a = _worker(tmp_path, "eager", "on", 29549)
    assert a["replayed"] == 0 and len(set(a["losses"].tolist())) == 5
    assert a["global_calls"] == 5
    runs = [("graph", "on", 29550), ("streams", "on", 29551), ("eager", "off", 29552)]
    for mode, key, port in runs:
        b = _worker(tmp_path, mode, key, port)
        tag = (mode, key)
        assert b["replayed"] == (0 if mode == "eager" else 3), tag
        assert mode == "eager" or b["mode"] == mode, tag
        assert (b["global_calls"] > 0) == (key == "on"), tag
        print(tag, a["losses"].tolist(), b["losses"].tolist())
        assert torch.equal(a["losses"], b["losses"]), (tag, a["losses"], b["losses"])
        assert torch.equal(a["master"], b["master"]), tag
        assert torch.equal(a["momentum"], b["momentum"]), tag
        assert len(a["buffers"]) == len(b["buffers"]) > 0
        assert all(torch.equal(x, y) for x, y in zip(a["buffers"], b["buffers"])), tag


@pytest.mark.timeout(600)
def test_cli_pretrains_with_the_key(tmp_path):
    """``main.py`` accepts the key and trains with it on one GPU.  One process has no
    communicating group (``main.py`` does not force one), so this run takes the per-rank
    kernels; the global path from ``main.py`` runs on 2 gloo ranks in tests/test_barlow_global.py
    and, with the kernels, on a forced 1-rank group in the test above."""
    run = tmp_path / "run"
    r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, str(ROOT / "main.py"),
                        "loss.kind=barlow", "loss.barlow_global=true", "data.synthetic=true",
                        "data.synthetic_size=256", "experiment.batches=32",
                        "experiment.base_cnn=resnet18", "parameter.epochs=1",
                        "experiment.save_model_epoch=1", f"hydra.run.dir={run}"],
                       cwd=str(tmp_path), capture_output=True, text=True)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "training step captured" in out, out[-4000:]
    line = [l for l in out.splitlines() if "Epoch:1/1 progress:1.000 loss:" in l][0]
    loss = float(line.split("loss:")[1].split(",")[0])
    assert loss == loss and 0.0 < loss < 1e4 and ", lr:" in line
    rec = [json.loads(l) for l in (run / "metrics.jsonl").read_text().splitlines()]
    assert set(rec[0]) == {"epoch", "step", "loss", "lr", "images_per_sec", "seconds", "time"}
    assert rec[0]["step"] == 8
    assert (run / "epoch=1-cifar10.pt").exists()
