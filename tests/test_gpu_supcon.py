"""The label-mode (SupCon) kernels of csrc/ntxent.hip against the fp32 twin ``sup_con_torch`` on
the same bf16 z: loss, dz and (gathered, with in-process fakes of the collectives) the column
gradient sent to the peers; bitwise identity with NT-Xent for distinct labels; repeatability;
a captured training step that must read every batch's own labels; the CLI.

Tolerances: the kernel family's own (test_ntxent, test_gathered_ntxent_kernel_path) — the
arithmetic is the same exact-fp32 MFMA: loss 1e-4·max(1, |ref|) (2e-4 gathered), relative L2 of
dz 1e-2 (bf16 output rounding), of the peers' column gradient 1e-3."""
import json
import subprocess
import sys
import types
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = Path(__file__).resolve().parents[1]


def _rel(a, b):
    return float((a.float() - b.float()).norm() / (b.float().norm() + 1e-12))


def _z(n, D, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(2 * n, D, device=DEV, generator=g).to(torch.bfloat16)


def _labels(n, kind):
    i = torch.arange(n, device=DEV)
    if kind == "mod3":
        return i % 3
    if kind == "mod5":
        return i % 5
    if kind == "mod10_unique":
        y = i % 10
        y[17] = 1000  # this image's rows have only their other view as a positive
        return y
    if kind == "equal":
        return torch.full((n,), 4, device=DEV, dtype=torch.int64)
    if kind == "mod100":
        return i % 100
    raise KeyError(kind)


@pytest.mark.parametrize("n,D,tau,kind", [(8, 32, 0.5, "mod3"), (24, 64, 0.1, "mod5"),
                                          (64, 128, 0.5, "mod10_unique"), (64, 128, 0.5, "equal"),
                                          (256, 128, 0.5, "mod100")])
@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_supcon_kernels_match_twin(n, D, tau, kind, reduction):
    from simclr_amd.loss.ntxent import SupCon, sup_con_torch
    from simclr_amd.ops import _ext
    _ext.require()
    z = _z(n, D, 11 * n + D)
    y = _labels(n, kind)
    zh = z.clone().requires_grad_(True)
    loss = SupCon(tau, reduction)(zh, y.to(torch.int32) if n % 16 else y)  # both label dtypes
    loss.backward()
    zr = z.float().requires_grad_(True)
    ref = sup_con_torch(zr, n, y, tau, reduction)
    ref.backward()
    print(kind, reduction, float(loss), float(ref), _rel(zh.grad, zr.grad))
    assert abs(float(loss) - float(ref)) < 1e-4 * max(1.0, abs(float(ref))), (float(loss),
                                                                              float(ref))
    assert zh.grad.dtype == torch.bfloat16
    assert _rel(zh.grad, zr.grad) < 1e-2, _rel(zh.grad, zr.grad)


def test_supcon_fp32_input_gradient():
    """fp32 z: the gradient comes back in fp32 (no bf16 output rounding of dz, but z itself is
    scored as bf16, so the oracle runs on the rounded z)."""
    from simclr_amd.loss.ntxent import SupCon, sup_con_torch
    n, D, tau = 24, 64, 0.5
    z = _z(n, D, 5).float()
    y = _labels(n, "mod5")
    zh = z.clone().requires_grad_(True)
    loss = SupCon(tau)(zh, y)
    loss.backward()
    zr = z.clone().requires_grad_(True)
    ref = sup_con_torch(zr, n, y, tau)
    ref.backward()
    assert abs(float(loss) - float(ref)) < 1e-4 * max(1.0, abs(float(ref)))
    assert zh.grad.dtype == torch.float32 and _rel(zh.grad, zr.grad) < 1e-2


@pytest.mark.parametrize("n,D", [
    pytest.param(24, 128, id="24"), pytest.param(256, 128, id="256"),
    # every D instantiation at R = 48: three 16-row tiles, no multiple of 32, a single split
    pytest.param(24, 32, id="24-32"), pytest.param(24, 64, id="24-64"),
    pytest.param(24, 256, id="24-256")])
def test_distinct_labels_are_ntxent_bitwise(n, D):
    from simclr_amd.loss.ntxent import NTXent, SupCon
    tau = 0.5
    z = _z(n, D, n)
    y = torch.randperm(n, device=DEV) * 7 - 50  # distinct, unordered, some negative
    za = z.clone().requires_grad_(True)
    la = NTXent(tau)(za)
    la.backward()
    zb = z.clone().requires_grad_(True)
    lb = SupCon(tau)(zb, y)
    lb.backward()
    assert torch.equal(la, lb), (float(la), float(lb))
    assert torch.equal(za.grad, zb.grad)


def test_unaligned_labels_take_the_scalar_loads_bitwise():
    """A label array that is 4- but not 16-byte aligned takes the kernels' non-vectorised label
    loads (every buffer the loss allocates itself is 16-byte aligned): forward partials, lse,
    1/|P|, the row losses and both gradient passes equal those of the aligned array."""
    ops = torch.ops.simclr_amd
    n, D, inv_t = 24, 64, 2.0
    R = 2 * n
    zn = torch.empty(R, D, device=DEV)
    inv = torch.empty(R, device=DEV)
    ops.nt_normalize(_z(n, D, 2), zn, inv)
    znT = torch.empty(D, R, device=DEV)
    ops.nt_transpose(zn, znT)
    y = (torch.arange(R, device=DEV) % n % 5).to(torch.int32)
    buf = torch.zeros(R + 8, device=DEV, dtype=torch.int32)
    buf[1:1 + R] = y
    assert y.data_ptr() % 16 == 0 and buf[1:1 + R].data_ptr() % 16 == 4
    g = torch.full((1,), 0.7, device=DEV)
    res = []
    for ycol in (y, buf[1:1 + R]):
        s_fwd = ops.nt_fwd_splits(R, R)
        part = torch.empty(s_fwd * R * 4, device=DEV)
        lse, inv_cnt, rows = (torch.empty(R, device=DEV) for _ in range(3))
        ops.nt_sup_forward_range(znT, ycol, 0, R, 0, n, inv_t, part, 0, R, s_fwd, 0)
        ops.nt_sup_finish(part, R, s_fwd, lse, inv_cnt, rows)
        s_bwd = ops.nt_bwd_splits(R, R)
        ws = torch.empty(s_bwd * R * D, device=DEV)
        d_cols, d_rows = torch.empty(R, D, device=DEV), torch.empty(R, D, device=DEV)
        ops.nt_sup_backward_part(False, zn, znT, lse, inv_cnt, ycol, R, 0, n, inv_t, 1.0 / R, g,
                                 ws, s_bwd, d_cols)
        ops.nt_sup_backward_part(True, zn, znT, lse, inv_cnt, ycol, R, 0, n, inv_t, 1.0 / R, g,
                                 ws, s_bwd, d_rows)
        res.append((part, lse, inv_cnt, rows, d_cols, d_rows))
    for a, b in zip(*res):
        assert torch.equal(a, b)  # (a NaN would not compare equal)
    assert float(res[0][2].min()) < 1.0 and res[0][5].abs().max() > 0  # (several positives)


def test_repeatable():
    from simclr_amd.loss.ntxent import SupCon
    n, D, tau = 256, 128, 0.5
    z = _z(n, D, 3)
    y = _labels(n, "mod100")
    res = []
    for _ in range(2):
        zh = z.clone().requires_grad_(True)
        loss = SupCon(tau)(zh, y)
        loss.backward()
        res.append((loss.detach().clone(), zh.grad.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_label_tensor_is_checked():
    from simclr_amd.loss.ntxent import NTXent, SupCon
    ops = torch.ops.simclr_amd
    n, D = 16, 32
    z = _z(n, D, 1)
    with pytest.raises(ValueError, match="labels"):
        SupCon(0.5)(z, torch.zeros(n + 1, device=DEV, dtype=torch.int64))
    with pytest.raises(TypeError, match="labels"):
        SupCon(0.5)(z, torch.zeros(n, device=DEV))
    with pytest.raises(ValueError, match="labels"):
        NTXent(0.5, supervised=True)(z)
    with pytest.raises(ValueError, match="supervised"):
        NTXent(0.5)(z, labels=torch.zeros(n, device=DEV, dtype=torch.int64))
    # the ops themselves
    R = 2 * n
    znT = torch.zeros(D, R, device=DEV)
    part = torch.zeros(R * 4, device=DEV)
    with pytest.raises(RuntimeError, match="ycol"):
        ops.nt_sup_forward_range(znT, torch.zeros(R, device=DEV, dtype=torch.int64), 0, R, 0, n,
                                 2.0, part, 0, R, 1, 0)
    with pytest.raises(RuntimeError, match="ycol"):
        ops.nt_sup_forward_range(znT, torch.zeros(R - 16, device=DEV, dtype=torch.int32), 0, R, 0,
                                 n, 2.0, part, 0, R, 1, 0)
    with pytest.raises(RuntimeError, match="ycol"):
        ops.nt_sup_backward_part(True, znT.t().contiguous(), znT, torch.zeros(R, device=DEV),
                                 torch.ones(R, device=DEV),
                                 torch.zeros(R + 16, device=DEV, dtype=torch.int32), R, 0, n, 2.0,
                                 1.0, None, torch.zeros(R * D, device=DEV), 1,
                                 torch.zeros(R, D, device=DEV))
    with pytest.raises(RuntimeError, match="out"):
        ops.nt_expand_labels(torch.zeros(n, device=DEV, dtype=torch.int64), None, 2,
                             torch.zeros(n, device=DEV, dtype=torch.int32))


def test_expand_labels_kernel():
    ops = torch.ops.simclr_amd
    g = torch.Generator(device=DEV).manual_seed(0)
    labels = torch.randint(-5, 100, (1000,), device=DEV, generator=g)
    idx = torch.randperm(1000, device=DEV, generator=g)[:300]
    out = torch.empty(600, device=DEV, dtype=torch.int32)
    ops.nt_expand_labels(labels, idx, 2, out)
    want = labels[idx].to(torch.int32)
    assert torch.equal(out, torch.cat([want, want]))
    one = torch.empty(300, device=DEV, dtype=torch.int32)
    ops.nt_expand_labels(labels.to(torch.int32), idx, 1, one)
    assert torch.equal(one, want)
    ops.nt_expand_labels(want, None, 2, out)
    assert torch.equal(out, torch.cat([want, want]))


# ------------------------------------------------------------------ gathered, in one process
def _oracle(z_local, y_local, peers, peer_y, r, n, tau):
    """fp32 SupCon of the local rows against [peer blocks with the local block at r]."""
    R = z_local.shape[0]
    blocks = [p for p in peers]
    blocks.insert(r, z_local)
    ys = [torch.cat([y, y]) for y in peer_y]
    ys.insert(r, torch.cat([y_local, y_local]))
    zall, ycol = torch.cat(blocks), torch.cat(ys)
    zn_all = F.normalize(zall.float(), dim=1)
    zn = zn_all[r * R:(r + 1) * R]
    sim = zn @ zn_all.t() / tau
    idx = torch.arange(R, device=zall.device)
    own = torch.zeros_like(sim, dtype=torch.bool)
    own[idx, r * R + idx] = True
    sim = sim.masked_fill(own, float("-inf"))
    pos = (ycol[r * R:(r + 1) * R, None] == ycol[None, :]) & ~own
    lse = torch.logsumexp(sim, dim=1)
    rows = lse - sim.masked_fill(~pos, 0.0).sum(1) / pos.sum(1)
    return rows.sum() / R


def _gathered(monkeypatch, W, r, n, D, tau, z, y, peers, peer_y, supervised=True):
    from simclr_amd.loss import ntxent as mod
    R = 2 * n
    seen = {}

    def fake_all_gather(out, inp, group=None):
        if inp.dtype == torch.int32:  # the view-expanded labels
            blocks = [torch.cat([p, p]).to(torch.int32) for p in peer_y]
            seen["labels"] = seen.get("labels", 0) + 1
        else:
            blocks = list(peers)
        blocks.insert(r, inp)
        out.copy_(torch.cat(blocks))

    def fake_reduce_scatter(out, inp, group=None):
        seen["d_cols"] = inp.clone()
        out.copy_(inp[r * R:(r + 1) * R])

    monkeypatch.setattr(mod.dist, "all_gather_into_tensor", fake_all_gather)
    monkeypatch.setattr(mod.dist, "reduce_scatter_tensor", fake_reduce_scatter)
    st = types.SimpleNamespace(comm=True, world_size=W, rank=r, group=None)
    monkeypatch.setattr(mod.pstate, "get", lambda: st)
    zh = z.clone().requires_grad_(True)
    if supervised:
        loss = mod.SupCon(tau, gather=True)(zh, y)
    else:
        loss = mod.NTXent(tau, gather=True)(zh)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), zh.grad, seen


def _peer_data(W, n, D, z, seed, classes):
    g = torch.Generator(device=DEV).manual_seed(seed)
    R = 2 * n
    peers = [(0.6 * z.float() + 0.8 * torch.randn(R, D, device=DEV, generator=g))
             .to(torch.bfloat16) for _ in range(W - 1)]
    # the peers' labels overlap the local ones (same small class set)
    peer_y = [torch.randint(0, classes, (n,), device=DEV, generator=g) for _ in range(W - 1)]
    return peers, peer_y


@pytest.mark.parametrize("W,r", [(2, 1), (8, 3)])
def test_gathered_supcon_kernel_path(monkeypatch, W, r):
    from simclr_amd.ops import _ext
    _ext.require()
    n, D, tau = 32, 128, 0.5
    R = 2 * n
    z = _z(n, D, 100 * W + r)
    y = torch.arange(n, device=DEV) % 6
    peers, peer_y = _peer_data(W, n, D, z, 7 * W + r, 6)
    loss, grad, seen = _gathered(monkeypatch, W, r, n, D, tau, z, y, peers, peer_y)
    assert seen["labels"] == 1  # one label collective per step

    zr = z.float().requires_grad_(True)
    pr = [p.float().requires_grad_(True) for p in peers]
    lr = _oracle(zr, y, pr, peer_y, r, n, tau)
    lr.backward()
    print(W, r, float(loss), float(lr), _rel(grad, zr.grad))
    assert abs(float(loss) - float(lr)) < 2e-4 * max(1.0, abs(float(lr))), (float(loss), float(lr))
    assert _rel(grad, zr.grad) < 1e-2, _rel(grad, zr.grad)
    # the column gradient sent to the peers, through the normalisation Jacobian of each block
    dc = seen["d_cols"]
    for j, (p, pg) in enumerate(zip(peers, pr)):
        blk = j if j < r else j + 1
        pn = F.normalize(p.float(), dim=1)
        inv = 1.0 / p.float().norm(dim=1, keepdim=True)
        d = dc[blk * R:(blk + 1) * R]
        dz = (d - pn * (pn * d).sum(1, keepdim=True)) * inv
        assert _rel(dz, pg.grad) < 1e-3, (blk, _rel(dz, pg.grad))


def test_gathered_distinct_labels_are_ntxent_bitwise(monkeypatch):
    W, r, n, D, tau = 2, 1, 32, 128, 0.5
    z = _z(n, D, 9)
    peers, _ = _peer_data(W, n, D, z, 4, 6)
    y = torch.arange(n, device=DEV) * 3
    peer_y = [torch.arange(n, device=DEV) * 3 + 1000 * (j + 1) for j in range(W - 1)]
    la, ga, sa = _gathered(monkeypatch, W, r, n, D, tau, z, None, peers, peer_y, supervised=False)
    lb, gb, sb = _gathered(monkeypatch, W, r, n, D, tau, z, y, peers, peer_y)
    assert torch.equal(la, lb), (float(la), float(lb))
    assert torch.equal(ga, gb)
    assert torch.equal(sa["d_cols"], sb["d_cols"])


def test_ring_with_supervised_raises():
    from simclr_amd.loss.ntxent import NTXent
    with pytest.raises(ValueError, match=r"loss\.supervised.*loss\.gather"):
        NTXent(0.5, gather="ring", supervised=True)


# ------------------------------------------------------------------ training path
def _run_steps(tmp_path, mode):
    out = tmp_path / f"{mode}.pt"
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable,
                        str(ROOT / "tests" / "_supcon_steps.py"), mode, str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, (mode, r.returncode, r.stdout[-2000:] + r.stderr[-3000:])
    return torch.load(out, weights_only=True)


@pytest.mark.timeout(600)
def test_captured_step_reads_each_batch_labels(tmp_path):
    """Eager against captured-and-replayed (after the second step), deterministic tiles, same
    seed, 5 steps with a different label vector each: bitwise equal losses and master weights.
    A replay that read the labels of the captured batch would give other losses."""
    a = _run_steps(tmp_path, "eager")
    b = _run_steps(tmp_path, "captured")  # (started only after the eager run ended well)
    assert b["replayed"] == 3 and a["replayed"] == 0
    print(a["losses"].tolist(), b["losses"].tolist(), b["mode"])
    assert torch.equal(a["losses"], b["losses"]), (a["losses"], b["losses"])
    assert torch.equal(a["master"], b["master"])


@pytest.mark.timeout(600)
def test_cli_pretrains_supervised(tmp_path):
    run = tmp_path / "run"
    r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, str(ROOT / "main.py"),
                        "loss.supervised=true", "data.synthetic=true", "experiment.batches=32",
                        "parameter.epochs=1", "runtime.max_steps=4", f"hydra.run.dir={run}"],
                       cwd=str(tmp_path), capture_output=True, text=True)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "Epoch:1/1 progress:1.000 loss:" in out
    line = [l for l in out.splitlines() if "Epoch:1/1" in l][0]
    loss = float(line.split("loss:")[1].split(",")[0])
    assert loss == loss and abs(loss) < 100
    assert ", lr:" in line
    rec = [json.loads(l) for l in (run / "metrics.jsonl").read_text().splitlines()]
    assert set(rec[0]) == {"epoch", "step", "loss", "lr", "images_per_sec", "seconds", "time"}
