"""NNCLR (``loss.kind=nnclr``, simclr_amd/loss/nnclr.py) on the CPU: the torch twin against an
fp64 double loop, the explicit backward formula against autograd, the reduction to a plain
cross-view cross-entropy when every row finds itself in the support set, the tie and NaN rules
of the lookup, the FIFO enqueue, the config checks, the Trainer, ``main.py`` (one process and 2
gloo ranks) and the resume file's ``nn_queue`` entry.

Tolerances: fp64 comparisons are held to 1e-12 (the measured differences are near 1e-16); the
fp32 reduction test to 1e-6 relative (two fp32 evaluations of the same sums of at most 32 terms:
n·2^-24 is about 2e-6 absolute on logits of size 10, printed before the assertion)."""
import json
import math
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
T = 0.1


def views(n, D, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((2 * n, D), generator=g, dtype=torch.float64).to(dtype)


def rand_queue(Q, D, seed):
    g = torch.Generator().manual_seed(seed)
    return F.normalize(torch.randn((Q, D), generator=g), dim=1).to(torch.bfloat16)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


# ------------------------------------------------------------------ 1. fp64 oracle
def test_unrounded_twin_matches_fp64_double_loop():
    from simclr_amd.loss.nnclr import nnclr_torch
    n, D, Q = 4, 8, 16
    z = views(n, D, 1, torch.float64)
    queue = rand_queue(Q, D, 2)
    qd = queue.double()
    zh = [[float(v) for v in row] for row in z]
    for row in zh:
        nrm = max(math.sqrt(sum(v * v for v in row)), 1e-12)
        row[:] = [v / nrm for v in row]
    want_idx, total = [], 0.0
    for r in range(2 * n):
        best, bk = -math.inf, 0
        for k in range(Q):
            s = sum(zh[r][d] * float(qd[k, d]) for d in range(D))
            if s > best:
                best, bk = s, k
        want_idx.append(bk)
    for r in range(2 * n):
        v, i = divmod(r, n)
        a = [float(x) for x in qd[want_idx[r]]]
        logits = [sum(a[d] * zh[(1 - v) * n + c][d] for d in range(D)) / T for c in range(n)]
        m = max(logits)
        total += m + math.log(sum(math.exp(x - m) for x in logits)) - logits[i]
    want = total / (2 * n)
    loss, idx, a = nnclr_torch(z, queue, n, T, return_nn=True)
    print(float(loss), want, abs(float(loss) - want))
    assert loss.dtype == torch.float64 and idx.tolist() == want_idx
    assert torch.equal(a, queue[idx])
    assert abs(float(loss) - want) <= 1e-12 * max(1.0, abs(want))


# ------------------------------------------------------------------ 2. backward formula
def test_backward_formula_matches_autograd():
    from simclr_amd.loss.nnclr import (_bf16_round, _normalize_exact, nnclr_backward_torch,
                                       nnclr_torch)
    n, D, Q = 12, 16, 64
    queue = rand_queue(Q, D, 3)
    # unrounded, fp64: autograd through the plain ops against the contract's formula
    z = views(n, D, 4, torch.float64).requires_grad_()
    loss, idx, a = nnclr_torch(z, queue, n, T, return_nn=True)
    (3.0 * loss).backward()
    nrm = z.detach().norm(dim=1, keepdim=True).clamp_min(1e-12)
    zh = z.detach() / nrm
    want = nnclr_backward_torch(zh, (1.0 / nrm).squeeze(1), zh, a.double(), n, T, 3.0)
    print("unrounded", rel_l2(z.grad, want))
    assert rel_l2(z.grad, want) <= 1e-12
    # rounded: the Function's dz against autograd on the rounded operands, chained through the
    # normalisation by a straight-through surrogate
    for dtype in (torch.float32, torch.bfloat16):
        zr = views(n, D, 5).to(dtype).requires_grad_()
        loss, idx, a = nnclr_torch(zr, queue, n, T, round_operands=True, return_nn=True)
        assert not idx.requires_grad and not a.requires_grad
        loss.backward()
        assert zr.grad.dtype == dtype
        zn, inv = _normalize_exact(zr.detach().float())
        zop = _bf16_round(zn).double().requires_grad_()
        av, zv = a.double().view(2, n, D), zop.view(2, n, D)
        S = torch.stack([av[0] @ zv[1].t(), av[1] @ zv[0].t()]) / T
        ref = (torch.logsumexp(S, 2) - torch.diagonal(S, dim1=1, dim2=2)).sum() / (2 * n)
        ref.backward()
        assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-5 * max(1.0, abs(float(ref.detach())))
        zf = zr.detach().double().requires_grad_()
        (F.normalize(zf, dim=1, eps=1e-12) * zop.grad).sum().backward()
        tol = 1e-5 if dtype == torch.float32 else 1e-2  # (dz itself is rounded to bf16)
        print(dtype, rel_l2(zr.grad, zf.grad), tol)
        assert rel_l2(zr.grad, zf.grad) <= tol


# ------------------------------------------------------------------ 3. reduction
def planted(n, D, Q, seed):
    """z, a queue of random rows with the batch's own bf16 ẑ rows at known positions, those
    positions, and the margin between the planted similarity and the best other one."""
    from simclr_amd.loss.nnclr import _normalize_exact
    z = views(n, D, seed)
    zb = _normalize_exact(z)[0].to(torch.bfloat16)
    queue = rand_queue(Q, D, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    pos = torch.randperm(Q, generator=g)[:2 * n]
    queue[pos] = zb
    sim = zb.double() @ queue.double().t()
    own = sim[torch.arange(2 * n), pos]
    sim[torch.arange(2 * n), pos] = -2.0
    return z, zb, queue, pos, float(own.min()), float(sim.max())


def test_planted_neighbours_reduce_to_cross_entropy():
    from simclr_amd.loss.nnclr import nnclr_torch
    n, D, Q = 32, 32, 256
    z, zb, queue, pos, own, other = planted(n, D, Q, 11)
    print("planted", own, "best other", other)
    assert own >= 0.99 and other <= 0.8  # a wide margin: no summation order can change a winner
    zv = zb.float().view(2, n, D)
    tgt = torch.arange(n)
    want = 0.5 * (F.cross_entropy(zv[0] @ zv[1].t() / T, tgt)
                  + F.cross_entropy(zv[1] @ zv[0].t() / T, tgt))
    for rounded in (True, False):
        loss, idx, a = nnclr_torch(z, queue, n, T, round_operands=rounded, return_nn=True)
        assert torch.equal(idx, pos)
        assert torch.equal(a, zb)
        if rounded:
            print(float(loss), float(want))
            assert abs(float(loss) - float(want)) <= 1e-6 * max(1.0, abs(float(want)))


# ------------------------------------------------------------------ 4. ties and NaN
def test_ties_take_the_lowest_index_and_nan_never_wins():
    from simclr_amd.loss.nnclr import NNCLR, nn_lookup_torch
    D, Q = 16, 32
    queue = rand_queue(Q, D, 21)
    queue[20] = queue[7]
    queue[29] = queue[7]
    queue[3] = queue[12]
    zq = torch.stack([queue[29], queue[12], queue[5]]).float()
    assert nn_lookup_torch(zq, queue).tolist() == [7, 3, 5]
    bad = queue.clone()
    bad[7] = float("nan")  # the lowest duplicate is gone: the next one wins
    bad[0] = float("nan")
    assert nn_lookup_torch(zq, bad).tolist() == [20, 3, 5]
    bad[:] = float("nan")
    assert nn_lookup_torch(zq, bad).tolist() == [0, 0, 0]
    # through the module (twin path): a NaN row is never selected
    mod = NNCLR(T, queue_size=Q, dim=D, seed=0)
    mod.queue.copy_(queue)
    mod.queue[0] = float("nan")
    z = torch.cat([queue[[29, 12, 5, 9]].float() * 3.0, queue[[20, 3, 1, 2]].float()])
    loss, idx, a = mod(z, update=False, return_nn=True)
    assert idx.tolist() == [7, 3, 5, 9, 7, 3, 1, 2] and math.isfinite(float(loss))
    assert torch.equal(a, mod.queue[idx])


# ------------------------------------------------------------------ 5. FIFO
def test_fifo_enqueue_wraps_and_lookups_see_the_pre_step_queue():
    from simclr_amd.loss.nnclr import NNCLR, _normalize_exact, nn_lookup_torch
    n, D, Q = 96, 32, 256
    mod = NNCLR(T, queue_size=Q, dim=D, seed=5)
    again = NNCLR(T, queue_size=Q, dim=D, seed=5)
    assert torch.equal(mod.queue, again.queue) and mod.queue.dtype == torch.bfloat16
    assert not torch.equal(mod.queue, NNCLR(T, queue_size=Q, dim=D, seed=6).queue)
    norms = mod.queue.float().norm(dim=1)
    assert float((norms - 1).abs().max()) < 2.0 ** -7 and int(mod.cursor) == 0
    want = mod.queue.clone()
    cur = 0
    for step in range(3):
        z = views(n, D, 30 + step)
        before = mod.queue.clone()
        q0, c0 = mod.queue.clone(), mod.cursor.clone()
        l0, i0, a0 = mod(z, update=False, return_nn=True)
        assert torch.equal(mod.queue, q0) and torch.equal(mod.cursor, c0)
        loss, idx, a = mod(z, return_nn=True)
        assert torch.equal(loss, l0) and torch.equal(idx, i0) and torch.equal(a, a0)
        zn = _normalize_exact(z)[0]
        assert torch.equal(idx, nn_lookup_torch(zn, before)) and torch.equal(a, before[idx])
        zb = zn.to(torch.bfloat16)
        for b in range(n):
            want[(cur + b) % Q] = zb[b]
        cur = (cur + n) % Q
        assert torch.equal(mod.queue, want) and int(mod.cursor) == cur
    assert cur == 32 and mod.cursor.dtype == torch.int32  # 3·96 = 288: the third write wrapped
    assert torch.equal(mod.queue[:32], zb[64:96]) and torch.equal(mod.queue[192:], zb[:64])
    # more rows than the set holds (never the kernels' case): the last Q remain
    small = NNCLR(T, queue_size=16, dim=D, seed=5)
    small(views(24, D, 40))
    zb = _normalize_exact(views(24, D, 40))[0].to(torch.bfloat16)
    assert int(small.cursor) == 8
    assert torch.equal(small.queue[8:], zb[8:16]) and torch.equal(small.queue[:8], zb[16:24])
    with pytest.raises(ValueError, match="parameter.d"):
        mod(views(n, 16, 1))
    with pytest.raises(ValueError, match="2n"):
        mod(views(n, D, 1)[:-1])


# ------------------------------------------------------------------ 6. config
def _cfg(ov):
    from simclr_amd.config import compose, task_config, CONF_DIR
    return task_config(compose(str(CONF_DIR), "config", ov))


def test_configuration_keys():
    from simclr_amd.config import check_pretrain_conf
    from simclr_amd.config.validate import LOSS_KINDS
    assert LOSS_KINDS == ("ntxent", "barlow", "nnclr")
    check_pretrain_conf(_cfg(["loss.kind=nnclr"]))
    for q in (512, 1024, 16384, 131072):
        check_pretrain_conf(_cfg(["loss.kind=nnclr", f"loss.nn_queue={q}"]))
    check_pretrain_conf(_cfg(["loss.kind=nnclr", "loss.nn_queue=256", "experiment.batches=256"]))
    check_pretrain_conf(_cfg(["loss.kind=nnclr", "loss.nn_queue=512", "experiment.batches=512",
                              "loss.gather=false", "loss.supervised=false",
                              "loss.barlow_global=false"]))
    for bad in ("lots", "512.0", "true", "0", "128", "300", "1000", "131328", "262144", "-256"):
        with pytest.raises(AssertionError, match=r"loss\.nn_queue"):
            check_pretrain_conf(_cfg(["loss.kind=nnclr", f"loss.nn_queue={bad}"]))
    with pytest.raises(AssertionError, match=r"loss\.nn_queue.*experiment\.batches"):
        check_pretrain_conf(_cfg(["loss.kind=nnclr", "loss.nn_queue=256",
                                  "experiment.batches=512"]))
    with pytest.raises(AssertionError, match=r"loss\.nn_queue.*experiment\.batches"):
        check_pretrain_conf(_cfg(["loss.kind=nnclr", "experiment.batches=32768"]))
    for kind in ([], ["loss.kind=ntxent"], ["loss.kind=barlow"]):
        with pytest.raises(AssertionError, match=r"loss\.nn_queue.*loss\.kind"):
            check_pretrain_conf(_cfg([*kind, "loss.nn_queue=1024"]))
    with pytest.raises(AssertionError, match=r"loss\.kind.*loss\.supervised"):
        check_pretrain_conf(_cfg(["loss.kind=nnclr", "loss.supervised=true"]))
    for gather in ("true", "ring"):
        with pytest.raises(AssertionError, match=r"loss\.kind.*loss\.gather"):
            check_pretrain_conf(_cfg(["loss.kind=nnclr", f"loss.gather={gather}"]))
    with pytest.raises(AssertionError, match=r"loss\.barlow_global"):
        check_pretrain_conf(_cfg(["loss.kind=nnclr", "loss.barlow_global=true"]))
    with pytest.raises(AssertionError, match=r"parameter\.temperature"):
        check_pretrain_conf(_cfg(["loss.kind=nnclr", "parameter.temperature=0"]))


# ------------------------------------------------------------------ 7. Trainer
def _trainer(ov):
    from simclr_amd.parallel import state as pstate
    from simclr_amd.train.pretrain import Trainer
    cfg = _cfg(["experiment.base_cnn=resnet18", "experiment.batches=8", "data.synthetic=true",
                "runtime.precision=fp32", "parameter.epochs=10", "parameter.warmup_epochs=1",
                *ov])
    pstate.reset()
    st = pstate.get()
    st.device = torch.device("cpu")
    torch.manual_seed(0)
    return Trainer(cfg, st, 64, precision="fp32")


@pytest.mark.timeout(300)
def test_trainer_picks_the_loss_and_steps():
    from simclr_amd.data.datasets import synthetic_dataset
    from simclr_amd.data.loader import ContrastiveLoader
    from simclr_amd.loss.nnclr import NNCLR, _normalize_exact, enqueue_torch, nnclr_torch
    from simclr_amd.loss.ntxent import NTXent
    plain = _trainer([])
    assert type(plain.loss_fn) is NTXent
    ov = ["loss.kind=nnclr", "loss.nn_queue=512", "parameter.temperature=0.2"]
    tr = _trainer(ov)
    assert type(tr.loss_fn) is NNCLR and tr.loss_fn.temperature == 0.2
    assert tuple(tr.loss_fn.queue.shape) == (512, 128)
    assert _trainer(["loss.kind=nnclr"]).loss_fn.queue_size == 16384
    # the support set comes from a generator of its own: the model is initialised as without it
    assert torch.equal(tr.store.master, plain.store.master)
    loader = ContrastiveLoader(synthetic_dataset(32, 3), 8, torch.device("cpu"), seed=7)
    xs = [x.clone() for x, _ in loader][:3]
    losses = [tr.step(x).clone() for x in xs]
    # the same three steps by hand on an identically initialised trainer (the first step's
    # warm-up lr is 0, the later ones move the weights): the same torch ops in the same order
    hand = _trainer(ov)
    queue, cursor = hand.loss_fn.queue.clone(), hand.loss_fn.cursor.clone()
    start = hand.store.master.clone()
    for x, loss in zip(xs, losses):
        z = hand.model(hand.prepare(x), segments=2)
        want = nnclr_torch(z, queue, 8, 0.2)
        enqueue_torch(queue, cursor, _normalize_exact(z[:8].detach().float())[0])
        hand.store.zero_grad()
        want.backward()
        hand.store.finish()
        hand.opt.step()
        assert math.isfinite(float(loss))
        assert torch.allclose(loss, want.detach()), (float(loss), float(want))
    assert torch.allclose(tr.store.master, hand.store.master)
    assert not torch.equal(tr.store.master, start)
    assert torch.equal(tr.loss_fn.queue, queue) and int(tr.loss_fn.cursor) == 24
    assert not torch.equal(queue, hand.loss_fn.queue)
    with pytest.raises(ValueError, match="labels"):
        tr.step(xs[0], torch.zeros(8, dtype=torch.int64))


# ------------------------------------------------------------------ 8 / 9. CLI and resume
CLI = ["loss.kind=nnclr", "loss.nn_queue=256", "data.synthetic=true", "data.synthetic_size=32",
       "experiment.batches=8", "experiment.base_cnn=resnet18", "experiment.save_model_epoch=1",
       "parameter.use_cuda=false"]


def _main(args, cwd):
    r = subprocess.run([sys.executable, str(ROOT / "main.py"), *args], cwd=str(cwd),
                       capture_output=True, text=True, timeout=500)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    return out


@pytest.mark.timeout(900)
def test_cli_pretrains_and_resumes_with_the_support_set(tmp_path):
    run = tmp_path / "run"
    out = _main([*CLI, "parameter.epochs=1", f"hydra.run.dir={run}"], tmp_path)
    lines = [l for l in out.splitlines() if "progress:" in l and "loss:" in l]
    assert len(lines) == 1 and "Epoch:1/1 progress:1.000 loss:" in lines[0]
    loss = float(lines[0].split("loss:")[1].split(",")[0])
    assert math.isfinite(loss) and ", lr:" in lines[0]
    ck = torch.load(run / "epoch=1-cifar10.pt", weights_only=True)
    assert len(ck) == 128 and all(k.startswith("module.") for k in ck)  # the reference format
    rec = [json.loads(l) for l in (run / "metrics.jsonl").read_text().splitlines()]
    assert len(rec) == 1
    assert set(rec[0]) == {"epoch", "step", "loss", "lr", "images_per_sec", "seconds", "time"}
    assert rec[0]["step"] == 4
    # 9. the resume file round-trips nn_queue
    from simclr_amd.loss.nnclr import NNCLR
    blob = torch.load(run / "resume-1.pt", weights_only=False)
    entry = blob["nn_queue"]
    assert set(entry) == {"queue", "cursor"} and int(entry["cursor"]) == 32
    assert tuple(entry["queue"].shape) == (256, 128) and entry["queue"].dtype == torch.bfloat16
    mod = NNCLR(0.1, queue_size=256, dim=128, seed=123)
    mod.load_queue_state(entry)
    assert torch.equal(mod.queue, entry["queue"]) and int(mod.cursor) == 32
    state = mod.queue_state()
    assert torch.equal(state["queue"], entry["queue"]) and torch.equal(
        state["cursor"], entry["cursor"])
    with pytest.raises(ValueError, match="nn_queue"):
        NNCLR(0.1, queue_size=512, dim=128, seed=1).load_queue_state(entry)
    resumed = _main([*CLI, "parameter.epochs=2", "runtime.max_steps=5",
                     f"runtime.resume={run / 'resume-1.pt'}", f"hydra.run.dir={tmp_path / 'b'}"],
                    tmp_path)
    assert "nn_queue" not in resumed and "Epoch:2/2" in resumed
    # a file without the entry: a warning and a fresh support set
    del blob["nn_queue"]
    torch.save(blob, tmp_path / "old.pt")
    old = _main([*CLI, "parameter.epochs=2", "runtime.max_steps=5",
                 f"runtime.resume={tmp_path / 'old.pt'}", f"hydra.run.dir={tmp_path / 'c'}"],
                tmp_path)
    assert "holds no nn_queue entry" in old and "Epoch:2/2" in old
    # another loss: no entry in the file
    _main([*CLI[2:], "parameter.epochs=1", "runtime.max_steps=1",
           f"hydra.run.dir={tmp_path / 'd'}"], tmp_path)
    assert "nn_queue" not in torch.load(tmp_path / "d" / "resume-1.pt", weights_only=False)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker_cli(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    os.chdir(out_dir)
    sys.path.insert(0, str(ROOT))
    import main as entry
    import simclr_amd.train.pretrain as P
    from simclr_amd.runtime.dist import cleanup
    seen = {}
    checks = []
    orig_step, orig_req = P.Trainer.step, P.require_replicas

    def step(self, x):
        loss = orig_step(self, x)
        seen["queue"], seen["cursor"] = self.loss_fn.queue.clone(), int(self.loss_fn.cursor)
        seen.setdefault("losses", []).append(float(loss))
        return loss

    def req(*a, **k):
        checks.append(k.get("where"))
        return orig_req(*a, **k)

    P.Trainer.step, P.require_replicas = step, req
    try:
        entry.main([*CLI, "parameter.epochs=1", "data.synthetic_size=64",
                    "runtime.save_resume=false", f"hydra.run.dir={out_dir}/run{rank}"])
    finally:
        cleanup()
    torch.save({**seen, "checks": checks}, os.path.join(out_dir, f"rank{rank}.pt"))


@pytest.mark.timeout(600)
def test_main_on_two_gloo_ranks_keeps_per_rank_support_sets(tmp_path):
    """``main.py loss.kind=nnclr`` on 2 gloo ranks, synthetic data, one epoch: each rank fills its
    own support set with its own images, the replica check (store, optimiser, model) passes, and
    rank 0 logs one loss per epoch."""
    mp.spawn(_worker_cli, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    a, b = (torch.load(tmp_path / f"rank{r}.pt", weights_only=False) for r in range(2))
    assert len(a["losses"]) == 4 and all(math.isfinite(v) for v in a["losses"] + b["losses"])
    assert a["checks"] == ["after epoch 1"] and b["checks"] == ["after epoch 1"]
    assert a["cursor"] == 32 and b["cursor"] == 32
    assert not torch.equal(a["queue"][:32], b["queue"][:32])  # other images on the other rank
    assert torch.equal(a["queue"][32:], b["queue"][32:])      # the same seed's initial rows
    rec = [json.loads(l) for l in (tmp_path / "run0" / "metrics.jsonl").read_text().splitlines()]
    assert len(rec) == 1 and rec[0]["loss"] == pytest.approx(a["losses"][-1])
    assert set(rec[0]) == {"epoch", "step", "loss", "lr", "images_per_sec", "seconds", "time"}
    assert not (tmp_path / "run1" / "metrics.jsonl").exists()
