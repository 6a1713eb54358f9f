"""SimCLR's Gaussian blur in the augmentation kernels (``csrc/augment.hip``) against the NumPy
twin: both kernels (register-resident up to 64x64, banded two-pass above), ``params_out``, the
untouched blur-off results, constant images, the binding's checks, the loader and a captured
training run."""
import subprocess
import sys
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest
import torch

from simclr_amd.data import augment_ref
from simclr_amd.data.augment_ref import Rng, image_key, sample_params

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
DEV = torch.device("cuda", 0)
VIEWS, COUNTER, STRENGTH = 2, 3, 0.5
TOL = 2.5 / 255 + 4e-3  # the existing augmentation tests' per-pixel tolerance
# (H, W, ks, n, seed): the seed is chosen with the twin so that at least a third of the
# (image, view) pairs are blurred (asserted in _case)
# (asserted in _case).  The two-pass kernel stages whole images up to about 60 KB / 7 bytes per
# pixel (80x80, 100x72) and walks bands above: 160x120 (bands of 50 rows, then 10, a gray blurred
# image among them) and 224x224 (bands of 17, then 3).
CASES = [(32, 32, 3, 16, 1), (64, 64, 7, 8, 1), (24, 40, 5, 8, 1), (80, 80, 9, 8, 1),
         (100, 72, 23, 4, 1), (224, 224, 23, 2, 5), (160, 120, 23, 2, 17)]
IDS = [f"{h}x{w}-ks{k}" for h, w, k, _, _ in CASES]


@pytest.fixture(scope="module")
def ops():
    from simclr_amd.ops import _ext
    _ext.require()
    return _ext.ops()


def _launch(ops, imgs, H, W, n, seed, ks, with_ks=True):
    out = torch.empty((VIEWS * n, H, W, 8), device=DEV, dtype=torch.bfloat16)
    params = torch.full((VIEWS * n, 16), -1.0, device=DEV, dtype=torch.float32)
    extra = (ks,) if with_ks else ()
    ops.augment(imgs, torch.arange(n, device=DEV), n, VIEWS, H, W, 8, STRENGTH, seed, COUNTER, 0, 1,
                out, params, *extra)
    torch.cuda.synchronize()
    return out, params


@lru_cache(maxsize=None)
def _case(i):
    """Inputs, twin parameters and twin outputs (blur on) of a case, computed once."""
    H, W, ks, n, seed = CASES[i]
    rng = np.random.default_rng(100 + i)
    imgs = rng.integers(0, 256, size=(n, H, W, 3), dtype=np.uint8)
    Ps = [sample_params(Rng(image_key(seed, COUNTER, v, b)), H, W, STRENGTH, blur=True)
          for v in range(VIEWS) for b in range(n)]
    assert 3 * sum(p["blur"] for p in Ps) >= VIEWS * n, "pick another seed: too few blurred"
    ref = augment_ref.augment_batch(imgs, np.arange(n), VIEWS, H, W, STRENGTH, seed, COUNTER,
                                    blur_kernel=ks)
    ref.setflags(write=False)
    return imgs, Ps, ref


@lru_cache(maxsize=None)
def _gpu(i):
    """The case's launches with blur on and off (the latter without the argument at all)."""
    from simclr_amd.ops import _ext
    H, W, ks, n, seed = CASES[i]
    imgs = torch.from_numpy(_case(i)[0]).to(DEV)
    on = _launch(_ext.ops(), imgs, H, W, n, seed, ks)
    off = _launch(_ext.ops(), imgs, H, W, n, seed, 0, with_ks=False)
    return on, off


def _nchw(out):
    return out.float().cpu().numpy()[..., :3].transpose(0, 3, 1, 2)


def _params_match(row, p):
    return (row[0] == p["ci"] and row[1] == p["cj"] and row[2] == p["ch"] and row[3] == p["cw"]
            and bool(row[4]) == p["flip"])


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_blur_matches_twin_per_image(ops, i):
    _, Ps, ref = _case(i)
    (out, params), _ = _gpu(i)
    assert (out.float()[..., 3:] == 0).all()
    got, P = _nchw(out), params.cpu().numpy()
    excluded = 0
    for m, p in enumerate(Ps):
        if not _params_match(P[m], p):
            excluded += 1
            continue
        share = float(np.mean(np.abs(got[m] - ref[m]) < TOL))
        print(f"image {m}: blur {p['blur']} sigma {p['sigma']:.3f} gray {p['gray']} "
              f"share inside the tolerance {share:.4f}")
        assert share > 0.97, (m, p)
    assert excluded <= 1


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_params_out_sigma_slot(ops, i):
    _, Ps, _ = _case(i)
    (_, params), (_, params_off) = _gpu(i)
    P, Poff = params.cpu().numpy(), params_off.cpu().numpy()
    want = np.array([np.float32(p["sigma"]) if p["blur"] else np.float32(0) for p in Ps])
    assert np.array_equal(P[:, 15].view(np.uint32), want.view(np.uint32))
    assert [bool(s > 0) for s in P[:, 15]] == [p["blur"] for p in Ps]
    assert (Poff[:, 15] == 0).all()
    assert np.array_equal(P[:, :15].view(np.uint32), Poff[:, :15].view(np.uint32))


@pytest.mark.parametrize("i", [0, 4, 6], ids=[IDS[0], IDS[4], IDS[6]])
def test_unblurred_images_are_bitwise_the_blur_off_launch(ops, i):
    H, W, ks, n, seed = CASES[i]
    _, Ps, _ = _case(i)
    (out, _), (out_off, _) = _gpu(i)
    # blur_kernel=0 given explicitly is the launch without the argument
    out0, params0 = _launch(ops, torch.from_numpy(_case(i)[0]).to(DEV), H, W, n, seed, 0)
    assert torch.equal(out0.view(torch.int16), out_off.view(torch.int16))
    assert (params0[:, 15] == 0).all()
    kept = [m for m, p in enumerate(Ps) if not p["blur"]]
    assert kept and len(kept) < len(Ps)
    for m in kept:
        assert torch.equal(out[m].view(torch.int16), out_off[m].view(torch.int16)), m


@pytest.mark.parametrize("H,W,ks,n,seed", [CASES[0], CASES[4], CASES[6]],
                         ids=[IDS[0], IDS[4], IDS[6]])
def test_constant_colour_images_are_unchanged(ops, H, W, ks, n, seed):
    """Un-normalised weights, zero or clamped padding and band seams all move a constant."""
    rng = np.random.default_rng(9)
    colours = rng.integers(0, 256, size=(n, 1, 1, 3), dtype=np.uint8)
    imgs = torch.from_numpy(np.broadcast_to(colours, (n, H, W, 3)).copy()).to(DEV)
    out, params = _launch(ops, imgs, H, W, n, seed, ks)
    out_off, _ = _launch(ops, imgs, H, W, n, seed, 0)
    assert int((params[:, 15] > 0).sum()) * 3 >= VIEWS * n
    assert torch.equal(out.view(torch.int16), out_off.view(torch.int16))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_it_blurs(ops, i):
    _, Ps, _ = _case(i)
    (out, _), (out_off, _) = _gpu(i)
    a, b = out.float()[..., :3], out_off.float()[..., :3]
    strong = [m for m, p in enumerate(Ps) if p["blur"] and p["sigma"] > 0.5]
    assert strong
    for m in strong:
        assert (a[m, :, 1:] - a[m, :, :-1]).abs().mean() < (b[m, :, 1:] - b[m, :, :-1]).abs().mean()
        assert (a[m, 1:] - a[m, :-1]).abs().mean() < (b[m, 1:] - b[m, :-1]).abs().mean()


@pytest.mark.parametrize("i", [0, 4, 6], ids=[IDS[0], IDS[4], IDS[6]])
def test_repeatable(ops, i):
    H, W, ks, n, seed = CASES[i]
    (out, params), _ = _gpu(i)
    out2, params2 = _launch(ops, torch.from_numpy(_case(i)[0]).to(DEV), H, W, n, seed, ks)
    assert torch.equal(out.view(torch.int16), out2.view(torch.int16))
    assert torch.equal(params.view(torch.int32), params2.view(torch.int32))


def test_binding_rejects_bad_blur_kernels(ops):
    imgs = torch.zeros((2, 32, 32, 3), dtype=torch.uint8, device=DEV)
    out = torch.empty((2, 32, 32, 8), device=DEV, dtype=torch.bfloat16)
    lim = ops.augment_max_blur_kernel()
    assert lim >= 23 and lim == augment_ref.MAX_BLUR_KERNEL

    def call(ks, flags=1, o=out, size=32):
        ops.augment(imgs, None, 2, 1, size, size, 8, 0.5, 0, 0, 0, flags, o, None, ks)

    for ks in (4, 1, -3, lim + 1, lim + 2):
        with pytest.raises(RuntimeError, match="blur_kernel"):
            call(ks)
    small = torch.empty((2, 8, 8, 8), device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="too large"):  # half width 8 > 8 - 1
        call(17, o=small, size=8)
    with pytest.raises(RuntimeError, match="augmented mode"):
        call(3, flags=0)
    call(3)
    call(15, o=small, size=8)
    torch.cuda.synchronize()


def test_loader_gpu_matches_its_cpu_path(ops):
    from simclr_amd.data.datasets import synthetic_dataset
    from simclr_amd.data.loader import ContrastiveLoader
    ds = synthetic_dataset(64, 10)
    g = ContrastiveLoader(ds, 16, DEV, seed=5, blur_kernel=3)
    c = ContrastiveLoader(ds, 16, torch.device("cpu"), seed=5, blur_kernel=3)
    idx = torch.arange(10, 26)
    x = g.batch_from_indices(idx.to(DEV), 2)
    ref = c.batch_from_indices(idx, 2).numpy()
    assert x.shape == (32, 8, 32, 32) and x.dtype == torch.bfloat16
    got = x.float().cpu().numpy()[:, :3]
    blurred = 0
    for m in range(32):
        p = sample_params(Rng(image_key(5, 2, m // 16, int(idx[m % 16]))), 32, 32, 0.5, blur=True)
        blurred += p["blur"]
        assert np.mean(np.abs(got[m] - ref[m]) < TOL) > 0.97, (m, p)
    assert 8 <= blurred <= 24


@pytest.mark.timeout(900)
def test_captured_training_step_with_blur(tmp_path):
    r = subprocess.run([sys.executable, str(ROOT / "main.py"), "data.synthetic=true",
                        "data.synthetic_size=512", "experiment.batches=64",
                        "experiment.base_cnn=resnet50", "model.cifar_stem=true", "data.blur=true",
                        "parameter.epochs=1", "parameter.warmup_epochs=1",
                        f"hydra.run.dir={tmp_path / 'run'}"], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=800)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "step 2: training step captured; replay mode streams" in out, out[-3000:]
    assert "Epoch:1/1 progress:1.000 loss:" in out
    loss = float([l for l in out.splitlines() if "Epoch:1/1" in l][0].split("loss:")[1].split(",")[0])
    assert loss == loss and 0.0 < loss < 20.0
