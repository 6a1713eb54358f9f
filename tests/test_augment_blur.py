"""SimCLR's Gaussian blur in the NumPy twin of the augmentation (``data/augment_ref.py``): the
twin against an independent fp64 2-D convolution, reflect padding by hand, constant images, the
two appended draws, the loader's CPU path, the opt-in configuration keys and the CLI."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from simclr_amd.data import augment_ref
from simclr_amd.data.augment_ref import Rng, gaussian_blur, image_key, sample_params

ROOT = Path(__file__).resolve().parents[1]
SIGMAS = [0.1, 0.3, 0.7, 1.3, 2.0]


def _oracle(img: np.ndarray, ks: int, sigma: float) -> np.ndarray:
    """fp64 2-D convolution with the outer-product kernel on the reflect-padded image."""
    r = (ks - 1) // 2
    x = torch.arange(ks, dtype=torch.float64) - r
    w = torch.exp(-0.5 * (x / sigma) ** 2)
    w = w / w.sum()
    k2 = torch.outer(w, w)
    t = torch.from_numpy(img.astype(np.float64)).permute(2, 0, 1)[None]
    t = F.pad(t, (r, r, r, r), mode="reflect")
    C = t.shape[1]
    y = F.conv2d(t, k2[None, None].repeat(C, 1, 1, 1), groups=C)
    return torch.round(y)[0].permute(1, 2, 0).numpy()


@pytest.mark.parametrize("H,W,ks", [(32, 32, 3), (24, 40, 5), (64, 64, 7), (80, 80, 9),
                                    (100, 72, 23), (224, 224, 23)])
def test_twin_matches_fp64_convolution(H, W, ks):
    rng = np.random.default_rng(H * 1000 + W + ks)
    img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    for sigma in SIGMAS:
        got = gaussian_blur(img, ks, sigma)
        assert got.dtype == np.float32 and got.shape == img.shape
        diff = np.abs(got.astype(np.float64) - _oracle(img, ks, sigma))
        share = float(np.mean(diff > 0))
        print(f"{H}x{W} ks {ks} sigma {sigma}: max diff {diff.max():.0f}, differing share {share:.2e}")
        assert diff.max() <= 1
        assert share <= 1e-3


def test_reflect_padding_by_hand():
    """A row that is 0 except 255 at column 1 (repeated down the image, so that the vertical pass
    sees constant columns): output column 0 takes the 255 twice, through the reflected index -1."""
    sigma = 1.0
    w = augment_ref.blur_weights(3, sigma)
    assert w.dtype == np.float32 and abs(float(w.sum()) - 1.0) < 1e-6 and w[0] == w[2]
    row = np.zeros(8, dtype=np.uint8)
    row[1] = 255
    img = np.tile(row, (6, 1))
    reflect = np.floor(np.float32(2.0) * w[0] * np.float32(255.0) + np.float32(0.5))
    zero_pad = np.floor(w[0] * np.float32(255.0) + np.float32(0.5))  # edge repeat gives the same
    assert reflect != zero_pad
    out = gaussian_blur(img, 3, sigma)
    assert (out[:, 0] == reflect).all()
    assert (out[:, 1] == np.floor(w[1] * np.float32(255.0) + np.float32(0.5))).all()
    assert (out[:, 2] == zero_pad).all() and (out[:, 3:] == 0).all()
    out_t = gaussian_blur(np.ascontiguousarray(img.T), 3, sigma)
    assert np.array_equal(out_t, out.T)


@pytest.mark.parametrize("ks", [3, 23])
def test_constant_image_stays_constant(ks):
    rng = np.random.default_rng(ks)
    for sigma in [0.1, 0.5, 1.0, 2.0]:
        for level in [0, 1, 127, 254, 255, int(rng.integers(2, 254))]:
            img = np.full((30, 26, 3), level, dtype=np.uint8)
            assert (gaussian_blur(img, ks, sigma) == level).all(), (sigma, level)


def test_gaussian_blur_rejects_bad_kernels():
    img = np.zeros((8, 8, 3), dtype=np.uint8)
    for ks in (0, 1, 4, 17):  # 17: half width 8 > 8 - 1
        with pytest.raises(ValueError):
            gaussian_blur(img, ks, 1.0)
    gaussian_blur(img, 15, 1.0)
    with pytest.raises(ValueError):
        augment_ref.check_blur_kernel(augment_ref.MAX_BLUR_KERNEL + 2, 224, 224)
    augment_ref.check_blur_kernel(augment_ref.MAX_BLUR_KERNEL, 224, 224)
    assert augment_ref.MAX_BLUR_KERNEL >= 23
    assert [augment_ref.default_blur_kernel(s) for s in (32, 64, 224)] == [3, 7, 23]


def test_sampling_blur_off_is_unchanged():
    """The sampler without blur against its recorded output (tests/golden, written by the code
    before the blur draws existed)."""
    rows = json.loads((ROOT / "tests" / "golden" / "augment_params_v1.json").read_text())
    assert len(rows) == 200
    for row in rows:
        key = image_key(row["seed"], row["counter"], row["view"], row["idx"])
        P = sample_params(Rng(key), row["H"], row["W"], row["strength"])
        assert P["blur"] is False and P["sigma"] == 0.0
        assert {k: P[k] for k in row["params"]} == row["params"]
        Q = sample_params(Rng(key), row["H"], row["W"], row["strength"], blur=True)
        assert {k: Q[k] for k in row["params"]} == row["params"]  # the blur draws come last


def test_sampling_blur_share_and_sigma():
    applied = 0
    for i in range(2000):
        P = sample_params(Rng(image_key(3, i // 50, i % 2, i)), 32, 32, 0.5, blur=True)
        assert isinstance(P["blur"], bool)
        assert 0.1 <= P["sigma"] <= 2.0
        assert np.float32(P["sigma"]) == P["sigma"]
        applied += P["blur"]
    assert abs(applied / 2000 - 0.5) <= 0.05


def test_loader_cpu_path_blurs_where_the_twin_says():
    from simclr_amd.data.datasets import synthetic_dataset
    from simclr_amd.data.loader import ContrastiveLoader
    ds = synthetic_dataset(32, 10)
    dev = torch.device("cpu")
    off = ContrastiveLoader(ds, 16, dev, seed=5)
    on = ContrastiveLoader(ds, 16, dev, seed=5, blur_kernel=3)
    idx = torch.arange(16)
    a, b = off.batch_from_indices(idx, 4), on.batch_from_indices(idx, 4)
    H, W = ds.images.shape[1:3]
    blurred = []
    for v in range(2):
        for i in range(16):
            P = sample_params(Rng(image_key(5, 4, v, i)), H, W, 0.5, blur=True)
            blurred.append(P["blur"])
            x, y = a[v * 16 + i], b[v * 16 + i]
            if not P["blur"]:
                assert torch.equal(x, y), (v, i)
                continue
            # blurred: exactly the twin's blur of the blur-off image (a sigma near 0.1 leaves
            # the centre tap alone, so only a sigma above 0.5 is required to change the image)
            pix = np.rint(x.numpy().transpose(1, 2, 0) * 255.0).astype(np.float32)
            want = gaussian_blur(pix, 3, P["sigma"]).transpose(2, 0, 1) / 255.0
            assert np.array_equal(y.numpy(), want.astype(np.float32)), (v, i)
            if P["sigma"] > 0.5:
                assert not torch.equal(x, y), (v, i, P)
    assert 8 <= sum(blurred) <= 24
    assert sum(1 for v in range(2) for i in range(16) if blurred[v * 16 + i]
               and not torch.equal(a[v * 16 + i], b[v * 16 + i])) >= 6
    with pytest.raises(ValueError):
        ContrastiveLoader(ds, 16, dev, blur_kernel=4)
    with pytest.raises(ValueError):
        ContrastiveLoader(ds, 16, dev, augment=False, blur_kernel=3)


def _cfg(overrides):
    from simclr_amd.config import CONF_DIR, compose, task_config
    return task_config(compose(str(CONF_DIR), "config", ["data.synthetic=true", *overrides]))


def test_configuration_keys():
    from simclr_amd.config import check_pretrain_conf, check_supervised_conf
    from simclr_amd.data.loader import blur_kernel_from_cfg
    cfg = _cfg([])
    check_pretrain_conf(cfg)
    assert blur_kernel_from_cfg(cfg, 32) == 0
    assert blur_kernel_from_cfg(_cfg(["data.blur_kernel=5"]), 32) == 0  # data.blur is the switch
    cfg = _cfg(["data.blur=true"])
    check_pretrain_conf(cfg)
    assert [blur_kernel_from_cfg(cfg, s) for s in (32, 64, 224)] == [3, 7, 23]
    cfg = _cfg(["data.blur=true", "data.blur_kernel=5"])
    check_pretrain_conf(cfg)
    assert blur_kernel_from_cfg(cfg, 32) == 5
    for bad in ("4", "-3", "1", str(augment_ref.MAX_BLUR_KERNEL + 2)):
        cfg = _cfg(["data.blur=true", f"data.blur_kernel={bad}"])
        with pytest.raises(AssertionError, match="data.blur_kernel"):
            check_pretrain_conf(cfg)
    sup = __import__("simclr_amd.config", fromlist=["compose"])
    scfg = sup.task_config(sup.compose(str(sup.CONF_DIR), "supervised_config",
                                       ["data.blur=true", "data.blur_kernel=6"]))
    with pytest.raises(AssertionError, match="data.blur_kernel"):
        check_supervised_conf(scfg)


@pytest.mark.timeout(600)
def test_cli_pretrains_with_blur(tmp_path):
    run = tmp_path / "run"
    r = subprocess.run([sys.executable, str(ROOT / "main.py"), "data.synthetic=true",
                        "data.synthetic_size=32", "experiment.batches=8",
                        "experiment.base_cnn=resnet18", "data.blur=true", "parameter.epochs=1",
                        f"hydra.run.dir={run}"], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = r.stdout + r.stderr
    assert "Epoch:1/1 progress:1.000 loss:" in out
    loss = float([l for l in out.splitlines() if "Epoch:1/1" in l][0].split("loss:")[1].split(",")[0])
    assert loss == loss and abs(loss) < 100
