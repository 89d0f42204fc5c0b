"""GPU parity of the pyramid / resampling kernels: oracle + golden fixtures + the reference's own
round-trip identity (tests/bfcnn/test_pyramid.py) on its own fixture image."""
import pathlib

import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import pyramid as P
from oracle import bfcnn_oracle as O
from guarded import dev as _dev, dev_f32 as _d, guard_bands

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guard_bands")]
G = pathlib.Path(__file__).resolve().parent / "golden"


def test_golden_resampling():
    z = np.load(G / "pyramid.npz")
    x = _d(z["x"])
    assert np.abs(P.upsample_2x(x).cpu().numpy() - z["up_bilinear"]).max() < 1e-6
    assert np.array_equal(P.upsample_2x(x, bilinear=False).cpu().numpy(), z["up_nearest"].astype(np.float32))
    assert np.array_equal(P.strided_slice_2(x).cpu().numpy(), z["slice2"].astype(np.float32))
    assert np.abs(P.avg_pool2_valid(x).cpu().numpy() - z["pool_valid"]).max() < 1e-6
    for k in (2, 3, 5):
        assert np.abs(P.avg_pool_s2_same(x, (k, k)).cpu().numpy() - z[f"pool{k}"]).max() < 1e-6


@pytest.mark.parametrize("shape", [(1, 7, 9, 3), (2, 16, 16, 4), (1, 33, 18, 16), (1, 1, 1, 1), (3, 2, 5, 8)])
@pytest.mark.parametrize("k", [(2, 2), (3, 3), (5, 5), (3, 5)])
def test_avgpool_and_upsample_vs_oracle(shape, k):
    x = np.random.default_rng(sum(shape)).standard_normal(shape)
    xd = _d(x)
    assert np.abs(P.avg_pool_s2_same(xd, k).cpu().numpy() - O.avg_pool_same(x, k, 2)).max() < 2e-6
    assert np.abs(P.upsample_2x(xd).cpu().numpy() - O.upsample_bilinear_2x(x)).max() < 2e-6
    other = np.random.default_rng(1).standard_normal((shape[0], 2 * shape[1], 2 * shape[2], shape[3]))
    got = P.upsample_2x(xd, _d(other), True, -1.0, 1.0).cpu().numpy()
    assert np.abs(got - (other - O.upsample_bilinear_2x(x))).max() < 4e-6


def test_multiscales_ground_truth_pyramid():
    x = np.random.default_rng(0).uniform(-10, 270, (2, 17, 20, 3))
    got = P.multiscales_generator_fn(no_scales=2, clip_values=True, round_values=True)(_d(x))
    ref = O.multiscales(x.astype(np.float32).astype(np.float64), 2)
    assert len(got) == 3
    for g, r in zip(got[1:], ref[1:]):
        d = np.abs(g.cpu().numpy() - r)
        assert d.max() <= 1.0 and (d > 0).mean() < 0.01       # rounding ties may flip by one level


def _lena(size, channels):
    from PIL import Image
    im = Image.open(G / "lena.jpg").convert("L" if channels == 1 else "RGB").resize((size, size), Image.BILINEAR)
    return (np.asarray(im, dtype=np.float32).reshape(1, size, size, channels) / 255.0 - 0.5).astype(np.float32)


@pytest.mark.parametrize("ptype", [None, "laplacian", "gaussian"])
@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("size", [64, 128, 256, 512, 1024])
def test_pyramid_round_trip_reference_identity(ptype, levels, channels, size):
    """tests/bfcnn/test_pyramid.py:22-409 verbatim in intent: same configs, same fixture, same bound."""
    if ptype is None:
        cfg, levels = None, 1
    else:
        cfg = {"levels": levels, "type": ptype, "kernel_size": (3, 3), "xy_max": (1.0, 1.0)}
    shape = (None, None, channels)
    pyr_model = bf.build_pyramid_model(input_dims=shape, config=cfg)
    inv_model = bf.build_inverse_pyramid_model(input_dims=shape, config=cfg)
    x = _lena(size, channels)
    x_pyramid = pyr_model.predict(x)
    assert len(x_pyramid) == levels
    x_recovered = inv_model.predict(x_pyramid)
    assert x_recovered.shape == x.shape
    assert np.mean(np.abs(x_recovered - x)) < 1e-7
    if ptype is not None and levels == 3 and size == 64:
        ref = O.build_pyramid(cfg)(x.astype(np.float64))
        for g, r in zip(x_pyramid, ref):
            assert np.abs(g - r).max() < 2e-6


def test_config5_scale_laplacian_split_merge():
    """BASELINE.json config 5 shape (batch 32, 512x512x3, 3 scales): round trip + linearity."""
    x = torch.rand((32, 512, 512, 3), device="cuda") - 0.5
    cfg = {"levels": 3, "type": "laplacian"}
    pyr = bf.build_pyramid_model((None, None, 3), cfg)(x)
    assert [tuple(p.shape[1:3]) for p in pyr] == [(512, 512), (256, 256), (128, 128)]
    rec = bf.build_inverse_pyramid_model((None, None, 3), cfg)(pyr)
    assert (rec - x).abs().mean().item() < 1e-7
    pyr2 = bf.build_pyramid_model((None, None, 3), cfg)(2.0 * x)       # the split is linear
    assert all((a * 2.0 - b).abs().max().item() < 1e-5 for a, b in zip(pyr, pyr2))


@pytest.mark.parametrize("seed", range(int(__import__("os").environ.get("BF_SWEEP_N", 40))))
def test_random_pyramid_configurations_match_oracle(seed):
    """a seeded sweep over the pyramid builder's options and ragged shapes (both types, 1-4 levels, square and rectangular pooling
    windows, 1 / 3 / 16 channels, batches, sizes that are multiples of 2^(levels-1) but otherwise arbitrary): every level against the
    oracle, the round trip, and device-tensor in / out"""
    rng = np.random.default_rng(13000 + seed)
    levels = int(rng.integers(1, 5))
    step = 2 ** (levels - 1)
    H, W = step * int(rng.integers(1, 40)), step * int(rng.integers(1, 40))
    C, B = int(rng.choice([1, 3, 16])), int(rng.integers(1, 4))
    ptype = str(rng.choice(["laplacian", "gaussian"]))
    k = (int(rng.choice([2, 3, 4, 5, 7])), int(rng.choice([2, 3, 4, 5, 7])))
    cfg = {"levels": levels, "type": ptype, "kernel_size": k}
    x = rng.uniform(-0.5, 0.5, (B, H, W, C)).astype(np.float32)
    pyr = bf.build_pyramid_model((None, None, C), cfg)
    inv = bf.build_inverse_pyramid_model((None, None, C), cfg)
    got = pyr.predict(x)
    ref = O.build_pyramid(cfg)(x.astype(np.float64))
    assert len(got) == len(ref) == levels
    for g, r in zip(got, ref):
        assert g.shape == r.shape and np.abs(g - r).max() < 3e-6, (cfg, x.shape)
    rec = inv.predict(got)
    want = O.build_inverse_pyramid(cfg)(ref)
    assert rec.shape == want.shape and np.abs(rec - want).max() < 5e-6
    if ptype == "laplacian":
        assert np.abs(rec - x).mean() < 1e-7
    xd = _dev(x)
    assert all(torch.equal(a, _dev(b)) for a, b in zip(pyr(xd), got))


@pytest.mark.parametrize("shape", [(2, 64, 64, 3), (1, 512, 512, 3), (3, 40, 56, 3), (2, 18, 20, 1), (1, 96, 130, 2), (2, 32, 48, 4),
                                   (1, 2, 4, 3), (2, 70, 36, 6), (1, 300, 260, 3)])
@pytest.mark.parametrize("k", [(5, 5), (3, 3), (7, 7), (3, 5), (5, 2)])
def test_fused_laplacian_split_is_bitwise_the_two_kernels(shape, k):
    """bf_laplacian_split (one kernel per level: x read once) against the two operators it replaces -- bitwise -- and against the
    oracle; shapes around every chunk / band boundary of the kernel, one-band and one-chunk images, all window sizes."""
    from blind_image_denoising_amd import _native as N
    x = _dev(np.random.default_rng(sum(shape) + k[0]).standard_normal(shape).astype(np.float32))
    B, H, W, C = shape
    down_f = torch.full((B, H // 2, W // 2, C), float("nan"), device="cuda")
    lap_f = torch.full(shape, float("nan"), device="cuda")
    rc = N.lib().bf_laplacian_split(N.ptr(x), N.ptr(down_f), N.ptr(lap_f), B, H, W, C, k[0], k[1], N.stream_ptr(x))
    down = P.avg_pool_s2_same(x, k)
    lap = P.upsample_2x(down, x, True, -1.0, 1.0)
    if rc == N.BF_EUNSUPPORTED:
        assert (W * C) % 4 != 0 or k[1] < 2 or C % 4 == 0
        d2, l2 = P.laplacian_split(x, k)                      # falls back to the two operators
        assert torch.equal(d2, down) and torch.equal(l2, lap)
        return
    assert rc == N.BF_OK
    assert torch.equal(down_f, down) and torch.equal(lap_f, lap)
    x64 = x.cpu().numpy().astype(np.float64)
    rd = O.avg_pool_same(x64, k)
    assert np.abs(down_f.cpu().numpy() - rd).max() < 1e-5
    assert np.abs(lap_f.cpu().numpy() - (x64 - O.upsample_bilinear_2x(rd))).max() < 1e-5


@pytest.mark.parametrize("shape", [(2, 32, 32, 3), (1, 256, 256, 3), (3, 20, 28, 3), (2, 9, 10, 1), (1, 48, 65, 2), (1, 1, 2, 3), (2, 35, 18, 6),
                                   (1, 150, 130, 3)])
@pytest.mark.parametrize("with_other", [True, False])
def test_upsample_band_kernel_is_bitwise_the_row_kernel(shape, with_other):
    """bf_upsample2x on C % 4 != 0 maps: the row-walking 16-byte kernel (default) against the 4-byte row kernel -- bitwise -- and the
    oracle; the merge step of the inverse Laplacian pyramid (alpha = beta = 1) and the bare up-sampling, shapes around the chunk / band
    boundaries."""
    from blind_image_denoising_amd import _native as N
    rng = np.random.default_rng(sum(shape))
    x = _dev(rng.standard_normal(shape).astype(np.float32))
    B, H, W, C = shape
    other = _dev(rng.standard_normal((B, 2 * H, 2 * W, C)).astype(np.float32)) if with_other else None
    got = P.upsample_2x(x, other, True, 0.5 if not with_other else 1.0, 1.0)
    N.lib().bf_debug_set_upsample_band(0)
    try:
        ref_rows = P.upsample_2x(x, other, True, 0.5 if not with_other else 1.0, 1.0)
    finally:
        N.lib().bf_debug_set_upsample_band(1)
    assert torch.equal(got, ref_rows)
    up = O.upsample_bilinear_2x(x.cpu().numpy().astype(np.float64))
    want = up + other.cpu().numpy() if with_other else 0.5 * up
    assert np.abs(got.cpu().numpy() - want).max() < 1e-5
