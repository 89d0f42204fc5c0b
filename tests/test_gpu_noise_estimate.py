"""GPU tests of bf_noise_estimate (csrc/noise_estimate.hip), blind_image_denoising_amd.noise_estimate and evaluate_blind.

Yardstick: tests/noise_reference.py, the NumPy int64 / float64 restatement of the three statistics, computed once per case.

Bounds.  uint8: S, the histogram and the clipped count are integer sums, so S and the count must be EQUAL; sigma_fast and sigma_mad
are one fp64 formula of a few operations on those identical integers: 1e-12 relative.  float32: the terms |L| are non-negative and
fewer than 1e5 at these shapes, summed in double in another order than NumPy's: n 2^-53 = 1.1e-11 bounds the relative reordering
error; the bar is 1e-10.

The kernel's tile is 32 rows (a workgroup's band; 8 rows per wave) x 64 pixel columns.  The shapes are the smallest that cross every
boundary it has: below a tile (3 x 3, 4 x 5), odd both ways across a band and a wave boundary (37 x 53), four column tiles plus one
column and a full second band (64 x 257), two band boundaries with a last band of 6 rows and a column tile that ends on a cell
(70 x 66), one row and one column past a tile (33 x 65), and every channel count."""
import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import _native as N
from oracle import bfcnn_oracle as O
import noise_reference as R
from guarded import dev as _dev, guard_bands

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guard_bands")]

SHAPES = [(1, 3, 3, 1), (2, 4, 5, 3), (1, 37, 53, 3), (3, 64, 257, 4), (2, 70, 66, 3), (1, 33, 65, 1), (2, 9, 130, 2)]
_ids = {"ids": lambda s: "x".join(map(str, s))}


def _check_u8(images: np.ndarray, what: str):
    got = bf.noise_statistics(_dev(images))
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (images.shape[0], images.shape[3], 4)
    got, ref = got.cpu().numpy(), R.noise_statistics(images)
    assert np.array_equal(got[:, :, 0], ref[:, :, 0]), f"{what}: S"
    assert np.array_equal(got[:, :, 3], ref[:, :, 3]), f"{what}: clipped count"
    for slot, name in ((1, "sigma_fast"), (2, "sigma_mad")):
        dev = float((np.abs(got[:, :, slot] - ref[:, :, slot]) / np.maximum(np.abs(ref[:, :, slot]), 1e-300)).max())
        print(f"{what} {name}: reference {ref[0, 0, slot]:.6f}, max relative deviation {dev:.3e}")
        assert dev <= 1e-12, f"{what}: {name}"
    return got


@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_uint8_random_bytes_match_numpy(shape):
    images = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    images[0, 0, 0, 0], images[-1, -1, -1, -1] = 255, 0                           # the corners count, once
    _check_u8(images, "x".join(map(str, shape)))


def test_uint8_saturated_regions_and_noise_match_numpy():
    rng = np.random.default_rng(11)
    images = rng.integers(0, 256, (2, 70, 131, 3), dtype=np.uint8)
    images[0, 10:45, 20:100] = 255                                               # a blown-out region across band and tile boundaries
    images[0, 50:, :30] = 0
    images[1, :, :, 1] = 255
    images[1, 31:33, :, 2] = 0
    got = _check_u8(images, "saturated")
    assert got[1, 1, 0] == 0 and got[1, 1, 2] == 0 and got[1, 1, 3] == 70 * 131    # a constant plane: all mass in bin 0
    # flat grey + Gaussian noise: the histogram is narrow, many lanes of a wave hit the same LDS bin
    for sigma in (0.3, 2.0, 25.0, 90.0):
        noisy = np.clip(np.round(128.0 + rng.normal(0.0, sigma, (1, 67, 200, 3))), 0, 255).astype(np.uint8)
        _check_u8(noisy, f"sigma {sigma}")
    for value in (0, 77, 255):
        got = _check_u8(np.full((1, 35, 66, 4), value, np.uint8), f"constant {value}")
        assert (got[:, :, :3] == 0).all() and (got[:, :, 3] == (35 * 66 if value in (0, 255) else 0)).all()
    checker = np.zeros((1, 34, 70, 1), np.uint8)                                  # the largest |L| = 2040 and q = 510 everywhere
    checker[0, 0::2, 0::2] = 255
    checker[0, 1::2, 1::2] = 255
    got = _check_u8(checker, "checkerboard")
    assert got[0, 0, 0] == 2040 * 32 * 68 and got[0, 0, 3] == 34 * 70


@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_float32_immerkaer_matches_numpy(shape):
    rng = np.random.default_rng(100 + sum(shape))
    images = (rng.uniform(0.0, 255.0, shape) + rng.normal(0.0, 10.0, shape)).astype(np.float32)
    got = bf.noise_statistics(_dev(images)).cpu().numpy()
    ref = R.noise_statistics(images)
    for slot in (0, 1):
        dev = float((np.abs(got[:, :, slot] - ref[:, :, slot]) / np.abs(ref[:, :, slot])).max())
        print(f"float32 {shape} slot {slot}: max relative deviation {dev:.3e}")
        assert dev <= 1e-10
    assert np.isnan(got[:, :, 2]).all() and np.isnan(got[:, :, 3]).all()
    sigma = bf.estimate_noise(_dev(images), method="immerkaer")
    assert np.allclose(sigma.cpu().numpy(), R.combine_channels(ref[:, :, 1]), rtol=1e-10, atol=0)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["uint8", "float32"])
def test_planes_do_not_depend_on_their_batch(dtype):
    """image b, channel c inside a batch = that plane evaluated alone, bit for bit; and two calls return the same bits"""
    images = np.random.default_rng(5).integers(0, 256, (3, 70, 131, 3)).astype(dtype)
    if dtype == np.float32:
        images += np.random.default_rng(6).uniform(-0.5, 0.5, images.shape).astype(np.float32)
    t = _dev(images)
    whole = bf.noise_statistics(t).cpu().numpy()
    assert np.array_equal(bf.noise_statistics(t).cpu().numpy().view(np.uint64), whole.view(np.uint64))
    for b in range(3):
        for c in range(3):
            alone = bf.noise_statistics(_dev(images[b:b + 1, :, :, c:c + 1])).cpu().numpy()
            assert np.array_equal(alone[0, 0].view(np.uint64), whole[b, c].view(np.uint64)), (b, c)


def test_estimate_noise_and_summary():
    rng = np.random.default_rng(8)
    images = np.clip(np.round(100.0 + rng.normal(0.0, [[[[5.0, 10.0, 20.0]]]], (2, 64, 96, 3))), 0, 255).astype(np.uint8)
    ref = R.noise_statistics(images)
    for method, slot in (("mad", 2), ("immerkaer", 1)):
        per_channel = bf.estimate_noise(images, method=method, per_channel=True)                 # NumPy in, NumPy out
        assert isinstance(per_channel, np.ndarray) and per_channel.shape == (2, 3)
        assert np.allclose(per_channel, ref[:, :, slot], rtol=1e-12, atol=0)
        assert np.all(np.abs(per_channel / np.sqrt(np.array([5.0, 10.0, 20.0]) ** 2 + 1.0 / 12.0) - 1.0) < 0.1)
        combined = bf.estimate_noise(_dev(images), method=method)
        assert combined.is_cuda and tuple(combined.shape) == (2,)
        assert np.allclose(combined.cpu().numpy(), R.combine_channels(ref[:, :, slot]), rtol=1e-12, atol=0)
    summary = bf.noise_summary(images)
    assert isinstance(summary, bf.NoiseEstimate) and np.allclose(summary.sigma_fast, ref[:, :, 1], rtol=1e-12, atol=0)
    assert np.allclose(summary.sigma_mad, ref[:, :, 2], rtol=1e-12, atol=0) and np.array_equal(summary.clipped_fraction, ref[:, :, 3] / (64 * 96))
    assert np.array_equal(bf.noise_summary(np.full((1, 8, 8, 1), 255, np.uint8)).clipped_fraction, [[1.0]])


def test_empty_batch_returns_without_a_launch():
    out = bf.noise_statistics(torch.zeros((0, 16, 16, 3), dtype=torch.uint8, device="cuda"))
    assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (0, 3, 4)


def test_entry_point_refuses_bad_arguments():
    lib = N.lib()
    images = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    nbytes = lib.bf_noise_estimate_scratch_bytes(1, 8, 8, 3)
    scratch = torch.zeros(nbytes // 8 + 1, dtype=torch.float64, device="cuda")
    out = torch.zeros((1, 3, 4), dtype=torch.float64, device="cuda")
    s = N.stream_ptr(images)
    assert lib.bf_noise_estimate(N.ptr(images), N.BF_DTYPE_U8, 1, 8, 8, 3, N.ptr(scratch), nbytes, N.ptr(out), s) == N.BF_OK
    assert lib.bf_noise_estimate(N.ptr(images), N.BF_DTYPE_U8, 1, 8, 8, 3, N.ptr(scratch), nbytes - 8, N.ptr(out), s) == N.BF_EINVAL
    assert lib.bf_noise_estimate(N.ptr(images), N.BF_DTYPE_U8, 1, 8, 8, 3, scratch.data_ptr() + 4, nbytes, N.ptr(out), s) == N.BF_EINVAL
    assert lib.bf_noise_estimate(N.ptr(images), 2, 1, 8, 8, 3, N.ptr(scratch), nbytes, N.ptr(out), s) == N.BF_EINVAL
    assert lib.bf_noise_estimate(None, N.BF_DTYPE_U8, 1, 8, 8, 3, N.ptr(scratch), nbytes, N.ptr(out), s) == N.BF_EINVAL
    assert lib.bf_noise_estimate(N.ptr(images), N.BF_DTYPE_U8, 1, 2, 32, 3, N.ptr(scratch), nbytes, N.ptr(out), s) == N.BF_EINVAL
    torch.cuda.synchronize()
    assert (out.cpu().numpy()[:, :, :3] == 0).all() and (out.cpu().numpy()[:, :, 3] == 64).all()


# ---- evaluate_blind ----------------------------------------------------------------------------------------------------------

class _Recording:
    def __init__(self, module):
        self.module, self.noisy, self.denoised = module, [], []

    def check_status(self, wait=True):
        return self.module.check_status(wait)

    def __call__(self, x):
        assert x.is_cuda and x.dtype == torch.uint8
        out = self.module(x)
        self.noisy.append(x.cpu().numpy())
        self.denoised.append(out.cpu().numpy())
        return out


_HYDRA = []


def _resnet():
    if not _HYDRA:
        cfg = O.canonical_config(no_layers=6)
        params, state = O.init_params(O.ResnetSpec.from_config(cfg["model"]), seed=42)
        m = bf.model_builder(cfg["model"], device="cuda").hydra
        m.set_weights(params, state)
        _HYDRA.append(m)
    return _HYDRA[0]


_KEYS = {"sigma_in", "sigma_out", "removed_rms", "ratio", "clipped_fraction"}


def _reference_rows(noisy, denoised, slot):
    """per image (sigma_in, sigma_out, removed_rms, ratio, clipped_fraction) from host arrays"""
    s_in, s_out = R.noise_statistics(noisy), R.noise_statistics(denoised)
    sigma_in, sigma_out = R.combine_channels(s_in[:, :, slot]), R.combine_channels(s_out[:, :, slot])
    d = noisy.astype(np.int64) - denoised.astype(np.int64)
    removed = np.sqrt((d * d).sum(axis=(1, 2, 3)) / float(np.prod(noisy.shape[1:])))
    return {"sigma_in": sigma_in, "sigma_out": sigma_out, "removed_rms": removed, "ratio": removed / sigma_in,
            "clipped_fraction": s_in[:, :, 3].sum(axis=1) / float(np.prod(noisy.shape[1:]))}


@pytest.mark.parametrize("method,slot", [("mad", 2), ("immerkaer", 1)])
def test_evaluate_blind_reports_what_the_arrays_say(method, slot):
    rec = _Recording(bf.DenoiserModule(_resnet()))
    _, n0 = O.synthetic_batch(2, 64, 64, seed=1)
    _, n1 = O.synthetic_batch(1, 40, 72, sigma=40.0, seed=2)                      # two shapes in one call
    n0, n1 = n0.astype(np.uint8), n1.astype(np.uint8)
    report = bf.evaluate_blind(rec, [n0, _dev(n1)], method=method)
    assert set(report) == {"method", "images", "batches", "aggregate"} and report["method"] == method and report["images"] == 3
    assert len(rec.noisy) == 2 and np.array_equal(rec.noisy[0], n0) and np.array_equal(rec.noisy[1], n1)
    refs = [_reference_rows(x, y, slot) for x, y in zip(rec.noisy, rec.denoised)]
    for row, ref, x in zip(report["batches"], refs, rec.noisy):
        assert set(row) == _KEYS | {"shape", "images"} and row["shape"] == list(x.shape) and row["images"] == x.shape[0]
        for k in _KEYS:
            print(f"{method} batch {row['shape']} {k}: {row[k]:.12f} reference {ref[k].mean():.12f}")
            assert abs(row[k] - ref[k].mean()) <= 1e-12 * max(1.0, abs(ref[k].mean())), k
    agg = report["aggregate"]
    assert set(agg) == _KEYS | {"images"} and agg["images"] == 3
    for k in _KEYS:
        every = np.concatenate([r[k] for r in refs])
        assert abs(agg[k] - every.mean()) <= 1e-12 * max(1.0, abs(every.mean())), k
    # removed_rms is sqrt of the MSE image_metrics reports for the same pair
    mse = bf.image_metrics(rec.noisy[0], rec.denoised[0]).mse
    assert abs(report["batches"][0]["removed_rms"] - np.sqrt(mse).mean()) <= 1e-12 * np.sqrt(mse).mean()
    assert 5.0 < report["batches"][0]["sigma_in"] < 40.0                          # sigma 20 truncated at 2 sigma, on a smooth field
    text = bf.noise_estimate.format_blind_report(report)
    assert len(text.splitlines()) == 5 and method in text.splitlines()[0]
    assert bf.metrics.json_safe(report) == report                                 # finite throughout


def test_evaluate_blind_accepts_every_module():
    _, noisy = O.synthetic_batch(2, 64, 64, seed=1)
    noisy = noisy.astype(np.uint8)
    plain = bf.evaluate_blind(bf.DenoiserModule(_resnet()), [noisy])
    for module in (bf.GraphedDenoiserModule(bf.DenoiserModule(_resnet())), bf.SelfEnsembleDenoiserModule(bf.DenoiserModule(_resnet()))):
        report = bf.evaluate_blind(module, [noisy])
        assert set(report) == set(plain) and report["images"] == 2 and len(report["batches"]) == 1
        assert set(report["batches"][0]) == set(plain["batches"][0]) and set(report["aggregate"]) == set(plain["aggregate"])
        assert all(np.isfinite(v) for k, v in report["aggregate"].items())
        assert report["aggregate"]["sigma_in"] == plain["aggregate"]["sigma_in"]             # the same frames went in
        assert report["aggregate"]["clipped_fraction"] == plain["aggregate"]["clipped_fraction"]
    graphed = bf.evaluate_blind(bf.GraphedDenoiserModule(bf.DenoiserModule(_resnet())), [noisy])
    assert graphed == plain                                                      # a replayed graph runs the same kernels
    identity = bf.evaluate_blind(lambda x: x, [noisy])
    assert identity["aggregate"]["removed_rms"] == 0.0 and identity["aggregate"]["ratio"] == 0.0
    assert identity["aggregate"]["sigma_out"] == identity["aggregate"]["sigma_in"]
