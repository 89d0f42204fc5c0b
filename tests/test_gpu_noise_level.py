"""GPU tests of bf_noise_level (csrc/noise_level.hip), bf_op_camera_noise_u8 (csrc/augment.hip), bf_op_risk_sums_affine
(csrc/risk.hip) and their host sides, blind_image_denoising_amd.noise_level and the affine entries of .risk.

Yardstick: tests/noise_level_reference.py, the NumPy restatement (int64 cells and histograms, fp64 everything else, Philox from the
oracle), computed once per case.

Bounds.
  bf_noise_level   n, the sums of s and the excluded counts are integer sums: EQUAL.  sigma_l is one fp64 formula of a few
                   operations on identical integers: 1e-12 relative, the bar of tests/test_gpu_noise_estimate.py for the same formula.
  the fit          sixteen numbers per plane in fp64, the same centred sums in torch and in NumPy: 1e-10 relative.
  camera noise     the kernel forms z in float32 (logf, cosf), the reference in fp64: z moves by about 1e-6 relative, so only a value
                   within about 1e-4 of a half-integer can round the other way (about 0.02 % of the samples).  No sample may differ by
                   more than one grey level, at most 0.1 % may differ at all.
  affine sums      R and D_p carry THE BITS of bf_op_risk_sums; Y is an integer: EQUAL.  Dy_p: fewer than 1e5 fp64 terms per image and
                   channel, added in another order than NumPy's: 1e-10 on the scale of the terms, sum y |f_p - f_0|, the bar
                   test_gpu_risk.py::test_sums_match_the_reference uses for D_p on sum |f_p - f_0|.
  end to end       1e-9 relative against the NumPy chain, as the blur case of tests/test_gpu_risk.py.

Shapes.  bf_noise_level has the tile of bf_noise_estimate (32 rows x 64 pixel columns, 8 rows per wave, 2 x 2 cells): the shapes of
tests/test_gpu_noise_estimate.py cross every boundary of it.  The camera noise and the sums walk an image by its flat element in
groups of four: one element, 90 elements unaligned, unaligned across a workgroup, aligned with two and with four channels."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import _native as N
from oracle import bfcnn_oracle as O
import noise_level_reference as L
import risk_reference as RR
from guarded import dev as _dev, guard_bands

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guard_bands")]

LEVEL_SHAPES = [(1, 3, 3, 1), (2, 4, 5, 3), (1, 37, 53, 3), (3, 64, 257, 4), (2, 70, 66, 3), (1, 33, 65, 1), (2, 9, 130, 2)]
NOISE_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 3), (1, 33, 65, 3), (2, 9, 130, 2), (3, 64, 257, 4)]
SUMS_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 3), (1, 37, 53, 3), (2, 9, 130, 2), (2, 65, 65, 1), (3, 64, 257, 4)]
PROBES = [1, 3, 8]
_ids = {"ids": lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else f"K{s}"}


# ---- 1. bf_noise_level -------------------------------------------------------------------------------------------------------

def _check_levels(images: np.ndarray, what: str):
    levels, excluded = bf.noise_level_statistics(_dev(images))
    B, C = images.shape[0], images.shape[3]
    assert levels.is_cuda and levels.dtype == torch.float64 and tuple(levels.shape) == (B, C, 16, 3)
    assert excluded.is_cuda and excluded.dtype == torch.float64 and tuple(excluded.shape) == (B, C)
    levels, excluded = levels.cpu().numpy(), excluded.cpu().numpy()
    ref_levels, ref_excluded = L.noise_level_statistics(images)
    assert np.array_equal(levels[..., 0], ref_levels[..., 0]), f"{what}: n"
    assert np.array_equal(levels[..., 1], ref_levels[..., 1]), f"{what}: sum of s"
    assert np.array_equal(excluded, ref_excluded), f"{what}: excluded"
    dev = float((np.abs(levels[..., 2] - ref_levels[..., 2]) / np.maximum(np.abs(ref_levels[..., 2]), 1e-300)).max())
    print(f"{what}: {int((ref_levels[..., 0] > 0).sum())} levels in use, sigma_l max relative deviation {dev:.3e}")
    assert dev <= 1e-12, f"{what}: sigma_l"
    assert (levels[..., 0].sum(axis=2) + excluded == (images.shape[1] // 2) * (images.shape[2] // 2)).all()
    return levels, excluded


@pytest.mark.parametrize("shape", LEVEL_SHAPES, **_ids)
def test_levels_of_random_bytes_and_of_noise_match_numpy(shape):
    rng = np.random.default_rng(sum(shape))
    images = rng.integers(0, 256, shape, dtype=np.uint8)
    images[0, 0, 0, 0], images[-1, -1, -1, -1] = 255, 0
    _check_levels(images, "x".join(map(str, shape)) + " random")
    # a ramp that visits all 16 levels, with a little noise; no sample is saturated
    ramp = np.linspace(4.0, 251.0, shape[2])[None, None, :, None] + rng.normal(0.0, 1.0, shape)
    levels, excluded = _check_levels(np.clip(np.rint(ramp), 1, 254).astype(np.uint8), "x".join(map(str, shape)) + " ramp")
    assert (excluded == 0).all()
    if shape[2] >= 130 and shape[1] >= 9:
        assert (levels[..., 0] > 0).all()                                         # every level holds cells


def test_levels_of_saturated_flat_and_constant_images_match_numpy():
    rng = np.random.default_rng(11)
    images = rng.integers(0, 256, (2, 70, 131, 3), dtype=np.uint8)
    images[0, 10:45, 20:100] = 255                                               # a blown-out region across band and tile boundaries
    images[0, 50:, :30] = 0                                                      # a black one
    images[1, :, :, 1] = 255
    images[1, 31:33, :, 2] = 0                                                   # one row of each of two wave bands
    levels, excluded = _check_levels(images, "saturated")
    assert excluded[1, 1] == 35 * 65 and (levels[1, 1] == 0).all()
    # flat grey + Gaussian noise: one or two levels, a narrow histogram: many lanes of a wave hit the same LDS bin
    for sigma in (0.3, 2.0, 25.0, 90.0):
        noisy = np.clip(np.round(128.0 + rng.normal(0.0, sigma, (1, 67, 200, 3))), 0, 255).astype(np.uint8)
        _check_levels(noisy, f"sigma {sigma}")
    for value in (0, 77, 255):
        levels, excluded = _check_levels(np.full((1, 35, 66, 4), value, np.uint8), f"constant {value}")
        if value == 77:
            assert (excluded == 0).all() and (levels[0, :, 4] == (17 * 33, 308 * 17 * 33, 0.0)).all() and levels[..., 0].sum() == 4 * 17 * 33
        else:
            assert (excluded == 17 * 33).all() and (levels == 0).all()
    checker = np.zeros((1, 34, 70, 1), np.uint8)                                  # 0 and 255: every cell is excluded
    checker[0, 0::2, 0::2] = 255
    checker[0, 1::2, 1::2] = 255
    levels, excluded = _check_levels(checker, "checkerboard")
    assert excluded[0, 0] == 17 * 35 and (levels == 0).all()


def test_levels_of_an_image_do_not_depend_on_its_batch():
    """image b, channel c inside a batch = that plane evaluated alone, bit for bit; and two calls return the same bits"""
    images = np.random.default_rng(5).integers(0, 256, (3, 70, 131, 3), dtype=np.uint8)
    images[1] = np.clip(np.rint(100.0 + np.random.default_rng(6).normal(0.0, 6.0, images[1].shape)), 0, 255)
    t = _dev(images)
    whole = [v.cpu().numpy() for v in bf.noise_level_statistics(t)]
    again = [v.cpu().numpy() for v in bf.noise_level_statistics(t)]
    assert all(np.array_equal(a.view(np.uint64), w.view(np.uint64)) for a, w in zip(again, whole))
    for b in range(3):
        for c in range(3):
            levels, excluded = bf.noise_level_statistics(_dev(images[b:b + 1, :, :, c:c + 1]))
            assert np.array_equal(levels.cpu().numpy()[0, 0].view(np.uint64), whole[0][b, c].view(np.uint64)), (b, c)
            assert excluded.cpu().numpy()[0, 0] == whole[1][b, c]


def test_noise_level_entry_refuses_bad_arguments():
    lib = N.lib()
    img = torch.full((1, 8, 8, 3), 9, dtype=torch.uint8, device="cuda")
    nbytes = lib.bf_noise_level_scratch_bytes(1, 8, 8, 3)
    assert nbytes == (3 * 16 * 512 + 3) * 8
    scratch = torch.zeros(nbytes // 8 + 1, dtype=torch.float64, device="cuda")
    levels = torch.zeros((1, 3, 16, 3), dtype=torch.float64, device="cuda")
    excluded = torch.ones((1, 3), dtype=torch.float64, device="cuda")
    s = N.stream_ptr(img)
    call = lambda im=N.ptr(img), B=1, H=8, W=8, C=3, sc=N.ptr(scratch), nb=nbytes, lv=N.ptr(levels), ex=N.ptr(excluded): \
        lib.bf_noise_level(im, B, H, W, C, sc, nb, lv, ex, s)
    assert call() == N.BF_OK
    for kw in ({"im": None}, {"sc": None}, {"lv": None}, {"ex": None}, {"B": 0}, {"H": 2}, {"W": 2}, {"C": 0}, {"C": 5}, {"nb": nbytes - 8},
               {"sc": scratch.data_ptr() + 4}, {"lv": levels.data_ptr() + 4}, {"ex": excluded.data_ptr() + 4}):
        assert call(**kw) == N.BF_EINVAL, kw
    for shape in ((0, 8, 8, 3), (1, 2, 8, 3), (1, 8, 8, 5), (1, 8, 2, 3)):
        assert lib.bf_noise_level_scratch_bytes(*shape) == N.BF_EINVAL
    torch.cuda.synchronize()
    assert (excluded.cpu().numpy() == 0).all() and (levels.cpu().numpy()[0, :, 0] == (16.0, 16.0 * 36.0, 0.0)).all()
    with pytest.raises(RuntimeError, match="MI355X"):
        bf.noise_level_statistics(torch.zeros((1, 8, 8, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        bf.noise_level_statistics(torch.zeros((1, 8, 8, 3), device="cuda"))


# ---- 2. the fit --------------------------------------------------------------------------------------------------------------

def _check_fit(images: np.ndarray, what: str, min_cells: int = 64):
    nlf = bf.noise_level_function(_dev(images), min_cells=min_cells)
    assert isinstance(nlf, bf.NoiseLevelFunction) and all(v.is_cuda and v.dtype == torch.float64 for v in nlf)
    B, H, W, C = images.shape
    assert [tuple(v.shape) for v in nlf] == [(B, C)] * 2 + [(B, C, 16)] * 3 + [(B, C)]
    gain, offset = L.noise_level_function(images, min_cells)
    got_gain, got_offset = nlf.gain.cpu().numpy(), nlf.offset.cpu().numpy()
    print(f"{what}: gain {got_gain.ravel()} (reference {gain.ravel()}), offset {got_offset.ravel()} (reference {offset.ravel()})")
    assert np.allclose(got_gain, gain, rtol=1e-10, atol=0) and np.allclose(got_offset, offset, rtol=1e-10, atol=0), what
    levels, excluded = L.noise_level_statistics(images)
    used = levels[..., 0] > 0
    assert np.array_equal(nlf.level_count.cpu().numpy(), levels[..., 0])
    assert np.array_equal(np.isnan(nlf.level_mean.cpu().numpy()), ~used) and np.array_equal(np.isnan(nlf.level_sigma.cpu().numpy()), ~used)
    assert np.allclose(nlf.level_mean.cpu().numpy()[used], (levels[..., 1] / (4.0 * np.maximum(levels[..., 0], 1)))[used], rtol=1e-15, atol=0)
    assert np.allclose(nlf.level_sigma.cpu().numpy()[used], levels[..., 2][used], rtol=1e-12, atol=0)
    assert np.array_equal(nlf.excluded_fraction.cpu().numpy(), excluded / float((H // 2) * (W // 2)))
    for x in (64.0, 128.0, 192.0):
        assert np.allclose(nlf.sigma_at(x).cpu().numpy(), L.sigma_at(gain, offset, x), rtol=1e-10, atol=0)
    return got_gain, got_offset


def test_fit_equals_the_reference_fit_on_the_cpu_cases():
    for a, read_sigma, seed in ((0.2, 1.0, 0), (1.0, 3.0, 2), (0.0, 10.0, 0)):
        _check_fit(L.fit_case(a, read_sigma, seed), f"a {a} read {read_sigma} seed {seed}")
    host = bf.noise_level_function(L.fit_case(0.5, 2.0, 1))                       # NumPy in, NumPy out
    assert all(isinstance(v, np.ndarray) and v.dtype == np.float64 for v in host)
    gain, offset = L.noise_level_function(L.fit_case(0.5, 2.0, 1))
    assert np.allclose(host.gain, gain, rtol=1e-10, atol=0) and np.allclose(host.offset, offset, rtol=1e-10, atol=0)
    assert np.allclose(host.sigma_at(128.0), L.sigma_at(gain, offset, 128.0), rtol=1e-10, atol=0)


def _cells_image(regions, height=32):
    """[1,height,W,1] of 2x2 cells (m + q, m; m, m): q is the cell's HH modulus, s = 4 m + q; `regions` = (m, q, cell columns)"""
    cols = []
    for m, q, n in regions:
        cell = np.array([[m + q, m], [m, m]], np.uint8)
        cols.append(np.tile(cell, (height // 2, n)))
    return np.concatenate(cols, axis=1)[None, :, :, None]


def test_fit_takes_every_fallback_branch():
    """histograms built by hand: every cell of a region has the same q, so the region's level has sigma_l = q / 2 / 0.6745 exactly"""
    k = 1.0 / 2.0 / 0.6745
    # two levels on a line through a positive intercept: the plain fit
    gain, offset = _check_fit(_cells_image([(40, 4, 16), (200, 8, 16)]), "two levels")
    assert gain[0, 0] > 0 and offset[0, 0] > 0
    # one usable level (the second holds 16 cells x 2 columns = 32 < 64): flat at its variance
    gain, offset = _check_fit(_cells_image([(40, 4, 16), (200, 8, 2)]), "one usable level")
    assert gain[0, 0] == 0 and offset[0, 0] == (4 * k) ** 2
    gain, _ = _check_fit(_cells_image([(40, 4, 16), (200, 8, 2)]), "min_cells 32", min_cells=32)
    assert gain[0, 0] > 0
    # a falling variance: flat at the weighted mean variance
    gain, offset = _check_fit(_cells_image([(40, 8, 16), (200, 2, 48)]), "falling variance")
    assert gain[0, 0] == 0 and abs(offset[0, 0] - (0.25 * (8 * k) ** 2 + 0.75 * (2 * k) ** 2)) <= 1e-12 * offset[0, 0]
    # a negative intercept: through the origin
    gain, offset = _check_fit(_cells_image([(40, 1, 16), (200, 16, 16)]), "negative intercept")
    assert offset[0, 0] == 0 and gain[0, 0] > 0
    # no usable level at all: the homoscedastic MAD estimate of the frame
    small = np.random.default_rng(2).integers(90, 110, (2, 8, 8, 3), dtype=np.uint8)
    gain, offset = _check_fit(small, "no usable level")
    assert (gain == 0).all()
    assert np.allclose(offset, bf.noise_statistics(_dev(small))[:, :, 2].cpu().numpy() ** 2, rtol=1e-15, atol=0)


# ---- 3. camera noise ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", NOISE_SHAPES, **_ids)
def test_camera_noise_matches_the_reference(shape):
    rng = np.random.default_rng(sum(shape))
    clean = rng.integers(0, 256, shape, dtype=np.uint8)
    clean.reshape(-1)[0], clean.reshape(-1)[-1] = 255, 0
    C = shape[3]
    for gain, read, seed in (([0.2, 0.5, 1.0, 0.0][:C], [1.0, 2.0, 3.0, 10.0][:C], 0), (0.5, 2.0, 2 ** 40 + 12345), (0.0, 25.0, 2 ** 64 - 1)):
        t = _dev(clean)
        got = bf.camera_noise(t, gain, read, seed)
        assert got.is_cuda and got.dtype == torch.uint8 and got.shape == t.shape and got.data_ptr() != t.data_ptr()
        assert torch.equal(bf.camera_noise(t, gain, read, seed), got)                          # the same seed: the same bits
        got = got.cpu().numpy()
        ref = L.camera_noise(clean, gain, read, seed)
        diff = np.abs(got.astype(int) - ref.astype(int))
        print(f"{shape} gain {gain} read {read}: {int((diff > 0).sum())} of {diff.size} samples differ, by at most {int(diff.max())}")
        assert diff.max() <= 1
        assert (diff > 0).sum() <= 1e-3 * diff.size
        if diff.size >= 1000:
            assert (got != clean).mean() > 0.5                                                 # it is noise
    assert torch.equal(bf.camera_noise(_dev(clean), 0.0, 0.0, 5), _dev(clean))                 # no noise: the input


def test_camera_noise_of_an_image_does_not_depend_on_its_batch_and_has_the_asked_variance():
    rng = np.random.default_rng(3)
    for shape in ((3, 37, 53, 3), (3, 64, 66, 4)):                                # unaligned and aligned image strides
        clean = rng.integers(0, 256, shape, dtype=np.uint8)
        whole = bf.camera_noise(_dev(clean), 0.5, 2.0, 77).cpu().numpy()
        for n in range(shape[0]):
            assert np.array_equal(bf.camera_noise(_dev(clean[n:n + 1]), 0.5, 2.0, 77).cpu().numpy()[0], whole[n]), (shape, n)
        assert not np.array_equal(bf.camera_noise(_dev(clean), 0.5, 2.0, 78).cpu().numpy(), whole)
    # the statistics of the draw: 2^17 samples per level, so the sample variance has a relative standard error of sqrt(2 / 2^17)
    # = 0.4 %; the bar is 2 % (five standard errors), on var = gain x + read^2 + 1/12
    flat = np.repeat(np.array([40, 200], np.uint8), 2 ** 17).reshape(1, 2, 2 ** 17, 1)
    noisy = bf.camera_noise(_dev(flat), 0.5, 2.0, 1).cpu().numpy().astype(np.float64)
    for row, x in ((0, 40.0), (1, 200.0)):
        want = 0.5 * x + 4.0 + 1.0 / 12.0
        assert abs(noisy[0, row].var() / want - 1.0) <= 0.02 and abs(noisy[0, row].mean() - x) <= 5.0 * np.sqrt(want / 2 ** 17)


def test_camera_noise_entry_refuses_bad_arguments():
    import ctypes
    lib = N.lib()
    src = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    dst = torch.zeros_like(src)
    three = lambda *v: (ctypes.c_float * 3)(*v)
    s = N.stream_ptr(src)
    call = lambda a=N.ptr(src), b=N.ptr(dst), B=1, H=8, W=8, C=3, g=three(0.1, 0.2, 0.3), r=three(1, 2, 3): \
        lib.bf_op_camera_noise_u8(a, b, B, H, W, C, g, r, 0, s)
    assert call() == N.BF_OK
    assert call(b=N.ptr(src)) == N.BF_OK                                          # in place is allowed
    for kw in ({"a": None}, {"b": None}, {"g": None}, {"r": None}, {"B": 0}, {"H": 0}, {"W": -1}, {"C": 0}, {"C": 5},
               {"g": three(0.1, -0.2, 0.3)}, {"r": three(1, 2, -3)}, {"g": three(0.1, float("nan"), 0.3)}, {"r": three(float("inf"), 2, 3)},
               {"H": 2 ** 16, "W": 2 ** 14}):
        assert call(**kw) == N.BF_EINVAL, kw
    torch.cuda.synchronize()


# ---- 4. the affine sums ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("probes", PROBES, **_ids)
@pytest.mark.parametrize("shape", SUMS_SHAPES, **_ids)
def test_affine_sums_carry_the_bits_of_risk_sums_and_match_the_reference(shape, probes):
    rng = np.random.default_rng(10 * sum(shape) + probes)
    y = rng.integers(0, 256, shape, dtype=np.uint8)
    flat = y.reshape(shape[0], -1)
    flat[:, :flat.shape[1] // 3] = 255                                            # saturated regions: the probe is reflected there
    flat[:, -(flat.shape[1] // 4):] = 0
    f = (rng.uniform(0.0, 255.0, ((1 + probes) * shape[0],) + shape[1:]) + rng.normal(0.0, 10.0, ((1 + probes) * shape[0],) + shape[1:])).astype(np.float32)
    yd, fd = _dev(y), _dev(f)
    K = probes
    for amplitude, seed in ((1, 2 ** 41 + 7), (16, 3)):
        got = bf.risk_sums_affine(yd, fd, probes, amplitude, seed)
        assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (shape[0], shape[3], 2 + 2 * K)
        again = bf.risk_sums_affine(yd, fd, probes, amplitude, seed).cpu().numpy()
        got = got.cpu().numpy()
        assert np.array_equal(got.view(np.uint64), again.view(np.uint64))                    # two calls: the same bits
        plain = bf.risk_sums(yd, fd, probes, amplitude, seed).cpu().numpy()
        assert np.array_equal(got[:, :, 0].view(np.uint64), plain[:, :, 0].view(np.uint64)), "R"
        assert np.array_equal(got[:, :, 2:2 + K].view(np.uint64), plain[:, :, 1:].view(np.uint64)), "D_p"
        assert np.array_equal(got[:, :, 1], y.astype(np.int64).sum(axis=(1, 2))), "Y"
        ref = L.risk_sums_affine(y, f, probes, amplitude, seed)
        members = f.astype(np.float64).reshape((1 + K, shape[0]) + shape[1:])
        scale = np.stack([(y * np.abs(members[p] - members[0])).sum(axis=(1, 2)) for p in range(1, K + 1)], axis=2)
        dev = float((np.abs(got[:, :, 2 + K:] - ref[:, :, 2 + K:]) / np.maximum(scale, 1e-300)).max())
        print(f"{shape} K = {K} amplitude {amplitude}: Dy / sum y |f_p - f_0| {dev:.3e}")
        assert dev <= 1e-10
        assert (np.abs(got[:, :, 2 + K:] - ref[:, :, 2 + K:]) <= 1e-10 * scale).all()


def test_affine_sums_of_an_image_do_not_depend_on_its_batch():
    for shape in ((3, 37, 53, 3), (3, 64, 66, 4)):
        rng = np.random.default_rng(shape[1])
        y = rng.integers(0, 256, shape, dtype=np.uint8)
        f = rng.uniform(0.0, 255.0, (3 * shape[0],) + shape[1:]).astype(np.float32)
        whole = bf.risk_sums_affine(_dev(y), _dev(f), 2, 1, 77).cpu().numpy()
        members = f.reshape((3,) + shape)
        for n in range(shape[0]):
            alone = bf.risk_sums_affine(_dev(y[n:n + 1]), _dev(members[:, n]), 2, 1, 77).cpu().numpy()
            assert np.array_equal(alone[0].view(np.uint64), whole[n].view(np.uint64)), (shape, n)


def test_affine_sums_refuse_bad_arguments():
    lib = N.lib()
    y = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    f = torch.ones((2, 8, 8, 3), dtype=torch.float32, device="cuda")
    nbytes = lib.bf_op_risk_sums_affine_scratch_bytes(1, 8, 8, 3, 1)
    assert nbytes > 0 and nbytes % 8 == 0
    scratch = torch.zeros(nbytes // 8 + 1, dtype=torch.float64, device="cuda")
    out = torch.zeros((1, 3, 4), dtype=torch.float64, device="cuda")
    s = N.stream_ptr(y)
    sums = lambda yy=N.ptr(y), ff=N.ptr(f), K=1, a=1, sc=N.ptr(scratch), nb=nbytes, o=N.ptr(out), C=3: \
        lib.bf_op_risk_sums_affine(yy, ff, 1, 8, 8, C, K, a, 0, sc, nb, o, s)
    assert sums() == N.BF_OK
    for kw in ({"K": 0}, {"K": 9}, {"a": 0}, {"a": 17}, {"C": 5}, {"yy": None}, {"ff": None}, {"sc": None}, {"o": None}, {"nb": nbytes - 8},
               {"sc": scratch.data_ptr() + 4}, {"o": out.data_ptr() + 4}, {"ff": f.data_ptr() + 2}):
        assert sums(**kw) == N.BF_EINVAL, kw
    for shape in ((0, 8, 8, 3, 1), (1, 8, 8, 5, 1), (1, 8, 8, 3, 9), (1, 8, 0, 3, 1)):
        assert lib.bf_op_risk_sums_affine_scratch_bytes(*shape) == N.BF_EINVAL
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), np.broadcast_to([64.0, 0.0, 0.0, 0.0], (1, 3, 4)))      # (1 - 0)^2 per pixel; y = 0; f_1 = f_0
    with pytest.raises(ValueError):
        bf.risk_sums_affine(y.float(), f, 1, 1, 0)                                # float images
    with pytest.raises(ValueError, match="stack_f32"):
        bf.risk_sums_affine(y, f[:1], 1, 1, 0)                                    # a wrong stack shape
    with pytest.raises(ValueError, match="stack_f32"):
        bf.risk_sums_affine(y, f, 2, 1, 0)
    for probes, amplitude in ((0, 1), (9, 1), (1, 0), (1, 17)):
        with pytest.raises(ValueError):
            bf.risk_sums_affine(y, f, probes, amplitude, 0)
    with pytest.raises(ValueError, match="gain"):
        bf.estimate_risk_affine(lambda u: u.float(), y, (-0.5, 1.0))
    with pytest.raises(ValueError, match="gain"):
        bf.camera_noise(y, -0.5, 1.0)
    with pytest.raises(ValueError, match="uint8"):
        bf.estimate_risk_affine(lambda u: u, y, (0.5, 1.0))


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------

def _half_field_blur_torch(u):
    """noise_level_reference.half_field_blur on the device.  The 3x3 sum is an integer below 2^12, exact in float32 in any order;
    n / 9 divided in float64 and rounded to float32: a quotient that is not a float32 itself lies at least 1 / (n 2^j) > 3e-9
    (relative; 2^-j the spacing of the rounding boundaries at n / 9) from every boundary, far beyond the float64 rounding of a true
    division or of a multiplication by the rounded reciprocal: the same bits wherever it is computed."""
    x = u.permute(0, 3, 1, 2).float()
    box = F.avg_pool2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), 3, stride=1, divisor_override=1)
    out = x.clone()
    half = x.shape[3] // 2
    out[:, :, :, :half] = (box[:, :, :, :half].double() / 9.0).float()
    return out.permute(0, 2, 3, 1).contiguous()


def test_estimate_risk_affine_equals_the_numpy_chain():
    H, W, K = 64, 96, 8
    clean = L.two_level_image(H, W)
    for seed in (100, 101):
        noisy_d = bf.camera_noise(_dev(clean), L.SURE_A, L.SURE_READ, seed)
        noisy = noisy_d.cpu().numpy()
        assert np.array_equal(_half_field_blur_torch(noisy_d).cpu().numpy(), L.half_field_blur(noisy))
        true = float(((L.half_field_blur(noisy).astype(np.float64) - clean) ** 2).mean())
        # given (a, b)
        est = bf.estimate_risk_affine(_half_field_blur_torch, noisy_d, (L.SURE_A, L.SURE_OFFSET), probes=K, amplitude=1, seed=seed)
        assert all(v.is_cuda and v.dtype == torch.float64 for v in est)
        assert [tuple(v.shape) for v in est] == [(1,)] * 2 + [(1, 1)] + [(1,)] * 3 + [(1, 1, 2 + 2 * K)]
        ref = L.estimate_risk_affine(L.half_field_blur, noisy, L.SURE_A, L.SURE_OFFSET, K, 1, seed)
        for k in ("mse", "sigma", "residual_rms", "divergence", "sums"):
            assert np.allclose(getattr(est, k).cpu().numpy(), ref[k], rtol=1e-9, atol=0), (seed, k)
        assert np.allclose(est.psnr.cpu().numpy(), 10.0 * np.log10(255.0 ** 2 / ref["mse"]), rtol=1e-9, atol=0)
        # nlf = None: the fit of the frame itself
        gain, offset = L.noise_level_function(noisy)
        blind = bf.estimate_risk_affine(_half_field_blur_torch, noisy_d, probes=K, amplitude=1, seed=seed)
        ref_blind = L.estimate_risk_affine(L.half_field_blur, noisy, gain, offset, K, 1, seed)
        for k in ("mse", "sigma", "residual_rms", "divergence", "sums"):
            assert np.allclose(getattr(blind, k).cpu().numpy(), ref_blind[k], rtol=1e-9, atol=0), (seed, k)
        fitted = bf.noise_level_function(noisy_d)
        assert torch.equal(bf.estimate_risk_affine(_half_field_blur_torch, noisy_d, fitted, probes=K, seed=seed).mse, blind.mse)
        print(f"seed {seed}: true mse {true:.3f}; affine SURE with the known (a, b) {float(est.mse):.3f}, with the fitted "
              f"({gain[0, 0]:.3f}, {offset[0, 0]:.3f}) {float(blind.mse):.3f}")
        host = bf.estimate_risk_affine(_half_field_blur_torch, noisy, (L.SURE_A, L.SURE_OFFSET), probes=K, seed=seed)      # NumPy in, NumPy out
        assert all(isinstance(v, np.ndarray) for v in host)
        assert all(np.array_equal(h, d.cpu().numpy(), equal_nan=True) for h, d in zip(host, est))


def test_estimate_risk_affine_runs_the_real_engine():
    cfg = O.canonical_config(no_layers=2)
    spec = O.ResnetSpec.from_config(cfg["model"])
    params, state = O.init_params(spec, seed=42)
    hydra = bf.model_builder(cfg["model"], device="cuda").hydra
    hydra.set_weights(params, state)
    clean, _ = O.synthetic_batch(2, 32, 32, seed=11)
    noisy = bf.camera_noise(_dev(clean), [0.3, 0.5, 0.8], 2.0, seed=4)
    module = bf.DenoiserModule(hydra)
    est = bf.estimate_risk_affine(module, noisy, probes=2, amplitude=1, seed=3)
    assert module.check_status()
    assert [tuple(v.shape) for v in est] == [(2,)] * 2 + [(2, 3)] + [(2,)] * 3 + [(2, 3, 6)]
    assert all(bool(torch.isfinite(v).all()) for v in est)
    plain = bf.estimate_risk(module, noisy, sigma=est.sigma, probes=2, amplitude=1, seed=3)
    assert torch.equal(plain.sums[:, :, 0], est.sums[:, :, 0]) and torch.equal(plain.sums[:, :, 1:], est.sums[:, :, 2:4])
    given = bf.estimate_risk_affine(module, noisy, ([0.3, 0.5, 0.8], 4.0 + 1.0 / 12.0), probes=2, amplitude=1, seed=3)
    assert torch.equal(given.sums, est.sums) and bool(torch.isfinite(given.mse).all()) and module.check_status()
