"""Correlated noise without a GPU: the properties of the definitions (tests/pixel_shuffle_reference.py), the stride rule on
noise of a known correlation, the stride rule of the package (tensor operations, which run anywhere) against the reference, and
every host-side error."""
import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import pixel_shuffle as PS
import pixel_shuffle_reference as R

SPLIT_CASES = [(1, 4, 4, 3, 2), (2, 7, 9, 3, 2), (1, 6, 200, 1, 3), (1, 65, 33, 3, 4), (3, 8, 8, 1, 1)]
# the circular kernel a white field is filtered with, per axis -> the stride the rule must find (max_stride 6, threshold 0.8)
KERNELS = {"white": ([1], 1), "box2": ([1, 1], 2), "binomial3": ([1, 2, 1], 2), "binomial5": ([1, 4, 6, 4, 1], 3)}
SEEDS = (0, 7, 19, 33, 39)


@pytest.mark.parametrize("case", SPLIT_CASES, ids=lambda c: "-".join(map(str, c)))
def test_merge_of_split_is_the_image(case):
    B, H, W, C, s = case
    x = np.random.default_rng(sum(case)).integers(0, 256, (B, H, W, C), dtype=np.uint8)
    members = R.split(x, s)
    assert members.shape == (B * s * s, -(H // -s), -(W // -s), C) and members.dtype == np.uint8
    assert np.array_equal(R.merge(members.astype(np.float32), B, H, W, s, True), x)
    assert np.array_equal(R.merge(members.astype(np.float32), B, H, W, s, False), x.astype(np.float32))


def test_split_repeats_the_last_pixel_of_the_same_phase():
    x = np.arange(7 * 9, dtype=np.uint8).reshape(1, 7, 9, 1)
    members = R.split(x, 2)                                         # 4 x 5 sub-images
    assert np.array_equal(members[0, :, :, 0], x[0, 0::2, 0::2, 0])          # phase (0, 0) is complete
    assert np.array_equal(members[3, :3, :4, 0], x[0, 1::2, 1::2, 0])        # phase (1, 1) has 3 x 4 pixels of its own
    assert np.array_equal(members[3, 3], members[3, 2]) and np.array_equal(members[3, :, 4], members[3, :, 3])


def test_the_statistic_is_blind_to_separable_content():
    rng = np.random.default_rng(1)
    f, g = rng.integers(0, 128, 40), rng.integers(0, 128, 30)
    x = (f[None, :] + g[:, None]).astype(np.uint8)[None, :, :, None]          # planes, axis-aligned edges, any f(x) + g(y)
    for s in range(1, 9):
        assert not R.dilated_haar(x, s).any()
    hist, sigma = R.correlation_statistics(x, 8)
    assert (hist[0, 0, :, 0] == [(30 - s) * (40 - s) for s in range(1, 9)]).all() and not hist[..., 1:].any() and not sigma.any()
    assert R.correlation(x, 8)[1].tolist() == [1]                   # a curve of zeros: stride 1


@pytest.mark.parametrize("name", list(KERNELS))
@pytest.mark.parametrize("sigma", [8.0, 20.0])
def test_stride_rule_on_noise_of_a_known_correlation(name, sigma):
    taps, want = KERNELS[name]
    for seed in SEEDS:
        image = R.correlated_noise_image(taps, sigma, seed)
        curve, stride, white = R.correlation(image, 6, 0.8)
        assert stride.tolist() == [want], (name, sigma, seed, curve)
        assert 0.85 <= white[0] / sigma <= 1.15, (name, sigma, seed, white[0])
    # and what the issue is about: the finest band alone reads a fraction of sigma under correlated noise
    if name == "binomial3":
        assert curve[0, 0] < 0.45 * sigma


def test_package_stride_rule_is_the_reference():
    rng = np.random.default_rng(5)
    for S in (1, 2, 6, 8):
        curves = np.concatenate([rng.uniform(0.0, 30.0, (40, S)), np.sort(rng.uniform(0.0, 30.0, (40, S)), axis=1), np.zeros((1, S))])
        for threshold in (0.8, 0.5, 1.0):
            stride, white = PS.stride_rule(torch.from_numpy(curves), threshold)
            ref_stride, ref_white = R.stride_rule(curves, threshold)
            assert stride.dtype == torch.int64 and np.array_equal(stride.numpy(), ref_stride)
            assert white.dtype == torch.float64 and np.array_equal(white.numpy(), ref_white)
    assert R.replace_threshold(0.0) == 0 == PS.replace_threshold(0.0) and PS.replace_threshold(1.0) == 2 ** 32 - 1
    assert PS.replace_threshold(0.16) == R.replace_threshold(0.16) == int(0.16 * 2 ** 32)


def test_reference_replacing_is_per_pixel_and_per_copy():
    masks = R.replace_masks(64, 64, 3, 0.16, 0)
    assert not np.array_equal(masks[0], masks[1]) and not np.array_equal(masks[0], R.replace_masks(64, 64, 1, 0.16, 1)[0])
    assert not R.replace_masks(5, 7, 2, 0.0, 3).any() and R.replace_masks(5, 7, 2, 1.0, 3).all()
    base, noisy = np.zeros((2, 5, 7, 3), np.uint8), np.full((2, 5, 7, 3), 9, np.uint8)
    copies = R.replace_copies(base, noisy, 2, 0.5, 4)
    assert np.array_equal(copies[:2], copies[2:])                   # every image of a batch gets the same masks
    assert ((copies == 9).all(axis=-1) | (copies == 0).all(axis=-1)).all()          # a pixel is replaced in all its channels


# ---- argument checks: everything raises before a GPU is needed ---------------------------------------------------------------

def test_noise_correlation_argument_errors():
    image = np.zeros((1, 9, 9, 3), np.uint8)
    for bad in (0, 9, 2.0, True):
        with pytest.raises(ValueError, match="max_stride"):
            bf.noise_correlation(image, max_stride=bad)
    for bad in (0.0, -0.1, 1.5, "0.8", float("nan")):
        with pytest.raises(ValueError, match="threshold"):
            bf.noise_correlation(image, threshold=bad)
    with pytest.raises(ValueError):
        bf.noise_correlation(image.astype(np.float32))
    with pytest.raises(ValueError):
        bf.noise_correlation(np.zeros((1, 9, 9, 5), np.uint8))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        bf.noise_correlation(torch.zeros((1, 9, 9, 3), dtype=torch.uint8))
    hist, sigma = bf.noise_correlation_statistics(image[:0], max_stride=4)         # an empty batch launches nothing
    assert tuple(hist.shape) == (0, 3, 4, 512) and hist.dtype == torch.int64 and tuple(sigma.shape) == (0, 3, 4)


def test_small_images_are_refused():
    with pytest.raises(ValueError, match="at least 9 x 9"):
        bf.noise_correlation(np.zeros((1, 8, 12, 3), np.uint8), max_stride=8)
    with pytest.raises(ValueError, match="at least 7 x 7"):
        bf.noise_correlation_statistics(np.zeros((1, 12, 6, 1), np.uint8))


def test_kernel_wrappers_refuse_host_tensors_and_bad_arguments():
    image = torch.zeros((1, 20, 20, 3), dtype=torch.uint8)
    members = torch.zeros((4, 10, 10, 3))
    for call in (lambda: bf.pd_split_u8(image, 2), lambda: bf.pd_merge(members, 1, 20, 20, 2),
                 lambda: bf.pd_replace_u8(image, image, 2), lambda: bf.pd_mean(members, 2)):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            call()
    for bad in (0, 9, 2.0, "2"):
        with pytest.raises(ValueError, match="stride"):
            bf.pd_split_u8(image, bad)
    with pytest.raises(ValueError, match="needs H, W >= 16"):
        bf.pd_merge(torch.zeros((64, 2, 3, 3)), 1, 15, 20, 8)
    with pytest.raises(ValueError, match="needs H, W >= 8"):
        bf.pd_split_u8(torch.zeros((1, 7, 20, 3), dtype=torch.uint8), 4)
    with pytest.raises(ValueError):
        bf.pd_split_u8(image.float(), 2)
    with pytest.raises(ValueError, match="members_f32 must be"):
        bf.pd_merge(members, 1, 20, 21, 2)
    with pytest.raises(ValueError, match="members_f32 must be"):
        bf.pd_merge(members[:3], 1, 20, 20, 2)
    with pytest.raises(ValueError):
        bf.pd_merge(members.double(), 1, 20, 20, 2)
    for bad in (0, 17, 1.0):
        with pytest.raises(ValueError, match="copies"):
            bf.pd_replace_u8(image, image, bad)
        with pytest.raises(ValueError, match="copies"):
            bf.pd_mean(members, bad)
    for bad in (-0.1, 1.1, "x"):
        with pytest.raises(ValueError, match="replace"):
            bf.pd_replace_u8(image, image, 2, replace=bad)
    with pytest.raises(ValueError, match="seed"):
        bf.pd_replace_u8(image, image, 2, seed=-1)
    with pytest.raises(ValueError, match="one shape"):
        bf.pd_replace_u8(image, image[:, :10], 2)
    with pytest.raises(ValueError, match="multiple of 3"):
        bf.pd_mean(members, 3)


def test_module_argument_errors():
    denoise = lambda u8: u8.float()
    for bad in ({"stride": 0}, {"stride": 9}, {"stride": "automatic"}, {"stride": 2.0}, {"stride": True}, {"max_stride": 0},
                {"max_stride": 9}, {"threshold": 0.0}, {"threshold": 2.0}, {"refine": -1}, {"refine": 17}, {"refine": 1.0},
                {"replace": 1.5}, {"replace": -0.1}, {"seed": -1}, {"seed": 2 ** 64}):
        with pytest.raises(ValueError, match=next(iter(bad))):
            bf.PixelShuffleDenoiserModule(denoise, **bad)
    with pytest.raises(ValueError):
        bf.PixelShuffleDenoiserModule(42)
    module = bf.PixelShuffleDenoiserModule(denoise, "auto", max_stride=3, threshold=0.7, refine=4, replace=0.2, seed=9)
    assert (module.stride, module.max_stride, module.threshold, module.refine, module.replace, module.seed) == ("auto", 3, 0.7, 4, 0.2, 9)
    assert module.last_stride is None and module.check_status() is True and module.model_hydra is None
    with pytest.raises(ValueError, match="already pixel-shuffled"):
        bf.PixelShuffleDenoiserModule(module)
    flt = module.float_form()
    assert isinstance(flt, bf.PixelShuffleDenoiserModule) and flt._cast_to_uint8 is False and flt._record is module._record
    assert (flt.stride, flt.max_stride, flt.threshold, flt.refine, flt.replace, flt.seed) == ("auto", 3, 0.7, 4, 0.2, 9)
    defaults = bf.PixelShuffleDenoiserModule(denoise)
    assert (defaults.stride, defaults.max_stride, defaults.threshold, defaults.refine, defaults.replace, defaults.seed) == \
        (2, 4, 0.8, 0, 0.16, 0)
    with pytest.raises(ValueError):
        defaults(np.zeros((1, 8, 8, 3), np.float32))
    with pytest.raises(ValueError, match="needs H, W >= 4"):
        defaults(np.zeros((1, 3, 8, 3), np.uint8))                  # refused before the GPU is touched
    empty = defaults(np.zeros((0, 8, 8, 3), np.uint8))
    assert empty.shape == (0, 8, 8, 3) and empty.dtype == np.uint8
    tiled = bf.TiledDenoiserModule(denoise, tile=64, margin=3)
    assert bf.PixelShuffleDenoiserModule(tiled)._module is tiled    # the other wrappers go inside


def test_load_model_checks_the_keyword_before_anything_is_loaded():
    for bad in ("yes", 0, 9, 2.5, {"strides": 2}, {"stride": 12}, {"refine": 99}, {"threshold": 0.0}, [2], {"cast_to_uint8": False}):
        with pytest.raises(ValueError, match="pixel_shuffle"):
            bf.load_model("no such model", pixel_shuffle=bad)       # the keyword is refused first
    with pytest.raises(ValueError, match="does not exist"):
        bf.load_model("no such model", pixel_shuffle={"stride": "auto", "refine": 8})
    assert PS.parse_setting(None) is None and PS.parse_setting(False) is None
    assert PS.parse_setting(True) == {"stride": "auto"} and PS.parse_setting(3) == {"stride": 3}
    assert PS.parse_setting("auto") == {"stride": "auto"} and PS.parse_setting({"refine": 2}) == {"refine": 2}
