"""GPU tests of csrc/pixel_shuffle.hip and PixelShuffleDenoiserModule.

Yardstick: tests/pixel_shuffle_reference.py.  The kernels count integers, move bytes and floats, compare Philox words, add in
fp64 in a fixed order, divide with correct rounding and round half to even, each of which NumPy does bit for bit the same:
nothing here has a tolerance.  The one statistical bar (the share of replaced pixels) is +-5 standard deviations of a binomial."""
import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from oracle import bfcnn_oracle as O
import pixel_shuffle_reference as R
from guarded import dev as _dev, guard_bands

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guard_bands")]

# (B, H, W, C, S): H = S + 1, one position at s = 8; across a 32-row and a 64-column tile edge; four channels, three column tiles
CORRELATION_CASES = [(1, 9, 9, 1, 8), (2, 40, 70, 3, 6), (1, 33, 130, 4, 4)]
SPLIT_CASES = [(1, 4, 4, 3, 2), (2, 7, 9, 3, 2), (1, 6, 200, 1, 3), (1, 65, 33, 3, 4), (3, 8, 8, 1, 1)]
# a workgroup owns 512 frame pixels of a row: the repeated last column is the FIRST of the third piece (Ws = 257 at 256 columns a
# piece); three pieces of 170 columns with the repeat inside the last; stride 8 and four channels (the largest LDS segments)
SPLIT_CASES += [(1, 4, 513, 3, 2), (2, 7, 1030, 1, 3), (1, 17, 530, 4, 8)]
_ids = {"ids": lambda c: "-".join(map(str, c))}


def _same(got, ref):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got, ref)


def _image(case):
    B, H, W, C = case[:4]
    return np.random.default_rng(sum(case)).integers(0, 256, (B, H, W, C), dtype=np.uint8)


# ---- bf_noise_correlation ----------------------------------------------------------------------------------------------------

def _check_correlation(x: np.ndarray, S: int):
    ref_hist, ref_sigma = R.correlation_statistics(x, S)
    hist, sigma = bf.noise_correlation_statistics(_dev(x), S)
    assert hist.is_cuda and _same(hist, ref_hist), "histograms"
    assert _same(sigma, ref_sigma), "sigma_s"
    ref = R.correlation(x, S, 0.8)
    got = bf.noise_correlation(_dev(x), S, 0.8)
    assert isinstance(got, bf.NoiseCorrelation) and all(v.is_cuda for v in got)
    host = bf.noise_correlation(x, S, 0.8)                          # NumPy in, NumPy out
    for g, h, r in zip(got, host, ref):
        assert _same(g, r) and isinstance(h, np.ndarray) and _same(h, r)
    return ref_hist, ref_sigma


@pytest.mark.parametrize("case", CORRELATION_CASES, **_ids)
def test_correlation_matches_numpy(case):
    B, H, W, C, S = case
    x = _image(case)
    x[0, :H // 2] //= 8                                             # two populations: the median sits away from the mode
    ref_hist, _ = _check_correlation(x, S)
    assert ref_hist[0, 0, S - 1].sum() == (H - S) * (W - S)
    if B > 1:                                                       # an image inside a batch gets the bits of that image alone
        for b in range(B):
            hist, sigma = bf.noise_correlation_statistics(_dev(x[b:b + 1]), S)
            assert _same(hist, ref_hist[b:b + 1]) and _same(sigma, R.correlation_statistics(x[b:b + 1], S)[1])


def test_correlation_of_flat_and_checkerboard_images():
    flat = np.full((1, 20, 70, 3), 255, np.uint8)
    hist, sigma = _check_correlation(flat, 4)
    assert (hist[..., 0] == [[[19 * 69, 18 * 68, 17 * 67, 16 * 66]] * 3]).all() and not hist[..., 1:].any() and not sigma.any()
    assert bf.noise_correlation(flat, 4).stride.tolist() == [1]
    y, x = np.mgrid[0:34, 0:66]
    board = (((y + x) & 1) * 255).astype(np.uint8)[None, :, :, None]
    hist, sigma = _check_correlation(board, 2)
    assert hist[0, 0, 0, 510] == 33 * 65 and hist[0, 0, 0].sum() == 33 * 65         # q_1 = 510, the top bin
    assert hist[0, 0, 1, 0] == 32 * 64 and sigma[0, 0, 1] == 0.0                    # q_2 = 0


def test_correlation_finds_the_stride_of_filtered_noise():
    batch = np.concatenate([R.correlated_noise_image(taps, 20.0, seed, C=3) for seed, taps in enumerate(([1], [1, 1], [1, 4, 6, 4, 1]))])
    got = bf.noise_correlation(_dev(batch), 6, 0.8)
    ref = R.correlation(batch, 6, 0.8)
    assert ref[1].tolist() == [1, 2, 3] and all(_same(g, r) for g, r in zip(got, ref))


# ---- split and merge ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", SPLIT_CASES, **_ids)
def test_split_and_merge_match_numpy(case):
    B, H, W, C, s = case
    x = _image(case)
    ref = R.split(x, s)
    members = bf.pd_split_u8(_dev(x), s)
    assert _same(members, ref)
    floats = np.random.default_rng(100 + sum(case)).uniform(-40.0, 300.0, ref.shape).astype(np.float32)
    for cast in (False, True):
        assert _same(bf.pd_merge(_dev(floats), B, H, W, s, cast_to_uint8=cast), R.merge(floats, B, H, W, s, cast)), cast
    assert _same(bf.pd_merge(members.float(), B, H, W, s), x)
    assert _same(bf.pd_merge(members.float(), B, H, W, s, cast_to_uint8=False), x.astype(np.float32))


def test_merge_ties_and_clips_decide():
    v = np.array([0.5, 1.5, 2.5, 253.5, 254.5, -0.5, -3.0, 255.5, 260.0, 254.49998, 0.49999997, 127.5, 128.5], np.float32)
    x = np.resize(v, (4, 4, 7, 3)).astype(np.float32)
    got = bf.pd_merge(_dev(x), 1, 8, 13, 2).cpu().numpy()
    assert _same(got, R.merge(x, 1, 8, 13, 2, True))
    assert got[0, 0, 0, 0] == 0 and got[0, 0, 0, 1] == 2 and got[0, 0, 0, 2] == 2 and got[0, 0, 2, 0] == 254


# ---- replace and mean --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("replace", [0.0, 0.16, 1.0])
@pytest.mark.parametrize("seed", [0, 2 ** 40 + 17])
def test_replace_matches_numpy(replace, seed):
    rng = np.random.default_rng(11)
    base, noisy = (rng.integers(0, 256, (2, 5, 7, 3), dtype=np.uint8) for _ in range(2))      # W = 7: Philox groups straddle rows
    ref = R.replace_copies(base, noisy, 3, replace, seed)
    assert _same(bf.pd_replace_u8(_dev(base), _dev(noisy), 3, replace, seed), ref)
    if replace == 0.0:
        assert np.array_equal(ref, np.repeat(base, 3, axis=0))
    if replace == 1.0:
        assert np.array_equal(ref, np.repeat(noisy, 3, axis=0))


def test_replace_matches_numpy_on_many_copies_and_whole_dwords():
    rng = np.random.default_rng(12)
    for shape in ((1, 33, 65, 1), (2, 16, 20, 3), (1, 6, 10, 4), (1, 9, 9, 2)):      # byte path; dword paths of 3, 4 and the tail of 2
        base, noisy = (rng.integers(0, 256, shape, dtype=np.uint8) for _ in range(2))
        assert _same(bf.pd_replace_u8(_dev(base), _dev(noisy), 16, 0.16, 3), R.replace_copies(base, noisy, 16, 0.16, 3)), shape


def test_share_of_replaced_pixels():
    share = R.replace_masks(64, 64, 1, 0.16, 0).mean()
    print(f"replaced share on 64 x 64 at 0.16: {share:.4f}")
    assert 0.13 <= share <= 0.19                                    # 0.16 +- 5 sqrt(0.16 0.84 / 4096) = 0.131 .. 0.189
    base, noisy = np.zeros((1, 64, 64, 1), np.uint8), np.ones((1, 64, 64, 1), np.uint8)
    assert bf.pd_replace_u8(_dev(base), _dev(noisy), 1, 0.16, 0).float().mean().item() == share


@pytest.mark.parametrize("B, T", [(2, 5), (3, 1)])
def test_mean_matches_numpy(B, T):
    x = np.random.default_rng(B + T).uniform(-40.0, 300.0, (B * T, 9, 11, 3)).astype(np.float32)
    x[0, 0, 0] = (0.5, 1.5, 2.5)
    if T > 1:
        x[1:T, 0, 0] = x[0, 0, 0]                                   # exact ties after the mean
    for cast in (False, True):
        assert _same(bf.pd_mean(_dev(x), T, cast_to_uint8=cast), R.mean(x, T, cast)), cast


# ---- the module around a callable --------------------------------------------------------------------------------------------

def _callable_denoiser(u8):
    return u8.float() * 0.5 + 3


def _callable_reference(u8: np.ndarray) -> np.ndarray:
    return u8.astype(np.float32) * np.float32(0.5) + np.float32(3)


@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("refine", [0, 2])
def test_module_is_the_reference_pipeline(s, refine):
    x = np.random.default_rng(s + refine).integers(0, 256, (2, 13, 17, 3), dtype=np.uint8)
    module = bf.PixelShuffleDenoiserModule(_callable_denoiser, s, refine=refine, replace=0.3, seed=5)
    ref = R.pipeline(_callable_reference, x, s, refine, 0.3, 5, cast=True)
    got = module(x)                                                 # NumPy in, NumPy out
    assert isinstance(got, np.ndarray) and _same(got, ref) and module.last_stride == s
    got = module(_dev(x))                                           # device tensor in, device tensor out
    assert isinstance(got, torch.Tensor) and got.is_cuda and _same(got, ref)
    flt = module.float_form()
    assert _same(flt(_dev(x)), R.pipeline(_callable_reference, x, s, refine, 0.3, 5, cast=False))
    assert module.check_status() is True


def test_stride_one_is_the_wrapped_callable():
    x = np.random.default_rng(0).integers(0, 256, (2, 5, 9, 3), dtype=np.uint8)
    module = bf.PixelShuffleDenoiserModule(_callable_denoiser, 1, cast_to_uint8=False)
    assert torch.equal(module(_dev(x)), _callable_denoiser(_dev(x))) and module.last_stride == 1
    assert _same(bf.PixelShuffleDenoiserModule(_callable_denoiser, 1)(x), R.to_uint8(_callable_reference(x)))


def test_auto_stride_reads_the_noise():
    box = np.concatenate([R.correlated_noise_image([1, 1], 20.0, seed, C=3) for seed in (0, 1)])
    module = bf.PixelShuffleDenoiserModule(_callable_denoiser, "auto", max_stride=4)
    assert _same(module(box), R.pipeline(_callable_reference, box, 2)) and module.last_stride == 2
    flt = module.float_form()
    white = R.correlated_noise_image([1], 20.0, 2, C=3)
    assert _same(flt(white), _callable_reference(white)) and module.last_stride == 1          # the record is shared
    mixed = np.concatenate([white, R.correlated_noise_image([1, 4, 6, 4, 1], 20.0, 3, C=3)])
    module(mixed)
    assert module.last_stride == 3                                  # the largest stride over the images
    module(mixed[:, :5, :40])                                       # H = 5 allows stride 2 at the most
    assert module.last_stride == 2


# ---- with a real model and the other wrappers --------------------------------------------------------------------------------

_MODEL = []


def _resnet():
    if not _MODEL:
        cfg = O.canonical_config(no_layers=6)
        spec = O.ResnetSpec.from_config(cfg["model"])
        params, state = O.init_params(spec, seed=42)
        m = bf.model_builder(cfg["model"], device="cuda").hydra
        m.set_weights(params, state)
        _MODEL.append(m)
    return _MODEL[0]


def test_real_model_is_the_hand_built_pipeline():
    module = bf.DenoiserModule(_resnet())
    x = _dev(np.random.default_rng(4).integers(0, 256, (1, 32, 48, 3), dtype=np.uint8))
    shuffled = bf.PixelShuffleDenoiserModule(module, 2)
    by_hand = bf.pd_merge(module.float_form()(bf.pd_split_u8(x, 2)), 1, 32, 48, 2)
    assert torch.equal(shuffled(x), by_hand) and shuffled.check_status() is True
    assert np.array_equal(shuffled(x.cpu().numpy()), by_hand.cpu().numpy())
    plain = bf.PixelShuffleDenoiserModule(module, 1)
    assert torch.equal(plain(x), module(x))                         # stride 1: exactly the wrapped module
    refined = bf.PixelShuffleDenoiserModule(module, 2, refine=2, replace=0.25, seed=1)
    copies = bf.pd_replace_u8(by_hand, x, 2, 0.25, 1)
    assert torch.equal(refined(x), bf.pd_mean(module.float_form()(copies), 2)) and refined.check_status() is True
    assert shuffled(x[:0]).shape == (0, 32, 48, 3)


def test_composes_with_tiles_underneath_and_stabilisation_on_top():
    module = bf.DenoiserModule(_resnet())
    tiled = bf.TiledDenoiserModule(module, tile=16, overlap=8, margin=2, tile_batch=8)
    x = _dev(np.random.default_rng(6).integers(0, 256, (1, 32, 48, 3), dtype=np.uint8))
    shuffled = bf.PixelShuffleDenoiserModule(tiled, 2)
    by_hand = bf.pd_merge(tiled.float_form()(bf.pd_split_u8(x, 2)), 1, 32, 48, 2)
    assert torch.equal(shuffled(x), by_hand) and tiled.last_plan.tiles == 2 and shuffled.check_status() is True
    level = ([0.3, 0.5, 0.8], 4.0 + 1.0 / 12.0)
    stabilised = bf.StabilisedDenoiserModule(shuffled, level)
    out = stabilised(x)
    assert out.dtype == torch.uint8 and stabilised.check_status() is True
    assert torch.equal(out, bf.unstabilise(shuffled.float_form()(bf.stabilise_u8(x, level)), level))


def test_load_model_wraps_tiles_then_pixel_shuffle_then_stabilisation(tmp_path):
    bf.save_model(_resnet(), str(tmp_path / "m"))
    x = np.random.default_rng(8).integers(0, 256, (1, 32, 48, 3), dtype=np.uint8)
    loaded = bf.load_model(str(tmp_path / "m"), device="cuda", pixel_shuffle=2)
    assert type(loaded) is bf.PixelShuffleDenoiserModule and type(loaded._module) is bf.DenoiserModule and loaded.stride == 2
    assert np.array_equal(loaded(x), bf.PixelShuffleDenoiserModule(bf.DenoiserModule(_resnet()), 2)(x)) and loaded.check_status()
    assert bf.load_model(str(tmp_path / "m"), device="cuda", pixel_shuffle=True).stride == "auto"
    assert type(bf.load_model(str(tmp_path / "m"), device="cuda", pixel_shuffle=False)) is bf.DenoiserModule
    full = bf.load_model(str(tmp_path / "m"), device="cuda", self_ensemble="flips", tiled={"tile": 16, "overlap": 8, "margin": 2},
                         pixel_shuffle={"stride": "auto", "refine": 2}, stabilise=True)
    assert type(full) is bf.StabilisedDenoiserModule and type(full._module) is bf.PixelShuffleDenoiserModule
    assert type(full._module._module) is bf.TiledDenoiserModule and type(full._module._module._module) is bf.SelfEnsembleDenoiserModule
    out = full(x)
    assert out.shape == x.shape and out.dtype == np.uint8 and full.check_status() and full._module.last_stride in (1, 2, 3, 4)
