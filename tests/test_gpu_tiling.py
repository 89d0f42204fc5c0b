"""GPU tests of tiled inference: bf_op_tile_split_u8 / bf_op_tile_blend (csrc/tiling.hip) and TiledDenoiserModule.

Yardstick: tests/tiling_reference.py, the NumPy statement of the plan, the split (slicing) and the blend (integer weights, fp64
sum in ascending tile order, one fp64 division, a cast to float32, np.clip and np.rint).  The kernels move bytes, multiply by small
integers (exact in fp64, so a fused multiply-add changes nothing), add in a fixed order, divide with correct rounding and round
half to even, each of which NumPy does bit for bit the same: nothing about the blend has a tolerance.  Only the locality test
has bars, those of tests/test_gpu_inference.py against the fp64 oracle on the whole frame."""
import math

import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import tiling as TL
from oracle import bfcnn_oracle as O
from oracle import unet_oracle as U
import tiling_reference as R
from guarded import dev as _dev, guard_bands

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guard_bands")]

# (B, H, W, C, T, O, M): one tile below T; three tiles over rows 23..26; the locality case, 21 tiles; one past a tile; R = 0, a
# hard crop; no nominal overlap
CASES = [(1, 1, 1, 3, 8, 4, 2), (2, 50, 70, 3, 32, 16, 5), (1, 64, 128, 3, 32, 16, 5), (1, 33, 65, 1, 32, 16, 0),
         (1, 7, 200, 3, 16, 8, 4), (3, 40, 40, 1, 16, 0, 0)]
_ids = {"ids": lambda c: "-".join(map(str, c))}


def _same(got, ref):
    return got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got, ref)


def _image(case):
    B, H, W, C = case[:4]
    return np.random.default_rng(sum(case)).integers(0, 256, (B, H, W, C), dtype=np.uint8)


# ---- the two kernels ---------------------------------------------------------------------------------------------------------

def test_the_cases_cover_what_they_name():
    assert R.plan(50, 70, 32, 16, 5)["ny"] == 3 and R.plan(64, 128, 32, 16, 5)["ny"] * R.plan(64, 128, 32, 16, 5)["nx"] == 21
    t, origins, w = R.axis_plan(50, 32, 16, 5)
    cover = np.zeros(50, dtype=int)
    for x0, wi in zip(origins, w):
        cover[x0:x0 + t] += wi > 0
    assert np.flatnonzero(cover == 3).tolist() == [23, 24, 25, 26]


@pytest.mark.parametrize("case", CASES, **_ids)
def test_split_matches_numpy(case):
    B, H, W, C, T, Ov, M = case
    x = _image(case)
    ref = R.split(x, T, Ov)
    assert _same(TL.tile_split_u8(_dev(x), T, Ov).cpu().numpy(), ref)
    if ref.shape[0] >= 12:
        part = TL.tile_split_u8(_dev(x), T, Ov, first=5, count=7).cpu().numpy()
        assert _same(part, ref[5:12])
        assert _same(TL.tile_split_u8(_dev(x), T, Ov, first=ref.shape[0] - 1).cpu().numpy(), ref[-1:])


def test_split_refuses_ranges_outside_the_plan():
    x = _dev(_image(CASES[1]))                                       # 2 x (3 x 4) tiles
    for first, count in ((24, 1), (-1, 1), (0, 25), (18, 7), (0, 0)):
        with pytest.raises(ValueError):
            TL.tile_split_u8(x, 32, 16, first=first, count=count)


@pytest.mark.parametrize("case", CASES, **_ids)
def test_blend_matches_numpy(case):
    B, H, W, C, T, Ov, M = case
    p = R.plan(H, W, T, Ov, M)
    shape = (B * p["ny"] * p["nx"], p["t_h"], p["t_w"], C)
    tiles = np.random.default_rng(100 + sum(case)).uniform(-40.0, 300.0, shape).astype(np.float32)
    for cast in (False, True):
        got = TL.tile_blend(_dev(tiles), B, H, W, T, Ov, M, cast_to_uint8=cast).cpu().numpy()
        assert _same(got, R.blend(tiles, B, H, W, T, Ov, M, cast)), cast


def test_blend_of_a_split_is_the_image():
    for case in CASES:
        B, H, W, C, T, Ov, M = case
        x = _image(case)
        tiles = TL.tile_split_u8(_dev(x), T, Ov).float()
        assert _same(TL.tile_blend(tiles, B, H, W, T, Ov, M).cpu().numpy(), x), case


def test_blend_ties_and_clips_decide():
    """a one-tile plan: the blend IS the input, so the ties and the out-of-range values are set by hand"""
    v = np.array([0.5, 1.5, 2.5, 253.5, 254.5, -0.5, -3.0, 255.5, 260.0, 254.49998, 0.49999997, 127.5, 128.5], np.float32)
    x = np.resize(v, (1, 7, 13, 3)).astype(np.float32)
    got = TL.tile_blend(_dev(x), 1, 7, 13, 16, 8, 2).cpu().numpy()
    assert _same(got, np.rint(np.clip(x, 0, 255)).astype(np.uint8))
    assert got[0, 0, 0, 0] == 0 and got[0, 0, 0, 1] == 2 and got[0, 0, 0, 2] == 2 and got[0, 0, 1, 0] == 254
    assert got[0, 0, 1, 1] == 254 and got[0, 0, 1, 2] == 0 and got[0, 0, 2, 1] == 255 and got[0, 0, 2, 2] == 255
    assert _same(TL.tile_blend(_dev(x), 1, 7, 13, 16, 8, 2, cast_to_uint8=False).cpu().numpy(), x)


def test_other_channel_counts_are_refused():
    for c in (2, 4):
        with pytest.raises(NotImplementedError):
            TL.tile_split_u8(torch.zeros((1, 20, 20, c), dtype=torch.uint8, device="cuda"), 8, 4)
        with pytest.raises(NotImplementedError):
            TL.tile_blend(torch.zeros((16, 8, 8, c), device="cuda"), 1, 20, 20, 8, 4, 1)


def test_blend_refuses_wrong_tile_batches():
    f = lambda *s: torch.zeros(s, device="cuda")
    for bad in (f(15, 8, 8, 3), f(17, 8, 8, 3), f(16, 8, 7, 3), f(16, 7, 8, 3), f(16, 8, 8, 3).double(), f(16, 8, 8)):
        with pytest.raises(ValueError):
            TL.tile_blend(bad, 1, 20, 20, 8, 4, 1)
    with pytest.raises(ValueError):
        TL.tile_blend(f(16, 8, 8, 3), 2, 20, 20, 8, 4, 1)            # the tiles of one frame given for two


# ---- the module --------------------------------------------------------------------------------------------------------------

def _resnet(no_layers=6, exact=False):
    cfg = O.canonical_config(no_layers=no_layers)
    spec = O.ResnetSpec.from_config(cfg["model"])
    params, state = O.init_params(spec, seed=42)
    m = bf.model_builder(cfg["model"], device="cuda").hydra
    m.set_weights(params, state)
    if exact:
        m.set_option("arith", 0)
    return m, spec, params, state


def _unet():
    cfg = U.canonical_config(depth=2, width=1)
    m = bf.model_builder(cfg["model"], device="cuda").hydra
    m.set_weights(U.init_params(U.UnetLaplacianSpec.from_config(cfg["model"]), seed=5))
    return m


_MODELS = {}


def _model(name):
    if name not in _MODELS:
        _MODELS[name] = {"resnet": lambda: _resnet()[0], "unet": _unet}[name]()
    return _MODELS[name]


def _by_hand(hydra, x: np.ndarray, T, Ov, M, tile_batch, cast):
    """the tiled call from its parts: NumPy split, the plain float module on the chunks of the batching contract, NumPy blend"""
    plain = bf.DenoiserModule(hydra, cast_to_uint8=False)
    B, H, W, _ = x.shape
    tiles = R.split(x, T, Ov)
    K, starts = R.chunk_starts(tiles.shape[0], tile_batch)
    results = np.empty(tiles.shape, dtype=np.float32)
    for s in starts:
        r = plain(tiles[s:s + K])
        assert r.dtype == np.float32 and r.shape == (K,) + tiles.shape[1:]
        results[s:s + K] = r
    return R.blend(results, B, H, W, T, Ov, M, cast)


@pytest.mark.parametrize("name, shape", [("resnet", (1, 50, 70, 3)), ("unet", (1, 48, 80, 3))], ids=["resnet", "unet"])
def test_end_to_end_is_the_hand_built_pipeline(name, shape):
    hydra = _model(name)
    x = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    for cast in (True, False):
        tiled = bf.TiledDenoiserModule(bf.DenoiserModule(hydra), tile=32, overlap=16, margin=4, tile_batch=5, cast_to_uint8=cast)
        ref = _by_hand(hydra, x, 32, 16, 4, 5, cast)
        got = tiled(x)                                               # NumPy in, NumPy out
        assert isinstance(got, np.ndarray) and _same(got, ref)
        assert tiled.last_plan == bf.tile_plan(shape[1], shape[2], 32, 16, 4) and tiled.last_plan.tiles > 5
        got_dev = tiled(_dev(x))                                     # device tensor in, device tensor out
        assert isinstance(got_dev, torch.Tensor) and got_dev.is_cuda and _same(got_dev.cpu().numpy(), ref)
        assert tiled.check_status() is True
        assert tiled(x[:0]).shape == (0,) + shape[1:] and tiled(x[:0]).dtype == np.uint8


def test_batching_contract_calls(monkeypatch):
    """what the hydra is called on: ceil(N / K) batches of [K, 32, 32, 3], the last one shifted back to tile N - K"""
    hydra = _model("resnet")
    tiled = bf.TiledDenoiserModule(bf.DenoiserModule(hydra), tile=32, overlap=16, margin=4, tile_batch=5)
    seen = []
    real = hydra.infer_u8
    monkeypatch.setattr(hydra, "infer_u8", lambda image, cast=True: (seen.append((image.cpu().numpy(), cast)), real(image, cast))[1])
    x = np.random.default_rng(3).integers(0, 256, (1, 64, 128, 3), dtype=np.uint8)
    tiled(_dev(x))
    tiles = R.split(x, 32, 16)
    n = tiles.shape[0]
    assert n == 21 and len(seen) == math.ceil(n / 5) and all(s[1] is False and s[0].shape == (5, 32, 32, 3) for s in seen)
    for k, s in enumerate(seen[:-1]):
        assert np.array_equal(s[0], tiles[5 * k:5 * k + 5])
    assert np.array_equal(seen[-1][0], tiles[n - 5:])
    del seen[:]
    tiled(_dev(x[:, :32, :48]))                                      # N = 2 < tile_batch: one call on both tiles
    assert len(seen) == 1 and np.array_equal(seen[0][0], R.split(x[:, :32, :48], 32, 16)) and seen[0][0].shape[0] == 2


def _errors(got, ref):
    d = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    return d.mean() / 255.0, d.max()


def test_locality_margin_of_the_receptive_radius_gives_the_whole_frame():
    """exact-fp32 kernels, 2 blocks: radius 5.  With M = 5 the tiled float output is the whole-frame oracle within the bars of
    test_gpu_inference.py (normalised MAE <= 1e-4, max error <= 0.05 grey levels); with M = 4, one pixel short, it is not (0.87
    grey levels on the CPU).  On 50 x 70 the whole frame is padded with black to 64 x 128 and a 32 x 32 tile is not: the bars hold
    outside the receptive radius of the bottom and right borders."""
    hydra, spec, params, state = _resnet(no_layers=2, exact=True)
    assert bf.receptive_radius(hydra) == 5
    module = bf.DenoiserModule(hydra)
    x = np.random.default_rng(1).integers(0, 256, (1, 64, 128, 3), dtype=np.uint8)
    ref = O.denoiser_module_call(spec, params, state, x, cast_to_uint8=False)
    tiled = bf.TiledDenoiserModule(module, tile=32, overlap=16, cast_to_uint8=False)
    assert tiled.margin == 5
    got = tiled(x)
    mae, worst = _errors(got, ref)
    print(f"M=5 on 64x128: normalised MAE {mae:.3e}, max error {worst:.3e}")
    assert got.dtype == np.float32 and np.isfinite(got).all()
    assert mae <= 1e-4 and worst <= 0.05
    short = bf.TiledDenoiserModule(module, tile=32, overlap=16, margin=4, cast_to_uint8=False)(x)
    print(f"M=4 on 64x128: max difference {_errors(short, ref)[1]:.3e}")
    assert _errors(short, ref)[1] > 0.5
    y = x[:, :50, :70]
    ref = O.denoiser_module_call(spec, params, state, y, cast_to_uint8=False)[:, :45, :65]
    mae, worst = _errors(tiled(y)[:, :45, :65], ref)
    print(f"M=5 on 50x70, [:45, :65]: normalised MAE {mae:.3e}, max error {worst:.3e}")
    assert mae <= 1e-4 and worst <= 0.05


@pytest.mark.parametrize("name", ["resnet", "unet"])
def test_a_tile_that_holds_the_frame_is_the_plain_module(name):
    hydra = _model(name)
    for shape, tile in (((2, 32, 32, 3), 32), ((1, 24, 40, 3) if name == "resnet" else (1, 32, 48, 3), 64)):
        x = np.random.default_rng(7).integers(0, 256, shape, dtype=np.uint8)
        for cast in (True, False):
            plain = bf.DenoiserModule(hydra, cast_to_uint8=cast)(x)
            tiled = bf.TiledDenoiserModule(bf.DenoiserModule(hydra), tile=tile, margin=4, cast_to_uint8=cast)
            got = tiled(x)
            assert got.dtype == (np.uint8 if cast else np.float32) and np.array_equal(got, plain), (shape, cast)
            assert tiled.last_plan.tiles == 1


# ---- with the other wrappers -------------------------------------------------------------------------------------------------

def test_composes_with_stabilisation_evaluation_and_the_risk_estimate():
    hydra = _model("resnet")
    module = bf.DenoiserModule(hydra)
    tiled = bf.TiledDenoiserModule(module, tile=32, overlap=16, margin=4, tile_batch=8)
    clean, noisy = O.synthetic_batch(2, 40, 56, seed=12)
    level = ([0.3, 0.5, 0.8], 4.0 + 1.0 / 12.0)
    stabilised = bf.StabilisedDenoiserModule(tiled, level)
    out = stabilised(_dev(noisy))
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == noisy.shape and stabilised.check_status()
    # the transform is per pixel: around the tiling it is the tiling of the transformed frame
    by_hand = bf.unstabilise(tiled.float_form()(bf.stabilise_u8(_dev(noisy), level)), level)
    assert torch.equal(out, by_hand)
    fitted = bf.StabilisedDenoiserModule(tiled)(noisy)
    assert isinstance(fitted, np.ndarray) and fitted.shape == noisy.shape and fitted.dtype == np.uint8

    plain = bf.evaluate(module, [clean], noise_std=(25,), seed=2)
    report = bf.evaluate(tiled, [clean], noise_std=(25,), seed=2)
    assert len(report) == 1 and set(report[0]) == set(plain[0]) and report[0]["images"] == 2
    assert all(np.isfinite(v) for v in report[0].values())
    assert report[0]["psnr_noisy"] == plain[0]["psnr_noisy"]        # the same noise went in

    base = bf.estimate_risk(module, _dev(noisy), probes=2)
    est = bf.estimate_risk(tiled, _dev(noisy), probes=2)
    assert all(bool(torch.isfinite(v).all()) for v in est) and tiled.check_status()
    assert torch.equal(est.sigma, base.sigma)
    whole = bf.TiledDenoiserModule(module, tile=64, margin=4)       # one tile per frame: the plain module, and so its estimate
    assert torch.equal(bf.estimate_risk(whole, _dev(noisy), probes=2).sums, base.sums)


def test_load_model_wraps_module_then_ensemble_then_tiles_then_stabilisation(tmp_path):
    hydra = _model("resnet")
    bf.save_model(hydra, str(tmp_path / "m"))
    _, noisy = O.synthetic_batch(1, 40, 56, seed=3)
    settings = {"tile": 32, "overlap": 16, "margin": 4, "tile_batch": 4}
    loaded = bf.load_model(str(tmp_path / "m"), device="cuda", tiled=settings)
    assert type(loaded) is bf.TiledDenoiserModule and type(loaded._module) is bf.DenoiserModule
    assert (loaded.tile, loaded.overlap, loaded.margin, loaded.tile_batch) == (32, 16, 4, 4)
    ref = bf.TiledDenoiserModule(bf.DenoiserModule(hydra), **settings)(noisy)
    assert np.array_equal(loaded(noisy), ref) and loaded.check_status()
    default = bf.load_model(str(tmp_path / "m"), device="cuda", tiled=True)
    assert (default.tile, default.margin, default.overlap) == (256, 13, 42)
    assert type(bf.load_model(str(tmp_path / "m"), device="cuda", tiled=False)) is bf.DenoiserModule

    full = bf.load_model(str(tmp_path / "m"), device="cuda", self_ensemble="flips", tiled=settings, stabilise=True)
    assert type(full) is bf.StabilisedDenoiserModule
    assert type(full._module) is bf.TiledDenoiserModule
    assert type(full._module._module) is bf.SelfEnsembleDenoiserModule
    assert type(full._module._module._module) is bf.DenoiserModule
    out = full(noisy)
    assert out.shape == noisy.shape and out.dtype == np.uint8 and full.check_status()
    assert full.last_noise_level is not None and full._module.last_plan.tiles == 6
    ensemble = bf.SelfEnsembleDenoiserModule(bf.DenoiserModule(hydra), "flips")
    assert np.array_equal(out, bf.StabilisedDenoiserModule(bf.TiledDenoiserModule(ensemble, **settings))(noisy))
