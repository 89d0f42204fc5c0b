"""GPU tests of csrc/burst.hip and BurstDenoiserModule.

Yardstick: tests/burst_reference.py.  The kernels add, compare and divide integers and make one correctly rounded fp64 division and
one cast, each of which NumPy does bit for bit the same: every comparison here is exact."""
import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from oracle import bfcnn_oracle as O
import burst_reference as R
from guarded import dev as _dev, guard_bands

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guard_bands")]

# (H, W, C, T, reference, levels, search) at B = 2.  5 x 7 is smaller than a tile, 16 x 16 is one tile, 37 x 45 is odd at every level
# and has cut edge tiles, 64 x 96 has six tiles in a row (two workgroups of four waves, the second half empty)
CASES = [(5, 7, 1, 1, 0, 1, 1), (5, 7, 3, 2, 1, 4, 4), (5, 7, 3, 5, 0, 3, 7),
         (16, 16, 3, 2, 0, 1, 4), (16, 16, 1, 5, 4, 3, 1), (16, 16, 3, 1, 0, 4, 7),
         (37, 45, 3, 5, 4, 3, 4), (37, 45, 1, 2, 0, 4, 7), (37, 45, 3, 2, 1, 1, 1), (37, 45, 1, 5, 0, 3, 7),
         (64, 96, 3, 5, 0, 3, 4), (64, 96, 1, 2, 1, 4, 1), (64, 96, 3, 2, 0, 1, 7), (64, 96, 3, 5, 4, 4, 4)]
_ids = {"ids": lambda c: "-".join(map(str, c))}


def _same(got, ref):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got, ref)


def _texture(H, W, C, seed):
    """smooth blobs under 4 x 4 blocks: structure at every level of the pyramid"""
    rng = np.random.default_rng(seed)
    blocks = np.kron(rng.integers(0, 120, (-(H // -4), -(W // -4), C)), np.ones((4, 4, 1), np.int64))[:H, :W]
    yy, xx = np.mgrid[0:H, 0:W]
    blobs = 60 + 60 * np.sin(yy / 7.0 + seed)[..., None] * np.cos(xx / 5.0)[..., None]
    return np.clip(blocks + blobs, 0, 255).astype(np.uint8)


def _scene(H, W, C, T, seed, shift=6, sigma=6.0, B=2):
    """B bursts of different content: crops of a texture at random shifts within +-`shift` under noise of `sigma`"""
    rng = np.random.default_rng(seed)
    frames = np.empty((B, T, H, W, C), np.uint8)
    for b in range(B):
        big = _texture(H + 2 * shift, W + 2 * shift, C, seed + 17 * b)
        for t in range(T):
            dy, dx = rng.integers(0, 2 * shift + 1, 2)
            crop = big[dy:dy + H, dx:dx + W].astype(np.float64)
            frames[b, t] = np.clip(np.rint(crop + rng.normal(0.0, sigma, crop.shape)), 0, 255)
    return frames


def _check_align(frames, ref, K, R_):
    want_pyramid, want_field = R.pyramid(frames, K), R.align(frames, ref, K, R_)
    got_pyramid = bf.burst_pyramid(_dev(frames), K)
    assert len(got_pyramid) == K and all(_same(g, w) for g, w in zip(got_pyramid, want_pyramid)), "pyramid"
    field = bf.burst_align(_dev(frames), ref, K, R_)
    assert field.is_cuda and _same(field, want_field), "field"
    return field, want_field


def _check_merge(frames, field, thr, ref):
    """every output form of the merge against the reference; returns the reference's counts"""
    d_frames, d_field, d_thr = _dev(frames), _dev(field), _dev(thr)
    want_u8, want_counts = R.merge(frames, field, thr, ref, True)
    want_f32, _ = R.merge(frames, field, thr, ref, False)
    got_u8, got_counts = bf.burst_merge(d_frames, d_field, d_thr, ref, return_counts=True)
    assert _same(got_u8, want_u8) and _same(got_counts, want_counts), "uint8 with counts"
    got_f32 = bf.burst_merge(d_frames, d_field, d_thr, ref, cast_to_uint8=False)
    assert isinstance(got_f32, torch.Tensor) and _same(got_f32, want_f32), "float32 without counts"
    assert _same(bf.burst_merge(d_frames, d_field, d_thr, ref), want_u8), "uint8 without counts"
    assert _same(bf.burst_merge(d_frames, d_field, d_thr, ref, False, True)[1], want_counts), "float32 with counts"
    return want_counts


# ---- pyramid, field and merge against the reference --------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, **_ids)
def test_pyramid_field_and_merge_match_numpy(case):
    H, W, C, T, ref, K, R_ = case
    frames = _scene(H, W, C, T, seed=sum(case))
    field, want_field = _check_align(frames, ref, K, R_)
    thr = R.thresholds([4.0, 7.0], C)                               # different thresholds per image, around the scene's sigma of 6
    counts = _check_merge(frames, want_field, thr, ref)
    if T == 1:
        assert (counts == (256, 65536)).all()
    if (H, T) == (64, 5):                                           # the scenes exercise the three weight branches
        den = counts[..., 0]
        assert (den == 256).any() and (den == 256 * T).any() and (den % 256 != 0).any()
    for b in range(2):                                              # an image inside a batch gets the bits of that image alone
        assert _same(bf.burst_align(_dev(frames[b:b + 1]), ref, K, R_), want_field[b:b + 1])


# ---- alignment inputs --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K, R_", [(1, 4), (3, 7), (4, 1)])
def test_alignment_of_noise_and_of_constant_frames(K, R_):
    noise = np.random.default_rng(K).integers(100, 104, (2, 3, 37, 45, 3), dtype=np.uint8)       # four grey levels: many near-ties
    _check_align(noise, 1, K, R_)
    flat = np.full((2, 3, 37, 45, 1), 77, np.uint8)
    flat[:, 1] = 0
    flat[1, 2] = 255                                                # other constants: every candidate of a tile costs the same
    field, _ = _check_align(flat, 0, K, R_)
    assert not field.any()                                          # the tie rule


@pytest.mark.parametrize("K, R_", [(1, 4), (3, 4), (2, 7)])
def test_alignment_of_shifts_past_the_frame_and_beyond_the_reach(K, R_):
    H, W = 37, 45
    big = _texture(H + 80, W + 80, 3, 5)
    shifts = [(0, 0), (3, -2), (-30, 38), (40, 40), (-40, -17)]      # within reach of (1, 4); windows far past the frame; beyond any reach here
    frames = np.stack([big[40 + dy:40 + dy + H, 40 + dx:40 + dx + W] for dy, dx in shifts])[None]
    field, _ = _check_align(frames, 0, K, R_)
    assert (field[0, 1, 1, 1].cpu().numpy() == (-3, 2)).all()       # the interior tile finds alt(p + d) = ref(p)
    _check_merge(frames, field.cpu().numpy(), R.thresholds([3.0], 3), 0)


# ---- merge inputs ------------------------------------------------------------------------------------------------------------

def test_merge_weight_branches_at_the_thresholds():
    frames = np.full((6, 2, 16, 20, 1), 100, np.uint8)
    frames[:, 1, 8, 8] = 110                                        # D = 100 in the 5 x 5 windows that hold (8, 8), else 0
    field = np.zeros((6, 2, 1, 2, 2), np.int32)
    # D == lo; D == hi; ramp in 32 bits; ramp of two steps; ramp in 64 bits (hi - lo >= 2^23); all below lo near 2^40
    thr = np.array([[100, 101], [99, 100], [0, 200], [99, 101], [50, 1 << 40], [(1 << 40) - 7, (1 << 40) + 5]], np.int64)
    counts = _check_merge(frames, field, thr, 0)
    assert counts[:, 8, 8, 0].tolist() == [512, 256, 384, 384, 511, 512] and (counts[:, 0, 0, 0] == 512).all()
    frames3 = np.repeat(frames, 3, axis=-1)                         # three channels: D = 300
    thr3 = np.array([[300, 301], [299, 300], [0, 600], [299, 301], [50, 1 << 40], [0, 1]], np.int64)
    counts = _check_merge(frames3, field, thr3, 1)                  # and the other frame as the reference
    assert counts[:, 8, 8, 0].tolist() == [512, 256, 384, 384, 511, 256]


def test_merge_with_sigma_zero_thresholds_and_any_displacement():
    frames = _scene(37, 45, 3, 4, seed=9, sigma=0.0, shift=3)
    frames[1] = frames[1, :1]                                       # identical frames: everything merges at (0, 1)
    thr = R.thresholds([0.0, 0.0], 3)
    assert thr.tolist() == [[0, 1], [0, 1]] and _same(bf.burst_thresholds(_dev(np.zeros(2)), 3), thr)
    zero = np.zeros((2, 4, 3, 3, 2), np.int32)
    counts = _check_merge(frames, zero, thr, 2)
    assert (counts[1] == (4 * 256, 4 * 65536)).all() and (counts[0, ..., 0] < 4 * 256).any()
    rng = np.random.default_rng(3)
    field = rng.integers(-60, 61, zero.shape).astype(np.int32)      # past the frame: the clamp path of every pixel
    field[0, 1, 0, 0], field[0, 1, 2, 2], field[1, 3, 1, 1] = (2 ** 31 - 1, -2 ** 31), (-2 ** 31, 2 ** 31 - 1), (2 ** 31 - 1, 2 ** 31 - 1)
    _check_merge(frames, field, R.thresholds([5.0, 40.0], 3), 0)    # hi - lo = 22 501 and 360 001


def test_thresholds_on_the_device_are_numpy():
    sigmas = np.array([0.0, 0.5, 1.0, 7.25, 20.0, 63.999, 255.0])
    for C, k in ((1, (1.5, 3.0)), (3, (1.5, 3.0)), (4, (1.25, 2.0))):
        got = bf.burst_thresholds(_dev(sigmas), C, *k)
        assert got.is_cuda and _same(got, R.thresholds(sigmas, C, *k))


# ---- the module around a callable --------------------------------------------------------------------------------------------

def _callable_denoiser(u8):
    return u8.float() * 0.5 + 3.25


def _callable_reference(u8: np.ndarray) -> np.ndarray:
    return u8.astype(np.float32) * np.float32(0.5) + np.float32(3.25)


def _to_uint8(x: np.ndarray) -> np.ndarray:
    return np.rint(np.clip(x, 0.0, 255.0)).astype(np.uint8)


def test_module_is_the_reference_pipeline():
    frames = _scene(37, 45, 3, 4, seed=21)
    sigma = [5.0, 8.0]
    field = R.align(frames, 1, 2, 3)
    merged, counts = R.merge(frames, field, R.thresholds(sigma, 3, 1.0, 2.5), 1)
    module = bf.BurstDenoiserModule(_callable_denoiser, reference=1, levels=2, search=3, sigma=sigma, k=(1.0, 2.5))
    want = _to_uint8(_callable_reference(merged))
    got = module(frames)                                            # NumPy in, NumPy out
    assert isinstance(got, np.ndarray) and _same(got, want)
    assert _same(module.last_counts, counts) and _same(module.last_field, field)
    got = module(_dev(frames))                                      # device tensor in, device tensor out
    assert isinstance(got, torch.Tensor) and got.is_cuda and _same(got, want)
    flt = module.float_form()
    assert _same(flt(_dev(frames)), _callable_reference(merged))    # before the rounding: the float denoiser on the merged uint8
    assert flt.last_counts is module.last_counts and module.check_status() is True
    alone = bf.BurstDenoiserModule(None, reference=1, levels=2, search=3, sigma=_dev(np.array(sigma)), k=(1.0, 2.5))
    assert _same(alone(frames), merged)
    assert _same(alone.float_form()(_dev(frames)), R.merge(frames, field, R.thresholds(sigma, 3, 1.0, 2.5), 1, False)[0])
    assert alone(frames[:0]).shape == (0, 37, 45, 3)


def test_module_estimates_sigma_on_the_device():
    frames = _scene(64, 96, 3, 3, seed=22, sigma=10.0)
    module = bf.BurstDenoiserModule(None)
    sigma = bf.estimate_noise(_dev(frames[:, 0]), "mad")
    thr = bf.burst_thresholds(sigma, 3).cpu().numpy()
    assert _same(module(frames), R.merge(frames, R.align(frames), thr, 0)[0])
    single = frames[:, :1]
    assert _same(module(single), single[:, 0]) and module.last_counts is None
    assert _same(bf.BurstDenoiserModule(_callable_denoiser)(single), _to_uint8(_callable_reference(single[:, 0])))


# ---- with a real model and the other wrappers --------------------------------------------------------------------------------

_MODEL = []


def _resnet():
    if not _MODEL:
        cfg = bf.CONFIGS_DICT["resnet_color_1x6_bn_16x3x3_256x256_l1_relu"]          # the shipped 1x6 configuration
        spec = O.ResnetSpec.from_config(cfg["model"])
        params, state = O.init_params(spec, seed=42)
        m = bf.model_builder(cfg["model"], device="cuda").hydra
        m.set_weights(params, state)
        _MODEL.append(m)
    return _MODEL[0]


def test_one_frame_is_the_wrapped_module():
    module = bf.DenoiserModule(_resnet())
    x = _dev(_scene(32, 32, 3, 1, seed=30))
    burst = bf.BurstDenoiserModule(module)
    assert torch.equal(burst(x), module(x[:, 0])) and burst.check_status() is True
    assert np.array_equal(burst(x.cpu().numpy()), module(x[:, 0].cpu().numpy()))
    assert torch.equal(burst.float_form()(x), module.float_form()(x[:, 0].contiguous()))
    assert burst(x[:0]).shape == (0, 32, 32, 3)


def test_real_model_is_the_hand_built_pipeline():
    module = bf.DenoiserModule(_resnet())
    x = _dev(_scene(32, 48, 3, 4, seed=31))
    burst = bf.BurstDenoiserModule(module, sigma=6.0)
    merged = bf.burst_merge(x, bf.burst_align(x), bf.burst_thresholds(_dev(np.full(2, 6.0)), 3))
    assert torch.equal(burst(x), module(merged)) and burst.check_status() is True
    assert np.array_equal(burst(x.cpu().numpy()), module(merged).cpu().numpy())
    assert torch.equal(burst.float_form()(x), module.float_form()(merged))


def test_stacks_over_tiles_and_self_ensemble():
    module = bf.DenoiserModule(_resnet())
    x = _dev(_scene(32, 48, 3, 3, seed=32))
    merged = bf.burst_merge(x, bf.burst_align(x), bf.burst_thresholds(_dev(np.full(2, 6.0)), 3))
    tiled = bf.TiledDenoiserModule(module, tile=16, overlap=8, margin=2, tile_batch=8)
    burst = bf.BurstDenoiserModule(tiled, sigma=6.0)
    assert torch.equal(burst(x), tiled(merged)) and tiled.last_plan.tiles > 1 and burst.check_status() is True
    ensemble = bf.SelfEnsembleDenoiserModule(module, transforms="flips")
    burst = bf.BurstDenoiserModule(ensemble, sigma=6.0)
    assert torch.equal(burst(x), ensemble(merged)) and burst.check_status() is True
    assert torch.equal(burst.float_form()(x), ensemble.float_form()(merged))


def test_a_call_replays_from_a_graph():
    module = bf.DenoiserModule(_resnet())
    burst = bf.BurstDenoiserModule(module, sigma=6.0)
    a, b = _dev(_scene(32, 48, 3, 3, seed=33)), _dev(_scene(32, 48, 3, 3, seed=34))
    want_a, want_b = burst(a), burst(b)                             # direct calls (also the warm-up: packing, workspace, attributes)
    static_in = a.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = burst(static_in)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out, want_a)
    static_in.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out, want_b) and not torch.equal(want_a, want_b)


def test_load_model_wraps_bursts_outermost(tmp_path):
    bf.save_model(_resnet(), str(tmp_path / "m"))
    x = _scene(32, 48, 3, 3, seed=35)
    loaded = bf.load_model(str(tmp_path / "m"), device="cuda", burst={"sigma": 6.0, "levels": 2})
    assert type(loaded) is bf.BurstDenoiserModule and type(loaded._module) is bf.DenoiserModule and loaded.levels == 2
    assert np.array_equal(loaded(x), bf.BurstDenoiserModule(bf.DenoiserModule(_resnet()), sigma=6.0, levels=2)(x)) and loaded.check_status()
    assert type(bf.load_model(str(tmp_path / "m"), device="cuda", burst=False)) is bf.DenoiserModule
    full = bf.load_model(str(tmp_path / "m"), device="cuda", tiled={"tile": 16, "overlap": 8, "margin": 2}, stabilise=True, burst=True)
    assert type(full) is bf.BurstDenoiserModule and type(full._module) is bf.StabilisedDenoiserModule
    assert type(full._module._module) is bf.TiledDenoiserModule
    out = full(x)
    assert out.shape == (2, 32, 48, 3) and out.dtype == np.uint8 and full.check_status() and full.last_counts.shape == (2, 32, 48, 2)
