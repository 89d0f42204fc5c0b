"""GPU tests of csrc/bm3d.hip and Bm3dDenoiserModule.

Yardstick: tests/bm3d_reference.py.  The kernels add, multiply, compare and shift integers, divide integers with exact results,
and sum into 64-bit integer accumulators, where the order of the additions does not matter; the finish makes one correctly
rounded fp64 division and one cast, each of which NumPy does bit for bit the same: every comparison of a filtered image here is
exact (dtype, shape, array_equal)."""
import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
import bm3d_reference as R
import burst_reference
import nlm_reference
import tiling_reference
from guarded import dev as _dev, guard_bands

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guard_bands")]

# (H, W, C, search, step) at B = 2.  8 x 8 is one block (K = 1), 8 x 13 has the extra position n - 8, 16 x 16 has few candidates
# (small K), 37 x 45 is odd, 70 x 83 is larger than any search region, so that windows and groups lie anywhere in the frame
CASES = [(8, 8, 1, 12, 4), (8, 13, 3, 3, 4), (16, 16, 3, 12, 4), (16, 16, 4, 2, 8), (37, 45, 3, 12, 4), (37, 45, 1, 5, 3),
         (37, 45, 4, 12, 4), (37, 45, 1, 12, 1), (70, 83, 3, 12, 4), (70, 83, 2, 7, 5)]
_ids = {"ids": lambda c: "-".join(map(str, c))}
SIGMAS = [9.0, 14.0]                                                 # different parameters per image, around the scenes' sigma of 12
SMALL_GROUPS = (300.0, 48.0)                                         # match thresholds under which few candidates count


def _same(got, ref):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got, ref)


def _scene(H, W, C, seed, sigma=12.0, B=2):
    """structure plus noise, built as the scenes of tests/test_gpu_nlm.py: 4 x 4 blocks over smooth blobs, a flat quarter (blocks
    that repeat) and two single bright pixels, under white noise of `sigma`"""
    rng = np.random.default_rng(seed)
    images = np.empty((B, H, W, C), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for b in range(B):
        blocks = np.kron(rng.integers(0, 120, (-(H // -4), -(W // -4), C)), np.ones((4, 4, 1), np.int64))[:H, :W]
        blobs = 60 + 60 * np.sin(yy / 7.0 + seed + b)[..., None] * np.cos(xx / 5.0)[..., None]
        clean = np.clip(blocks + blobs, 0, 255).astype(np.float64)
        clean[:H // 2, :W // 2] = 40.0
        noisy = np.clip(np.rint(clean + rng.normal(0.0, sigma, clean.shape)), 0, 255)
        if H >= 16:
            noisy[H // 4, W // 4] = 255
            noisy[H - 3, W - 4] = 255
        images[b] = noisy
    return images


class _Reference:
    """both steps of the reference on one batch, computed once: step one, and step two on step one's uint8 result"""

    def __init__(self, images, prm, search, step):
        self.images, self.prm, self.search, self.step = images, prm, search, step
        self.one = R.step_batch(images, images, prm, search, step, False)
        self.basic = R.finish(self.one[0], self.one[1], True)
        self.two = R.step_batch(images, self.basic, prm, search, step, True)


_REFERENCES = {}


def _reference(case, match=R.MATCH) -> _Reference:
    if (case, match) not in _REFERENCES:
        H, W, C, r, st = case
        _REFERENCES[case, match] = _Reference(_scene(H, W, C, seed=sum(case)), R.params(SIGMAS, C, match=match), r, st)
    return _REFERENCES[case, match]


def _check_every_form(ref: _Reference):
    """step one alone, step two given the reference's basic estimate and bm3d end to end; uint8 and float32, with and without
    weights; each image alone"""
    r, st = ref.search, ref.step
    d_images, d_basic, d_prm = _dev(ref.images), _dev(ref.basic), _dev(ref.prm)
    for name, (num, den, _, _), guide, wiener in (("one", ref.one, d_images, False), ("two", ref.two, d_basic, True)):
        want_u8, want_f32 = R.finish(num, den, True), R.finish(num, den, False)
        got_u8, got_w = bf.bm3d_step(d_images, guide, d_prm, wiener, r, st, return_weights=True)
        assert got_u8.is_cuda and _same(got_u8, want_u8) and _same(got_w, den), f"step {name}: uint8 with weights"
        assert _same(bf.bm3d_step(d_images, guide, d_prm, wiener, r, st, cast_to_uint8=False), want_f32), f"step {name}: float32"
        assert _same(bf.bm3d_step(d_images, guide, d_prm, wiener, r, st), want_u8), f"step {name}: uint8 without weights"
        assert _same(bf.bm3d_step(d_images, guide, d_prm, wiener, r, st, False, True)[1], den), f"step {name}: float32 with weights"
        got_u8, got_w = bf.bm3d(d_images, d_prm, r, st, wiener, return_weights=True)
        assert _same(got_u8, want_u8) and _same(got_w, den), f"end to end, wiener {wiener}: uint8 with weights"
        assert _same(bf.bm3d(d_images, d_prm, r, st, wiener, cast_to_uint8=False), want_f32), f"end to end, wiener {wiener}: float32"
        for b in range(ref.images.shape[0]):                         # an image inside a batch gets the bits of that image alone
            assert _same(bf.bm3d(d_images[b:b + 1], d_prm[b:b + 1], r, st, wiener, False), want_f32[b:b + 1])


@pytest.mark.parametrize("case", CASES, **_ids)
def test_every_output_form_matches_numpy(case):
    _check_every_form(_reference(case))


def test_small_groups_match_numpy():
    ref = _reference((37, 45, 3, 12, 4), SMALL_GROUPS)
    for hist in (ref.one[2], ref.two[2]):
        assert hist[:4].sum() > hist[4] > 0, hist                    # groups below 16 dominate
    _check_every_form(ref)


def test_the_cases_reach_every_group_size_and_both_sides_of_the_shrinkage():
    """asserted on the reference's own outputs: over the case list every K in {1, 2, 4, 8, 16} occurs in each step, and
    coefficients are kept and zeroed in each"""
    refs = [_reference(case) for case in CASES]
    for step in ("one", "two"):
        hist = sum(getattr(ref, step)[2] for ref in refs)
        kept, zeroed = (sum(getattr(ref, step)[3][i] for ref in refs) for i in (0, 1))
        assert (hist > 0).all() and kept > 0 and zeroed > 0, (step, hist, kept, zeroed)
    assert _reference((8, 8, 1, 12, 4)).one[2].tolist() == [2, 0, 0, 0, 0]      # one block per image: K = 1


def _two_level_scene(H, W, C, seed, sigma=12.0, B=2):
    """random 4 x 4 blocks of 0 or 255 per channel and a flat quarter of 40 under white noise: values at both ends of the range"""
    rng = np.random.default_rng(seed)
    blocks = np.kron(rng.integers(0, 2, (B, -(H // -4), -(W // -4), C)) * 255, np.ones((1, 4, 4, 1), np.int64))[:, :H, :W].astype(np.float64)
    blocks[:, :H // 2, :W // 2] = 40.0
    return np.clip(np.rint(blocks + rng.normal(0.0, sigma, blocks.shape)), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("C", [1, 3])
def test_both_ends_of_the_range_are_clipped_as_numpy_clips(C):
    images = _two_level_scene(37, 45, C, seed=5)
    ref = _Reference(images, R.params([14.0, 14.0], C), 12, 4)
    for num, den, _, _ in (ref.one, ref.two):                        # the scene reaches both clips in both steps
        assert (num < 0).any() and (R.finish(num, den, False) > 255.0).any()
    _check_every_form(ref)


def test_ties_are_ordered_by_the_index():
    """a noise-free piecewise-constant image: many candidates have D = 0 and the index alone orders them"""
    rng = np.random.default_rng(31)
    images = np.kron(rng.integers(0, 256, (2, 4, 4, 3)), np.ones((1, 12, 12, 1), np.int64))[:, :37, :45].astype(np.uint8)
    images[:, :20, :24] = 40
    ref = _Reference(images, R.params([10.0, 10.0], 3), 12, 4)
    assert ref.one[2][4] > 0 and ref.two[2][4] > 0                   # full groups, of candidates at distance 0
    _check_every_form(ref)


def test_sigma_zero_returns_one_image_of_a_batch_unchanged():
    images = _scene(37, 45, 3, seed=3)
    prm = R.params([0.0, 12.0], 3)
    assert prm[0, 1] == 0 and prm[0, 3] == 0
    for wiener in (False, True):
        for cast in (True, False):
            out, weights = bf.bm3d(_dev(images), _dev(prm), 12, 4, wiener, cast, True)
            want, want_w = R.bm3d(images, prm, 12, 4, wiener, cast)
            assert _same(out, want) and _same(weights, want_w)
            out = out.cpu().numpy()
            assert np.array_equal(out[0], images[0]) and (out[1] != images[1]).mean() > 0.5


def test_params_on_the_device_are_numpy():
    sigmas = np.array([0.0, 0.5, 1.0, 7.25, 10.83, 20.0, 63.999, 255.0])
    for C in (1, 2, 3, 4):
        for threshold, match in ((2.7, R.MATCH), (3.1, SMALL_GROUPS)):
            got = bf.bm3d_params(_dev(sigmas), C, threshold, match)
            assert got.is_cuda and _same(got, R.params(sigmas, C, threshold, match))


# ---- the module --------------------------------------------------------------------------------------------------------------

def test_module_is_the_reference():
    images = _scene(37, 45, 3, seed=11)
    prm = R.params(SIGMAS, 3, 3.0)
    want, want_w = R.bm3d(images, prm, 5, 3)
    module = bf.Bm3dDenoiserModule(sigma=SIGMAS, search=5, step=3, threshold=3.0)
    got = module(images)                                             # NumPy in, NumPy out
    assert isinstance(got, np.ndarray) and _same(got, want) and _same(module.last_weights, want_w)
    got = module(_dev(images))                                       # device tensor in, device tensor out
    assert isinstance(got, torch.Tensor) and got.is_cuda and _same(got, want)
    flt = module.float_form()
    assert _same(flt(_dev(images)), R.bm3d(images, prm, 5, 3, cast_to_uint8=False)[0])
    assert flt.last_weights is module.last_weights and _same(flt.last_weights, want_w)
    per_channel = np.array([[9.0, 9.0, 9.0], [14.0, 14.0, 14.0]])    # [B,C]: the root mean square over the channels
    assert _same(bf.Bm3dDenoiserModule(sigma=per_channel, search=5, step=3, threshold=3.0)(images), want)
    grey = images[..., :1]                                           # one channel, the first step alone, sigma on the device
    module = bf.Bm3dDenoiserModule(sigma=_dev(np.array(SIGMAS)), search=3, wiener=False)
    assert _same(module(grey), R.bm3d(grey, R.params(SIGMAS, 1), 3, 4, False)[0])
    assert module(images[:0]).shape == (0, 37, 45, 3)


def test_module_estimates_sigma_on_the_device():
    images = _scene(37, 45, 3, seed=12)
    sigma = bf.estimate_noise(_dev(images), "mad")
    got = bf.Bm3dDenoiserModule(search=5)(_dev(images))
    assert torch.equal(got, bf.bm3d(_dev(images), bf.bm3d_params(sigma, 3), 5))
    assert _same(got, R.bm3d(images, R.params(sigma.cpu().numpy(), 3), 5)[0])


def test_inside_the_tiling_wrapper_it_is_the_hand_built_pipeline():
    images = _scene(37, 45, 3, seed=13)
    T, O, M = 16, 8, 2
    module = bf.TiledDenoiserModule(bf.Bm3dDenoiserModule(sigma=10.0, search=3), tile=T, overlap=O, margin=M, tile_batch=5)
    tiles = tiling_reference.split(images, T, O)
    filtered = R.bm3d(tiles, R.params(np.full(len(tiles), 10.0), 3), 3, 4, True, False)[0]
    want = tiling_reference.blend(filtered, 2, 37, 45, T, O, M, True)
    assert _same(module(images), want) and module.last_plan.tiles > 1 and module.check_status() is True
    assert _same(module(_dev(images)), want)


def test_inside_the_burst_wrapper_it_is_the_hand_built_pipeline():
    rng = np.random.default_rng(14)
    base = _scene(37 + 8, 45 + 8, 3, seed=14, sigma=0.0, B=1)[0].astype(np.float64)
    frames = np.empty((2, 3, 37, 45, 3), np.uint8)
    for b in range(2):
        for t in range(3):
            dy, dx = rng.integers(0, 9, 2)
            frames[b, t] = np.clip(np.rint(base[dy:dy + 37, dx:dx + 45] + rng.normal(0.0, 6.0, (37, 45, 3))), 0, 255)
    module = bf.BurstDenoiserModule(bf.Bm3dDenoiserModule(sigma=4.0, search=3), levels=2, search=3, sigma=6.0)
    field = burst_reference.align(frames, 0, 2, 3)
    merged, counts = burst_reference.merge(frames, field, burst_reference.thresholds([6.0, 6.0], 3), 0)
    filtered = R.bm3d(merged, R.params([4.0, 4.0], 3), 3, 4, True, False)[0]
    want = np.rint(np.clip(filtered, 0.0, 255.0)).astype(np.uint8)
    assert _same(module(frames), want) and _same(module.last_counts, counts)
    assert _same(module.float_form()(_dev(frames)), filtered)


def test_a_call_with_a_fixed_sigma_replays_from_a_graph():
    module = bf.Bm3dDenoiserModule(sigma=12.0, search=5)
    a, b = _dev(_scene(37, 45, 3, seed=15)), _dev(_scene(37, 45, 3, seed=16))
    want_a, want_b = module(a), module(b)                            # direct calls
    static_in = a.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = module(static_in)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out, want_a)
    static_in.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out, want_b) and not torch.equal(want_a, want_b)


# ---- quality -----------------------------------------------------------------------------------------------------------------

def test_load_model_bm3d_is_above_non_local_means_on_lena():
    """lena[128:384, 128:384] at sigma 20: the NumPy prototype gave 32.53 dB against about 30.5 of non-local means"""
    clean, noisy = nlm_reference.noisy_crop(nlm_reference.load_lena(), slice(128, 384), slice(128, 384), 20.0)
    module = bf.load_model("bm3d")
    assert type(module) is bf.Bm3dDenoiserModule
    out, nlm = module(noisy), bf.load_model("nlm")(noisy)
    psnr = nlm_reference.psnr
    print(f"noisy {psnr(noisy, clean):.2f} dB, nlm {psnr(nlm, clean):.2f} dB, bm3d {psnr(out, clean):.2f} dB")
    assert out.dtype == np.uint8 and out.shape == noisy.shape and psnr(out, clean) >= psnr(nlm, clean) + 1.5
    grey, clean_grey = noisy[..., 1:2], clean[..., 1:2]              # grey-scale frames: no network in the package takes them
    out, nlm = module(grey), bf.load_model("nlm")(grey)
    print(f"green channel: noisy {psnr(grey, clean_grey):.2f} dB, nlm {psnr(nlm, clean_grey):.2f} dB, bm3d {psnr(out, clean_grey):.2f} dB")
    assert psnr(out, clean_grey) >= psnr(nlm, clean_grey) + 1.0
