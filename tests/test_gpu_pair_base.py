"""GPU tests of the base convolution inside the first two-block launch (option h3_pair_base, csrc/fused_h3w.hip H3WMem<4>): the x0
rows that launch produces in LDS are bit for bit what base_conv_rows_kernel writes, so the whole forward is; against the fp64
oracle; and the forward status word, which that launch clears as the forward's first kernel.  uint8 input throughout; pairs are
forced with h3_pair = 2 and the row-streaming base kernel with base_rows = 2, so that small shapes reach both kernels."""
import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from oracle import bfcnn_oracle as O

pytestmark = pytest.mark.gpu

VECTOR, ROWS, IN_PAIR = "base_conv_kernel", "base_conv_rows_kernel", "fused_block2_h3w_kernel"


def _model(no_layers, seed):
    cfg = O.canonical_config(no_layers=no_layers)
    spec = O.ResnetSpec.from_config(cfg["model"])
    params, state = O.init_params(spec, seed=seed, nontrivial_bn=True)
    m = bf.model_builder(cfg["model"], device="cuda").hydra
    m.set_weights(params, state)
    return spec, params, state, m


@pytest.fixture
def forced():
    """h3_pair = 2 / base_rows = 2 on the models a test registers; base_rows is process-wide and goes back to its default"""
    models = []

    def register(m):
        m.set_option("h3_pair", 2)
        m.set_option("base_rows", 2)
        models.append(m)
        return m
    yield register
    for m in models:
        m.set_option("base_rows", 1)


def _f32(m, images):
    return m.infer_u8(images, cast_to_uint8=False).cpu().numpy()


# (blocks, (B, H, W), the path option 1 takes).  base_activation is linear: the engine builds no other (bf_create refuses relu, held
# in tests/test_base_path.py), so the producer's ReLU floor cannot be reached through a forward.  Padded frames: 1x1, 2x32, 8x128,
# 16x256 (two strips, one column of the second inside the image), 16x256, 64x256, 32x512 (four strips of 128 columns, the third
# partly and the fourth wholly outside the image: interior strips), 64x64 with a virtual band of 24 rows and 14 columns / exactly
# the frame, 70 images (280 units for 256 workgroups: bands that start inside the image), four blocks (only the first launch
# produces), three blocks (the single block runs first: the base kernel runs and the option has no effect)
CASES = [
    (2, (1, 1, 1), IN_PAIR),
    (2, (1, 2, 17), IN_PAIR),
    (2, (2, 5, 128), IN_PAIR),
    (2, (1, 13, 129), IN_PAIR),
    (2, (1, 9, 144), IN_PAIR),
    (2, (2, 40, 256), IN_PAIR),
    (2, (1, 24, 300), IN_PAIR),
    (2, (3, 40, 50), IN_PAIR),
    (2, (3, 64, 64), IN_PAIR),
    (2, (70, 40, 256), IN_PAIR),
    (4, (2, 40, 256), IN_PAIR),
    (3, (2, 40, 256), ROWS),
]


@pytest.mark.parametrize("no_layers,shape,path", CASES, ids=[f"{c[0]}blocks-{'x'.join(map(str, c[1]))}" for c in CASES])
def test_forward_is_bit_identical_with_the_base_convolution_inside_the_first_pair(no_layers, shape, path, forced):
    spec, params, state, m = _model(no_layers, seed=100 + no_layers)
    forced(m)
    B, H, W = shape
    rng = np.random.default_rng(B * 1000003 + H * 1009 + W)
    images = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).cuda()
    m.set_option("h3_pair_base", 1)
    assert m.base_path(B, H, W) == path                     # the fused path is taken where the rule says so: no passing by falling back
    fused = _f32(m, images)
    assert m.block_kernel()[0] == "fused_block2_h3w_kernel" and m.check_status()
    m.set_option("h3_pair_base", 0)
    assert m.base_path(B, H, W) == ROWS
    separate = _f32(m, images)
    assert m.check_status()
    assert np.isfinite(fused).all()
    assert np.array_equal(fused, separate)


def test_against_the_oracle_on_a_padded_ragged_shape(forced):
    """40 x 150 -> a 64 x 256 frame: two strips, the second one partly outside the image, 24 virtual rows; uint8 within 1 LSB and the
    float output at the bars of tests/test_gpu_inference.py"""
    spec, params, state, m = _model(4, seed=77)
    forced(m)
    _, noisy = O.synthetic_batch(3, 40, 150, seed=9)
    assert m.base_path(3, 40, 150) == IN_PAIR
    got = bf.DenoiserModule(m)(noisy)
    ref = O.denoiser_module_call(spec, params, state, noisy)
    d = np.abs(got.astype(np.int32) - ref.astype(np.int32))
    assert got.dtype == np.uint8 and got.shape == ref.shape and d.max() <= 1, f"max LSB diff {d.max()}"
    assert (d > 0).mean() < 0.01, f"{(d > 0).mean():.4f} of the pixels differ by 1 LSB"
    f = np.asarray(bf.DenoiserModule(m, cast_to_uint8=False)(noisy), np.float64)
    rf = O.denoiser_module_call(spec, params, state, noisy, cast_to_uint8=False)
    assert np.isfinite(f).all() and np.abs(f - rf).mean() / 255.0 <= 1e-4 and np.abs(f - rf).max() <= 0.05


def test_status_word_is_reported_and_then_cleared_by_the_first_pair_launch(forced):
    """activations beyond the f16 range are reported; the next ordinary forward, whose first kernel is the pair launch, starts
    from a clean status word"""
    spec, params, state, m = _model(2, seed=5)
    forced(m)
    m.auto_exact_fallback = False
    _, noisy = O.synthetic_batch(2, 64, 64, seed=3)
    assert m.base_path(2, 64, 64) == IN_PAIR
    big = params.copy()
    off = spec.offsets()
    for name in ("base/kernel", "block0/conv0/kernel"):
        o, shape = off[name]
        big[o:o + int(np.prod(shape))] *= 3000.0
    m.set_weights(big, state)
    with pytest.raises(FloatingPointError):
        bf.DenoiserModule(m)(noisy)
    assert not m.check_status(raise_on_overflow=False)
    m.set_weights(params, state)
    out = bf.DenoiserModule(m)(noisy)
    assert m.check_status()
    ref = O.denoiser_module_call(spec, params, state, noisy)
    assert np.abs(out.astype(np.int32) - ref.astype(np.int32)).max() <= 1
