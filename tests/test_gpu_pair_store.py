"""The store side of the pair kernel (csrc/fused_h3w.hip, H3W_DIRECT_STORE): the waves of the last role store their own 8-byte
half-records of an output row from registers (csrc/h3v_core.h h3_stream_store8) instead of staging the row in LDS for another role.
What can go wrong is addressing, not arithmetic: the plane, row or column of a record, the guards of the halo group of a strip, of a
ragged width and of the rows outside a band, the walk from the bottom, an offset that leaks into the neighbouring image.  So the
kernel's split-planar output is read where it lies, in the middle of the debug entry's scratch buffer, between the input planes
and the packed weights, inside a larger allocation full of sentinels."""
import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import _native as N
from oracle import bfcnn_oracle as O
from helpers import assert_close, conv3x3_gpu, dev, fused_block2_h3_gpu, host
from test_gpu_inference import _check_f32, _check_u8, _model
from test_gpu_kernels import _rand

pytestmark = pytest.mark.gpu

# smallest image; ragged W below one strip; second strip of one column; the 144-column grid clamped to the right edge, exact fit and
# one column over; the bench's strip geometry; three strips; interior strips with halo on both sides
SHAPES = [(1, 1, 1), (1, 3, 17), (2, 5, 129), (1, 13, 143), (1, 13, 144), (1, 13, 145), (3, 24, 256), (1, 7, 257), (1, 9, 520)]
GUARD = 4096                 # floats in front of and behind the scratch buffer
SENTINEL = 0x7FC5A5A5        # a quiet NaN as fp32, two NaNs as f16: nothing the kernels compute

_inputs, _runs = {}, {}


def _case(shape, relu):
    """small integers that hi + lo hold exactly through both blocks and their float64 result: once per (shape, activation), shared
    by both walking directions and both tests, never modified"""
    if (shape, relu) not in _inputs:
        B, H, W = shape
        rng = np.random.default_rng(7)                       # the weights first: the same at every shape

        def sparse(p, lo, hi):
            w = rng.integers(lo, hi + 1, (3, 3, 16, 16)).astype(np.float32)
            return w * (rng.random((3, 3, 16, 16)) < p)

        w4 = np.stack([sparse(0.15, -2, 2), sparse(0.15, -2, 2), sparse(0.06, -1, 1), sparse(0.06, -1, 1)])
        sc2, sh2 = np.ones((2, 16), np.float32), rng.integers(-3, 4, (2, 16)).astype(np.float32)
        x = rng.integers(-3, 4, (B, H, W, 16)).astype(np.float32)
        y = x.astype(np.float64)
        for b in range(2):
            t = O.conv2d_same(y, w4[2 * b].astype(np.float64))
            if relu:
                t = np.maximum(t, 0)
            y = y + O.conv2d_same(t, w4[2 * b + 1].astype(np.float64)) * sc2[b] + sh2[b]
            # every ring row is exact as f16 hi + f16 lo: integers below 2^15 (hi holds 11 bits, the rest is below 32)
            assert np.abs(t).max() < 2 ** 15 and np.abs(y).max() < 2 ** 15
        _inputs[(shape, relu)] = (x, w4, sc2, sh2, y)
    return _inputs[(shape, relu)]


def _run(shape, relu, reverse):
    """one launch through bf_debug_fused_block2_h3 with its scratch buffer inside a sentinel-filled allocation: (fp32 output, the whole
    allocation as int32 on the host); once per case"""
    key = (shape, relu, reverse)
    if key not in _runs:
        L = N.lib()
        B, H, W = shape
        x, w4, sc2, sh2, _ = _case(shape, relu)
        n = int(L.bf_debug_fused_block2_h3_scratch_floats(B, H, W))
        big = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
        xd, wd, sd, hd = dev(x), dev(w4), dev(sc2), dev(sh2)
        out = torch.full((B, H, W, 16), float("nan"), dtype=torch.float32, device="cuda")
        rc = L.bf_debug_fused_block2_h3(N.ptr(xd), N.ptr(wd), N.ptr(sd), N.ptr(hd), N.ptr(out), N.ptr(big[GUARD:GUARD + n]), B, H, W, relu,
                                        reverse, N.stream_ptr(xd))
        assert rc == 0, rc
        _runs[key] = (host(out), host(big.view(torch.int32)))
    return _runs[key]


def _planes(words, B, H, W):
    """[B * H * W * 16] fp32 words of a split-planar tensor -> (hi, lo) as float64 [B, H, W, 16]"""
    p = np.ascontiguousarray(words).view(np.float16).reshape(B, 4, H, W, 8).astype(np.float64)
    return np.concatenate([p[:, 0], p[:, 1]], axis=-1), np.concatenate([p[:, 2], p[:, 3]], axis=-1)


@pytest.mark.parametrize("reverse", [0, 1], ids=["down", "up"])
@pytest.mark.parametrize("relu", [1, 0], ids=["relu", "linear"])
@pytest.mark.parametrize("shape", SHAPES)
def test_pair_store_is_exact_on_small_integers(shape, relu, reverse):
    """as test_fused_block2_h3_is_exact_on_small_integers: every partial sum is exact, so the output equals the float64 result, not
    merely within a tolerance -- a record in the wrong row, column, plane or half shows as a wrong integer"""
    ref = _case(shape, relu)[4]
    got, _ = _run(shape, relu, reverse)
    assert np.array_equal(got.astype(np.float64), ref)


@pytest.mark.parametrize("reverse", [0, 1], ids=["down", "up"])
@pytest.mark.parametrize("relu", [1, 0], ids=["relu", "linear"])
@pytest.mark.parametrize("shape", SHAPES)
def test_pair_store_writes_every_record_and_nothing_else(shape, relu, reverse):
    """the kernel's own output, the split-planar tensor in the second B*H*W*16 floats of the scratch buffer: every record written (no
    sentinel left), every image's planes hold that image's values, and nothing around it touched -- the guard bands at both ends of
    the allocation keep their sentinels, the input planes in front of the output still hold the input, and the packed weights behind it
    are, word for word, what the same weights give at another shape"""
    B, H, W = shape
    x, _, _, _, ref = _case(shape, relu)
    _, words = _run(shape, relu, reverse)
    act = B * H * W * 16
    assert (words[:GUARD] == SENTINEL).all() and (words[-GUARD:] == SENTINEL).all(), "a guard band was written"
    body = words[GUARD:-GUARD]
    ya = body[act:2 * act]
    assert not (ya == SENTINEL).any(), f"{int((ya == SENTINEL).sum())} words of the output were never written"
    hi, lo = _planes(ya, B, H, W)
    for b in range(B):
        assert np.array_equal(hi[b] + lo[b], ref[b]), f"the planes of image {b} do not hold image {b}"
    xhi, xlo = _planes(body[:act], B, H, W)
    assert np.array_equal(xhi, x.astype(np.float64)) and not xlo.any(), "the input planes in front of the output changed"
    other = (1, 1, 1) if shape != (1, 1, 1) else (1, 3, 17)
    _, words2 = _run(other, relu, reverse)
    assert np.array_equal(body[2 * act:], words2[GUARD:-GUARD][2 * other[0] * other[1] * other[2] * 16:]), "the words behind the output changed"


def test_pair_store_more_units_than_workgroups():
    """70 x 40 x 256: 280 (image, band, strip) units on 256 workgroups, so some workgroups store the rows of a second unit, with the
    offsets of another image and strip; against the unfused exact-fp32 path at the bar of
    test_fused_block2_h3_many_units_persistent_schedule"""
    B, H, W = 70, 40, 256
    x = _rand((B, H, W, 16), 20)
    w4 = _rand((4, 3, 3, 16, 16), 21) * 0.1
    sc2, sh2 = np.ones((2, 16), np.float32), np.zeros((2, 16), np.float32)
    got = fused_block2_h3_gpu(x, w4, sc2, sh2, 1, 0)
    y = x
    for b in range(2):
        t = conv3x3_gpu(y, w4[2 * b], N.EPI_RELU)
        y = conv3x3_gpu(t, w4[2 * b + 1], N.EPI_RES, res=y)
    assert_close(got, y, rel=1e-5, what=f"two blocks vs unfused {(B, H, W)}")


@pytest.mark.parametrize("shape", [(2, 37, 150), (1, 24, 300)])
@pytest.mark.parametrize("no_layers", [2, 3, 6])
def test_pair_store_whole_networks(no_layers, shape):
    """whole networks on the uint8 path at ragged sizes (frames of 64 x 256: two strips, and 32 x 512: four), the blocks two per launch
    (h3_pair = 2: wherever there are two), the first pair launch of an even count computing the base convolution itself; the oracle
    bars of test_two_blocks_per_launch, and one grey level against one block per launch"""
    cfg, spec, params, state, m = _model(no_layers, seed=21)
    m.set_option("h3_pair", 2)
    B, H, W = shape
    line, launches = m.forward_plan(B, H, W)
    assert line.count("fused_block2_h3w_kernel") == no_layers // 2 and launches == (no_layers + 1) // 2, line
    _, noisy = O.synthetic_batch(B, H, W, seed=H + 3 * W)
    ref8 = O.denoiser_module_call(spec, params, state, noisy)
    got = bf.DenoiserModule(m)(noisy)
    _check_u8(got, ref8)
    _check_f32(bf.DenoiserModule(m, cast_to_uint8=False)(noisy), O.denoiser_module_call(spec, params, state, noisy, cast_to_uint8=False))
    m.set_option("h3_pair", 0)
    one = bf.DenoiserModule(m)(noisy)
    m.set_option("h3_pair", 1)
    _check_u8(one, ref8)
    assert np.abs(one.astype(int) - got.astype(int)).max() <= 1


def test_pair_store_head_launch_keeps_the_staging_rows():
    """h3_pair_head = 1 on a 2-block model: the launch with the head still stages its rows for the head storer; same bars"""
    cfg, spec, params, state, m = _model(2, seed=21)
    m.set_option("h3_pair", 2)
    m.set_option("h3_pair_head", 1)
    B, H, W = 2, 37, 150
    line, _ = m.forward_plan(B, H, W)
    assert "fused_block2_h3w_kernel:0+1" in line and "head" in line.split()[-1] and not line.endswith(" head"), line
    _, noisy = O.synthetic_batch(B, H, W, seed=H + 3 * W)
    _check_u8(bf.DenoiserModule(m)(noisy), O.denoiser_module_call(spec, params, state, noisy))
    _check_f32(bf.DenoiserModule(m, cast_to_uint8=False)(noisy), O.denoiser_module_call(spec, params, state, noisy, cast_to_uint8=False))
    m.set_option("h3_pair_head", 0)
    m.set_option("h3_pair", 1)
