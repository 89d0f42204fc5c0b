"""The schedule of a step of the pair kernel (csrc/fused_h3w.hip, H3W_EPI_ORDER and H3W_PREFETCH): the order of a group's MFMAs, the
place of the epilogues in their shadows, and the operands that are read one step early and carried across the barrier.  No
accumulator's own MFMA order changes, so the results are the same BITS as before; what can go wrong is an accumulator read too early or
a stale one, an epilogue in the wrong slot or phase of the accumulator rotation, and a prefetched operand that is not final yet or
belongs to the workgroup's previous band.  So: exact integers at shapes that put every phase, rotation, group and wave under a
position-dependent value; the recorded digests of the parent's output on ordinary floats; the launch that produces its x0 rows itself
against the one that fetches them; and more units than workgroups."""
import importlib.util
import json
import pathlib

import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import _native as N
from oracle import bfcnn_oracle as O
from helpers import dev, host

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
_spec = importlib.util.spec_from_file_location("record_pair_golden", ROOT / "tools" / "record_pair_golden.py")
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

# two strips, the second grid clamped to the right edge, 31 steps = every phase s % 6 five times; a second strip of one column; bands
# shorter than the pipeline; three strips
SHAPES = [(2, 19, 145), (1, 19, 129), (1, 3, 17), (1, 1, 1), (1, 7, 257)]

_inputs = {}


def _weights():
    """the recipe of tests/test_gpu_pair_store.py::_case: small sparse integer weights, the same at every shape"""
    rng = np.random.default_rng(7)

    def sparse(p, lo, hi):
        w = rng.integers(lo, hi + 1, (3, 3, 16, 16)).astype(np.float32)
        return w * (rng.random((3, 3, 16, 16)) < p)

    w4 = np.stack([sparse(0.15, -2, 2), sparse(0.15, -2, 2), sparse(0.06, -1, 1), sparse(0.06, -1, 1)])
    sc2, sh2 = np.ones((2, 16), np.float32), rng.integers(-3, 4, (2, 16)).astype(np.float32)
    return rng, w4, sc2, sh2


def _two_blocks_f64(x, w4, sc2, sh2, relu):
    y = x.astype(np.float64)
    for b in range(2):
        t = O.conv2d_same(y, w4[2 * b].astype(np.float64))
        if relu:
            t = np.maximum(t, 0)
        y = y + O.conv2d_same(t, w4[2 * b + 1].astype(np.float64)) * sc2[b] + sh2[b]
        # every ring row is exact as f16 hi + f16 lo: integers below 2^15 (hi holds 11 bits, the rest is below 32)
        assert np.abs(t).max() < 2 ** 15 and np.abs(y).max() < 2 ** 15
    return y


def _case(shape, relu):
    """small integers that hi + lo hold exactly through both blocks, and their float64 result: once per (shape, activation), shared by
    both walking directions, never modified"""
    if (shape, relu) not in _inputs:
        rng, w4, sc2, sh2 = _weights()
        x = rng.integers(-3, 4, shape + (16,)).astype(np.float32)
        _inputs[(shape, relu)] = (x, w4, sc2, sh2, _two_blocks_f64(x, w4, sc2, sh2, relu))
    return _inputs[(shape, relu)]


def _run(x, w4, sc2, sh2, relu, reverse):
    L = N.lib()
    B, H, W, _ = x.shape
    xd, wd, sd, hd = dev(x), dev(w4), dev(sc2), dev(sh2)
    out = torch.full((B, H, W, 16), float("nan"), dtype=torch.float32, device="cuda")
    scratch = torch.full((int(L.bf_debug_fused_block2_h3_scratch_floats(B, H, W)),), float("nan"), dtype=torch.float32, device="cuda")
    rc = L.bf_debug_fused_block2_h3(N.ptr(xd), N.ptr(wd), N.ptr(sd), N.ptr(hd), N.ptr(out), N.ptr(scratch), B, H, W, relu, reverse,
                                    N.stream_ptr(xd))
    assert rc == 0, rc
    return host(out)


@pytest.mark.parametrize("reverse", [0, 1], ids=["down", "up"])
@pytest.mark.parametrize("relu", [1, 0], ids=["relu", "linear"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pair_schedule_is_exact_on_small_integers(shape, relu, reverse):
    """every partial sum is exact, so the output EQUALS the float64 result: an accumulator read before its last MFMA, an epilogue of
    the wrong rotation phase or group, a residual operand of another row all show as a wrong integer"""
    x, w4, sc2, sh2, ref = _case(shape, relu)
    got = _run(x, w4, sc2, sh2, relu, reverse)
    assert np.array_equal(got.astype(np.float64), ref)


@pytest.mark.parametrize("reverse", [0, 1], ids=["down", "up"])
@pytest.mark.parametrize("shape", G.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pair_schedule_gives_the_parents_bits_on_ordinary_floats(shape, reverse):
    """seeded normal inputs and weights, where every partial sum rounds: the fp32 output has the sha256 recorded with the library from
    before the schedule changed (tools/record_pair_golden.py -> tests/golden/pair_schedule_parent.json)"""
    golden = json.loads((ROOT / "tests" / "golden" / "pair_schedule_parent.json").read_text())
    out = G.output(shape, reverse)
    assert np.isfinite(out).all()
    assert G.digest(out) == golden[G.key(shape, reverse)]


def _model(no_layers, seed):
    cfg = O.canonical_config(no_layers=no_layers)
    spec = O.ResnetSpec.from_config(cfg["model"])
    params, state = O.init_params(spec, seed=seed, nontrivial_bn=True)
    m = bf.model_builder(cfg["model"], device="cuda").hydra
    m.set_weights(params, state)
    return spec, params, state, m


@pytest.fixture
def forced():
    """h3_pair = 2 / base_rows = 2 as in tests/test_gpu_pair_base.py; base_rows is process-wide and goes back to its default"""
    models = []

    def register(m):
        m.set_option("h3_pair", 2)
        m.set_option("base_rows", 2)
        models.append(m)
        return m
    yield register
    for m in models:
        m.set_option("base_rows", 1)


@pytest.mark.parametrize("shape", [(2, 19, 145), (3, 40, 50)], ids=lambda s: "x".join(map(str, s)))
def test_producer_launch_equals_loader_launch(shape, forced):
    """two blocks: the one pair launch computes its x0 rows itself (h3_pair_base = 1: a row is complete only at the barrier in front of
    the step that consumes it) or fetches them (0); whatever one of the two reads early, the other does not"""
    spec, params, state, m = _model(2, seed=102)
    forced(m)
    B, H, W = shape
    rng = np.random.default_rng(B * 1000003 + H * 1009 + W)
    images = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).cuda()
    m.set_option("h3_pair_base", 1)
    assert m.base_path(B, H, W) == "fused_block2_h3w_kernel"
    fused = m.infer_u8(images, cast_to_uint8=False).cpu().numpy()
    assert m.block_kernel()[0] == "fused_block2_h3w_kernel" and m.check_status()
    m.set_option("h3_pair_base", 0)
    assert m.base_path(B, H, W) == "base_conv_rows_kernel"
    separate = m.infer_u8(images, cast_to_uint8=False).cpu().numpy()
    assert m.check_status()
    assert np.isfinite(fused).all() and np.array_equal(fused, separate)


def test_producer_launch_against_the_oracle():
    """four blocks at 40 x 150 (a 64 x 256 frame, two strips, the seed-9 batch of tests/test_gpu_pair_base.py): a producer launch and a
    loader launch; the bars of tests/test_gpu_inference.py: uint8 within 1 LSB, fewer than 1 % of the values off by one"""
    spec, params, state, m = _model(4, seed=77)
    m.set_option("h3_pair", 2)
    m.set_option("base_rows", 2)
    try:
        _, noisy = O.synthetic_batch(3, 40, 150, seed=9)
        assert m.base_path(3, 40, 150) == "fused_block2_h3w_kernel"
        got = bf.DenoiserModule(m)(noisy)
    finally:
        m.set_option("base_rows", 1)
    ref = O.denoiser_module_call(spec, params, state, noisy)
    d = np.abs(got.astype(np.int32) - ref.astype(np.int32))
    assert got.dtype == np.uint8 and got.shape == ref.shape and d.max() <= 1, f"max LSB diff {d.max()}"
    assert (d > 0).mean() < 0.01, f"{(d > 0).mean():.4f} of the values differ by 1 LSB"


def test_pair_schedule_more_units_than_workgroups():
    """70 x 40 x 256: 280 (image, band, strip) units on 256 workgroups, so some workgroups walk a second band, of another image: it must
    not see an operand prefetched in the first.  Exact integers; seven distinct images repeated ten times keep the float64 reference
    small (units u and u + 256 lie 64 images apart: 64 mod 7 = 1, never the same image)"""
    rng, w4, sc2, sh2 = _weights()
    base = rng.integers(-3, 4, (7, 40, 256, 16)).astype(np.float32)
    ref7 = _two_blocks_f64(base, w4, sc2, sh2, True)
    idx = np.arange(70) % 7
    got = _run(base[idx], w4, sc2, sh2, 1, 0)
    assert np.array_equal(got.astype(np.float64), ref7[idx])
