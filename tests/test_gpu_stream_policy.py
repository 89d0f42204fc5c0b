"""The activation stream of the pair, one-block and head kernels under its cache policy (csrc/h3v_core.h: H3_LOAD_POLICY,
H3_STORE_POLICY, h3_dma16 / h3_stream_store16 / h3_stream_load16).  A policy moves the same bytes, so what can go wrong is not
arithmetic: a store that goes nowhere (a buffer resource with the wrong extent drops a record without a fault), a row or column
that is never written, a 32-bit extent or offset on a tensor of more than 4 GiB, a store past the end of the output.  Every test
starts from buffers full of sentinels and holds the result to the oracle and the bars of the existing tests of the same kernel."""
import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import _native as N
from oracle import bfcnn_oracle as O
from helpers import assert_close, fused_block2_h3_gpu, fused_block_h3_gpu
from test_gpu_inference import _check_f32, _check_u8
from test_gpu_kernels import _rand, _two_blocks_oracle

pytestmark = pytest.mark.gpu

_refs = {}


def _pair_case(H, W):
    """inputs and the fp64 oracle of a pair case: computed once per shape, shared by both walking directions, never modified"""
    if (H, W) not in _refs:
        x = _rand((3, H, W, 16), 15)
        w4 = _rand((4, 3, 3, 16, 16), 16) * 0.1
        sc2, sh2 = _rand((2, 16), 18), _rand((2, 16), 19)
        _refs[(H, W)] = (x, w4, sc2, sh2, _two_blocks_oracle(x, w4, sc2, sh2, 1))
    return _refs[(H, W)]


# a strip of one column (1, 129, 257), a grid clamped to the right edge (129, 144), to both (1, 127), the last strip of three (257);
# a band shorter than the 12-step pipeline (both heights); the last row and column of the last image (B = 3)
@pytest.mark.parametrize("reverse", [0, 1], ids=["down", "up"])
@pytest.mark.parametrize("H", [1, 13])
@pytest.mark.parametrize("W", [1, 127, 129, 144, 257])
def test_pair_kernel_writes_every_element(W, H, reverse):
    """fused_block2_h3w_kernel through its debug entry: the fp32 output and the scratch buffer (which holds the kernel's split-planar
    output) start as NaN; a record the kernel does not store stays NaN in the hi or the lo plane and comes out as NaN."""
    x, w4, sc2, sh2, ref = _pair_case(H, W)
    got = fused_block2_h3_gpu(x, w4, sc2, sh2, 1, reverse)
    assert not np.isnan(got).any(), f"{int(np.isnan(got).sum())} elements were never written"
    assert_close(got, ref, what=f"two fused h3 blocks {(3, H, W)} reverse {reverse}")


def test_pair_kernel_batch_tensor_larger_than_4_gib():
    """B = 65 at 1024 x 1024: 4.36 GB per split-planar tensor, so image 64 starts past 2^32 bytes.  Images 0 and 64 of the batched launch
    must equal, bit for bit, the same images launched alone (B = 1): a 32-bit extent or offset in the store (or load) path drops or
    misplaces the records of the last image.  Everything stays on the device."""
    L = N.lib()
    B, H, W = 65, 1024, 1024
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn((B, H, W, 16), dtype=torch.float32, device="cuda", generator=g)
    w = torch.randn((4, 3, 3, 16, 16), dtype=torch.float32, device="cuda", generator=g) * 0.1
    sc = torch.randn((2, 16), dtype=torch.float32, device="cuda", generator=g)
    sh = torch.randn((2, 16), dtype=torch.float32, device="cuda", generator=g)

    def run(xin):
        b = xin.shape[0]
        out = torch.full((b, H, W, 16), float("nan"), dtype=torch.float32, device="cuda")
        scratch = torch.full((int(L.bf_debug_fused_block2_h3_scratch_floats(b, H, W)),), float("nan"), dtype=torch.float32, device="cuda")
        rc = L.bf_debug_fused_block2_h3(N.ptr(xin), N.ptr(w), N.ptr(sc), N.ptr(sh), N.ptr(out), N.ptr(scratch), b, H, W, 1, 0,
                                        N.stream_ptr(xin))
        assert rc == 0, rc
        return out

    try:
        assert x.numel() * 4 > 1 << 32
        full = run(x)
        for i in (0, B - 1):
            alone = run(x[i:i + 1])
            assert not torch.isnan(alone).any()
            assert torch.equal(full[i:i + 1], alone), f"image {i} of the batch differs from the image launched alone"
            del alone
    finally:
        del x
        full = None
        torch.cuda.empty_cache()


def test_pair_kernel_image_larger_than_2_gib():
    """One image of 6000 x 6000: 2.3 GB split-planar, so the last 1600 rows of its fourth plane lie past 2^31 bytes inside the image: the
    sizes at which a SIGNED 32-bit extent, row offset or lane offset of the store path goes wrong (the >4 GiB test does not reach them: its
    images are 64 MiB).  No element stays NaN, and the first and last 36 rows equal, bit for bit, the same rows computed from the
    first / last 40 rows alone (two blocks see four rows up and down)."""
    L = N.lib()
    H, W, K = 6000, 6000, 40
    g = torch.Generator(device="cuda").manual_seed(6)
    x = torch.randn((1, H, W, 16), dtype=torch.float32, device="cuda", generator=g)
    w = torch.randn((4, 3, 3, 16, 16), dtype=torch.float32, device="cuda", generator=g) * 0.1
    sc = torch.randn((2, 16), dtype=torch.float32, device="cuda", generator=g)
    sh = torch.randn((2, 16), dtype=torch.float32, device="cuda", generator=g)

    def run(xin):
        h = xin.shape[1]
        out = torch.full((1, h, W, 16), float("nan"), dtype=torch.float32, device="cuda")
        scratch = torch.full((int(L.bf_debug_fused_block2_h3_scratch_floats(1, h, W)),), float("nan"), dtype=torch.float32, device="cuda")
        rc = L.bf_debug_fused_block2_h3(N.ptr(xin), N.ptr(w), N.ptr(sc), N.ptr(sh), N.ptr(out), N.ptr(scratch), 1, h, W, 1, 0,
                                        N.stream_ptr(xin))
        assert rc == 0, rc
        return out

    try:
        assert 1 << 31 < H * W * 64 < 1 << 32
        full = run(x)
        assert not torch.isnan(full).any(), "elements were never written"
        top, bottom = run(x[:, :K].contiguous()), run(x[:, H - K:].contiguous())
        assert torch.equal(full[:, :K - 4], top[:, :K - 4]), "first rows"
        assert torch.equal(full[:, H - K + 4:], bottom[:, 4:]), "last rows (past 2^31 bytes inside the image)"
    finally:
        del x
        full = top = bottom = None
        torch.cuda.empty_cache()


@pytest.fixture(params=[4, 260], ids=["fullrow", "fullrow_up"])
def fullrow(request):
    N.lib().bf_debug_set_h3_variant(request.param)
    yield request.param
    N.lib().bf_debug_set_h3_variant(-1)


# one column, the last column missing from the last 64-column piece (255), every piece full (256)
@pytest.mark.parametrize("H", [1, 13])
@pytest.mark.parametrize("W", [1, 255, 256])
def test_one_block_kernel_writes_every_element(W, H, fullrow):
    """fused_block_h3v_kernel (shares the helpers) through its debug entry, both walking directions: output and scratch start as NaN."""
    x = _rand((3, H, W, 16), 15)
    w1, w2 = _rand((3, 3, 16, 16), 16) * 0.1, _rand((3, 3, 16, 16), 17) * 0.1
    sc, sh = _rand(16, 18), _rand(16, 19)
    x64 = x.astype(np.float64)
    t = np.maximum(O.conv2d_same(x64, w1.astype(np.float64)), 0)
    ref = x64 + O.conv2d_same(t, w2.astype(np.float64)) * sc + sh
    got = fused_block_h3_gpu(x, w1, w2, sc, sh, 1)
    assert not np.isnan(got).any(), f"{int(np.isnan(got).sum())} elements were never written"
    assert_close(got, ref, what=f"fused h3 {(3, H, W)} variant {fullrow}")


GUARD = 4096      # elements behind the output that the head must leave alone


# one pixel; a crop in both directions (19 x 23 out of the 32 x 32 frame: the public entries pad to powers of two, a 24-row frame is
# not reachable through them) with B = 2; several workgroups whose last one is ragged (1800 pixels)
@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 19, 23), (3, 20, 30)])
def test_head_kernel_writes_its_output_and_nothing_behind_it(shape, u8):
    """head_kernel on the split-planar activation (bf_forward_u8 / bf_forward_u8_f32 into a caller's buffer full of sentinels, with a
    guard band behind it): the bars of test_gpu_inference.py against the oracle, every element written, none past B*Ho*Wo*3."""
    cfg = O.canonical_config(no_layers=2)
    spec = O.ResnetSpec.from_config(cfg["model"])
    params, state = O.init_params(spec, seed=21, nontrivial_bn=True)
    m = bf.model_builder(cfg["model"], device="cuda").hydra
    m.set_weights(params, state)
    m.set_option("h3_variant", 4)                     # the full-row streaming kernels at this size: split-planar activations
    B, H, W = shape
    line, _ = m.forward_plan(B, H, W)
    assert line.startswith("split ") and line.endswith(" head"), line          # the head KERNEL runs, on split-planar features
    _, noisy = O.synthetic_batch(B, H, W, seed=H + 3 * W)
    ref = O.denoiser_module_call(spec, params, state, noisy, cast_to_uint8=u8)
    image = torch.from_numpy(noisy).cuda()
    n = B * H * W * 3
    ws = m.workspace(N.BF_MODE_INFERENCE, B, H, W)
    fn = m._lib.bf_forward_u8 if u8 else m._lib.bf_forward_u8_f32
    results = []
    for sentinel in ((255, 0) if u8 else (float("nan"),)):
        buf = torch.full((n + GUARD,), sentinel, dtype=torch.uint8 if u8 else torch.float32, device="cuda")
        N.check(fn(m._h, N.ptr(m.packed()), N.ptr(image), N.ptr(buf), B, H, W, N.ptr(ws), ws.numel(), N.stream_ptr(image)), m._h, "forward")
        torch.cuda.synchronize()
        got, guard = buf[:n].cpu().numpy().reshape(B, H, W, 3), buf[n:].cpu().numpy()
        if u8:
            assert (guard == sentinel).all(), "the head wrote behind its output"
            _check_u8(got, ref)
        else:
            assert np.isnan(guard).all(), "the head wrote behind its output"
            assert not np.isnan(got).any(), "elements were never written"
            _check_f32(got, ref)
        results.append(got)
    if u8:      # an element the head does not write keeps its sentinel: the two fills would differ there
        assert np.array_equal(results[0], results[1])
