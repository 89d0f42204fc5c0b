"""GPU tests of bf_op_vst_forward_u8 and bf_op_vst_inverse (csrc/vst.hip) and their host side, blind_image_denoising_amd.vst.

Yardstick: tests/vst_reference.py, the fp64 NumPy restatement, computed once per case.

Bounds.
  forward        the kernel builds its table in fp64 with the operations of the restatement, none contracted: equality is expected.
                 The bar is bf_op_camera_noise_u8's: no sample off by more than one level, at most 0.1 % off at all.
  inverse        float32 arithmetic on constants rounded from fp64: fewer than 16 float32 roundings of values below 512, 16 x 2^-24
                 x 512 = 4.9e-4; the bar is 1e-3 absolute.  uint8: only a value that close to a half-integer can round the other
                 way: no sample off by more than one level, at most 0.1 % off at all.
  batch          an image alone and inside a batch: the same bits, both kernels.

Shapes.  Both kernels walk an image by its flat element in groups of four aligned to the image's base: one element, 45 elements with
an unaligned second image, 6435 elements unaligned, aligned with two and with four channels across several workgroups; a
workgroup serves a span of 16 384 (forward) or 4 096 (inverse) elements and issues all its loads first when the span holds only whole
groups: 3 x 64 x 257 x 4 and 3 x 64 x 66 x 4 have such spans aligned, the alignment tests (2 x 77 x 143 x 3) at every offset."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import _native as N
from oracle import bfcnn_oracle as O
import noise_level_reference as L
import vst_reference as V
from guarded import dev as _dev, guard_bands

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guard_bands")]

SHAPES = [(1, 1, 1, 1), (2, 3, 5, 3), (1, 33, 65, 3), (2, 9, 130, 2), (3, 64, 257, 4)]
_ids = {"ids": lambda s: "x".join(map(str, s))}
FLOAT_BAR = 1e-3


def _parameters(B: int, C: int, shift: int = 0):
    """(gain [B,C], offset [B,C]): every image and channel its own pair of vst_reference.MAP_PARAMETERS"""
    pick = (np.arange(B * C).reshape(B, C) + shift) % len(V.MAP_PARAMETERS)
    table = np.array(V.MAP_PARAMETERS, np.float64)
    return table[pick, 0], table[pick, 1]


def _assert_levels(got: np.ndarray, ref: np.ndarray, what: str):
    diff = np.abs(got.astype(int) - ref.astype(int))
    print(f"{what}: {int((diff > 0).sum())} of {diff.size} samples differ, by at most {int(diff.max())}")
    assert diff.max() <= 1, what
    assert (diff > 0).sum() <= 1e-3 * diff.size, what


# ---- 1. forward --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_forward_matches_the_reference(shape):
    rng = np.random.default_rng(sum(shape))
    images = rng.integers(0, 256, shape, dtype=np.uint8)
    images.reshape(-1)[0], images.reshape(-1)[-1] = 255, 0
    B, C = shape[0], shape[3]
    for shift in (0, 3):
        gain, offset = _parameters(B, C, shift)
        t = _dev(images)
        got = bf.stabilise_u8(t, (_dev(gain), _dev(offset)))
        assert got.is_cuda and got.dtype == torch.uint8 and got.shape == t.shape and got.data_ptr() != t.data_ptr()
        assert torch.equal(bf.stabilise_u8(t, (gain, offset)), got)                            # two calls (host-given values): the same bits
        _assert_levels(got.cpu().numpy(), V.stabilise_u8(images, gain, offset), f"{shape} shift {shift}")
        # in place, through the entry
        g, o = _dev(gain), _dev(offset)
        N.call("bf_op_vst_forward_u8", N.ptr(t), N.ptr(t), B, shape[1], shape[2], C, N.ptr(g), N.ptr(o), N.stream_ptr(t))
        assert torch.equal(t, got)
    if C == 3:
        assert torch.equal(bf.stabilise_u8(_dev(images), (0.0, [100.0, 0.0, 1.0])), _dev(images))       # gain 0: the identity


def test_forward_serves_every_alignment_of_source_and_destination():
    """images that start 0..3 bytes into a dword, source and destination agreeing (whole groups move as dwords) or not; 33 033
    elements: a first span with a head, an interior span (16 384 elements, all loads in front) and a last one with a tail"""
    rng = np.random.default_rng(5)
    B, H, W, C = 2, 77, 143, 3
    n = B * H * W * C
    images = rng.integers(0, 256, (B, H, W, C), dtype=np.uint8)
    gain, offset = _parameters(B, C)
    g, o = _dev(gain), _dev(offset)
    ref = bf.stabilise_u8(_dev(images), (g, o)).cpu().numpy()                     # the bits do not depend on the alignment
    _assert_levels(ref, V.stabilise_u8(images, gain, offset), "2x77x143x3")
    for head_s in range(4):
        for head_d in range(4):
            src = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
            dst = torch.full((n + 8,), 7, dtype=torch.uint8, device="cuda")
            src[head_s:head_s + n] = _dev(images).reshape(-1)
            rc = N.lib().bf_op_vst_forward_u8(src.data_ptr() + head_s, dst.data_ptr() + head_d, B, H, W, C, N.ptr(g), N.ptr(o),
                                              N.stream_ptr(src))
            assert rc == N.BF_OK
            out = dst.cpu().numpy()
            assert np.array_equal(out[head_d:head_d + n].reshape(ref.shape), ref), (head_s, head_d)
            assert (out[:head_d] == 7).all() and (out[head_d + n:] == 7).all(), (head_s, head_d)      # nothing outside the images


# ---- 2. batch independence ---------------------------------------------------------------------------------------------------

def test_an_image_does_not_depend_on_its_batch():
    for shape in ((3, 37, 53, 3), (3, 64, 66, 4)):                                # unaligned and aligned image strides
        rng = np.random.default_rng(shape[1])
        B, C = shape[0], shape[3]
        images = rng.integers(0, 256, shape, dtype=np.uint8)
        w = rng.uniform(-8.0, 263.0, shape).astype(np.float32)
        gain, offset = _parameters(B, C, 1)
        whole_v = bf.stabilise_u8(_dev(images), (gain, offset)).cpu().numpy()
        whole_x = {(inv, u8): bf.unstabilise(_dev(w), (gain, offset), inv, u8).cpu().numpy()
                   for inv in ("exact", "algebraic") for u8 in (True, False)}
        for n in range(B):
            level = (gain[n:n + 1], offset[n:n + 1])
            assert np.array_equal(bf.stabilise_u8(_dev(images[n:n + 1]), level).cpu().numpy()[0], whole_v[n]), (shape, n)
            for (inv, u8), whole in whole_x.items():
                alone = bf.unstabilise(_dev(w[n:n + 1]), level, inv, u8).cpu().numpy()[0]
                assert np.array_equal(alone.view(np.uint8), whole[n].view(np.uint8)), (shape, n, inv, u8)


# ---- 3. inverse --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_inverse_matches_the_reference(shape):
    rng = np.random.default_rng(sum(shape) + 1)
    w = rng.uniform(-8.0, 263.0, shape).astype(np.float32)
    w.reshape(-1)[0], w.reshape(-1)[-1] = 300.0, -1.0
    B, C = shape[0], shape[3]
    gain, offset = _parameters(B, C, 2)
    t = _dev(w)
    for inverse in ("exact", "algebraic"):
        ref = V.unstabilise(w, gain, offset, exact=inverse == "exact", cast_to_uint8=False)
        got = bf.unstabilise(t, (_dev(gain), _dev(offset)), inverse, cast_to_uint8=False)
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == t.shape
        assert torch.equal(bf.unstabilise(t, (gain, offset), inverse, cast_to_uint8=False), got)
        dev = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
        print(f"{shape} {inverse}: float32 max |deviation| {dev:.3e}")
        assert dev <= FLOAT_BAR
        as_u8 = bf.unstabilise(t, (gain, offset), inverse)
        assert as_u8.dtype == torch.uint8 and as_u8.shape == t.shape
        _assert_levels(as_u8.cpu().numpy(), np.rint(ref).astype(np.uint8), f"{shape} {inverse} uint8")
        assert torch.equal(torch.round(got).to(torch.uint8), as_u8)               # the same value, rounded half to even
    # float32 in place, through the entry
    g, o = _dev(gain), _dev(offset)
    want = bf.unstabilise(t, (g, o), "exact", cast_to_uint8=False)
    N.call("bf_op_vst_inverse", N.ptr(t), N.ptr(t), B, shape[1], shape[2], C, N.ptr(g), N.ptr(o), 1, 0, N.stream_ptr(t))
    assert torch.equal(t, want)


def test_inverse_serves_every_alignment_of_source_and_destination():
    rng = np.random.default_rng(6)
    B, H, W, C = 2, 77, 143, 3                                                     # spans of 4 096 elements: head, interior, tail
    n = B * H * W * C
    w = rng.uniform(-8.0, 263.0, (B, H, W, C)).astype(np.float32)
    gain, offset = _parameters(B, C)
    g, o = _dev(gain), _dev(offset)
    want_f = bf.unstabilise(_dev(w), (g, o), "exact", cast_to_uint8=False).cpu().numpy()
    want_u = bf.unstabilise(_dev(w), (g, o), "exact").cpu().numpy()
    for head_s in range(4):
        src = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
        src[head_s:head_s + n] = _dev(w).reshape(-1)
        for head_d in range(4):
            dst_f = torch.full((n + 8,), 7.0, dtype=torch.float32, device="cuda")
            dst_u = torch.full((n + 8,), 7, dtype=torch.uint8, device="cuda")
            for dst, u8, want, size in ((dst_f, 0, want_f, 4), (dst_u, 1, want_u, 1)):
                rc = N.lib().bf_op_vst_inverse(src.data_ptr() + 4 * head_s, dst.data_ptr() + size * head_d, B, H, W, C, N.ptr(g), N.ptr(o),
                                               1, u8, N.stream_ptr(src))
                assert rc == N.BF_OK
                out = dst.cpu().numpy()
                assert np.array_equal(out[head_d:head_d + n].reshape(want.shape), want), (head_s, head_d, u8)
                assert (out[:head_d] == 7).all() and (out[head_d + n:] == 7).all(), (head_s, head_d, u8)


# ---- 4. sanitising on the device ---------------------------------------------------------------------------------------------

def test_unusable_parameters_are_sanitised_on_the_device():
    gains, offsets = [float("nan"), -1.0, float("inf"), 1e9], [float("nan"), -5.0, 0.0, float("inf")]
    gain = np.repeat(np.array(gains)[:, None], 4, axis=1)                         # image b: gains[b]; channel c: offsets[c]
    offset = np.repeat(np.array(offsets)[None, :], 4, axis=0)
    rng = np.random.default_rng(7)
    images = rng.integers(0, 256, (4, 16, 16, 4), dtype=np.uint8)
    images[:, 0, :, :] = np.arange(16, dtype=np.uint8)[None, :, None] * 17        # 0 .. 255
    w = rng.uniform(-8.0, 263.0, images.shape).astype(np.float32)
    level = (_dev(gain), _dev(offset))                                            # device tensors: not validated on the host
    got = bf.stabilise_u8(_dev(images), level).cpu().numpy()
    _assert_levels(got, V.stabilise_u8(images, gain, offset), "unusable parameters")
    assert np.array_equal(got[:3], images[:3])                                    # NaN, negative, infinite gain: the identity
    assert not np.array_equal(got[3], images[3])                                  # 1e9: capped at 64
    a_eff, o_eff = V.sanitise(gain, offset)
    assert a_eff[:, 0].tolist() == [0.0, 0.0, 0.0, 64.0] and o_eff[0].tolist() == [1 / 12] * 4
    assert np.array_equal(got, bf.stabilise_u8(_dev(images), (a_eff, o_eff)).cpu().numpy())       # ... the sanitised values, given
    for inverse in ("exact", "algebraic"):
        x = bf.unstabilise(_dev(w), level, inverse, cast_to_uint8=False).cpu().numpy().astype(np.float64)
        assert np.isfinite(x).all()
        assert np.abs(x - V.unstabilise(w, gain, offset, inverse == "exact", False)).max() <= FLOAT_BAR
    with pytest.raises(ValueError):                                               # the same values given on the host are refused
        bf.stabilise_u8(_dev(images), (gain, offset))


# ---- 5. bad arguments --------------------------------------------------------------------------------------------------------

def test_entries_refuse_bad_arguments_and_leave_the_destination_untouched():
    lib = N.lib()
    src_u = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    src_f = torch.zeros((1, 8, 8, 3), dtype=torch.float32, device="cuda")
    dst = torch.full((1, 8, 8, 3), 7.0, dtype=torch.float32, device="cuda")      # serves both as float32 and as bytes
    g = torch.full((1, 3), 0.5, dtype=torch.float64, device="cuda")
    o = torch.full((1, 3), 4.0, dtype=torch.float64, device="cuda")
    s = N.stream_ptr(dst)
    fwd = lambda a=N.ptr(src_u), b=N.ptr(dst), B=1, H=8, W=8, C=3, gg=N.ptr(g), oo=N.ptr(o): \
        lib.bf_op_vst_forward_u8(a, b, B, H, W, C, gg, oo, s)
    inv = lambda a=N.ptr(src_f), b=N.ptr(dst), B=1, H=8, W=8, C=3, gg=N.ptr(g), oo=N.ptr(o), exact=1, u8=0: \
        lib.bf_op_vst_inverse(a, b, B, H, W, C, gg, oo, exact, u8, s)
    for call in (fwd, inv):
        for kw in ({"a": None}, {"b": None}, {"gg": None}, {"oo": None}, {"gg": g.data_ptr() + 4}, {"oo": o.data_ptr() + 2}, {"B": 0},
                   {"B": 65536}, {"H": 0}, {"W": -1}, {"C": 0}, {"C": 5}, {"H": 2 ** 16, "W": 2 ** 14}):
            assert call(**kw) == N.BF_EINVAL, kw
    assert inv(a=src_f.data_ptr() + 2) == N.BF_EINVAL and inv(b=dst.data_ptr() + 2) == N.BF_EINVAL
    assert inv(a=N.ptr(dst), u8=1) == N.BF_EINVAL                                 # bytes over their own floats
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all())
    assert fwd(b=N.ptr(src_u)) == N.BF_OK and inv(b=N.ptr(src_f)) == N.BF_OK      # in place is allowed
    assert fwd() == N.BF_OK
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="gain"):
        bf.stabilise_u8(src_u, (-0.5, 1.0))
    with pytest.raises(ValueError, match="offset"):
        bf.unstabilise(src_f, (0.5, [1.0, 2.0]))
    with pytest.raises(ValueError):
        bf.stabilise_u8(src_f, (0.5, 1.0))
    with pytest.raises(ValueError, match="gain"):
        bf.stabilise_u8(src_u, (torch.zeros((2, 3), dtype=torch.float64, device="cuda"), 1.0))       # [B,C] of another batch


# ---- 6. the wrapper ----------------------------------------------------------------------------------------------------------

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


def _numpy_chain(noisy: np.ndarray, gain, offset, exact: bool, cast_to_uint8: bool) -> np.ndarray:
    return V.unstabilise(L.half_field_blur(V.stabilise_u8(noisy, gain, offset)), gain, offset, exact, cast_to_uint8)


def test_wrapper_equals_the_numpy_chain():
    clean = L.two_level_image(64, 96)
    known = (L.SURE_A, L.SURE_OFFSET)
    for seed in (100, 101):
        noisy_d = bf.camera_noise(_dev(clean), L.SURE_A, L.SURE_READ, seed)
        noisy = noisy_d.cpu().numpy()
        fit_gain, fit_offset = L.noise_level_function(noisy)
        for level, (gain, offset), what in ((known, known, "known"), (None, (fit_gain, fit_offset), "fitted")):
            for inverse in ("exact", "algebraic"):
                as_u8 = bf.StabilisedDenoiserModule(_half_field_blur_torch, level, inverse)
                as_f32 = bf.StabilisedDenoiserModule(_half_field_blur_torch, level, inverse, cast_to_uint8=False)
                got_u8, got_f32 = as_u8(noisy_d), as_f32(noisy_d)
                assert got_u8.is_cuda and got_u8.dtype == torch.uint8 and got_u8.shape == noisy_d.shape
                assert got_f32.is_cuda and got_f32.dtype == torch.float32 and got_f32.shape == noisy_d.shape
                if level is None:
                    fit = as_f32.last_noise_level
                    assert isinstance(fit, bf.NoiseLevelFunction) and fit.gain.is_cuda
                    assert np.allclose(fit.gain.cpu().numpy(), fit_gain, rtol=1e-10, atol=0)
                    assert np.allclose(fit.offset.cpu().numpy(), fit_offset, rtol=1e-10, atol=0)
                    # a fit that differs by 1e-10 relative moves s, rc and a by as much: below 1e-7 on values up to 255, unless it
                    # moves an entry of the table across a rounding boundary -- so the tables are compared first
                    assert np.array_equal(bf.stabilise_u8(noisy_d, fit).cpu().numpy(), V.stabilise_u8(noisy, fit_gain, fit_offset))
                ref = _numpy_chain(noisy, gain, offset, inverse == "exact", False)
                dev = float(np.abs(got_f32.cpu().numpy().astype(np.float64) - ref).max())
                print(f"seed {seed} {what} ({float(np.mean(gain)):.4f}, {float(np.mean(offset)):.4f}) {inverse}: float32 max |deviation| {dev:.3e}; "
                      f"MSE noisy {((noisy.astype(float) - clean) ** 2).mean():.2f}, result {((ref - clean) ** 2).mean():.2f}")
                assert dev <= FLOAT_BAR + 1e-6
                _assert_levels(got_u8.cpu().numpy(), np.rint(ref).astype(np.uint8), f"seed {seed} {what} {inverse} uint8")
                host = as_u8(noisy)                                               # NumPy in, NumPy out
                assert isinstance(host, np.ndarray) and np.array_equal(host, got_u8.cpu().numpy())
        nlf = bf.noise_level_function(noisy_d)                                    # a NoiseLevelFunction, device tensors or NumPy
        want = bf.StabilisedDenoiserModule(_half_field_blur_torch, None)(noisy_d)
        assert torch.equal(bf.StabilisedDenoiserModule(_half_field_blur_torch, nlf)(noisy_d), want)
        assert torch.equal(bf.StabilisedDenoiserModule(_half_field_blur_torch, bf.noise_level_function(noisy))(noisy_d), want)
    with pytest.raises(ValueError, match="float32"):
        bf.StabilisedDenoiserModule(lambda u: u, known)(noisy_d)                  # a module that returns uint8


# ---- 7, 8. the real engine ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def resnet():
    cfg = O.canonical_config(no_layers=2)
    spec = O.ResnetSpec.from_config(cfg["model"])
    params, state = O.init_params(spec, seed=42)
    hydra = bf.model_builder(cfg["model"], device="cuda").hydra
    hydra.set_weights(params, state)
    return cfg, hydra


def test_gain_zero_is_the_module_itself(resnet):
    _, hydra = resnet
    clean, _ = O.synthetic_batch(2, 32, 32, seed=11)
    noisy = bf.camera_noise(_dev(clean), 0.0, 10.0, seed=4)
    module = bf.DenoiserModule(hydra)
    stabilised = bf.StabilisedDenoiserModule(module, (0.0, 100.0), cast_to_uint8=False)
    got = stabilised(noisy)
    want = bf.DenoiserModule(hydra, cast_to_uint8=False)(noisy)
    assert got.dtype == torch.float32 and got.shape == want.shape
    dev = float((got.double() - want.double()).abs().max())
    print(f"gain 0: max |stabilised - module| {dev:.3e}; the module's output spans {float(want.min()):.3f} .. {float(want.max()):.3f}")
    assert dev <= FLOAT_BAR
    _assert_levels(bf.StabilisedDenoiserModule(module, (0.0, 100.0))(noisy).cpu().numpy(), module(noisy).cpu().numpy(), "gain 0 uint8")
    assert stabilised.check_status() and module.check_status()
    assert stabilised.last_noise_level is stabilised.noise_level


def test_wrapper_composes_with_the_self_ensemble_the_risk_estimate_and_load_model(resnet, tmp_path):
    cfg, hydra = resnet
    clean, _ = O.synthetic_batch(2, 32, 48, seed=12)
    noisy = bf.camera_noise(_dev(clean), [0.3, 0.5, 0.8], 2.0, seed=5)
    module = bf.DenoiserModule(hydra)
    ens = bf.SelfEnsembleDenoiserModule(module, "flips")
    stabilised = bf.StabilisedDenoiserModule(ens)
    out = stabilised(noisy)
    assert out.is_cuda and out.dtype == torch.uint8 and out.shape == noisy.shape and stabilised.check_status()
    fit = stabilised.last_noise_level
    assert isinstance(fit, bf.NoiseLevelFunction) and tuple(fit.gain.shape) == (2, 3)
    # the same chain by hand
    by_hand = bf.unstabilise(bf.SelfEnsembleDenoiserModule(module, "flips", cast_to_uint8=False)(bf.stabilise_u8(noisy, fit)), fit)
    assert torch.equal(out, by_hand)
    host = stabilised(noisy.cpu().numpy())
    assert isinstance(host, np.ndarray) and np.array_equal(host, out.cpu().numpy())
    est = bf.estimate_risk_affine(stabilised, noisy, probes=2)
    assert [tuple(v.shape) for v in est] == [(2,)] * 2 + [(2, 3)] + [(2,)] * 3 + [(2, 3, 6)]
    assert all(bool(torch.isfinite(v).all()) for v in est) and module.check_status()
    est = bf.estimate_risk_affine(bf.StabilisedDenoiserModule(module, ([0.3, 0.5, 0.8], 4.0 + 1.0 / 12.0)), noisy, probes=2)
    assert all(bool(torch.isfinite(v).all()) for v in est) and module.check_status()
    bf.save_model(hydra, str(tmp_path / "m"))
    loaded = bf.load_model(str(tmp_path / "m"), device="cuda", stabilise=True)
    assert type(loaded) is bf.StabilisedDenoiserModule
    assert torch.equal(loaded(noisy), bf.StabilisedDenoiserModule(module)(noisy)) and loaded.check_status()
    report = bf.evaluate_camera(module, [clean, clean[:1, :24]], 0.5, 2.0, seed=3)
    assert report["images"] == 3 and len(report["batches"]) == 2
    assert all(np.isfinite(v) for v in report["aggregate"].values())
    print(bf.format_camera_report(report))


# ---- 9. the trained network: recorded, not gated beyond shape, finiteness and status -----------------------------------------

def test_trained_network_on_camera_noise_is_recorded():
    """PSNR / MAE against the clean 128 x 128 KITTI crop of the noisy frame, the network applied directly, stabilised with the
    known (gain, read_sigma^2 + 1/12) and stabilised with the frame's own fit.  Measured (DESIGN.md 7.11 has the table)."""
    import unet_v56 as K
    z, _ = K.load()
    clean = np.ascontiguousarray(z["kitti"][:1, :128, :128])
    module = bf.load_denoiser_model("unet_laplacian_v5.6")
    for gain, read in ((0.5, 2.0), (2.0, 2.0), (4.0, 1.0)):
        noisy_d = bf.camera_noise(_dev(clean), gain, read, seed=9)
        fitted = bf.StabilisedDenoiserModule(module)
        results = {"noisy": noisy_d, "direct": module(noisy_d),
                   "stabilised, known": bf.StabilisedDenoiserModule(module, (gain, V.offset_of(read)))(noisy_d),
                   "stabilised, fitted": fitted(noisy_d)}
        assert module.check_status()
        fit = fitted.last_noise_level
        print(f"gain {gain} read {read}: fitted gain {fit.gain.cpu().numpy().round(3).tolist()} offset {fit.offset.cpu().numpy().round(2).tolist()}")
        for what, t in results.items():
            out = t.cpu().numpy()
            assert out.dtype == np.uint8 and out.shape == clean.shape
            print(f"    {what:<20} PSNR {K.psnr(clean, out):6.2f} dB   MAE {K.mae(clean, out):6.3f}")
        assert bool(torch.isfinite(fit.gain).all()) and bool(torch.isfinite(fit.offset).all())


# ---- 10. a stack three deep: the outermost wrapper finds the model's own argument checks ---------------------------------------

def test_a_three_deep_stack_checks_channels_and_empty_batches_as_its_model_does():
    """Every wrapper finds the DenoiserModule at the bottom through the whole chain (DenoiserWrapper._base): a wrong channel count
    is the model's ValueError, raised by the outermost wrapper's input check before anything is uploaded, and an empty batch
    comes back as the model's empty output (its out_channels), not as the input."""
    hydra = bf.model_builder(O.canonical_config(no_layers=6)["model"], device="cuda").hydra
    base = bf.DenoiserModule(hydra)
    stack = bf.StabilisedDenoiserModule(bf.PixelShuffleDenoiserModule(bf.TiledDenoiserModule(base)))
    assert stack._base is base and stack._module._base is base and stack._module._module._base is base
    wrong = np.zeros((1, 16, 16, 4), np.uint8)
    with pytest.raises(ValueError) as of_the_model:
        base(wrong)
    assert "3..3 channels" in str(of_the_model.value)
    for given in (wrong, _dev(wrong), wrong[:0], _dev(wrong[:0])):
        with pytest.raises(ValueError) as e:
            stack(given)
        assert str(e.value).replace("(0, ", "(1, ") == str(of_the_model.value)
    assert stack.last_noise_level is None and stack._module.last_stride is None         # nothing ran
    for given in (np.zeros((0, 16, 16, 3), np.uint8), torch.zeros((0, 16, 16, 3), dtype=torch.uint8)):
        out = stack(given)
        assert type(out) is type(given) and out is not given and "uint8" in str(out.dtype)
        assert tuple(out.shape) == (0, 16, 16, hydra.desc.out_channels)
