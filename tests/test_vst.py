"""CPU tests of the variance-stabilising chain: the properties of the NumPy restatement in tests/vst_reference.py, which is what
the GPU tests compare the kernels of csrc/vst.hip against, and the argument checks of blind_image_denoising_amd.vst (raised before a
device is touched).

Measured on the reference (fixed seeds; DESIGN.md 7.11 lists them):
  stabilisation   std(v) / s on flat patches of 2^17 Poisson-Gaussian samples over the 18 cases: the worst deviation from 1 is
                  0.0151 (gain 1, read sigma 3, x = 100); the bar is 1.5 x that, 0.0226.  At most 1.31 % of the samples of a case
                  touch 0 or 255 (condition: 2 %).
  the inverse     a patch replaced by its mean in the stabilised domain, 36 cases: |exact - x| is at most 0.1636 grey levels (gain
                  4, x = 100, where the standard error of the mean alone is 0.055); the bar is 1.5 x that, 0.2454.  The algebraic
                  inverse is low by 0.1987 .. 0.3801 gain; the bar is 0.75 x the smallest, 0.1490 gain.
  the Lee filter  stabilised MSE / direct MSE over the nine cases: 0.827 .. 0.842 at (0.5, 2), 0.700 .. 0.716 at (2, 2), 0.679 ..
                  0.688 at (4, 1); the bar is < 1."""
import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import _native as N
from blind_image_denoising_amd import vst as VS
from oracle import bfcnn_oracle as O
import vst_reference as V

STD_MEASURED, STD_BAR = 0.0151, 1.5 * 0.0151
EXACT_MEASURED, EXACT_BAR = 0.1636, 1.5 * 0.1636
DEFICIT_MEASURED, DEFICIT_BAR = 0.1987, 0.75 * 0.1987                   # in units of gain
SATURATED_SHARE = 0.02


# ---- 1. the shape of the map -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gain,offset", V.MAP_PARAMETERS)
def test_reference_map_is_monotone_keeps_the_ends_and_inverts_to_half_a_step(gain, offset):
    table = V.forward_map(gain, offset).astype(np.int64)
    assert table.shape == (256,) and (np.diff(table) >= 0).all()
    assert table[0] == 0 and table[255] == 255
    if gain == 0:
        assert np.array_equal(table, np.arange(256))
    # v is within 1/2 of f(y) = s u(y), and the algebraic inverse g = f^-1 has the increasing slope g'(w) = (rc + a w / (2 s)) / s:
    # |g(v) - y| <= 1/2 g'(f(y) + 1/2), half a step of the map's local spacing of y (1e-9: fp64 rounding of g(f(y)) = y)
    a, _, rc, s = V.constants(gain, offset)
    y = np.arange(256.0)
    f = V.forward_float(y, gain, offset)
    assert (np.abs(table - f) <= 0.5).all()
    back = V.inverse(table.astype(np.float64), gain, offset, exact=False)
    spacing = (rc + a * (f + 0.5) / s / 2.0) / s
    print(f"gain {gain} offset {offset:.3f}: s {float(s):.4f}, max |algebraic(v) - y| {np.abs(back - y).max():.4f}, "
          f"in steps {(np.abs(back - y) / spacing).max():.4f}")
    assert (np.abs(back - y) <= 0.5 * spacing + 1e-9).all()
    # sanitising: what is not usable reads as (0, 1/12)
    assert V.sanitise(np.array([np.nan, -1.0, np.inf, 1e9, 0.5]), np.array([np.nan, -5.0, 0.0, np.inf, 7e4]))[0].tolist() == [0, 0, 0, 64, 0.5]
    assert V.sanitise(np.array([np.nan, -1.0, np.inf, 1e9, 0.5]), np.array([np.nan, -5.0, 0.0, np.inf, 7e4]))[1].tolist() == \
        [1 / 12, 1 / 12, 1 / 12, 1 / 12, 65025.0]


def test_reference_exact_inverse_is_the_closed_form_of_makitalo_and_foi():
    """the cancelled form against the uncancelled a (D^2/4 + K1/D - K2/D^2 + K3/D^3 - 1/8 - o/a^2), D = (2/a) sqrt(a y + 3/8 a^2 + o),
    where that one is well conditioned (a = 1 .. 4): the same to 1e-9"""
    for gain, offset in ((1.0, 9.08), (4.0, 1.08), (2.0, 4.08)):
        a, c, rc, s = V.constants(gain, offset)
        w = np.linspace(0.0, 255.0, 1001)
        D = w / s + 2.0 * rc / a                                                  # u + the value at 0
        plain = a * (D * D / 4.0 + V.K1 / D - V.K2 / (D * D) + V.K3 / D ** 3 - 0.125 - offset / (a * a))
        assert np.allclose(V.inverse(w, gain, offset, exact=True), np.clip(plain, 0.0, 255.0), rtol=0, atol=1e-9)


# ---- 2. stabilisation --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gain,read_sigma", V.STABILISATION_PARAMETERS)
def test_reference_transform_stabilises_the_variance(gain, read_sigma):
    """measured worst |std(v) / s - 1| over the 18 cases: 0.0151; bar 1.5 x = 0.0226"""
    offset = V.offset_of(read_sigma)
    s = float(V.constants(gain, offset)[3])
    for i, x in enumerate(V.flat_levels(gain)):
        y = V.poisson_gaussian(np.full(V.FLAT_SAMPLES, x), gain, read_sigma, seed=1000 + i)
        share = float(((y == 0) | (y == 255)).mean())
        v = V.forward_map(gain, offset)[y].astype(np.float64)
        print(f"gain {gain} read {read_sigma} x {x:.0f}: saturated {share:.4f}, std(y) {y.std():.3f}, std(v) / s - 1 = {v.std() / s - 1.0:+.4f}")
        assert share <= SATURATED_SHARE
        assert abs(v.std() / s - 1.0) <= STD_BAR


# ---- 3. the inverse ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("gain,read_sigma", [(1.0, 3.0), (2.0, 2.0), (4.0, 1.0)])
def test_reference_exact_inverse_is_unbiased_where_the_algebraic_one_is_low(gain, read_sigma, seed):
    """the "denoiser" replaces a flat patch by its mean in the stabilised domain.  Measured over the 36 cases: |exact - x| <= 0.1636
    (bar 1.5 x = 0.2454); x - algebraic = 0.1987 .. 0.3801 gain (bar: at least 0.75 x 0.1987 gain)"""
    offset = V.offset_of(read_sigma)
    for x in (16.0, 40.0, 100.0):
        y = V.poisson_gaussian(np.full(V.FLAT_SAMPLES, x), gain, read_sigma, seed=2000 + seed)
        w = V.forward_map(gain, offset)[y].astype(np.float64).mean()
        exact, algebraic = float(V.inverse(w, gain, offset, True)), float(V.inverse(w, gain, offset, False))
        print(f"gain {gain} read {read_sigma} x {x:.0f} seed {seed}: exact - x {exact - x:+.4f}, algebraic - x {algebraic - x:+.4f} "
              f"= {(algebraic - x) / gain:+.4f} gain")
        assert abs(exact - x) < abs(algebraic - x)
        assert abs(exact - x) <= EXACT_BAR
        assert algebraic - x <= -DEFICIT_BAR * gain


# ---- 4. what stabilisation is worth ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("gain,read_sigma", [(0.5, 2.0), (2.0, 2.0), (4.0, 1.0)])
def test_reference_stabilisation_pays_for_a_filter_tuned_to_one_sigma(gain, read_sigma, seed):
    """a 5 x 5 Lee filter given the noise variance: the frame average directly, s^2 between the transform and its exact inverse.
    Measured ratios of the MSEs: 0.827 .. 0.842, 0.700 .. 0.716, 0.679 .. 0.688"""
    clean = V.ramp_with_bars()
    assert clean.shape == (128, 128) and clean.min() >= 4.0 and clean.max() <= 228.0
    offset = V.offset_of(read_sigma)
    y = V.poisson_gaussian(clean, gain, read_sigma, seed)
    direct = float(((V.lee_direct(y, gain, offset) - clean) ** 2).mean())
    stabilised = float(((V.lee_stabilised(y, gain, offset) - clean) ** 2).mean())
    print(f"gain {gain} read {read_sigma} seed {seed}: direct MSE {direct:.3f}, stabilised {stabilised:.3f}, ratio {stabilised / direct:.4f}")
    assert stabilised < direct


# ---- 5. host argument checks -------------------------------------------------------------------------------------------------

BAD_VALUES = ((-0.1, 1.0), (0.1, -1.0), (64.5, 1.0), (0.1, 65026.0), (float("nan"), 1.0), (0.1, float("inf")), (0.1,), (0.1, 1.0, 2.0),
              0.1, "ab", (None, 1.0), ("a", 1.0), (np.zeros((1, 1, 3)), 1.0), ([0.1, -0.2, 0.3], 1.0))
BAD_LEVELS = BAD_VALUES + (None, ([0.1, 0.2], 1.0), (0.1, np.zeros((2, 3))))      # ... and what does not fit a [1,8,8,3] batch


def test_bad_arguments_of_the_two_directions_are_refused_without_a_device():
    u8, f32 = torch.zeros((1, 8, 8, 3), dtype=torch.uint8), torch.zeros((1, 8, 8, 3))
    for level in BAD_LEVELS:
        with pytest.raises(ValueError):
            bf.stabilise_u8(u8, level)
        with pytest.raises(ValueError):
            bf.unstabilise(f32, level)
    for bad in (f32, u8[0], u8.numpy(), torch.zeros((1, 8, 8, 5), dtype=torch.uint8), torch.zeros((0, 8, 8, 3), dtype=torch.uint8), "x"):
        with pytest.raises(ValueError):
            bf.stabilise_u8(bad, (0.5, 4.0))
    for bad in (u8, f32[0], f32.numpy(), f32.double(), torch.zeros((1, 8, 8, 5)), torch.zeros((0, 8, 8, 3))):
        with pytest.raises(ValueError):
            bf.unstabilise(bad, (0.5, 4.0))
    for inverse in ("", "Exact", None, 1):
        with pytest.raises(ValueError, match="inverse"):
            bf.unstabilise(f32, (0.5, 4.0), inverse=inverse)
    nlf = bf.NoiseLevelFunction(np.full((1, 3), 0.5), np.full((1, 3), 4.0), None, None, None, None)
    for level in ((0.5, 4.0), (0.0, 0.0), (64.0, 65025.0), ([0.1, 0.2, 0.3], 4.0), (np.full((1, 3), 0.5), torch.full((3,), 4.0)), nlf):
        with pytest.raises(RuntimeError, match="no CPU execution path"):          # well-formed, but on the host
            bf.stabilise_u8(u8, level)
        with pytest.raises(RuntimeError, match="no CPU execution path"):
            bf.unstabilise(f32, level, inverse="algebraic", cast_to_uint8=False)
    wrong_batch = bf.NoiseLevelFunction(np.full((2, 3), 0.5), np.full((2, 3), 4.0), None, None, None, None)
    with pytest.raises(ValueError, match="gain"):
        bf.stabilise_u8(u8, wrong_batch)


def _cpu_module():
    return bf.DenoiserModule(bf.model_builder(O.canonical_config(no_layers=1)["model"], device="cpu").hydra)


def test_module_delegates_and_checks_like_the_wrapped_module():
    module = _cpu_module()
    for inner in (module, bf.SelfEnsembleDenoiserModule(module, "flips")):
        st = bf.StabilisedDenoiserModule(inner)
        assert st.model_hydra is module.model_hydra and st.name == module.name and st.check_status() is True
        assert st.noise_level is None and st.inverse == "exact" and st.min_cells == 64 and st.last_noise_level is None
        for bad in (np.zeros((1, 8, 8, 3), np.float32), np.zeros((8, 8, 3), np.uint8), np.zeros((1, 8, 8, 1), np.uint8), "image"):
            with pytest.raises(ValueError):
                st(bad)
        empty = st(np.zeros((0, 8, 8, 3), np.uint8))
        assert isinstance(empty, np.ndarray) and empty.shape == (0, 8, 8, 3) and empty.dtype == np.uint8
        with pytest.raises(RuntimeError, match="no CPU execution path"):
            st(np.zeros((1, 8, 8, 3), np.uint8))
    for level in BAD_VALUES:
        with pytest.raises(ValueError):
            bf.StabilisedDenoiserModule(module, level)
    for kw in ({"inverse": "x"}, {"min_cells": 0}, {"min_cells": 1.5}, {"min_cells": True}):
        with pytest.raises(ValueError):
            bf.StabilisedDenoiserModule(module, **kw)
    for not_a_module in (None, 3, bf.StabilisedDenoiserModule(module)):
        with pytest.raises(ValueError):
            bf.StabilisedDenoiserModule(not_a_module)
    with pytest.raises(ValueError):                                               # GraphedDenoiserModule around the wrapper is out of scope
        bf.GraphedDenoiserModule(bf.StabilisedDenoiserModule(module))
    # a fixed [B,C] level must match the batch
    fixed = bf.StabilisedDenoiserModule(module, (np.full((2, 3), 0.5), 4.0), inverse="algebraic", cast_to_uint8=False)
    assert fixed.inverse == "algebraic"
    with pytest.raises(ValueError, match="gain"):
        fixed(np.zeros((1, 8, 8, 3), np.uint8))
    with pytest.raises(ValueError, match="offset"):
        bf.StabilisedDenoiserModule(module, (0.5, [1.0, 2.0]))(np.zeros((1, 8, 8, 3), np.uint8))
    # any callable uint8 -> float32: tensors must be on the device, arrays need one
    plain = bf.StabilisedDenoiserModule(lambda u: u.float(), (0.5, 4.0))
    assert plain.model_hydra is None and plain.check_status() is True
    with pytest.raises(RuntimeError, match="no CPU execution path"):
        plain(torch.zeros((1, 8, 8, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU execution path"):
        bf.StabilisedDenoiserModule(lambda u: u.float())(torch.zeros((1, 8, 8, 3), dtype=torch.uint8))
    with pytest.raises(ValueError):
        plain(torch.zeros((1, 8, 8, 5), dtype=torch.uint8))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU execution path"):
            plain(np.zeros((1, 8, 8, 3), np.uint8))


def test_the_float_form_of_the_wrapper_keeps_its_settings():
    module = _cpu_module()
    ens = bf.SelfEnsembleDenoiserModule(module, "flips")
    st = bf.StabilisedDenoiserModule(ens, ([0.1, 0.2, 0.3], 4.0), inverse="algebraic", min_cells=32)
    fn = bf.module_denoiser.float_form(st)
    assert type(fn) is bf.StabilisedDenoiserModule and fn is not st
    assert fn._cast_to_uint8 is False and fn.inverse == "algebraic" and fn.min_cells == 32 and fn.model_hydra is module.model_hydra
    assert fn.noise_level[0].tolist() == [0.1, 0.2, 0.3] and float(fn.noise_level[1]) == 4.0
    assert type(fn._float) is bf.SelfEnsembleDenoiserModule and fn._float.transforms == (0, 2, 4, 6)
    assert bf.module_denoiser.float_form(bf.StabilisedDenoiserModule(module)).noise_level is None
    with pytest.raises(RuntimeError, match="GPU"):
        bf.estimate_risk_affine(st, torch.zeros((1, 8, 8, 3), dtype=torch.uint8), (0.1, 1.0))


def test_load_model_stabilise_keyword(tmp_path):
    cfg = O.canonical_config(no_layers=1)
    bf.save_model(bf.model_builder(cfg["model"], device="cpu", seed=3).hydra, str(tmp_path / "m"))
    path = str(tmp_path / "m")
    st = bf.load_model(path, device="cpu", stabilise=True)
    assert type(st) is bf.StabilisedDenoiserModule and st.noise_level is None and type(st._module) is bf.DenoiserModule
    with pytest.raises(RuntimeError, match="no CPU execution path"):
        st(np.zeros((1, 16, 16, 3), np.uint8))
    fixed = bf.load_model(path, device="cpu", self_ensemble="flips", stabilise=(0.5, 4.0))
    assert type(fixed) is bf.StabilisedDenoiserModule and type(fixed._module) is bf.SelfEnsembleDenoiserModule      # wrapped last
    assert float(fixed.noise_level[0]) == 0.5 and float(fixed.noise_level[1]) == 4.0
    assert type(bf.load_model(path, device="cpu")) is bf.DenoiserModule
    assert type(bf.load_model(path, device="cpu", stabilise=None)) is bf.DenoiserModule
    assert type(bf.load_model(path, device="cpu", stabilise=False)) is bf.DenoiserModule
    for bad in ("x", 1.5, (0.5,), (-0.5, 4.0), (0.5, float("nan"))):
        with pytest.raises(ValueError):
            bf.load_model(path, device="cpu", stabilise=bad)


def test_evaluate_camera_checks_its_arguments():
    module = _cpu_module()
    batch = np.zeros((1, 16, 16, 3), np.uint8)
    for gain, read in ((-1.0, 1.0), (1.0, -1.0), (float("nan"), 1.0), ("a", 1.0), (True, 1.0), (65.0, 1.0)):
        with pytest.raises(ValueError):
            bf.evaluate_camera(module, [batch], gain, read)
    with pytest.raises(ValueError):
        bf.evaluate_camera(module, [], 0.5, 2.0)
    with pytest.raises(ValueError):
        bf.evaluate_camera(module, [batch.astype(np.float32)], 0.5, 2.0)
    with pytest.raises(ValueError):
        bf.evaluate_camera(None, [batch], 0.5, 2.0)


def test_native_entries_refuse_bad_arguments_before_launching():
    lib = N.lib()
    for name in ("bf_op_vst_forward_u8", "bf_op_vst_inverse"):
        assert name in N.SIGNATURES and hasattr(lib, name)
    a, b, g, o = 4096, 8192, 12288, 16384                                         # never dereferenced: every call below is refused
    fwd = lambda s=a, d=b, B=1, H=4, W=4, C=3, gg=g, oo=o: lib.bf_op_vst_forward_u8(s, d, B, H, W, C, gg, oo, None)
    inv = lambda s=a, d=b, B=1, H=4, W=4, C=3, gg=g, oo=o, u8=0: lib.bf_op_vst_inverse(s, d, B, H, W, C, gg, oo, 1, u8, None)
    for call in (fwd, inv):
        for kw in ({"s": None}, {"d": None}, {"gg": None}, {"oo": None}, {"gg": g + 4}, {"oo": o + 2}, {"B": 0}, {"H": 0}, {"W": -1},
                   {"C": 0}, {"C": 5}, {"B": 65536}, {"H": 2 ** 16, "W": 2 ** 14}):
            assert call(**kw) == N.BF_EINVAL, kw
    assert inv(s=a + 2) == N.BF_EINVAL and inv(d=b + 2) == N.BF_EINVAL            # float32 images: 4 bytes
    assert inv(d=a, u8=1) == N.BF_EINVAL                                          # bytes over their own floats


def test_names_are_exported():
    assert all(callable(getattr(bf, n)) for n in ("stabilise_u8", "unstabilise", "StabilisedDenoiserModule", "evaluate_camera",
                                                  "format_camera_report"))
    assert bf.vst is VS and VS.INVERSES == ("exact", "algebraic")
