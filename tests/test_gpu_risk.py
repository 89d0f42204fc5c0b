"""GPU tests of bf_op_risk_probe_u8 / bf_op_risk_sums (csrc/risk.hip) and blind_image_denoising_amd.risk.

Yardstick: tests/risk_reference.py, the NumPy restatement (probe signs from the oracle's Philox, fp64 sums, the host formula).

Bounds.  The probe stack is integers: EQUAL.  The sums are fewer than 1e5 fp64 terms per image and channel at these shapes, added in
another order than NumPy's: n 2^-53 = 1.1e-11 bounds the relative reordering error of the non-negative terms of R, and of D on the
scale sum |f_p - f_0|; the bar is 1e-10 (as tests/test_gpu_noise_estimate.py).  Known answers (a scaling, the identity) are exact
in fp64 and must be EQUAL.

Both kernels walk an image by its flat element index in groups of four (one Philox call): the probe kernel 1024 elements per
workgroup, the sums kernel 4096 (C = 1, 2, 4) or 6144 (C = 3: units of 12 elements, so that a lane's channels are fixed).  Shapes
whose H W C is a multiple of four take dword / float4 accesses, the others bytes / floats.  The shapes are the smallest that cross
each of these: one element (1x1x1x1), 45 elements (2x3x5x3), unaligned across a tile (1x37x53x3), aligned over 17 tiles with four
channels (3x64x257x4), aligned inside one tile with two channels (2x9x130x2), aligned across a tile with three (2x40x64x3),
exactly one tile (1x32x64x3) -- and the two that straddle a workgroup tile of the sums kernel by one row and one column:
2x65x65x1 (tile = 64 x 64 x 1) and 1x33x65x3 (tile = 32 x 64 x 3)."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import _native as N
from oracle import bfcnn_oracle as O
import risk_reference as R
from test_gpu_inference import _check_f32
from guarded import dev as _dev, guard_bands

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guard_bands")]

SHAPES = [(1, 1, 1, 1), (2, 3, 5, 3), (1, 37, 53, 3), (3, 64, 257, 4), (2, 9, 130, 2), (2, 65, 65, 1), (1, 33, 65, 3), (2, 40, 64, 3),
          (1, 32, 64, 3)]
PROBES = [1, 3, 8]
_ids = {"ids": lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else f"K{s}"}


# ---- 1. the probe stack ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("probes", PROBES, **_ids)
@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_probe_stack_is_bit_equal_to_the_reference(shape, probes):
    rng = np.random.default_rng(sum(shape) + probes)
    y = rng.integers(0, 256, shape, dtype=np.uint8)
    y.reshape(-1)[0], y.reshape(-1)[-1] = 255, 0
    for amplitude, seed in ((1, 0), (5, 2 ** 40 + 12345), (16, 2 ** 64 - 1)):
        got = bf.risk_probe_stack_u8(_dev(y), probes, amplitude, seed)
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == ((1 + probes) * shape[0],) + shape[1:]
        assert np.array_equal(got.cpu().numpy(), R.probe_stack(y, probes, amplitude, seed)), (amplitude, seed)


@pytest.mark.parametrize("amplitude", [1, 16])
def test_probe_of_a_saturated_image_stays_in_range(amplitude):
    y = np.where(np.random.default_rng(4).integers(0, 2, (2, 33, 65, 3)) > 0, 255, 0).astype(np.uint8)
    got = bf.risk_probe_stack_u8(_dev(y), 3, amplitude, 9).cpu().numpy()
    assert np.array_equal(got, R.probe_stack(y, 3, amplitude, 9))
    members = got.reshape((4,) + y.shape).astype(int)
    assert np.array_equal(members[0], y)
    for p in (1, 2, 3):
        assert np.array_equal(members[p], np.where(y == 0, amplitude, 255 - amplitude))      # reflected: exactly a away, inside


# ---- 2. the sums -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("probes", PROBES, **_ids)
@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_sums_match_the_reference(shape, probes):
    rng = np.random.default_rng(10 * sum(shape) + probes)
    y = rng.integers(0, 256, shape, dtype=np.uint8)
    y.reshape(-1)[0] = 255
    f = (rng.uniform(0.0, 255.0, ((1 + probes) * shape[0],) + shape[1:]) + rng.normal(0.0, 10.0, ((1 + probes) * shape[0],) + shape[1:])).astype(np.float32)
    amplitude, seed = 3, 2 ** 41 + 7
    yd, fd = _dev(y), _dev(f)
    got = bf.risk_sums(yd, fd, probes, amplitude, seed)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (shape[0], shape[3], 1 + probes)
    again = bf.risk_sums(yd, fd, probes, amplitude, seed).cpu().numpy()
    got = got.cpu().numpy()
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))                        # two calls: the same bits
    ref, scale = R.risk_sums(y, f, probes, amplitude, seed), R.abs_difference_sums(f, probes)
    dev_r = float((np.abs(got[:, :, 0] - ref[:, :, 0]) / ref[:, :, 0]).max())
    dev_d = float((np.abs(got[:, :, 1:] - ref[:, :, 1:]) / scale).max())
    print(f"{shape} K = {probes}: R relative {dev_r:.3e}, D / sum |f_p - f_0| {dev_d:.3e}")
    assert dev_r <= 1e-10 and dev_d <= 1e-10


def test_sums_of_an_image_do_not_depend_on_its_batch():
    """image n inside a batch = that image evaluated alone, bit for bit (unaligned and aligned shapes, more than one tile)"""
    for shape in ((3, 37, 53, 3), (3, 64, 66, 4)):
        rng = np.random.default_rng(shape[1])
        y = rng.integers(0, 256, shape, dtype=np.uint8)
        f = rng.uniform(0.0, 255.0, (3 * shape[0],) + shape[1:]).astype(np.float32)
        whole = bf.risk_sums(_dev(y), _dev(f), 2, 1, 77).cpu().numpy()
        members = f.reshape((3,) + shape)
        for n in range(shape[0]):
            alone = bf.risk_sums(_dev(y[n:n + 1]), _dev(members[:, n]), 2, 1, 77).cpu().numpy()
            assert np.array_equal(alone[0].view(np.uint64), whole[n].view(np.uint64)), (shape, n)


def test_entry_points_refuse_bad_arguments():
    lib = N.lib()
    y = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    stack = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device="cuda")
    f = torch.ones((2, 8, 8, 3), dtype=torch.float32, device="cuda")
    nbytes = lib.bf_op_risk_sums_scratch_bytes(1, 8, 8, 3, 1)
    assert nbytes > 0 and nbytes % 8 == 0
    scratch = torch.zeros(nbytes // 8 + 1, dtype=torch.float64, device="cuda")
    out = torch.zeros((1, 3, 2), dtype=torch.float64, device="cuda")
    s = N.stream_ptr(y)
    probe = lambda src, dst, B=1, H=8, W=8, C=3, K=1, a=1: lib.bf_op_risk_probe_u8(src, dst, B, H, W, C, K, a, 0, s)
    assert probe(N.ptr(y), N.ptr(stack)) == N.BF_OK
    for kw in ({"K": 0}, {"K": 9}, {"a": 0}, {"a": 17}, {"C": 0}, {"C": 5}, {"B": 0}, {"H": 0}, {"W": -1}, {"H": 2 ** 16, "W": 2 ** 14}):
        assert probe(N.ptr(y), N.ptr(stack), **kw) == N.BF_EINVAL, kw
    assert probe(None, N.ptr(stack)) == N.BF_EINVAL and probe(N.ptr(y), None) == N.BF_EINVAL and probe(N.ptr(y), N.ptr(y)) == N.BF_EINVAL
    sums = lambda yy=N.ptr(y), ff=N.ptr(f), K=1, a=1, sc=N.ptr(scratch), nb=nbytes, o=N.ptr(out), C=3: \
        lib.bf_op_risk_sums(yy, ff, 1, 8, 8, C, K, a, 0, sc, nb, o, s)
    assert sums() == N.BF_OK
    for kw in ({"K": 0}, {"K": 9}, {"a": 0}, {"a": 17}, {"C": 5}, {"yy": None}, {"ff": None}, {"sc": None}, {"o": None}, {"nb": nbytes - 8},
               {"sc": scratch.data_ptr() + 4}, {"o": out.data_ptr() + 4}, {"ff": f.data_ptr() + 2}):
        assert sums(**kw) == N.BF_EINVAL, kw
    for shape in ((0, 8, 8, 3, 1), (1, 8, 8, 5, 1), (1, 8, 8, 3, 9), (1, 8, 0, 3, 1)):
        assert lib.bf_op_risk_sums_scratch_bytes(*shape) == N.BF_EINVAL
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), np.broadcast_to([64.0, 0.0], (1, 3, 2)))         # (1 - 0)^2 per pixel; f_1 = f_0


# ---- 3. known answers end to end ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,probes,amplitude", [((2, 37, 53, 3), 1, 1), ((1, 64, 66, 4), 3, 4), ((2, 9, 130, 1), 8, 16)])
def test_known_answers_with_torch_callables(shape, probes, amplitude):
    y = np.random.default_rng(3).integers(0, 256, shape, dtype=np.uint8)
    sigma = 12.5
    est = bf.estimate_risk(lambda u: 0.25 * u.float(), _dev(y), sigma=sigma, probes=probes, amplitude=amplitude, seed=5)
    assert all(v.is_cuda and v.dtype == torch.float64 for v in est)
    assert [tuple(v.shape) for v in est] == [(shape[0],)] * 2 + [(shape[0], shape[3])] + [(shape[0],)] * 3 + [(shape[0], shape[3], 1 + probes)]
    est = bf.RiskEstimate(*(v.cpu().numpy() for v in est))
    assert (est.divergence == 0.25).all() and (est.sigma == sigma).all()
    y64 = y.astype(np.float64)
    closed = (0.75 ** 2 * (y64 * y64).sum(axis=(1, 2)) / (shape[1] * shape[2]) - sigma ** 2 + 2.0 * sigma ** 2 * 0.25).mean(axis=1)
    assert np.allclose(est.mse, closed, rtol=1e-12, atol=0)
    assert np.allclose(est.psnr, 10.0 * np.log10(255.0 ** 2 / closed), rtol=1e-12, atol=0)
    assert np.allclose(est.residual_rms, 0.75 * np.sqrt((y64 * y64).mean(axis=(1, 2, 3))), rtol=1e-12, atol=0)
    assert np.isnan(est.probe_spread).all() if probes == 1 else (est.probe_spread == 0).all()
    ident = bf.estimate_risk(lambda u: u.float(), _dev(y), sigma=sigma, probes=probes, amplitude=amplitude, seed=5)
    assert (ident.mse.cpu().numpy() == sigma ** 2).all() and (ident.divergence.cpu().numpy() == 1.0).all()
    assert (ident.residual_rms.cpu().numpy() == 0.0).all()
    per_channel = np.arange(1.0, 1.0 + shape[3])
    ident = bf.estimate_risk(lambda u: u.float(), _dev(y), sigma=per_channel, probes=probes, amplitude=amplitude)
    assert np.allclose(ident.mse.cpu().numpy(), (per_channel ** 2).mean(), rtol=1e-15, atol=0)
    assert np.array_equal(ident.sigma.cpu().numpy(), np.broadcast_to(per_channel, (shape[0], shape[3])))


def test_results_that_cannot_carry_the_probe_are_refused():
    y = _dev(np.zeros((1, 8, 8, 3), np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        bf.estimate_risk(lambda u: u, y, sigma=1.0)
    with pytest.raises(ValueError):
        bf.estimate_risk(lambda u: u.double(), y, sigma=1.0)
    with pytest.raises(ValueError):
        bf.estimate_risk(lambda u: u.float()[:1], y, sigma=1.0)
    with pytest.raises(ValueError):
        bf.estimate_risk(lambda u: u.float().cpu().numpy(), y, sigma=1.0)


# ---- 4. the blur case of the CPU test ----------------------------------------------------------------------------------------

def _half_blur_torch(u):
    """risk_reference.half_blur on the device: the numerator is an integer up to 4590, exact in float32 in any order; divided in
    float64 and rounded to float32 it has the reference's bits (see there)"""
    x = u.permute(0, 3, 1, 2).float()
    box = F.avg_pool2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), 3, stride=1, divisor_override=1)
    return ((9.0 * x + box).double() / 18.0).float().permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("amplitude,seed", [(1, 0), (4, 1)])
def test_blur_case_equals_the_reference_and_tracks_the_truth(amplitude, seed):
    for sigma, clean, noisy in R.noisy_cases():
        est = bf.estimate_risk(_half_blur_torch, _dev(noisy), sigma=sigma, probes=1, amplitude=amplitude, seed=seed)
        ref = R.estimate_risk(R.half_blur, noisy, sigma, 1, amplitude, seed)
        for k in ("mse", "psnr", "residual_rms", "divergence"):
            got = getattr(est, k).cpu().numpy()
            assert np.allclose(got, ref[k], rtol=1e-9, atol=0), (sigma, k, got, ref[k])
        assert np.allclose(est.sums.cpu().numpy(), ref["sums"], rtol=1e-9, atol=0)
        true = ((R.half_blur(noisy).astype(np.float64) - clean) ** 2).mean(axis=(1, 2, 3))
        rel = np.abs(est.mse.cpu().numpy() - true) / true
        print(f"sigma {sigma} amplitude {amplitude} seed {seed}: relative error of the estimate {np.round(rel, 4)}")
        assert (rel <= 0.10).all()


# ---- 5. the real engine ------------------------------------------------------------------------------------------------------

_ENGINE = {}
D_BAR = 4 * 1.736e-6      # 4 x the larger measurement in the docstring of test_real_engine_sums_match_the_oracle


def _engine():
    if not _ENGINE:
        cfg = O.canonical_config(no_layers=2)
        spec = O.ResnetSpec.from_config(cfg["model"])
        params, state = O.init_params(spec, seed=42)
        m = bf.model_builder(cfg["model"], device="cuda").hydra
        m.set_weights(params, state)
        _, noisy = O.synthetic_batch(2, 32, 32, seed=11)
        probes, amplitude, seed = 2, 1, 3
        stack = R.probe_stack(noisy, probes, amplitude, seed)
        ref_f = O.hydra_forward(spec, params, state, stack.astype(np.float64))               # 32 x 32: no padding
        _ENGINE.update(hydra=m, noisy=noisy, stack=stack, ref_f=ref_f, probes=probes, amplitude=amplitude, seed=seed,
                       ref_sums=R.risk_sums(noisy, ref_f, probes, amplitude, seed), scale=R.abs_difference_sums(ref_f, probes))
    return _ENGINE


@pytest.mark.parametrize("arith", [1, 0], ids=["f16x3", "f32"])
def test_real_engine_sums_match_the_oracle(arith):
    """canonical resnet, 2 layers, oracle.init_params(seed=42), batch 2 of 32 x 32 x 3, K = 2, amplitude 1: `sums` of estimate_risk
    against sums formed in fp64 from oracle.hydra_forward on the reference's probe stack.

    R: every float output is within 0.05 of the oracle (the limit of _check_f32, checked here on the same stack), so
    |R - R_ref| = |sum (f - r)(f + r - 2 y)| <= 0.05 (2 sum |r - y| + 0.05 HW) per image and channel.

    D: |D - D_ref| / sum |r_p - r_0|, the largest over images, channels and probes, is a measured number, taken once on an MI355X
    against the fp64 oracle: 1.736e-6 with the default split-f16 blocks, 1.501e-6 with set_option("arith", 0) (exact fp32).  The bar
    is 4 x the larger, 6.944e-6: seeds and weights move it.  On the same run |R - R_ref| reached 1.0e-4 (split-f16)
    and 7.6e-5 (exact) of its bound, and the estimated mse of the two paths differed by 3e-8 relative."""
    e = _engine()
    m, noisy = e["hydra"], e["noisy"]
    m.set_option("arith", arith)
    try:
        module = bf.DenoiserModule(m)
        f = bf.DenoiserModule(m, cast_to_uint8=False)(_dev(e["stack"])).cpu().numpy()
        _check_f32(f, e["ref_f"])
        est = bf.estimate_risk(module, _dev(noisy), sigma=20.0, probes=e["probes"], amplitude=e["amplitude"], seed=e["seed"])
        assert module.check_status()
    finally:
        m.set_option("arith", 1)
    got, ref = est.sums.cpu().numpy(), e["ref_sums"]
    own = R.risk_sums(noisy, f, e["probes"], e["amplitude"], e["seed"])                      # the module's own float output, in fp64
    assert np.allclose(got[:, :, 0], own[:, :, 0], rtol=1e-10, atol=0)
    assert (np.abs(got[:, :, 1:] - own[:, :, 1:]) <= 1e-10 * R.abs_difference_sums(f, e["probes"])).all()
    r0 = e["ref_f"][:2]
    bound = 0.05 * (2.0 * np.abs(r0 - noisy.astype(np.float64)).sum(axis=(1, 2)) + 0.05 * 32 * 32)
    dev_r = np.abs(got[:, :, 0] - ref[:, :, 0])
    dev_d = float((np.abs(got[:, :, 1:] - ref[:, :, 1:]) / e["scale"]).max())
    ref_mse = R.risk_from_sums(ref, np.full((2, 3), 20.0), 32, 32, e["amplitude"])["mse"]
    print(f"arith {arith}: |R - R_ref| / bound {float((dev_r / bound).max()):.3e}, |D - D_ref| / sum |r_p - r_0| {dev_d:.3e}, "
          f"estimated mse {est.mse.cpu().numpy()} (oracle sums: {ref_mse})")
    assert (dev_r <= bound).all()
    assert dev_d <= D_BAR


# ---- 6. wiring ---------------------------------------------------------------------------------------------------------------

def test_every_module_form_runs():
    e = _engine()
    m = e["hydra"]
    _, noisy = O.synthetic_batch(2, 32, 48, seed=5)
    plain = bf.DenoiserModule(m)
    base = bf.estimate_risk(plain, _dev(noisy), probes=2)
    assert all(bool(torch.isfinite(v).all()) for v in base) and plain.check_status()
    sigma_mad = bf.noise_statistics(_dev(noisy))[:, :, 2]
    assert torch.equal(base.sigma, sigma_mad)                                                # sigma=None: the MAD column
    assert torch.equal(bf.estimate_risk(plain, _dev(noisy), probes=2, method="immerkaer").sigma, bf.noise_statistics(_dev(noisy))[:, :, 1])
    for module in (bf.SelfEnsembleDenoiserModule(plain, "flips"), bf.GraphedDenoiserModule(plain),
                   bf.SelfEnsembleDenoiserModule(plain, "d4", cast_to_uint8=False)):
        est = bf.estimate_risk(module, _dev(noisy), probes=2)
        assert all(bool(torch.isfinite(v).all()) for v in est) and module.check_status()
        assert torch.equal(est.sigma, base.sigma)
    one = bf.estimate_risk(bf.SelfEnsembleDenoiserModule(plain, transforms=[0]), _dev(noisy), probes=2)
    assert torch.equal(one.sums, base.sums)                                                  # the mean over one member is that member
    assert torch.equal(bf.estimate_risk(bf.GraphedDenoiserModule(plain), _dev(noisy), probes=2).sums, base.sums)
    host = bf.estimate_risk(plain, noisy, probes=2)                                          # NumPy in, NumPy out
    assert all(isinstance(v, np.ndarray) and v.dtype == np.float64 for v in host)
    assert all(np.array_equal(h, d.cpu().numpy(), equal_nan=True) for h, d in zip(host, base))
    empty = bf.estimate_risk(plain, torch.zeros((0, 32, 48, 3), dtype=torch.uint8, device="cuda"), probes=2)
    assert all(v.is_cuda for v in empty) and [tuple(v.shape) for v in empty] == [(0,), (0,), (0, 3), (0,), (0,), (0,), (0, 3, 3)]


def test_evaluate_blind_risk_aggregates_batches_of_different_shapes():
    m = _engine()["hydra"]
    module = bf.DenoiserModule(m)
    _, n0 = O.synthetic_batch(2, 64, 64, seed=1)
    _, n1 = O.synthetic_batch(1, 40, 72, sigma=40.0, seed=2)
    n1[0, :8, :8] = 255
    report = bf.evaluate_blind_risk(module, [n0, _dev(n1)], probes=2, amplitude=2, seed=2 ** 64 - 1)
    assert set(report) == {"method", "probes", "amplitude", "images", "batches", "aggregate"}
    assert (report["method"], report["probes"], report["amplitude"], report["images"]) == ("mad", 2, 2, 3)
    keys = {"mse", "psnr", "sigma_in", "divergence", "clipped_fraction"}
    per_image = {k: [] for k in keys}
    for k, (row, noisy) in enumerate(zip(report["batches"], (n0, n1))):
        assert set(row) == keys | {"shape", "images"} and row["shape"] == list(noisy.shape) and row["images"] == noisy.shape[0]
        est = bf.estimate_risk(module, noisy, probes=2, amplitude=2, seed=(2 ** 64 - 1 + k) % 2 ** 64)      # batch k: seed + k
        want = {"mse": est.mse, "psnr": est.psnr, "sigma_in": np.sqrt((est.sigma ** 2).mean(axis=1)), "divergence": est.divergence,
                "clipped_fraction": bf.noise_summary(noisy).clipped_fraction.mean(axis=1)}
        for key in keys:
            assert abs(row[key] - want[key].mean()) <= 1e-12 * max(1.0, abs(want[key].mean())), (k, key)
            per_image[key] += list(want[key])
    assert report["batches"][1]["clipped_fraction"] >= 64.0 / (40 * 72)
    for key in keys:
        assert abs(report["aggregate"][key] - np.mean(per_image[key])) <= 1e-12 * max(1.0, abs(np.mean(per_image[key]))), key
    given = bf.evaluate_blind_risk(module, [n0], sigma=20.0)
    assert given["method"] == "given" and given["aggregate"]["sigma_in"] == 20.0
    text = bf.format_risk_report(report)
    assert len(text.splitlines()) == 5
    assert json.loads(json.dumps(bf.metrics.json_safe(report), allow_nan=False))["images"] == 3
    # a report with an infinite PSNR (the identity at sigma = 0 estimates mse = 0) still serialises
    zero = bf.evaluate_blind_risk(lambda u: u.float(), [n0], sigma=0.0)
    assert zero["aggregate"]["mse"] == 0.0 and zero["aggregate"]["psnr"] == float("inf")
    assert json.loads(json.dumps(bf.metrics.json_safe(zero), allow_nan=False))["aggregate"]["psnr"] is None
