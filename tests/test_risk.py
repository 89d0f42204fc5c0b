"""CPU tests of the risk estimation (blind_image_denoising_amd/risk.py): the argument checks, raised before a device is touched; the
host formula on hand-made sums; and the NumPy restatement in tests/risk_reference.py -- the yardstick of the GPU tests -- against
the truth it estimates.

The estimator must track the true mean squared error: clean images are at hand here, so |estimate - true| / true can be formed.
The bar of 10 % per image is the issue's, a cap and not a measurement; observed here over the 48 (sigma, amplitude, seed, image)
cases: at most 0.059 (DESIGN.md 7.8 lists all of them)."""
import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import risk as K
import risk_reference as R

_U8 = np.zeros((1, 8, 8, 3), np.uint8)
_float = lambda u: u.float()


# ---- argument checks ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [{"probes": 0}, {"probes": 9}, {"amplitude": 0}, {"amplitude": 17}, {"probes": 1.5}, {"amplitude": True},
                                {"seed": -1}, {"seed": 2 ** 64}, {"method": "median"}, {"sigma": -1.0}, {"sigma": [1.0, 2.0]},
                                {"sigma": np.zeros((2, 3))}, {"sigma": float("nan")}], ids=str)
def test_bad_arguments_are_refused_without_a_device(kw):
    with pytest.raises(ValueError):
        bf.estimate_risk(_float, _U8, **kw)
    with pytest.raises(ValueError):
        bf.evaluate_blind_risk(_float, [_U8], **kw)


def test_bad_modules_and_images_are_refused_without_a_device():
    for module in (None, 3, "unet", object()):
        with pytest.raises(ValueError, match="module"):
            bf.estimate_risk(module, _U8)
        with pytest.raises(ValueError, match="module"):
            bf.evaluate_blind_risk(module, [_U8])
    for bad in (np.zeros((8, 8, 3), np.uint8), np.zeros((1, 8, 8, 3), np.float32), np.zeros((1, 8, 8, 5), np.uint8),
                torch.zeros((8, 8, 3), dtype=torch.uint8), torch.zeros((1, 8, 8, 3)), [[1, 2, 3]]):
        with pytest.raises(ValueError):
            bf.estimate_risk(_float, bad)
        with pytest.raises(ValueError):
            bf.evaluate_blind_risk(_float, [bad])
    with pytest.raises(ValueError):
        bf.evaluate_blind_risk(_float, [])
    with pytest.raises(RuntimeError, match="GPU"):
        bf.estimate_risk(_float, torch.zeros((1, 8, 8, 3), dtype=torch.uint8), sigma=1.0)        # a host tensor is not uploaded


def test_low_level_calls_check_before_the_device():
    host = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    for kw in ({"probes": 0}, {"probes": 9}, {"amplitude": 0}, {"amplitude": 17}):
        with pytest.raises(ValueError):
            bf.risk_probe_stack_u8(host, **kw)
        with pytest.raises(ValueError):
            bf.risk_sums(host, torch.zeros((2, 8, 8, 3)), **{"probes": 1, "amplitude": 1, "seed": 0, **kw})
    for bad in (torch.zeros((8, 8, 3), dtype=torch.uint8), torch.zeros((1, 8, 8, 3)), torch.zeros((1, 8, 8, 5), dtype=torch.uint8),
                torch.zeros((0, 8, 8, 3), dtype=torch.uint8), np.zeros((1, 8, 8, 3), np.uint8)):
        with pytest.raises(ValueError):
            bf.risk_probe_stack_u8(bad)
    with pytest.raises(ValueError):
        bf.risk_sums(host, torch.zeros((2, 8, 8, 3), dtype=torch.float64), 1, 1, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        bf.risk_probe_stack_u8(host)
    with pytest.raises(RuntimeError, match="GPU"):
        bf.risk_sums(host, torch.zeros((2, 8, 8, 3)), 1, 1, 0)


def test_empty_batch_needs_no_device():
    for noisy in (np.zeros((0, 8, 9, 3), np.uint8), torch.zeros((0, 8, 9, 3), dtype=torch.uint8)):
        est = bf.estimate_risk(_float, noisy, probes=3)
        assert isinstance(est, bf.RiskEstimate) and all(isinstance(v, type(noisy)) for v in est)
        assert [tuple(v.shape) for v in est] == [(0,), (0,), (0, 3), (0,), (0,), (0,), (0, 3, 4)]
        assert all(str(v.dtype).endswith("float64") for v in est)


def test_names_are_exported():
    assert bf.RiskEstimate._fields == ("mse", "psnr", "sigma", "residual_rms", "divergence", "probe_spread", "sums")
    assert all(callable(getattr(bf, n)) for n in ("risk_probe_stack_u8", "risk_sums", "estimate_risk", "evaluate_blind_risk",
                                                  "format_risk_report"))


# ---- the host formula --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("probes,amplitude", [(1, 1), (3, 4)])
def test_host_formula_on_a_scaling(probes, amplitude):
    """f = alpha y: R = (1 - alpha)^2 sum y^2 and D_p = alpha HW a per channel, so the estimate is (1 - alpha)^2 sum y^2 / N -
    sigma^2 + 2 sigma^2 alpha"""
    H, W, alpha = 6, 10, 0.25
    y = np.random.default_rng(0).integers(0, 256, (2, H, W, 3)).astype(np.float64)
    sigma = np.array([[5.0, 10.0, 20.0], [7.0, 7.0, 7.0]])
    sums = np.empty((2, 3, 1 + probes))
    sums[:, :, 0] = (1.0 - alpha) ** 2 * (y * y).sum(axis=(1, 2))
    sums[:, :, 1:] = alpha * H * W * amplitude
    want = ((1.0 - alpha) ** 2 * (y * y).sum(axis=(1, 2)) / (H * W) - sigma ** 2 + 2.0 * sigma ** 2 * alpha).mean(axis=1)
    for arg in (sums, torch.from_numpy(sums)):
        est = K.risk_from_sums(arg, sigma, H, W, amplitude)
        assert all(isinstance(v, type(arg)) for v in est)
        get = lambda v: np.asarray(v)
        assert np.allclose(get(est.mse), want, rtol=1e-13, atol=0)
        assert np.allclose(get(est.psnr), 10.0 * np.log10(255.0 ** 2 / want), rtol=1e-13, atol=0)
        assert np.array_equal(get(est.divergence), [alpha, alpha]) and np.array_equal(get(est.sigma), sigma)
        assert np.allclose(get(est.residual_rms), (1.0 - alpha) * np.sqrt((y * y).mean(axis=(1, 2, 3))), rtol=1e-13, atol=0)
        assert np.isnan(get(est.probe_spread)).all() if probes == 1 else np.allclose(get(est.probe_spread), 0.0, atol=1e-9)
        ref = R.risk_from_sums(sums, sigma, H, W, amplitude)
        for k in ("mse", "psnr", "residual_rms", "divergence"):
            assert np.allclose(get(getattr(est, k)), ref[k], rtol=1e-13, atol=0), k


def test_host_formula_edge_cases():
    # the identity: R = 0, D = HW a: exactly sigma^2
    sums = np.zeros((1, 3, 3))
    sums[:, :, 1:] = 35 * 2.0
    est = K.risk_from_sums(sums, np.full((1, 3), 12.3), 5, 7, 2)
    assert est.mse[0] == 12.3 ** 2 and est.divergence[0] == 1.0 and est.residual_rms[0] == 0.0 and est.probe_spread[0] == 0.0
    # a negative estimate has no PSNR: +inf, and the spread of two probes is their sample standard deviation
    sums = np.array([[[10.0, 4.0, 8.0]]])
    est = K.risk_from_sums(sums, np.array([[3.0]]), 2, 5, 1)
    per_probe = 1.0 - 9.0 + 18.0 * np.array([0.4, 0.8])
    assert np.allclose(est.mse, 1.0 - 9.0 + 18.0 * 0.6, rtol=1e-14) and np.allclose(est.probe_spread, per_probe.std(ddof=1), rtol=1e-12)
    est = K.risk_from_sums(np.array([[[10.0, 1.0]]]), np.array([[3.0]]), 2, 5, 1)
    assert est.mse[0] < 0 and est.psnr[0] == np.inf
    for bad_sums, bad_sigma in ((np.zeros((1, 3)), np.zeros((1, 3))), (np.zeros((1, 3, 1)), np.zeros((1, 3))), (np.zeros((1, 3, 2)), np.zeros((3,)))):
        with pytest.raises(ValueError):
            K.risk_from_sums(bad_sums, bad_sigma, 4, 4, 1)


def test_report_formats_and_survives_strict_json():
    import json
    row = {"shape": [1, 8, 8, 3], "images": 1, "mse": -2.0, "psnr": float("inf"), "sigma_in": 3.0, "divergence": 0.5, "clipped_fraction": 0.25}
    report = {"method": "mad", "probes": 2, "amplitude": 1, "images": 1, "batches": [row], "aggregate": {k: v for k, v in row.items() if k != "shape"}}
    text = bf.format_risk_report(report)
    assert len(text.splitlines()) == 4 and "mad" in text.splitlines()[0] and "25.00%" in text
    assert json.loads(json.dumps(bf.metrics.json_safe(report), allow_nan=False))["aggregate"]["psnr"] is None


# ---- the reference -----------------------------------------------------------------------------------------------------------

def test_reference_probe_signs_and_stack():
    y = np.random.default_rng(1).integers(0, 256, (2, 5, 7, 3), dtype=np.uint8)
    y[0, 0, 0], y[1, -1, -1] = (0, 255, 3), (252, 1, 255)
    for a in (1, 4, 16):
        stack = R.probe_stack(y, 3, a, seed=5)
        assert stack.shape == (8, 5, 7, 3) and stack.dtype == np.uint8 and np.array_equal(stack[:2], y)
        d = stack.reshape(4, 2, 5, 7, 3).astype(int) - y.astype(int)
        assert (np.abs(d[1:]) == a).all()
        s0, s1 = R.probe_signs(y[0], 2, a, 5), R.probe_signs(y[1], 2, a, 5)
        free = (y[0].astype(int) - a >= 0) & (y[0].astype(int) + a <= 255) & (y[1].astype(int) - a >= 0) & (y[1].astype(int) + a <= 255)
        assert np.array_equal(s0[free], s1[free]) and free.mean() > 0.5          # image-local: the same bits for every image
    s = np.stack([R.probe_signs(np.full((64, 64, 3), 128, np.uint8), p, 1, seed) for p in (1, 2) for seed in (0, 2 ** 40 + 1)])
    assert abs(s.mean()) < 0.02 and len({t.tobytes() for t in s}) == 4            # fair, and (p, seed) select different vectors
    # word i of group j: elements 0..3 are the four words of Philox(counter = (0, 0, p, 2)), known-answer path of the oracle
    from oracle import bfcnn_oracle as O
    words = O._philox4x32_10([0], [0], [1], [2], 7, 0)
    want = [1 if int(w[0]) >> 31 else -1 for w in words]
    assert R.probe_signs(np.full((1, 4, 1), 100, np.uint8), 1, 1, 7).ravel().tolist() == want


@pytest.mark.parametrize("amplitude", [1, 4])
@pytest.mark.parametrize("seed", [0, 1])
def test_reference_estimator_tracks_the_truth(seed, amplitude):
    for sigma, clean, noisy in R.noisy_cases():
        est = R.estimate_risk(R.half_blur, noisy, sigma, probes=1, amplitude=amplitude, seed=seed)
        true = ((R.half_blur(noisy).astype(np.float64) - clean) ** 2).mean(axis=(1, 2, 3))
        rel = np.abs(est["mse"] - true) / true
        print(f"sigma {sigma} amplitude {amplitude} seed {seed}: true {np.round(true, 2)}, estimate {np.round(est['mse'], 2)}, "
              f"relative error {np.round(rel, 4)}")
        assert (rel <= 0.10).all()
