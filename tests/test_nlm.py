"""CPU tests of non-local means (blind_image_denoising_amd/nlm.py): the argument checks of every public entry and of
load_model("nlm", ...), nlm_params against tests/nlm_reference.py bit for bit, the weight table, and the quality of the definition
itself, measured with the reference on crops of tests/golden/lena.jpg.  No kernel is launched here."""
import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
import nlm_reference as R
import noise_reference
import risk_reference


def _batch(B=2, H=8, W=9, C=3):
    return np.zeros((B, H, W, C), np.uint8)


def _params(B=2):
    return torch.zeros((B, 2), dtype=torch.int64)


# ---- argument checks ---------------------------------------------------------------------------------------------------------

def test_nlm_params_argument_checks():
    for bad in ({"C": 0}, {"C": 5}, {"C": 3.0}, {"patch": 0}, {"patch": 4}, {"strength": -1.0}, {"strength": "auto"},
                {"strength": float("nan")}, {"strength": [0.5]}, {"strength": [[0.5, 0.5]]}):
        with pytest.raises(ValueError):
            bf.nlm_params(**{"sigma": [1.0, 2.0], "C": 3, **bad})
    for bad in (3.0, [[1.0, 2.0]]):
        with pytest.raises(ValueError, match="sigma"):
            bf.nlm_params(bad, 3)
    assert bf.nlm_params(torch.zeros(0), 3).shape == (0, 2)


def test_nlm_argument_checks():
    for images in (_batch().astype(np.float32), _batch()[0], np.zeros((2, 8, 9, 5), np.uint8), "x", None):
        with pytest.raises(ValueError, match="images"):
            bf.nlm(images, _params())
    for params in (_params(3), _params().int(), _params()[:, :1], _params().numpy(), None):
        with pytest.raises(ValueError, match="params"):
            bf.nlm(_batch(), params)
    for setting in ({"patch": 0}, {"patch": 4}, {"patch": 1.0}, {"search": 0}, {"search": 11}, {"search": True}):
        with pytest.raises(ValueError, match=next(iter(setting))):
            bf.nlm(_batch(), _params(), **setting)
    with pytest.raises(RuntimeError, match="must live on the GPU: non-local means has no CPU execution path"):
        bf.nlm(torch.from_numpy(_batch()), _params())
    out, weights = bf.nlm(_batch(0), _params(0), return_weights=True)             # an empty batch: no device is needed
    assert isinstance(out, np.ndarray) and out.shape == (0, 8, 9, 3) and out.dtype == np.uint8
    assert weights.shape == (0, 8, 9) and weights.dtype == np.int32
    out = bf.nlm(torch.from_numpy(_batch(0)), _params(0), cast_to_uint8=False)
    assert isinstance(out, torch.Tensor) and out.shape == (0, 8, 9, 3) and out.dtype == torch.float32


def test_module_argument_checks():
    for bad in ({"sigma": -1.0}, {"sigma": "x"}, {"sigma": np.zeros((2, 3, 1))}, {"patch": 4}, {"search": 0}, {"strength": -0.5},
                {"strength": "best"}, {"strength": np.zeros((2, 2))}):
        with pytest.raises(ValueError, match=next(iter(bad))):
            bf.NlmDenoiserModule(**bad)
    module = bf.NlmDenoiserModule(sigma=[[3.0, 4.0, 5.0], [0.0, 0.0, 0.0]], patch=2, search=7, strength="auto")
    assert (module.patch, module.search, module.strength) == (2, 7, "auto") and module.last_weights is None
    assert torch.allclose(module.sigma, torch.tensor([np.sqrt(50.0 / 3.0), 0.0], dtype=torch.float64), rtol=1e-15, atol=0.0)   # root mean square
    assert module.model_hydra is None and module.check_status() is True
    flt = module.float_form()
    assert type(flt) is bf.NlmDenoiserModule and flt._record is module._record and (flt.patch, flt.search) == (2, 7)
    for images in (_batch().astype(np.float32), _batch()[0], np.zeros((2, 8, 9, 5), np.uint8)):
        with pytest.raises(ValueError, match="image"):
            module(images)
    with pytest.raises(ValueError, match="sigma"):
        module(_batch(3))                                            # [2] sigmas, three images
    with pytest.raises(ValueError, match="strength"):
        bf.NlmDenoiserModule(sigma=5.0, strength=[0.5, 0.6, 0.7])(_batch(2))
    with pytest.raises(RuntimeError, match="no CPU execution path"):
        bf.NlmDenoiserModule(sigma=5.0)(torch.from_numpy(_batch()))
    assert bf.NlmDenoiserModule()(_batch(0)).shape == (0, 8, 9, 3)
    assert bf.NlmDenoiserModule()(torch.from_numpy(_batch(0, C=1))).shape == (0, 8, 9, 1)


def test_tune_argument_checks():
    for bad in ({"strengths": ()}, {"strengths": 0.5}, {"strengths": (0.5, -1.0)}, {"patch": 0}, {"search": 11}, {"sigma": -2.0},
                {"sigma": [1.0, 2.0, 3.0]}):
        with pytest.raises(ValueError, match=next(iter(bad))):
            bf.nlm_tune(_batch(), **bad)
    with pytest.raises(ValueError, match="images"):
        bf.nlm_tune(_batch().astype(np.float32))
    best, mse = bf.nlm_tune(_batch(0), strengths=(0.5, 1.0))
    assert best.shape == (0,) and mse.shape == (0, 2) and best.dtype == mse.dtype == np.float64


def test_load_model_takes_nlm_as_a_name():
    assert "nlm" not in bf.models and len(bf.configs) == 3
    module = bf.load_model("nlm")
    assert type(module) is bf.NlmDenoiserModule and (module.sigma, module.patch, module.search, module.strength) == (None, 1, 10, 0.55)
    module = bf.load_model("nlm", nlm={"sigma": 12.0, "patch": 2, "search": 5, "strength": 0.75})
    assert (module.sigma, module.patch, module.search, module.strength) == (12.0, 2, 5, 0.75)
    for bad in ({"bandwidth": 1.0}, {"patch": 9}, {"search": 0}, {"sigma": -1.0}, {"strength": "best"}, True, 0.55, "auto"):
        with pytest.raises(ValueError, match="nlm"):
            bf.load_model("nlm", nlm=bad)
    with pytest.raises(ValueError, match="nlm"):
        bf.load_model("unet_laplacian_v5.6", nlm={})
    with pytest.raises(ValueError, match="nlm"):
        bf.load_model("/definitely/not/here", nlm={"patch": 1})
    with pytest.raises(ValueError, match="burst"):                   # the other settings are still checked first
        bf.load_model("nlm", burst={"levels": 9})
    with pytest.raises(ValueError, match="must be a DenoiserModule"):          # the self-ensemble wraps networks only
        bf.load_model("nlm", self_ensemble="flips")
    full = bf.load_model("nlm", nlm={"sigma": 8.0}, tiled={"tile": 64}, pixel_shuffle=2, stabilise=True, burst=True)
    chain = []
    while full is not None:
        chain.append(type(full))
        full = getattr(full, "_module", None)
    assert chain == [bf.BurstDenoiserModule, bf.StabilisedDenoiserModule, bf.PixelShuffleDenoiserModule, bf.TiledDenoiserModule,
                     bf.NlmDenoiserModule]


# ---- the parameters and the table --------------------------------------------------------------------------------------------

def test_params_on_cpu_tensors_are_the_reference():
    sigmas = np.array([0.0, 0.25, 1.0, 7.25, 10.83, 20.0, 63.999, 255.0])
    for C in (1, 2, 3, 4):
        for patch in (1, 2, 3):
            for strength in (0.0, 0.25, 0.55, 1.4, 4.0):
                got = bf.nlm_params(torch.from_numpy(sigmas), C, patch, strength)
                want = R.params(sigmas, C, patch, strength)
                assert got.dtype == torch.int64 and got.shape == (8, 2) and np.array_equal(got.numpy(), want), (C, patch, strength)
    strengths = np.array([0.25, 0.4, 0.55, 0.75, 1.0, 1.4, 4.0, 0.0])
    got = bf.nlm_params(sigmas, 3, 1, strengths)                     # NumPy sigma, strength [B]
    assert np.array_equal(got.numpy(), R.params(sigmas, 3, 1, strengths))
    assert got[0].tolist() == [0, R.MULT_OFF] and got[7, 1] == R.MULT_OFF          # sigma 0 and strength 0: the clamp
    tiny = bf.nlm_params([1e-3], 1, 1, 0.25)
    assert tiny.tolist() == [[0, R.MULT_OFF]] and np.array_equal(tiny.numpy(), R.params([1e-3], 1, 1, 0.25))    # clamped, not overflowed
    extreme = R.params([255.0], 4, 3, 4.0)
    assert np.array_equal(bf.nlm_params([255.0], 4, 3, 4.0).numpy(), extreme)
    assert extreme[0, 0] == 2 * 255 * 255 * 196 and 0 < extreme[0, 1] < 2 ** 32 - 1


def test_table_properties():
    table = bf.nlm_table()
    assert table.dtype == np.int32 and table.shape == (1024,) and np.array_equal(table, R.table())
    assert (np.diff(table) <= 0).all()
    assert table[0] == 4078 and table[-2] == 1 and table[-1] == 0


# ---- the definition's own quality --------------------------------------------------------------------------------------------

def _mad_sigma(noisy):
    return noise_reference.combine_channels(noise_reference.noise_statistics(noisy)[:, :, 2])


def test_reference_quality_on_lena_with_the_estimated_sigma():
    """the reference gains 8.25 dB at sigma 20 and 5.57 dB at sigma 10 on lena[128:384, 128:384], sigma from the MAD estimator"""
    lena = R.load_lena()
    for sigma, gain in ((20.0, 6.0), (10.0, 4.0)):
        clean, noisy = R.noisy_crop(lena, slice(128, 384), slice(128, 384), sigma)
        estimate = _mad_sigma(noisy)
        assert abs(estimate[0] - sigma) < 1.5
        out, weights = R.nlm(noisy, R.params(estimate, 3, 1, 0.55), 1, 10)
        assert R.psnr(out, clean) - R.psnr(noisy, clean) >= gain, (sigma, R.psnr(noisy, clean), R.psnr(out, clean))
        assert weights.min() >= 1 and weights.max() <= 441 * 4096


def test_the_risk_estimate_picks_the_strength_of_least_true_error():
    """SURE (probes 2, amplitude 1, seed 5) on the noisy crop alone and the true error agree on the strength: 0.75"""
    clean, noisy = R.noisy_crop(R.load_lena(), slice(192, 320), slice(192, 320), 10.0)
    sets = [R.params([10.0], 3, 1, s) for s in R.STRENGTHS]
    true_mse = [np.mean((R.finish(num, den, False).astype(np.float64) - clean) ** 2) for num, den, *_ in R.nlm_many(noisy, sets, 1, 10)]
    stack = risk_reference.probe_stack(noisy, 2, 1, 5)
    results = [R.finish(num, den, False) for num, den, *_ in R.nlm_many(stack, [np.tile(p, (3, 1)) for p in sets], 1, 10)]
    estimated = [risk_reference.estimate_risk(lambda _, f=f: f, noisy, 10.0, probes=2, amplitude=1, seed=5)["mse"][0] for f in results]
    assert R.STRENGTHS[int(np.argmin(true_mse))] == R.STRENGTHS[int(np.argmin(estimated))] == 0.75, (true_mse, estimated)
