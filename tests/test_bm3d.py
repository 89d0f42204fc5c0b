"""CPU tests of BM3D (blind_image_denoising_amd/bm3d.py): the argument checks of every public entry and of load_model("bm3d", ...),
bm3d_params against tests/bm3d_reference.py bit for bit, the wrapper protocol of Bm3dDenoiserModule, and the definition itself,
measured with the reference on crops of tests/golden/lena.jpg.  No kernel is launched here."""
import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import _args as A
import bm3d_reference as R
import nlm_reference


def _batch(B=2, H=8, W=9, C=3):
    return np.zeros((B, H, W, C), np.uint8)


def _params(B=2):
    return torch.zeros((B, 4), dtype=torch.int64)


# ---- argument checks ---------------------------------------------------------------------------------------------------------

def test_bm3d_params_argument_checks():
    for bad in ({"C": 0}, {"C": 5}, {"C": 3.0}, {"threshold": -1.0}, {"threshold": "x"}, {"threshold": float("nan")},
                {"match": 2500.0}, {"match": (2500.0,)}, {"match": (2500.0, -1.0)}, {"match": ("a", 1.0)}):
        with pytest.raises(ValueError, match=next(k for k in bad)):
            bf.bm3d_params(**{"sigma": [1.0, 2.0], "C": 3, **bad})
    for bad in (3.0, [[1.0, 2.0]]):
        with pytest.raises(ValueError, match="sigma"):
            bf.bm3d_params(bad, 3)
    assert bf.bm3d_params(torch.zeros(0), 3).shape == (0, 4)


@pytest.mark.parametrize("entry", ["bm3d", "bm3d_step"])
def test_operator_argument_checks(entry):
    if entry == "bm3d":
        def run(images, params, **settings):
            return bf.bm3d(images, params, **settings)
    else:
        def run(images, params, **settings):
            return bf.bm3d_step(images, images, params, settings.pop("wiener", False), **settings)
    for images in (_batch().astype(np.float32), _batch()[0], np.zeros((2, 8, 9, 5), np.uint8), _batch(H=7), _batch(W=7), "x", None):
        with pytest.raises(ValueError, match="images|noisy"):
            run(images, _params())
    for params in (_params(3), _params().int(), _params()[:, :2], _params().numpy(), None):
        with pytest.raises(ValueError, match="params"):
            run(_batch(), params)
    for setting in ({"search": 0}, {"search": 13}, {"search": 1.0}, {"step": 0}, {"step": 9}, {"step": True}, {"wiener": 1}):
        with pytest.raises(ValueError, match=next(iter(setting))):
            run(_batch(), _params(), **setting)
    with pytest.raises(RuntimeError, match="must live on the GPU: BM3D has no CPU execution path"):
        run(torch.from_numpy(_batch()), _params())
    out, weights = run(_batch(0), _params(0), return_weights=True)    # an empty batch: no device is needed
    assert isinstance(out, np.ndarray) and out.shape == (0, 8, 9, 3) and out.dtype == np.uint8
    assert weights.shape == (0, 8, 9) and weights.dtype == np.int64
    out = run(torch.from_numpy(_batch(0)), _params(0), cast_to_uint8=False)
    assert isinstance(out, torch.Tensor) and out.shape == (0, 8, 9, 3) and out.dtype == torch.float32


def test_step_wants_a_guide_like_noisy():
    for guide in (_batch(H=9), _batch(C=1), _batch(3), torch.from_numpy(_batch()), _batch().astype(np.float32), None):
        with pytest.raises(ValueError, match="guide"):
            bf.bm3d_step(_batch(), guide, _params(), True)


def test_module_argument_checks():
    for bad in ({"sigma": -1.0}, {"sigma": "x"}, {"sigma": np.zeros((2, 3, 1))}, {"search": 0}, {"search": 13}, {"step": 0},
                {"step": 9}, {"threshold": -0.5}, {"threshold": "soft"}, {"wiener": 1}, {"wiener": None}):
        with pytest.raises(ValueError, match=next(iter(bad))):
            bf.Bm3dDenoiserModule(**bad)
    module = bf.Bm3dDenoiserModule(sigma=[[3.0, 4.0, 5.0], [0.0, 0.0, 0.0]], search=7, step=3, threshold=3.0, wiener=False)
    assert (module.search, module.step, module.threshold, module.wiener) == (7, 3, 3.0, False) and module.last_weights is None
    assert torch.allclose(module.sigma, torch.tensor([np.sqrt(50.0 / 3.0), 0.0], dtype=torch.float64), rtol=1e-15, atol=0.0)   # root mean square
    assert module.model_hydra is None and module.check_status() is True
    flt = module.float_form()
    assert type(flt) is bf.Bm3dDenoiserModule and flt._record is module._record and (flt.search, flt.step, flt.wiener) == (7, 3, False)
    for images in (_batch().astype(np.float32), _batch()[0], np.zeros((2, 8, 9, 5), np.uint8), _batch(H=7)):
        with pytest.raises(ValueError, match="image"):
            module(images)
    with pytest.raises(ValueError, match="sigma"):
        module(_batch(3))                                            # [2] sigmas, three images
    with pytest.raises(RuntimeError, match="no CPU execution path"):
        bf.Bm3dDenoiserModule(sigma=5.0)(torch.from_numpy(_batch()))
    assert bf.Bm3dDenoiserModule()(_batch(0)).shape == (0, 8, 9, 3)
    assert bf.Bm3dDenoiserModule()(torch.from_numpy(_batch(0, C=1))).shape == (0, 8, 9, 1)


def test_load_model_takes_bm3d_as_a_name():
    assert "bm3d" not in bf.models and bf.bm3d_settings is bf._bm3d.parse_setting and bf._bm3d.MODEL_NAME == "bm3d"
    module = bf.load_model("bm3d")
    assert type(module) is bf.Bm3dDenoiserModule
    assert (module.sigma, module.search, module.step, module.threshold, module.wiener) == (None, 12, 4, 2.7, True)
    module = bf.load_model("bm3d", bm3d={"sigma": 12.0, "search": 5, "step": 3, "threshold": 3.0, "wiener": False})
    assert (module.sigma, module.search, module.step, module.threshold, module.wiener) == (12.0, 5, 3, 3.0, False)
    for bad in ({"patch": 1}, {"search": 13}, {"step": 0}, {"sigma": -1.0}, {"threshold": "hard"}, {"wiener": "yes"}, True, 2.7, "auto"):
        with pytest.raises(ValueError, match="bm3d"):
            bf.load_model("bm3d", bm3d=bad)
    with pytest.raises(ValueError, match="bm3d may set"):
        bf.bm3d_settings({"radius": 2})
    assert bf.bm3d_settings(None) == {} and bf.bm3d_settings({"step": 2}) == {"step": 2}
    for path in ("unet_laplacian_v5.6", "/definitely/not/here", "nlm"):
        with pytest.raises(ValueError, match="bm3d"):                # the option belongs to the name
            bf.load_model(path, bm3d={})
    with pytest.raises(ValueError, match="nlm"):
        bf.load_model("bm3d", nlm={})
    with pytest.raises(ValueError, match="burst"):                   # the other settings are still checked first
        bf.load_model("bm3d", burst={"levels": 9})
    with pytest.raises(ValueError, match="must be a DenoiserModule"):          # the self-ensemble wraps networks only
        bf.load_model("bm3d", self_ensemble="flips")
    full = bf.load_model("bm3d", bm3d={"sigma": 8.0}, tiled={"tile": 64}, pixel_shuffle=2, stabilise=True, burst=True)
    chain = []
    while full is not None:
        chain.append(type(full))
        full = getattr(full, "_module", None)
    assert chain == [bf.BurstDenoiserModule, bf.StabilisedDenoiserModule, bf.PixelShuffleDenoiserModule, bf.TiledDenoiserModule,
                     bf.Bm3dDenoiserModule]


# ---- the protocol of DenoiserWrapper (tests/test_args.py states it for every other wrapper) ------------------------------------

def test_the_module_holds_the_base_protocol(monkeypatch):
    cls, settings = bf.Bm3dDenoiserModule, {"sigma": 7.0, "search": 5, "step": 3, "threshold": 3.0, "wiener": False}
    w = cls(**settings)
    assert isinstance(w, bf.DenoiserWrapper) and tuple(cls.SETTINGS) == tuple(settings) and w._cast_to_uint8 is True
    assert w._module is None and w._base is None
    f = w.float_form()
    assert type(f) is cls and f is not w and f._cast_to_uint8 is False and f._module is None and f._base is None
    assert isinstance(w._record, dict) and f._record is w._record
    for name, value in settings.items():
        assert type(getattr(f, name)) is type(value) and getattr(f, name) == getattr(w, name) == value
        assert getattr(w, name) is getattr(w, "_" + name)
        with pytest.raises(AttributeError):
            setattr(w, name, value)
    assert w.check_status() is True and f.check_status(wait=False) is True and w.model_hydra is None
    with pytest.raises(RuntimeError, match="no CPU execution path") as e:       # a well-formed host tensor: there is nowhere to run it
        w(torch.zeros((1, 16, 16, 3), dtype=torch.uint8))
    assert "must live on the GPU" in str(e.value)

    def touched(*args, **kwargs):                                    # an empty batch comes back before anything is placed or launched
        raise AssertionError("an empty batch reached the GPU")
    monkeypatch.setattr(bf._native, "call", touched)
    monkeypatch.setattr(A, "to_device", touched)
    for given in (np.zeros((0, 16, 16, 3), np.uint8), torch.zeros((0, 16, 16, 3), dtype=torch.uint8)):
        for m in (w, f):
            out = m(given)
            assert type(out) is type(given) and tuple(out.shape) == (0, 16, 16, 3) and "uint8" in str(out.dtype)


# ---- the parameters ----------------------------------------------------------------------------------------------------------

def test_params_on_cpu_tensors_are_the_reference():
    sigmas = np.array([0.0, 0.5, 1.0, 7.25, 10.83, 20.0, 63.999, 255.0])
    for C in (1, 2, 3, 4):
        for threshold, match in ((2.7, (2500.0, 400.0)), (3.1, (300.0, 48.0)), (0.0, (0.0, 1e-3))):
            got = bf.bm3d_params(torch.from_numpy(sigmas), C, threshold, match)
            want = R.params(sigmas, C, threshold, match)
            assert got.dtype == torch.int64 and got.shape == (8, 4) and np.array_equal(got.numpy(), want), (C, threshold, match)
    got = bf.bm3d_params(sigmas, 3)                                  # NumPy sigma, the defaults
    assert np.array_equal(got.numpy(), R.params(sigmas, 3))
    assert got[0].tolist() == [480000, 0, 76800, 0]                  # sigma 0: nothing is shrunk
    assert got[5].tolist() == [480000, int(np.floor(2.7 * 2.7 * 400.0 * 64.0)), 76800, 25600]
    assert np.array_equal(bf.bm3d_params([255.0], 4).numpy(), R.params([255.0], 4))


# ---- the definition itself ---------------------------------------------------------------------------------------------------

def test_positions_and_matrices_of_the_reference():
    assert R.positions(8, 4) == [0] and R.positions(13, 4) == [0, 4, 5] and R.positions(16, 8) == [0, 8] and R.positions(45, 3)[-2:] == [36, 37]
    for C, (Af, n2, Bk, s) in R.CHANNELS.items():
        assert np.array_equal(Bk @ Af, s * np.eye(C, dtype=np.int64)) and np.array_equal((Af * Af).sum(axis=1), n2)
    h = R.hadamard(16)
    assert np.array_equal(h @ h, 16 * np.eye(16, dtype=np.int64)) and np.array_equal(h[:2, :2], [[1, 1], [1, -1]])


def test_sigma_zero_is_the_identity_of_the_reference():
    rng = np.random.default_rng(3)
    for C in (1, 3):
        images = rng.integers(0, 256, (1, 21, 19, C), dtype=np.uint8)
        images[0, :10, :10] = 40                                     # blocks that repeat: groups of more than one
        prm = R.params([0.0], C)
        basic, weights = R.bm3d_step(images, images, prm, False, 5, 3)
        assert np.array_equal(basic, images) and weights.min() >= 1
        assert np.array_equal(R.bm3d_step(images, basic, prm, True, 5, 3)[0], images)
        assert np.array_equal(R.bm3d(images, prm, 5, 3, cast_to_uint8=False)[0], images.astype(np.float32))


_TABLE = {10.0: (28.16, 36.30, 36.61), 20.0: (22.26, 32.13, 32.80), 30.0: (18.90, 29.63, 30.44)}      # noisy, first step, both


@pytest.mark.parametrize("sigma", sorted(_TABLE))
def test_reference_quality_on_lena(sigma):
    """the 128 x 128 crop lena[192:320, 192:320], noise of seed 0: the reference's PSNR is the table's (within 0.05 dB), both steps
    are at least 1.5 dB above non-local means (patch 1, search 10, strength 0.55), and the second step is above the first"""
    clean, noisy = nlm_reference.noisy_crop(nlm_reference.load_lena(), slice(192, 320), slice(192, 320), sigma)
    prm = R.params([sigma], 3)
    basic = R.bm3d_step(noisy, noisy, prm, False)[0]
    both = R.bm3d_step(noisy, basic, prm, True)[0]
    nlm = nlm_reference.nlm(noisy, nlm_reference.params([sigma], 3, 1, 0.55), 1, 10)[0]
    got = tuple(nlm_reference.psnr(a, clean) for a in (noisy, basic, both))
    print(f"sigma {sigma}: noisy {got[0]:.2f}, nlm {nlm_reference.psnr(nlm, clean):.2f}, first step {got[1]:.2f}, both {got[2]:.2f} dB")
    assert all(abs(g - t) <= 0.05 + 0.005 for g, t in zip(got, _TABLE[sigma])), got      # the table is rounded to 0.01
    assert got[2] >= nlm_reference.psnr(nlm, clean) + 1.5 and got[2] > got[1]


def test_reference_quality_on_one_channel():
    """the green channel alone at sigma 20: 22.35 dB noisy, 29.71 after the first step, 30.39 after both"""
    clean, noisy = nlm_reference.noisy_crop(nlm_reference.load_lena(), slice(192, 320), slice(192, 320), 20.0)
    clean, noisy = clean[..., 1:2], noisy[..., 1:2]
    prm = R.params([20.0], 1)
    basic = R.bm3d_step(noisy, noisy, prm, False)[0]
    both = R.bm3d_step(noisy, basic, prm, True)[0]
    got = tuple(nlm_reference.psnr(a, clean) for a in (noisy, basic, both))
    assert all(abs(g - t) <= 0.055 for g, t in zip(got, (22.35, 29.71, 30.39))), got
