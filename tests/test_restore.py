"""The restoration loop without a GPU: the properties of the NumPy reference (tests/restore_reference.py) the GPU tests lean on, and
every refusal of restore, mask_constraint and block_constraint, each of which happens before a device is touched."""
import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from oracle import bfcnn_oracle as O
import restore_reference as R

RS = bf._restore                                                    # the module: bf.restore is its main function


def _constraints(rng, B=2, H=16, W=24, C=3):
    x = rng.uniform(0, 255, (B, H, W, C))
    yield ("mask", (rng.random((B, H, W, 1)) < 0.5).astype(np.uint8), x)
    yield ("mask", (rng.random((B, H, W, C)) < 0.3).astype(np.uint8), x)
    yield ("mask", R.bayer_mask(B, H, W), x)
    for s in (2, 4, 8):
        yield ("block", s, rng.uniform(0, 255, (B, H // s, W // s, C)))


# ---- reference properties ------------------------------------------------------------------------------------------------------

def test_projections_are_idempotent_and_symmetric():
    rng = np.random.default_rng(0)
    for con in _constraints(rng):
        shape = R.constraint_shape(con)
        v, w = rng.normal(0, 300, shape), rng.normal(0, 300, shape)
        pv = R.project(con, v)
        assert np.abs(R.project(con, pv) - pv).max() <= 1e-12 * 300, con[:2]
        assert abs((pv * w).sum() - (v * R.project(con, w)).sum()) <= 1e-9 * np.abs(v).sum(), con[:2]      # orthogonal: P = P^T
        assert np.abs(R.project(con, R.anchor(con, shape)) - R.anchor(con, shape)).max() <= 1e-12 * 255   # a lies in the range of P


def test_direction_closes_the_measured_gap():
    """P d = a - P y, and (I - P) d = (I - P)(D - y)"""
    rng = np.random.default_rng(1)
    for con in _constraints(rng):
        shape = R.constraint_shape(con)
        y, D = rng.normal(128, 400, shape), rng.normal(128, 400, shape)
        d, sumsq = R.direction(con, y, D)
        assert np.abs(R.project(con, d) - (R.anchor(con, shape) - R.project(con, y))).max() <= 1e-9
        assert np.abs((d - R.project(con, d)) - ((D - y) - R.project(con, D - y))).max() <= 1e-9
        assert np.allclose(sumsq, (d ** 2).sum(axis=(1, 2, 3)), rtol=1e-14)


def test_gamma_squared_is_never_negative():
    for beta in np.linspace(0.0, 1.0, 21):
        for h in np.concatenate([np.geomspace(1e-6, 1.0, 40), [R.step_size(t) for t in (1, 2, 10, 100, 1000, 100000)]]):
            assert R.gamma_squared(h, beta, 3.0) >= 0.0, (beta, h)
    assert R.gamma_squared(0.37, 1.0, 3.0) == 0.0                                   # beta = 1: no noise after y_0
    assert R.gamma_squared(0.5, 0.0, 2.0) == pytest.approx((1.0 - 0.25) * 4.0)


def test_step_size_schedule():
    for h0 in (0.01, 0.1, 1.0):
        h = np.array([R.step_size(t, h0) for t in range(1, 2000)])
        assert h[0] == h0 and (np.diff(h) >= 0).all() and h[-1] <= 1.0
        assert np.allclose(1.0 / h, 1.0 + (1.0 / h0 - 1.0) / np.arange(1, 2000))     # 1 / h_t - 1 = (1 / h0 - 1) / t
        assert RS.step_size(7, h0) == R.step_size(7, h0)
    assert R.step_size(10 ** 6, 0.01) > 0.9999


def test_normals_layout_and_statistics():
    z = R.normals((2, 3, 3), seed=5, sample_id=1, t=2)                              # n = 18: four full groups and half of a fifth
    r = O._philox4x32_10([4], [1], [2], [6], 5, 0)
    u1, u2 = ((int(r[0][0]) >> 8) + 1.0) / 2 ** 24, (int(r[1][0]) >> 8) / 2 ** 24
    rad = np.sqrt(-2.0 * np.log(u1))
    assert z.reshape(-1)[16] == rad * np.cos(2 * np.pi * u2) and z.reshape(-1)[17] == rad * np.sin(2 * np.pi * u2)
    big = R.normals((64, 64, 4), seed=9, sample_id=0, t=0)
    assert abs(big.mean()) < 5 / np.sqrt(big.size) and abs(big.var() - 1.0) < 5 * np.sqrt(2.0 / big.size)
    assert not np.array_equal(big, R.normals((64, 64, 4), 9, 1, 0)) and not np.array_equal(big, R.normals((64, 64, 4), 9, 0, 1))


_RUNS = {}


def _run(name):
    if name not in _RUNS:
        con, clean, base = R.cases()[name]
        _RUNS[name] = (con, clean, base, R.restore(R.linear_denoiser, con, beta=1.0, max_iterations=200))
    return _RUNS[name]


@pytest.mark.parametrize("name", ["mask", "bayer", "s2", "s4"])
def test_loop_freezes_and_keeps_the_constraint(name):
    con, clean, base, run = _run(name)
    steps, trace = run["iterations"], run["trace"]
    print(name, "iterations", steps.tolist(), "psnr", [round(R.psnr(run["image"][b], clean[b], R.unmeasured(con, clean.shape)[b]), 2)
                                                      for b in range(3)])
    assert (steps < 200).all() and len(trace) <= 200                               # every image froze
    for b in range(3):
        assert trace[steps[b], b] <= R.SIGMA_L < trace[steps[b] - 1, b]            # it froze when sigma_t first fell to sigma_l
        assert (trace[steps[b]:, b] == trace[steps[b], b]).all()                   # and never moved again
    x = run["image"]
    if con[0] == "mask":
        m = R.measured(con, x.shape)
        assert np.array_equal(x[m], con[2].astype(np.float64)[m])                  # measured samples: exactly the measurement
    else:
        s = con[1]
        assert np.abs(R.block_means(x, s) - con[2].astype(np.float64)).max() <= s * s * 2.0 ** -52 * 255
    where = R.unmeasured(con, x.shape)
    assert R.psnr(x, clean, where) > R.psnr(base, clean, where)                    # and beats the fill / nearest up-sampling


def test_loop_float32_storage_stays_close():
    con, _, _, run = _run("mask")
    f32 = R.restore(R.linear_denoiser, con, beta=1.0, max_iterations=200, storage=np.float32)
    assert np.array_equal(f32["iterations"], run["iterations"])
    assert np.abs(f32["image"] - run["image"]).max() <= 1e-3 and np.abs(f32["trace"] - run["trace"]).max() <= 1e-4


def test_frozen_image_does_not_move_in_the_reference_step():
    y = np.full((2, 2, 2, 1), 5.0)
    d = np.ones_like(y)
    out, steps, sigma = R.step(y, d, np.array([4.0 * 1.0, 4.0 * 100.0]), np.array([3, 3]), 4, 0.5, beta=1.0, sigma_l=2.55)
    assert np.array_equal(out[0], y[0]) and steps.tolist() == [3, 4] and np.array_equal(out[1], y[1] + 0.5)
    assert sigma.tolist() == [1.0, 10.0]
    out, steps, _ = R.step(y, d, np.array([400.0, 400.0]), np.array([2, 3]), 4, 0.5, beta=1.0)      # image 0 froze earlier
    assert np.array_equal(out[0], y[0]) and steps.tolist() == [2, 4]


# ---- refusals: all before a device is touched ----------------------------------------------------------------------------------

@pytest.fixture
def no_device(monkeypatch):
    """any upload, device query or native call fails the test"""
    def touched(*a, **k):
        raise AssertionError("a device was touched before the arguments were refused")
    monkeypatch.setattr(RS.A, "to_device", touched)
    monkeypatch.setattr(RS.A, "device_of", touched)
    monkeypatch.setattr(RS.N, "call", touched)
    monkeypatch.setattr(RS.N, "scratch", touched)


def _image(B=2, H=8, W=12, C=3, dtype=np.uint8):
    return np.zeros((B, H, W, C), dtype)


def test_constraint_refusals(no_device):
    img = _image()
    for bad in (np.ones((2, 8, 12, 2), np.uint8), np.ones((2, 8, 11, 1), np.uint8), np.ones((1, 8, 12, 1), np.uint8),
                np.ones((2, 8, 12), np.uint8), np.ones((2, 8, 12, 1), np.float32), np.ones((2, 8, 12, 1), bool), None):
        with pytest.raises(ValueError, match="mask"):
            bf.mask_constraint(img, bad)
    for bad in (_image(dtype=np.float64), _image(dtype=np.int32), np.zeros((8, 12, 3), np.uint8), _image(C=5), "x"):
        with pytest.raises(ValueError, match="image"):
            bf.mask_constraint(bad, np.ones((2, 8, 12, 1), np.uint8))
    for bad in (1, 9, 0, -2, 2.0, True, None):
        with pytest.raises(ValueError, match="factor"):
            bf.block_constraint(img, bad)
    for size in ((17, 24), (16, 25), (24, 24), (16, 12)):                           # a factor that does not divide, or another frame
        with pytest.raises(ValueError, match="factor"):
            bf.block_constraint(img, 2, size=size)
    with pytest.raises(ValueError, match="low"):
        bf.block_constraint(_image(dtype=np.float64), 2)
    con = bf.block_constraint(img, 3)
    assert con.shape == (2, 24, 36, 3) and con.kind == "block" and con.was_numpy
    assert bf.block_constraint(img, 2, size=(16, 24)).shape == (2, 16, 24, 3)
    con = bf.mask_constraint(torch.zeros((1, 4, 4, 1)), torch.ones((1, 4, 4, 1), dtype=torch.uint8))
    assert con.shape == (1, 4, 4, 1) and not con.was_numpy and con.factor == 1


def _identity(y):
    return y


def test_restore_refusals(no_device):
    con = bf.mask_constraint(_image(), np.ones((2, 8, 12, 1), np.uint8))
    bad_settings = [dict(beta=-0.1), dict(beta=1.5), dict(beta=float("nan")), dict(beta="1"), dict(h0=0.0), dict(h0=1.01), dict(h0=-1.0),
                    dict(sigma_l=300.0), dict(sigma_l=3.0, sigma_0=2.0), dict(sigma_l=0.0), dict(sigma_0=float("inf")),
                    dict(max_iterations=0), dict(max_iterations=-3), dict(max_iterations=2.5), dict(samples=0), dict(samples=1.5),
                    dict(check_every=0), dict(seed=-1), dict(seed=2 ** 64), dict(sample_ids=[0]), dict(sample_ids=[0, 1, 2]),
                    dict(sample_ids=[0, -1]), dict(sample_ids=[0, 2 ** 32]), dict(samples=2, sample_ids=[0, 1])]
    for settings in bad_settings:
        with pytest.raises(ValueError):
            bf.restore(_identity, con, **settings)
    with pytest.raises(ValueError, match="constraint"):
        bf.restore(_identity, ("mask", None, None))
    with pytest.raises(ValueError, match="constraint"):
        bf.restore(_identity, None)


def test_restore_refuses_wrong_denoisers(no_device):
    con = bf.mask_constraint(_image(), np.ones((2, 8, 12, 1), np.uint8))
    module = bf.DenoiserModule(bf.model_builder(O.canonical_config(no_layers=1)["model"], device="cpu").hydra)
    wrappers = [bf.NlmDenoiserModule(), bf.SelfEnsembleDenoiserModule(module), bf.StabilisedDenoiserModule(module),
                bf.TiledDenoiserModule(module), bf.PixelShuffleDenoiserModule(module, stride=2), bf.BurstDenoiserModule(module)]
    for wrapper in wrappers:
        with pytest.raises(ValueError, match="uint8 only"):
            bf.restore(wrapper, con)
    for bad in (None, 3, "unet_laplacian_v5.6", module.model_hydra.desc):
        with pytest.raises(ValueError, match="denoiser"):
            bf.restore(bad, con)
    grey = bf.mask_constraint(_image(C=1), np.ones((2, 8, 12, 1), np.uint8))
    for m in (module, bf.GraphedDenoiserModule(module)):                            # a 3-channel model on 1-channel images
        with pytest.raises(ValueError, match="channels"):
            bf.restore(m, grey)
    with pytest.raises(ValueError, match="uint8 only"):
        bf.inpaint(wrappers[0], _image(), np.ones((2, 8, 12, 1), np.uint8))
    with pytest.raises(ValueError, match="factor"):
        bf.super_resolve(module, _image(), 9)


def test_no_cpu_path():
    """well-formed arguments on the host: the repository's usual error"""
    module = bf.DenoiserModule(bf.model_builder(O.canonical_config(no_layers=1)["model"], device="cpu").hydra)
    con = bf.mask_constraint(_image(), np.ones((2, 8, 12, 1), np.uint8))
    with pytest.raises(RuntimeError, match="no CPU execution path"):
        bf.restore(module, con)                                                     # the model lives on the CPU
    host = bf.mask_constraint(torch.zeros((1, 4, 4, 3)), torch.ones((1, 4, 4, 1), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU execution path"):
        bf.restore(_identity, host)                                                 # host tensors are never uploaded
    with pytest.raises(RuntimeError, match="no CPU execution path"):
        bf.restore_init(host)
    with pytest.raises(RuntimeError, match="no CPU execution path"):
        bf.restore_direction(torch.zeros((1, 4, 4, 3)), torch.zeros((1, 4, 4, 3)), host)
    with pytest.raises(RuntimeError, match="no CPU execution path"):
        bf.restore_finish(torch.zeros((1, 4, 4, 3)), host)
    with pytest.raises(RuntimeError, match="no CPU execution path"):
        bf.restore_step(torch.zeros((1, 4, 4, 3)), torch.zeros((1, 4, 4, 3)), torch.zeros(1, dtype=torch.float64),
                        torch.zeros(1, dtype=torch.int32), 1, 0.01)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU execution path"):
            bf.restore(_identity, con)                                              # host arrays, but no GPU to upload them to


def test_operator_argument_checks(no_device):
    host = bf.mask_constraint(torch.zeros((1, 4, 4, 3)), torch.ones((1, 4, 4, 1), dtype=torch.uint8))
    with pytest.raises(ValueError, match="y"):
        bf.restore_direction(torch.zeros((1, 4, 5, 3)), torch.zeros((1, 4, 4, 3)), host)
    with pytest.raises(ValueError, match="denoised"):
        bf.restore_finish(torch.zeros((1, 4, 4, 3), dtype=torch.float64), host)
    with pytest.raises(ValueError, match="sigma_0"):
        bf.restore_init(host, sigma_0=-1.0)
    with pytest.raises(ValueError, match="sample_ids"):
        bf.restore_init(host, sample_ids=[0, 1])


def test_bayer_mask_measures_one_channel_per_pixel():
    m = bf.bayer_mask(2, 5, 6)
    assert m.shape == (2, 5, 6, 3) and m.dtype == np.uint8 and (m.sum(axis=3) == 1).all()
    assert np.array_equal(m, R.bayer_mask(2, 5, 6)) and m[0, 0, 0].tolist() == [1, 0, 0] and m[0, 1, 1].tolist() == [0, 0, 1]
