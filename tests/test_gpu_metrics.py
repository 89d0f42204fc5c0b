"""GPU tests of bf_image_metrics (csrc/metrics.hip), blind_image_denoising_amd.metrics and the validation inside train_loop.

Yardsticks: NumPy int64 / float64 for the sums, oracle.bfcnn_oracle.ssim_mean_and_grad (fp64, one-image batches) for SSIM.

Bounds.  The kernel carries the window moments, S and every sum in fp64, so what is left is fp64 rounding amplified by the
cancellation in q - a^2 - b^2.  Measured on an MI355X over the whole set of test_ssim_matches_the_oracle the largest
|ssim - oracle| was 6.9e-13 (a constant 128 against a constant 131: the variance terms are pure cancellation; on the
lena crops and on noise it is 1e-16 to 3.3e-14) and over test_float32_sums_match_numpy the largest relative deviation of a sum was 3.8e-16;
each test prints its figure before it asserts 4 x the measured value."""
import json
import os

import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import _native as N
from blind_image_denoising_amd import metrics as M
from oracle import bfcnn_oracle as O
import unet_v56 as V
from guarded import dev as _dev, guard_bands

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guard_bands")]

SSIM_BOUND = 4 * 6.9e-13            # 4 x the largest |ssim - oracle| measured over test_ssim_matches_the_oracle's cases
F32_SUM_REL_BOUND = 4 * 3.8e-16     # 4 x the largest relative deviation measured over test_float32_sums_match_numpy's cases
TRAIN_SSIM_REL_BOUND = 1e-5         # the bar tests/test_gpu_training.py holds bf_train_step's ssim_loss to (relative, floor 1e-3)
LENA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lena.jpg")


def _oracle_ssim(a, b, filter_size=11, max_val=255.0):
    """per-image SSIM of two [B,H,W,C] arrays through the fp64 oracle (one-image batches)"""
    return np.array([O.ssim_mean_and_grad(a[i:i + 1].astype(np.float64), b[i:i + 1].astype(np.float64), max_val, filter_size, 1.5)[0]
                     for i in range(a.shape[0])])


def _noisy(clean, sigma, seed):
    rng = np.random.default_rng(seed)
    return np.clip(np.round(clean.astype(np.float64) + rng.normal(0.0, sigma, clean.shape)), 0, 255).astype(np.uint8)


def _lena(h, w, y0=100, x0=120):
    img = bf.load_image(path=LENA, image_size=None, num_channels=3, expand_dims=False, normalize=False)
    return np.ascontiguousarray(img[None, y0:y0 + h, x0:x0 + w, :]).astype(np.uint8)


@pytest.mark.parametrize("shape", [(1, 11, 11, 3), (1, 37, 53, 3), (3, 37, 53, 1), (5, 256, 256, 3), (1, 375, 1242, 3), (2, 64, 300, 4),
                                   (7, 27, 80, 2)], ids=lambda s: "x".join(map(str, s)))
def test_uint8_sums_are_exact(shape):
    rng = np.random.default_rng(sum(shape))
    a, b = rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8)
    a[0, 0, 0, 0], b[0, 0, 0, 0], a[-1, -1, -1, -1], b[-1, -1, -1, -1] = 255, 0, 0, 255        # the corners count, once
    sums = bf.image_metric_sums(_dev(a), _dev(b)).cpu().numpy()
    d = a.astype(np.int64) - b.astype(np.int64)
    assert sums.dtype == np.float64 and sums.shape == (shape[0], 4)
    assert np.array_equal(sums[:, 0], (d * d).sum(axis=(1, 2, 3)).astype(np.float64))
    assert np.array_equal(sums[:, 1], np.abs(d).sum(axis=(1, 2, 3)).astype(np.float64))
    assert np.array_equal(sums[:, 3], np.full(shape[0], (shape[1] - 10) * (shape[2] - 10) * shape[3], np.float64))
    m = bf.image_metrics(a, b)                                                   # NumPy in, NumPy out
    n = float(np.prod(shape[1:]))
    assert isinstance(m.psnr, np.ndarray) and np.array_equal(m.mse, sums[:, 0] / n) and np.array_equal(m.mae, sums[:, 1] / n)
    assert np.allclose(m.psnr, 20 * np.log10(255.0) - 10 * np.log10(sums[:, 0] / n), rtol=1e-14, atol=0)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_identical_images(dtype):
    a = np.random.default_rng(3).integers(0, 256, (3, 40, 70, 3)).astype(dtype)
    t = _dev(a)
    m = bf.image_metrics(t, t.clone())
    assert all(v.is_cuda and v.dtype == torch.float64 and v.shape == (3,) for v in m)
    assert (m.mse == 0).all() and (m.mae == 0).all() and torch.isinf(m.psnr).all() and (m.psnr > 0).all()
    dev = float((m.ssim - 1.0).abs().max())
    print(f"identical images ({np.dtype(dtype).name}): max |ssim - 1| = {dev:.3e}")
    assert dev <= SSIM_BOUND
    assert torch.isinf(bf.psnr(t, t)).all() and float((bf.ssim(t, t) - 1).abs().max()) <= SSIM_BOUND and (bf.mae(t, t) == 0).all()


def _ssim_cases():
    cases = []
    for sigma in (10.0, 30.0):
        clean = _lena(256, 256)
        cases.append((f"lena256 sigma {sigma:g}", clean, _noisy(clean, sigma, 1)))
    clean = _lena(97, 141, 30, 40)
    cases.append(("lena 97x141 sigma 10", clean, _noisy(clean, 10.0, 2)))
    const = np.full((2, 33, 45, 3), 128, np.uint8)
    cases.append(("constant vs noise", const, _noisy(const, 20.0, 3)))
    cases.append(("constant vs constant", const, np.full_like(const, 131)))
    rng = np.random.default_rng(4)
    cases.append(("random", rng.integers(0, 256, (3, 37, 53, 3), dtype=np.uint8), rng.integers(0, 256, (3, 37, 53, 3), dtype=np.uint8)))
    cases.append(("random 1ch", rng.integers(0, 256, (2, 64, 200, 1), dtype=np.uint8), rng.integers(0, 256, (2, 64, 200, 1), dtype=np.uint8)))
    return cases


def test_ssim_matches_the_oracle():
    worst = 0.0
    for name, a, b in _ssim_cases():
        for filter_size in (11, 7):
            ref = _oracle_ssim(a, b, filter_size)
            for dtype in (np.uint8, np.float32):
                x, y = a.astype(dtype), b.astype(dtype)
                if dtype == np.float32 and name.startswith("lena256"):           # float images off the integer grid
                    y = (y + np.random.default_rng(5).uniform(-0.5, 0.5, y.shape)).astype(np.float32)
                    r = _oracle_ssim(x, y, filter_size)
                else:
                    r = ref
                got = bf.ssim(_dev(x), _dev(y), filter_size=filter_size).cpu().numpy()
                dev = float(np.abs(got - r).max())
                worst = max(worst, dev)
                print(f"ssim {name} {filter_size}x{filter_size} {np.dtype(dtype).name}: {got[0]:.6f}, max |dev| = {dev:.3e}")
    print(f"largest |ssim - oracle| = {worst:.3e} (bound {SSIM_BOUND:.3e})")
    assert worst <= SSIM_BOUND


def test_float32_sums_match_numpy():
    worst = 0.0
    rng = np.random.default_rng(6)
    for shape in [(1, 11, 11, 3), (2, 37, 53, 3), (3, 256, 256, 3), (1, 375, 1242, 3), (2, 50, 70, 1)]:
        a = rng.uniform(0, 255, shape).astype(np.float32)
        b = (a + rng.normal(0, 10, shape)).astype(np.float32)
        sums = bf.image_metric_sums(_dev(a), _dev(b)).cpu().numpy()
        d = a.astype(np.float64) - b.astype(np.float64)
        ref = np.stack([(d * d).sum(axis=(1, 2, 3)), np.abs(d).sum(axis=(1, 2, 3))], axis=1)
        dev = float((np.abs(sums[:, :2] - ref) / ref).max())
        worst = max(worst, dev)
        print(f"float32 sums {shape}: max relative deviation {dev:.3e}")
    print(f"largest relative deviation = {worst:.3e} (bound {F32_SUM_REL_BOUND:.3e})")
    assert worst <= F32_SUM_REL_BOUND


def test_agrees_with_the_training_loss_ssim():
    """1 - mean ssim (7 x 7, float32) against losses[BF_LOSS_SSIM] of a bf_train_step on the same prediction and ground truth"""
    cfg = O.canonical_config(no_layers=2)
    cfg["loss"].update({"ssim_multiplier": 1.0})
    spec = O.ResnetSpec.from_config(cfg["model"])
    params, state = O.init_params(spec, seed=42, nontrivial_bn=True)
    m = bf.model_builder(cfg["model"], device="cuda").hydra
    m.set_weights(params, state)
    fns = bf.build_train_functions(m, bf.loss_function_builder(cfg["loss"]))
    clean, noisy = O.synthetic_batch(3, 24, 40, seed=11)
    gt = _dev(clean.astype(np.float32))
    _, _, dl, pred, _ = fns.train_step_single_gpu(gt, _dev(noisy.astype(np.float32)), (1.0,), 0.0, None)
    loss = float(dl[0]["ssim_loss"].item())
    got = 1.0 - float(bf.ssim(gt, pred.contiguous(), filter_size=7).mean())
    bound = SSIM_BOUND + TRAIN_SSIM_REL_BOUND * max(abs(loss), 1e-3)
    print(f"ssim loss: train step {loss:.9f}, image_metrics {got:.9f}, |diff| = {abs(got - loss):.3e} (bound {bound:.3e})")
    assert abs(got - loss) <= bound


def test_two_calls_are_bitwise_equal():
    clean = np.concatenate([_lena(256, 256)] * 5)
    a, b = _dev(clean), _dev(_noisy(clean, 20.0, 7))
    for x, y in ((a, b), (a.float(), b.float())):
        first = bf.image_metric_sums(x, y).cpu().numpy()
        for _ in range(3):
            assert np.array_equal(bf.image_metric_sums(x, y).cpu().numpy().view(np.uint64), first.view(np.uint64))


# ---- evaluate -----------------------------------------------------------------------------------

class _Recording:
    def __init__(self, module):
        self.module, self.noisy, self.denoised = module, [], []

    def check_status(self, wait=True):
        return self.module.check_status(wait) if hasattr(self.module, "check_status") else True

    def __call__(self, x):
        assert x.is_cuda and x.dtype == torch.uint8
        out = self.module(x)
        self.noisy.append(x.cpu().numpy())
        self.denoised.append(out.cpu().numpy())
        return out


def _small_module():
    cfg = O.canonical_config(no_layers=2)
    spec = O.ResnetSpec.from_config(cfg["model"])
    params, state = O.init_params(spec, seed=42)
    model = bf.model_builder(cfg["model"], device="cuda:0").hydra
    model.set_weights(params, state)
    return bf.DenoiserModule(model)


def _reference_level(clean, noisy, denoised):
    """one level of evaluate from host arrays: NumPy for PSNR / MAE, the oracle for SSIM"""
    def per_image(x):
        d = clean.astype(np.int64) - x.astype(np.int64)
        mse = (d * d).sum(axis=(1, 2, 3)) / float(np.prod(clean.shape[1:]))
        with np.errstate(divide="ignore"):
            return 20 * np.log10(255.0) - 10 * np.log10(mse), _oracle_ssim(clean, x), np.abs(d).sum(axis=(1, 2, 3)) / float(np.prod(clean.shape[1:]))
    return per_image(noisy), per_image(denoised)


def test_evaluate_reports_what_the_arrays_say():
    rec = _Recording(_small_module())
    c0, _ = O.synthetic_batch(3, 48, 64, seed=1)
    c1, _ = O.synthetic_batch(2, 33, 80, seed=2)                                 # two shapes in one call
    levels = (10, 25)
    report = bf.evaluate(rec, [c0, _dev(c1)], noise_std=levels, seed=5)
    assert [r["noise_std"] for r in report] == [10.0, 25.0] and len(rec.noisy) == 4
    for li, r in enumerate(report):
        parts = [_reference_level(c, rec.noisy[2 * li + bi], rec.denoised[2 * li + bi]) for bi, c in enumerate((c0, c1))]
        n = [np.concatenate([p[0][k] for p in parts]) for k in range(3)]
        d = [np.concatenate([p[1][k] for p in parts]) for k in range(3)]
        assert r["images"] == 5
        noise = rec.noisy[2 * li].astype(np.float64) - c0
        inner = (c0 > 2 * levels[li]) & (c0 < 255 - 2 * levels[li])             # away from the clipping: truncated at 2 sigma
        assert np.abs(noise[inner]).max() <= 2 * levels[li] + 0.5 and 0.7 * levels[li] < noise[inner].std() < levels[li]
        for key, ref, tol in (("psnr_noisy", n[0], 1e-12), ("psnr_denoised", d[0], 1e-12), ("ssim_noisy", n[1], SSIM_BOUND),
                              ("ssim_denoised", d[1], SSIM_BOUND), ("mae_noisy", n[2], 1e-12), ("mae_denoised", d[2], 1e-12)):
            print(f"sigma {levels[li]} {key}: {r[key]:.12f} reference {ref.mean():.12f}")
            assert abs(r[key] - ref.mean()) <= tol * max(1.0, abs(ref.mean())), key
        assert r["improved_psnr"] == int((n[0] < d[0]).sum()) and r["improved_ssim"] == int((n[1] < d[1]).sum())
        assert r["improved_mae"] == int((d[2] < n[2]).sum())
    again = bf.evaluate(_small_module(), [c0, c1], noise_std=levels, seed=5)
    assert again == report                                                       # same seed, same record
    assert bf.evaluate(_small_module(), [c0, c1], noise_std=levels, seed=6) != report


def test_evaluate_with_an_identity_module():
    c0, _ = O.synthetic_batch(2, 40, 40, seed=3)
    report = bf.evaluate(lambda x: x, [c0], noise_std=(0, 20))
    for r in report:
        assert r["images"] == 2 and r["improved_psnr"] == r["improved_ssim"] == r["improved_mae"] == 0
        for k in ("psnr", "ssim", "mae"):
            assert r[f"{k}_denoised"] == r[f"{k}_noisy"]
    assert report[0]["psnr_noisy"] == float("inf") and report[0]["mae_noisy"] == 0.0 and np.isfinite(report[1]["psnr_noisy"])


def test_shipped_unet_v56_on_the_kitti_crops():
    """the acceptance inequalities of tests/test_gpu_unet_pretrained.py through image_metrics, then through evaluate"""
    z, _ = V.load()
    module = bf.load_denoiser_model("unet_laplacian_v5.6")
    kitti = z["kitti"]
    for std in (15.0, 20.0, 25.0, 30.0):
        for i in range(kitti.shape[0]):
            clean = kitti[i:i + 1]
            noisy = V.corrupt(clean, std, seed=int(std))
            n, d = bf.image_metrics(clean, noisy), bf.image_metrics(clean, module(noisy))
            print(f"numpy noise sigma {std:g} frame {i}: psnr {n.psnr[0]:.3f} -> {d.psnr[0]:.3f}, ssim {n.ssim[0]:.5f} -> {d.ssim[0]:.5f}, "
                  f"mae {n.mae[0]:.3f} -> {d.mae[0]:.3f}")
            assert n.psnr[0] < d.psnr[0] and n.ssim[0] < d.ssim[0] and d.mae[0] < n.mae[0], (std, i)
    report = bf.evaluate(module, [kitti], noise_std=(10, 15, 20, 25, 30))
    print(M.format_report(report))
    full = bf.evaluate(module, [z["kitti_full"][None]], noise_std=(10, 15, 20, 25, 30))
    print("whole frame:\n" + M.format_report(full))
    for r in report[1:]:                                                         # sigma 10 is printed, not asserted
        assert r["images"] == 2
        assert r["improved_psnr"] == r["improved_ssim"] == r["improved_mae"] == r["images"], r


# ---- validation inside train_loop ---------------------------------------------------------------

def _train_run(tmp_path, name, evaluation):
    cfg = O.canonical_config(no_layers=6)
    cfg["train"].update({"epochs": 1, "gpu_batches_per_step": 1, "seed": 7})
    if evaluation is not None:
        cfg["train"]["evaluation"] = evaluation
    data = []
    for s in range(4):
        clean, noisy = O.synthetic_batch(2, 32, 32, seed=10 + s)
        data.append((torch.from_numpy(clean.astype(np.float32)), torch.from_numpy(noisy.astype(np.float32))))
    held_out, _ = O.synthetic_batch(3, 32, 48, seed=99)
    model, history = bf.train_loop(cfg, str(tmp_path / name), dataset=data, evaluation_batches=None if evaluation is None else [held_out])
    ck = np.load(sorted((tmp_path / name).glob("ckpt-*.npz"))[-1]) if list((tmp_path / name).glob("ckpt-*.npz")) else None
    return model, history, ck


def test_train_loop_validation_does_not_disturb_training(tmp_path):
    plain, hist0, ck0 = _train_run(tmp_path, "plain", None)
    model, hist1, ck1 = _train_run(tmp_path, "eval", {"every": 2, "noise_std": [0, 20, 40]})
    assert not (tmp_path / "plain" / "evaluation.jsonl").exists() and plain.evaluation_history == []
    lines = (tmp_path / "eval" / "evaluation.jsonl").read_text().splitlines()
    records = [json.loads(l) for l in lines]
    assert [r["step"] for r in records] == [2, 4] and [r["epoch"] for r in records] == [0, 0]
    keys = {"noise_std", "images", "psnr_noisy", "psnr_denoised", "ssim_noisy", "ssim_denoised", "mae_noisy", "mae_denoised",
            "improved_psnr", "improved_ssim", "improved_mae"}
    for r in records:
        assert [l["noise_std"] for l in r["levels"]] == [0.0, 20.0, 40.0]
        assert all(set(l) == keys and l["images"] == 3 for l in r["levels"])
        assert r["levels"][0]["psnr_noisy"] is None and r["levels"][0]["mae_noisy"] == 0.0       # sigma 0: infinite PSNR -> null
        assert all(np.isfinite(l["psnr_denoised"]) for l in r["levels"])
    assert len(model.evaluation_history) == 2 and model.evaluation_history[0]["levels"][0]["psnr_noisy"] == float("inf")
    # the same noise at both evaluations (fixed seed), different weights
    assert records[0]["levels"][1]["psnr_noisy"] == records[1]["levels"][1]["psnr_noisy"]
    assert records[0]["levels"][1]["psnr_denoised"] != records[1]["levels"][1]["psnr_denoised"]
    # training itself: bitwise the run without the section
    assert len(hist0) == 4 and np.array_equal(np.array(hist0).view(np.uint64), np.array(hist1).view(np.uint64))
    assert torch.equal(plain.params, model.params) and torch.equal(plain.state, model.state)
    assert ck0 is not None and ck1 is not None and sorted(ck0.files) == sorted(ck1.files)
    for k in ck0.files:                                                          # weights, BN statistics, Adam slots, step
        assert np.array_equal(ck0[k], ck1[k]), k
