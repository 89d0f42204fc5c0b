"""CPU tests of blind_image_denoising_amd.metrics: argument refusals of image_metrics / evaluate and of the C entry points (the
host-side checks run before anything is launched), and the parsing of the `train.evaluation` section."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import _native as N
from blind_image_denoising_amd import metrics as M


def _u8(*shape):
    return np.zeros(shape, np.uint8)


def test_public_names():
    for name in ("image_metrics", "image_metric_sums", "psnr", "ssim", "mae", "evaluate", "ImageMetrics"):
        assert hasattr(bf, name), name
    assert bf.ImageMetrics._fields == ("psnr", "ssim", "mae", "mse")
    assert {"bf_image_metrics", "bf_image_metrics_scratch_bytes"} <= set(N.SIGNATURES)


@pytest.mark.parametrize("a,b,kw", [
    (_u8(1, 16, 16, 3), np.zeros((1, 16, 16, 3), np.float32), {}),              # mixed dtypes
    (_u8(1, 16, 16, 3), _u8(1, 16, 17, 3), {}),                                 # shape mismatch
    (_u8(16, 16, 3), _u8(16, 16, 3), {}),                                       # rank 3
    (_u8(1, 1, 16, 16, 3), _u8(1, 1, 16, 16, 3), {}),                           # rank 5
    (_u8(1, 10, 16, 3), _u8(1, 10, 16, 3), {}),                                 # height below the default 11 x 11 window
    (_u8(1, 16, 6, 3), _u8(1, 16, 6, 3), {"filter_size": 7}),                   # width below the window
    (_u8(1, 16, 16, 3), _u8(1, 16, 16, 3), {"filter_size": 8}),                 # even window
    (_u8(1, 16, 16, 3), _u8(1, 16, 16, 3), {"filter_size": 13}),                # window out of range
    (_u8(1, 16, 16, 3), _u8(1, 16, 16, 3), {"filter_size": 1}),
    (_u8(1, 16, 16, 5), _u8(1, 16, 16, 5), {}),                                 # channels outside 1..4
    (np.zeros((1, 16, 16, 3), np.float64), np.zeros((1, 16, 16, 3), np.float64), {}),
    (_u8(1, 16, 16, 3), torch.zeros((1, 16, 16, 3), dtype=torch.uint8), {}),    # an array and a tensor
], ids=["dtype", "shape", "rank3", "rank5", "small_h", "small_w", "even", "large", "tiny", "channels", "f64", "mixed_kind"])
def test_image_metrics_refuses(a, b, kw):
    with pytest.raises(ValueError):
        bf.image_metrics(a, b, **kw)


def test_cpu_tensors_have_no_execution_path():
    t = torch.zeros((1, 16, 16, 3), dtype=torch.uint8)
    for fn in (bf.image_metrics, bf.psnr, bf.ssim, bf.mae):
        with pytest.raises(RuntimeError, match="no CPU execution path"):
            fn(t, t)


def test_evaluate_refuses():
    ident = lambda x: x
    with pytest.raises(ValueError):
        bf.evaluate(None, [_u8(1, 16, 16, 3)])                                  # not callable
    with pytest.raises(ValueError):
        bf.evaluate(ident, [np.zeros((1, 16, 16, 3), np.float32)])              # batches must be uint8
    with pytest.raises(ValueError):
        bf.evaluate(ident, [_u8(16, 16, 3)])                                    # rank
    with pytest.raises(ValueError):
        bf.evaluate(ident, [])                                                  # nothing to evaluate on
    with pytest.raises(ValueError):
        bf.evaluate(ident, [_u8(1, 16, 16, 3)], noise_std=())
    with pytest.raises(ValueError):
        bf.evaluate(ident, [_u8(1, 16, 16, 3)], noise_std=(10, -1))
    with pytest.raises(ValueError):
        bf.evaluate(ident, [_u8(1, 16, 16, 3)], filter_size=4)


def test_c_entry_points_refuse_on_the_host():
    """BF_EINVAL comes from host-side checks: no device is needed to see it"""
    L = N.lib()
    assert L.bf_image_metrics_scratch_bytes(1, 11, 11, 3, 11) == 1 * 1 * 3 * 8                   # one tile
    # 375 x 1242 x 3, 11 x 11: ceil(1232 * 3 / 64) x ceil(365 / 16) tiles, three doubles each
    assert L.bf_image_metrics_scratch_bytes(2, 375, 1242, 3, 11) == 2 * 58 * 23 * 3 * 8
    for args in [(0, 16, 16, 3, 11), (1, 10, 16, 3, 11), (1, 16, 10, 3, 11), (1, 16, 16, 0, 11), (1, 16, 16, 5, 11),
                 (1, 16, 16, 3, 8), (1, 16, 16, 3, 13), (1, 16, 16, 3, 1)]:
        assert L.bf_image_metrics_scratch_bytes(*args) == N.BF_EINVAL, args
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    ok = dict(a=p, b=p, dtype=N.BF_DTYPE_U8, B=1, H=16, W=16, Cn=3, F=11, out=p, scratch=p, nbytes=24)
    for bad in [dict(a=None), dict(b=None), dict(out=None), dict(scratch=None), dict(dtype=2), dict(H=10), dict(W=10), dict(Cn=5),
                dict(F=8), dict(F=13), dict(nbytes=16)]:
        k = dict(ok, **bad)
        rc = L.bf_image_metrics(k["a"], k["b"], k["dtype"], k["B"], k["H"], k["W"], k["Cn"], 255.0, k["F"], 1.5, 0.01, 0.03, k["out"],
                                k["scratch"], k["nbytes"], None)
        assert rc == N.BF_EINVAL, bad


def test_evaluation_section_parsing_and_defaults():
    assert M.parse_evaluation_config({}) is None
    assert M.parse_evaluation_config({"epochs": 1, "optimizer": {}}) is None
    c = M.parse_evaluation_config({"evaluation": {}})
    assert c.every == 0 and c.noise_std == (0.0, 20.0, 40.0, 60.0, 80.0) and c.inputs == [] and c.no_images == 16
    c = M.parse_evaluation_config({"evaluation": {"every": 500, "noise_std": [10, 30], "inputs": ["a", "b"], "no_images": 4}})
    assert c == M.EvaluationConfig(500, (10.0, 30.0), ["a", "b"], 4)
    assert M.parse_evaluation_config({"evaluation": {"every": -3, "inputs": "dir"}}) == \
        M.EvaluationConfig(0, (0.0, 20.0, 40.0, 60.0, 80.0), ["dir"], 16)
    for bad in ({"evaluation": {"evry": 2}}, {"evaluation": {"noise_std": []}}, {"evaluation": {"noise_std": [-1]}},
                {"evaluation": {"no_images": 0}}, {"evaluation": [1, 2]}):
        with pytest.raises(ValueError):
            M.parse_evaluation_config(bad)


def test_no_evaluation_section_yields_no_evaluator():
    assert M.build_evaluator({"epochs": 1}, model=None, model_dir=None) is None
    with pytest.raises(ValueError):                                              # a section, but no images from anywhere
        M.build_evaluator({"evaluation": {"every": 2}}, model=None, model_dir=None)


def test_evaluator_schedule():
    cfg = M.EvaluationConfig(every=2, noise_std=(0.0,), inputs=[], no_images=1)
    e = M.Evaluator.__new__(M.Evaluator)
    e.config = cfg
    assert [s for s in range(7) if e.due(s)] == [2, 4, 6]
    e.config = cfg._replace(every=0)
    assert not any(e.due(s) for s in range(7))


def test_infinite_psnr_is_null_in_strict_json():
    rec = {"step": 1, "levels": [{"psnr_noisy": float("inf"), "psnr_denoised": 31.5, "images": 2}]}
    text = json.dumps(M.json_safe(rec), allow_nan=False)
    assert json.loads(text) == {"step": 1, "levels": [{"psnr_noisy": None, "psnr_denoised": 31.5, "images": 2}]}
