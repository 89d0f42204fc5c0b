"""GPU tests of the blind degradations: bf_op_degrade_jpeg / _blur / _pointwise (csrc/degrade.hip) bit for bit against the NumPy
restatement of their contracts (tests/degrade_reference.py), the stages inside PrepareData, and a training run on a directory of
images with all four degradations on."""
import pathlib

import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from oracle import bfcnn_oracle as O
import degrade_reference as R
from guarded import dev as _dev, guard_bands

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guard_bands")]

# one pixel; one block; one block and a bit (padding on both axes); one 4:2:0 unit; a unit and a bit; grey, several tiles of the
# blur across; three images, tiles and a tail on both axes
JPEG_SHAPES = [(1, 1, 1, 1), (1, 8, 8, 3), (2, 9, 17, 3), (1, 16, 16, 3), (2, 17, 33, 3), (1, 40, 72, 1), (3, 50, 130, 3)]
BLUR_SHAPES = JPEG_SHAPES + [(1, 3, 5, 3)]                         # smaller than the radius
SEEDS = [0, 2 ** 40 + 12345, 2 ** 64 - 1]


def _ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


def _batch(shape, dtype, seed=0):
    """uint8 noise, or integer-valued float32 samples that leave 0..255 on both sides"""
    rng = np.random.default_rng(2000 + seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return rng.integers(-40, 300, shape).astype(np.float32)


def _smooth(shape, seed=0):
    """an image with structure at every quality: a ramp plus noise"""
    B, H, W, C = shape
    rng = np.random.default_rng(3000 + seed)
    ramp = np.add.outer(np.arange(H) * 3.0, np.arange(W) * 2.0)[None, :, :, None] + 40.0 * np.arange(C) + 30.0 * np.arange(B)[:, None, None, None]
    return np.clip(np.rint(ramp + rng.normal(0.0, 12.0, shape)), 0, 255).astype(np.uint8)


def _gpu(fn, x, *args, **kwargs):
    out = fn(_dev(x), *args, **kwargs)
    outs = out if isinstance(out, tuple) else (out,)
    assert all(t.is_cuda and t.is_contiguous() for t in outs) and outs[0].dtype == torch.float32 and outs[0].shape == x.shape
    return tuple(t.cpu().numpy() for t in outs) if isinstance(out, tuple) else out.cpu().numpy()


def _same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the kernels ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("subsampling", ["444", "420"])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("shape", JPEG_SHAPES, ids=_ids(JPEG_SHAPES))
def test_jpeg_equals_the_reference_bit_for_bit(shape, dtype, subsampling):
    quality = [[1, 50, 100][b % 3] for b in range(shape[0])]
    for x in (_batch(shape, dtype), _smooth(shape).astype(dtype)):
        assert _same_bits(_gpu(bf.degrade_jpeg, x, quality, subsampling), R.jpeg(x, quality, int(subsampling))), (shape, quality)
    x = _smooth(shape, seed=1).astype(dtype)
    for quality in (25, 90):                                         # a scalar holds for every image
        assert _same_bits(_gpu(bf.degrade_jpeg, x, quality, subsampling), R.jpeg(x, quality, int(subsampling))), (shape, quality)


@pytest.mark.parametrize("subsampling", ["444", "420"])
def test_jpeg_leaves_the_images_of_quality_0_unencoded(subsampling):
    x = _batch((3, 17, 33, 3), np.float32, seed=2)
    out = _gpu(bf.degrade_jpeg, x, [0, 30, 0], subsampling)
    assert _same_bits(out, R.jpeg(x, [0, 30, 0], int(subsampling)))
    assert np.array_equal(out[0], np.clip(x[0], 0, 255)) and not np.array_equal(out[1], np.clip(x[1], 0, 255))


def test_jpeg_refuses_four_channels():
    for C in (2, 4):
        with pytest.raises(ValueError):
            bf.degrade_jpeg(torch.zeros((1, 8, 8, C), dtype=torch.uint8, device="cuda"), 50)
    from blind_image_denoising_amd import _native as N                # and the C entry itself
    x, q = torch.zeros((1, 8, 8, 4), dtype=torch.uint8, device="cuda"), torch.full((1,), 50, dtype=torch.int32, device="cuda")
    out = torch.empty(x.shape, dtype=torch.float32, device="cuda")
    assert N.lib().bf_op_degrade_jpeg(N.ptr(x), 1, N.ptr(out), 1, 8, 8, 4, N.ptr(q), 420, None, 0, N.stream_ptr(x)) == N.BF_EINVAL


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("shape", BLUR_SHAPES, ids=_ids(BLUR_SHAPES))
def test_blur_equals_the_reference_bit_for_bit(shape, dtype):
    x = _batch(shape, dtype, seed=3)
    for first in range(4):                                           # every image meets every sigma
        sigma = [[0, 0.5, 1.3, 4][(first + b) % 4] for b in range(shape[0])]
        out = _gpu(bf.degrade_blur, x, sigma)
        assert _same_bits(out, R.blur(x, sigma)), (shape, sigma)
        for b, s in enumerate(sigma):
            if s == 0:
                assert np.array_equal(out[b], np.clip(x[b], 0, 255))
    flat = np.full(shape, 255, dtype)                                # the largest sums: 255 * 65536, 255 * 256 * 65536
    assert np.array_equal(_gpu(bf.degrade_blur, flat, 4.0), flat.astype(np.float32))


def test_blur_on_two_and_four_channels():
    for shape in ((2, 21, 70, 2), (1, 33, 67, 4)):
        x = _batch(shape, np.uint8, seed=4)
        assert _same_bits(_gpu(bf.degrade_blur, x, 2.0), R.blur(x, 2.0))


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("shape", BLUR_SHAPES, ids=_ids(BLUR_SHAPES))
def test_pointwise_equals_the_reference_bit_for_bit(shape, dtype):
    x = _batch(shape, dtype, seed=5)
    B = shape[0]
    for k, seed in enumerate(SEEDS):
        step = [[1, 2, 8, 255][(k + b) % 4] for b in range(B)]
        rate = [[0.0, 0.3, 0.9][(k + b) % 3] for b in range(B)]
        out, mask = _gpu(bf.degrade_pointwise, x, step, rate, seed, return_mask=True)
        r_out, r_mask = R.pointwise(x, step, rate, seed)
        assert mask.dtype == np.uint8 and mask.shape == shape[:3] and np.array_equal(mask, r_mask), (shape, seed)
        assert _same_bits(out, r_out), (shape, step, rate, seed)
        assert _same_bits(_gpu(bf.degrade_pointwise, x, step, rate, seed), r_out)            # without the mask output
    for step in (1, 2, 8, 255):
        assert _same_bits(_gpu(bf.degrade_pointwise, x, step), R.pointwise(x, step)[0])


def test_drop_does_not_depend_on_the_batch_size():
    x = _batch((3, 50, 130, 3), np.uint8, seed=6)
    _, mask = _gpu(bf.degrade_pointwise, x, 1, 0.3, 77, return_mask=True)
    _, alone = _gpu(bf.degrade_pointwise, x[:1], 1, 0.3, 77, return_mask=True)
    assert np.array_equal(alone[0], mask[0]) and not np.array_equal(mask[0], mask[1])
    n = mask.size
    assert abs(int(mask.sum()) - 0.3 * n) <= 5 * np.sqrt(n * 0.3 * 0.7)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
def test_a_base_pointer_off_alignment_gives_the_same_bits(dtype):
    shape = (2, 17, 33, 3)
    x = _batch(shape, np.uint8 if dtype == torch.uint8 else np.float32, seed=7)
    buf = torch.zeros(x.size + 1, dtype=dtype, device="cuda")
    buf[1:].copy_(torch.from_numpy(x).reshape(-1))
    shifted = buf[1:].view(shape)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 != 0
    for sub in ("444", "420"):
        assert _same_bits(bf.degrade_jpeg(shifted, [20, 80], sub).cpu().numpy(), R.jpeg(x, [20, 80], int(sub)))
    assert _same_bits(bf.degrade_blur(shifted, [1.3, 4.0]).cpu().numpy(), R.blur(x, [1.3, 4.0]))
    out, mask = bf.degrade_pointwise(shifted, [8, 3], 0.3, 5, return_mask=True)
    r_out, r_mask = R.pointwise(x, [8, 3], 0.3, 5)
    assert _same_bits(out.cpu().numpy(), r_out) and np.array_equal(mask.cpu().numpy(), r_mask)


# ---- the stages inside PrepareData ------------------------------------------------------------------------------------------

NOISE = {"random_left_right": True, "random_up_down": True, "additional_noise": [5, 25], "multiplicative_noise": [0.05, 0.1]}


def _section(p):
    return {"blur": {"sigma": [0.5, 3.0], "probability": p}, "quantization": {"step": [2, 4, 8], "probability": p},
            "jpeg": {"quality": [25, 75], "subsampling": "420", "probability": p}, "drop": {"rate": [0.05, 0.3], "probability": p}}


def test_probability_0_is_prepare_data_without_the_section():
    x = _dev(np.random.default_rng(3).uniform(0, 255, (3, 19, 23, 3)).astype(np.float32))
    plain, quiet = bf.PrepareData(NOISE, seed=9), bf.PrepareData(dict(NOISE, degradations=_section(0.0)), seed=9)
    for _ in range(6):
        (c0, n0), (c1, n1) = plain(x), quiet(x)
        assert torch.equal(c0, c1) and torch.equal(n0.view(torch.int32), n1.view(torch.int32))


def test_probability_1_is_the_composition_of_the_standalone_functions():
    x = _dev(np.random.default_rng(4).uniform(0, 255, (3, 19, 23, 3)).astype(np.float32))
    prep, twin = bf.PrepareData(dict(NOISE, degradations=_section(1.0)), seed=10), bf.PrepareData(dict(NOISE, degradations=_section(1.0)), seed=10)
    plain = bf.PrepareData(NOISE, seed=10)
    seen_noise = 0
    for _ in range(6):
        clean, noisy = prep(x)
        d, p = twin.draw(), twin.degradations.draw(3)                 # the parameters `prep` drew
        assert (p["sigma"] > 0).all() and (p["step"] > 1).all() and (p["quality"] > 0).all() and (p["rate"] > 0).all()
        undegraded_clean, _ = plain(x)
        assert torch.equal(clean, undegraded_clean)                   # the clean output is never degraded
        y = bf.degrade_blur(clean, p["sigma"])
        if d["mult_std"] > 0 or d["add_std"] > 0:
            seen_noise += 1
            _, y = bf.noise_augment(y, False, False, d["mult_std"], d["add_std"], d["seed"])
        y = bf.degrade_pointwise(y, p["step"])
        y = bf.degrade_jpeg(y, p["quality"], "420")
        y = bf.degrade_pointwise(y, 1, p["rate"], d["seed"])
        assert torch.equal(noisy.view(torch.int32), y.view(torch.int32))
        # and the NumPy restatement of the stages behind the noise
        ref = R.pointwise(R.jpeg(R.pointwise(_noisy_before_quantisation(clean, p, d), p["step"])[0], p["quality"], 420), 1, p["rate"], d["seed"])[0]
        assert np.array_equal(noisy.cpu().numpy(), ref)
    assert seen_noise > 0


def _noisy_before_quantisation(clean, p, d):
    y = bf.degrade_blur(clean, p["sigma"])
    if d["mult_std"] > 0 or d["add_std"] > 0:
        _, y = bf.noise_augment(y, False, False, d["mult_std"], d["add_std"], d["seed"])
    return y.cpu().numpy()


def test_single_stages_launch_alone():
    """every stage alone, and quantisation with the drop in one launch: the composition again"""
    x = _dev(_smooth((2, 19, 23, 3), seed=8).astype(np.float32))
    for keep in (("blur",), ("quantization",), ("jpeg",), ("drop",), ("quantization", "drop")):
        section = {k: v for k, v in _section(1.0).items() if k in keep}
        prep, twin = bf.PrepareData({"degradations": section}, seed=11), bf.PrepareData({"degradations": section}, seed=11)
        clean, noisy = prep(x)
        d, p = twin.draw(), twin.degradations.draw(2)
        assert torch.equal(clean, x)
        ref = R.blur(x.cpu().numpy(), p["sigma"])
        ref = R.pointwise(R.jpeg(R.pointwise(ref, p["step"])[0], p["quality"], 420), 1, p["rate"], d["seed"])[0]
        assert np.array_equal(noisy.cpu().numpy(), ref), keep
        assert not torch.equal(noisy, clean)


def test_train_loop_runs_with_all_four_degradations(tmp_path):
    from PIL import Image
    lena = Image.open(pathlib.Path(__file__).parent / "golden" / "lena.jpg")
    imgs = tmp_path / "images"
    imgs.mkdir()
    for k in range(4):
        lena.crop((60 * k, 50 * k, 60 * k + 160, 50 * k + 128)).save(imgs / f"im{k}.png")
    cfg = O.canonical_config(no_layers=2)
    cfg["train"].update({"epochs": 2, "gpu_batches_per_step": 1})
    cfg["dataset"] = {"batch_size": 4, "color_mode": "rgb", "no_crops_per_image": 2, "value_range": [0, 255], "clip_value": True,
                      "round_values": True, "random_up_down": True, "random_left_right": True, "input_shape": [32, 32, 3],
                      "multiplicative_noise": [0.05, 0.1], "additional_noise": [5, 10, 20], "inputs": [{"directory": str(imgs)}],
                      "degradations": _section(0.75)}
    model, hist = bf.train_loop(cfg, str(tmp_path / "run"))
    assert len(hist) == 2 * (4 * 2 // 4) and np.isfinite(hist).all()


def test_the_tool_writes_degraded_copies_of_a_folder(tmp_path):
    import importlib.util
    from PIL import Image
    spec = importlib.util.spec_from_file_location("degrade_tool", pathlib.Path(__file__).parent.parent / "tools" / "degrade.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    lena = Image.open(pathlib.Path(__file__).parent / "golden" / "lena.jpg")
    src = tmp_path / "in"
    src.mkdir()
    lena.crop((0, 0, 75, 51)).save(src / "a.png")
    lena.crop((100, 100, 180, 164)).save(src / "b.png")
    written = tool.main([str(src), str(tmp_path / "out"), "--jpeg", "20", "--blur", "1.5", "--step", "8", "--drop", "0.1", "--seed", "3"])
    assert [pathlib.Path(w).name for w in written] == ["a.png", "b.png"]
    a = np.asarray(Image.open(src / "a.png").convert("RGB"))[None]
    ref = R.pointwise(R.jpeg(R.pointwise(R.blur(a, 1.5), 8)[0], 20, 420), 1, 0.1, 3)[0]
    assert np.array_equal(np.asarray(Image.open(written[0])), ref[0].astype(np.uint8))
    with pytest.raises(SystemExit):
        tool.main([str(src), str(tmp_path / "out")])                  # nothing to do
