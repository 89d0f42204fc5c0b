"""GPU tests of the Neighbor2Neighbor pairs: bf_op_neighbor_pairs (csrc/neighbor.hip) against the NumPy restatement of its contract
(tests/neighbor_reference.py), NeighborPairs in front of the training step, and `train.self_supervised` through train_loop for the
three families of train functions -- the engine learns to denoise from ONE noisy image."""
import json
import pathlib

import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from oracle import bfcnn_oracle as O
import neighbor_reference as R
import pruning_models as PM
from guarded import dev as _dev, guard_bands

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guard_bands")]

# the smallest shapes that cross each path: one cell; one partial group per row; a full group plus a tail; exactly aligned groups
# (the 16-byte path); several workgroups per image with a tail (W2 = 65) and C = 4; W2 = 129 and C = 3; C = 2
SHAPES = [(1, 2, 2, 1), (2, 4, 6, 3), (1, 6, 10, 3), (2, 16, 8, 3), (3, 34, 130, 4), (1, 66, 258, 3), (2, 8, 12, 2)]
SEEDS = [0, 2 ** 40 + 12345, 2 ** 64 - 1]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def _batch(shape, dtype, seed=0):
    rng = np.random.default_rng(1000 + seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return rng.uniform(-40.0, 300.0, shape).astype(np.float32)


def _gpu_pairs(y, seed, f=None, weight=0.0):
    out = bf.neighbor_pairs(_dev(y), seed, None if f is None else _dev(f), weight)
    assert all(t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() for t in out)
    return tuple(t.cpu().numpy() for t in out)


# ---- the kernel -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_pairs_equal_the_reference_bit_for_bit(shape, dtype):
    y = _batch(shape, dtype)
    for seed in SEEDS:
        inp, tgt = _gpu_pairs(y, seed)
        r_inp, r_tgt = R.pairs(y, seed)
        assert inp.shape == (shape[0], shape[1] // 2, shape[2] // 2, shape[3])
        assert np.array_equal(inp.view(np.uint32), r_inp.view(np.uint32)), (shape, seed)
        assert np.array_equal(tgt.view(np.uint32), r_tgt.view(np.uint32)), (shape, seed)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
def test_a_base_pointer_off_alignment_takes_the_scalar_path_to_the_same_bits(dtype):
    shape = (2, 16, 8, 3)                                            # whole groups: only the base keeps it from the 16-byte path
    y = _batch(shape, np.uint8 if dtype == torch.uint8 else np.float32, seed=1)
    f = _batch(shape, np.float32, seed=2)
    n = y.size
    buf = torch.zeros(n + 1, dtype=dtype, device="cuda")
    buf[1:].copy_(torch.from_numpy(y).reshape(-1))
    shifted = buf[1:].view(shape)
    assert shifted.is_contiguous() and shifted.data_ptr() % 8 != 0
    fbuf = torch.zeros(n + 1, dtype=torch.float32, device="cuda")
    fbuf[1:].copy_(torch.from_numpy(f).reshape(-1))
    f_shifted = fbuf[1:].view(shape)
    aligned = bf.neighbor_pairs(_dev(y), 9, _dev(f), 0.25)
    for yy, ff in ((shifted, None), (shifted, f_shifted), (_dev(y), f_shifted)):
        inp, tgt = bf.neighbor_pairs(yy, 9, ff, 0.25 if ff is not None else 0.0)
        r_inp, r_tgt = R.pairs(y, 9)
        assert np.array_equal(inp.cpu().numpy(), r_inp)
        if ff is None:
            assert np.array_equal(tgt.cpu().numpy(), r_tgt)
        else:
            assert torch.equal(tgt, aligned[1]) and torch.equal(inp, aligned[0])      # both paths: the same fma of the same values


@pytest.mark.parametrize("weight", [0.25, 2.0 / 3.0], ids=["0.25", "2/3"])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_target_with_the_denoised_pair_is_within_one_ulp(shape, dtype, weight):
    """the difference f[p1] - f[p2] is rounded to fp32 (as the reference rounds it), the fma rounds once: one float32 ulp of the
    fp64 value; `input` is still EQUAL"""
    y, f = _batch(shape, dtype), _batch(shape, np.float32, seed=5)
    inp, tgt = _gpu_pairs(y, SEEDS[1], f, weight)
    r_inp, r_tgt = R.pairs(y, SEEDS[1], f, weight)
    assert np.array_equal(inp, r_inp)
    ulp = np.spacing(np.abs(r_tgt).astype(np.float32)).astype(np.float64)
    err = np.abs(tgt.astype(np.float64) - r_tgt)
    assert (err <= ulp).all(), float((err / ulp).max())
    assert (tgt != R.pairs(y, SEEDS[1])[1]).any() or shape == (1, 2, 2, 1)     # the blend is in


def test_sampling_a_float_tensor_gives_the_pairs_of_the_regulariser():
    """the entry with f = NULL on f itself is (g1(f), g2(f)) for the same seed: target - y[p2] = weight * (g1(f) - g2(f))"""
    shape = (2, 16, 24, 3)
    y, f = _batch(shape, np.uint8), _batch(shape, np.float32, seed=3)
    g1, g2 = _gpu_pairs(f, 77)
    r1, r2 = R.pairs(f, 77)
    assert np.array_equal(g1, r1) and np.array_equal(g2, r2)
    _, y2 = _gpu_pairs(y, 77)
    _, tgt = _gpu_pairs(y, 77, f, 0.5)
    d = (g1 - g2).astype(np.float32)
    assert np.array_equal(tgt, (y2.astype(np.float64) + 0.5 * d.astype(np.float64)).astype(np.float32))   # 0.5 d is exact: one rounding


def test_the_entry_refuses_what_the_contract_excludes():
    from blind_image_denoising_amd import _native as N
    y = torch.zeros((1, 4, 4, 3), dtype=torch.float32, device="cuda")
    a, b = torch.zeros((1, 2, 2, 3), device="cuda"), torch.zeros((1, 2, 2, 3), device="cuda")
    call = lambda *args: N.lib().bf_op_neighbor_pairs(*args, N.stream_ptr(y))
    assert call(N.ptr(y), 0, None, 0.0, N.ptr(a), N.ptr(b), 1, 4, 4, 3, 0) == N.BF_OK
    for args in [(None, 0, None, 0.0, N.ptr(a), N.ptr(b), 1, 4, 4, 3, 0), (N.ptr(y), 0, None, 0.0, None, N.ptr(b), 1, 4, 4, 3, 0),
                 (N.ptr(y), 0, None, 0.0, N.ptr(a), None, 1, 4, 4, 3, 0), (N.ptr(y), 0, None, 0.0, N.ptr(a), N.ptr(b), 0, 4, 4, 3, 0),
                 (N.ptr(y), 0, None, 0.0, N.ptr(a), N.ptr(b), 1, 3, 4, 3, 0), (N.ptr(y), 0, None, 0.0, N.ptr(a), N.ptr(b), 1, 4, 0, 3, 0),
                 (N.ptr(y), 0, None, 0.0, N.ptr(a), N.ptr(b), 1, 4, 4, 5, 0), (N.ptr(y), 0, None, 0.0, N.ptr(a), N.ptr(b), 1, 4, 4, 0, 0),
                 (N.ptr(y), 0, None, 1.0, N.ptr(a), N.ptr(b), 1, 4, 4, 3, 0), (N.ptr(y), 0, None, -0.5, N.ptr(a), N.ptr(b), 1, 4, 4, 3, 0),
                 (N.ptr(y), 0, None, float("nan"), N.ptr(a), N.ptr(b), 1, 4, 4, 3, 0),
                 (N.ptr(y), 0, None, 0.0, N.ptr(a), N.ptr(a), 1, 4, 4, 3, 0), (N.ptr(y), 0, None, 0.0, N.ptr(y), N.ptr(b), 1, 4, 4, 3, 0),
                 (N.ptr(y), 0, N.ptr(y), 0.0, N.ptr(a), N.ptr(y), 1, 4, 4, 3, 0)]:
        assert call(*args) == N.BF_EINVAL, args
    torch.cuda.synchronize()


def test_pairs_can_be_captured_into_a_graph():
    y = _dev(_batch((2, 16, 8, 3), np.uint8))
    f = _dev(_batch((2, 16, 8, 3), np.float32, seed=4))
    want = bf.neighbor_pairs(y, 3, f, 0.5)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = bf.neighbor_pairs(y, 3, f, 0.5)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- NeighborPairs ----------------------------------------------------------------------------------------------------------

class _Stub:
    """in place of the model: uint8 [B,H,W,C] -> float32, counted"""

    def __init__(self):
        self.calls = 0

    def __call__(self, u8):
        assert u8.dtype == torch.uint8 and u8.is_cuda
        self.calls += 1
        return u8.float() * 0.75 + torch.arange(u8.shape[2], device=u8.device, dtype=torch.float32).reshape(1, 1, -1, 1)


def _noisy_list():
    return [(None, _dev(_batch((2, 8, 12, 3), np.uint8, seed=s).astype(np.float32))) for s in range(3)]


def test_neighbor_pairs_dataset_without_regulariser_never_calls_the_model():
    stub, data = _Stub(), _noisy_list()
    ds = bf.NeighborPairs(data, model=stub, gamma=0.0, seed=5)
    rng = np.random.default_rng(5)
    for _ in range(2):                                               # re-iterable; the draws go on
        got = list(ds)
        assert len(got) == 3
        for (tgt, inp), (_, y) in zip(got, data):
            r_inp, r_tgt = R.pairs(y.cpu().numpy(), int(rng.integers(0, 2 ** 63 - 1)))
            assert np.array_equal(inp.cpu().numpy(), r_inp) and np.array_equal(tgt.cpu().numpy(), r_tgt)
    assert stub.calls == 0
    # ramp at 0 % done: the weight is 0 and the model is not called either
    ramped = bf.NeighborPairs(data, model=stub, gamma=2.0, ramp=True, seed=5)
    assert ramped.percentage_done == 0.0 and len(list(ramped)) == 3 and stub.calls == 0
    ramped.percentage_done = 0.5
    assert len(list(ramped)) == 3 and stub.calls == 3
    # bare noisy batches, uint8
    bare = list(bf.NeighborPairs([y.to(torch.uint8) for _, y in data], seed=5))
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(bare, list(bf.NeighborPairs(data, seed=5))))


def test_neighbor_pairs_dataset_with_regulariser_calls_the_model_once_per_batch():
    stub, data, gamma = _Stub(), _noisy_list(), 2.0
    got = list(bf.NeighborPairs(data, model=stub, gamma=gamma, ramp=False, seed=11))
    assert stub.calls == 3
    rng = np.random.default_rng(11)
    for (tgt, inp), (_, y) in zip(got, data):
        want = bf.neighbor_pairs(y, int(rng.integers(0, 2 ** 63 - 1)), denoised=_Stub()(y.to(torch.uint8)), weight=gamma / (1.0 + gamma))
        assert torch.equal(inp, want[0]) and torch.equal(tgt, want[1])
        assert not torch.equal(tgt, bf.neighbor_pairs(y, 0)[1])


def test_neighbor_pairs_dataset_runs_the_model_through_the_float_inference_module():
    """with a hydra: DenoiserModule(model, cast_to_uint8=False) on the rounded, clamped batch -- the current weights"""
    cfg = O.canonical_config(no_layers=2)
    model = bf.model_builder(cfg["model"], device="cuda", seed=3).hydra
    y = _dev(_batch((2, 16, 16, 3), np.float32))                                 # values outside 0..255 and off the integers
    (tgt, inp), = list(bf.NeighborPairs([y], model=model, gamma=1.0, ramp=False, seed=2))
    f = bf.DenoiserModule(model, cast_to_uint8=False)(y.round().clamp(0, 255).to(torch.uint8))
    want = bf.neighbor_pairs(y, int(np.random.default_rng(2).integers(0, 2 ** 63 - 1)), denoised=f, weight=0.5)
    assert torch.equal(inp, want[0]) and torch.equal(tgt, want[1])


# ---- through train_loop -----------------------------------------------------------------------------------------------------------

def _lena():
    from PIL import Image
    return np.asarray(Image.open(pathlib.Path(__file__).parent / "golden" / "lena.jpg").convert("RGB"))


def _noisy_u8(clean, seed, sigma=20.0):
    return np.clip(np.round(clean + np.random.default_rng(seed).normal(0, sigma, clean.shape)), 0, 255).astype(np.uint8)


def _write_noisy_training_image(tmp_path):
    """ONE noisy PNG of lena[0:384]: the only pixels the loop is given"""
    from PIL import Image
    (tmp_path / "img").mkdir()
    Image.fromarray(_noisy_u8(_lena()[0:384], 1)).save(tmp_path / "img" / "noisy.png")
    return tmp_path / "img"


def _config(directory, seed, gamma, epochs, steps_per_epoch, validation=None):
    cfg = O.canonical_config(no_layers=6)
    cfg["train"].update({"epochs": epochs, "gpu_batches_per_step": 1, "seed": seed,
                         "self_supervised": {"type": "neighbor2neighbor", "gamma": gamma, "ramp": True}})
    if validation is not None:
        cfg["train"]["self_supervised"]["validation"] = validation
    cfg["train"]["optimizer"]["schedule"]["config"]["learning_rate"] = 2e-3
    cfg["loss"] = {"hinge": 0.0, "cutoff": 255.0, "mae_multiplier": 1.0, "ssim_multiplier": 0.0, "regularization": 0.01}
    cfg["dataset"] = {"batch_size": 16, "color_mode": "rgb", "no_crops_per_image": steps_per_epoch * 16, "value_range": [0, 255],
                      "clip_value": True, "round_values": True, "random_up_down": True, "random_left_right": True,
                      "input_shape": [64, 64, 3], "inputs": [{"directory": str(directory)}]}          # no noise option: it yields (y, y)
    return cfg


# half of the smallest of the gains measured on the MI355X for train seeds 7, 8, 9: +4.51, +4.01, +7.43 dB (see the docstring below)
GAIN_MARGIN_DB = 2.0


def test_the_engine_learns_from_noisy_images_alone(tmp_path):
    """end to end through the public API with no clean pixel of the training rows anywhere: one noisy PNG (lena[0:384] + sigma 20,
    rounded) -> the directory pipeline without a noise option -> train_loop with train.self_supervised (gamma 0: 1 024 steps of 16
    pairs of 32 x 32 from 64 x 64 crops; canonical resnet 1x6, L1, Adam 2e-3) -> load_model, judged like the reference's
    test_pretrained.py on the held-out rows lena[384:512] + sigma 20: PSNR higher and MAE lower than the noisy frame's
    (tools/exp/learn_from_noisy.py is the same run as a script).  Measured for train seeds 7, 8, 9: 22.26 -> 26.77, 26.27, 29.69 dB
    (MAE 15.75 -> 9.48, 9.63, 6.59); the margin asserted on top of the acceptance rule is half of the smallest gain, 2.0 dB.  The
    supervised test_the_engine_learns_to_denoise, which sees the clean crops for 1 920 steps, measures 22.3 -> 30.5 dB."""
    directory = _write_noisy_training_image(tmp_path)
    held = _lena()[384:512][None]
    model, hist = bf.train_loop(_config(directory, 7, 0.0, 16, 64), str(tmp_path / "run"))
    assert len(hist) == 1024 and np.isfinite(hist).all()
    noisy = _noisy_u8(held, 0)
    den = bf.load_model(str(tmp_path / "run" / "final"))(noisy)
    psnr = lambda a, b: 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    mae = lambda a, b: np.abs(a.astype(np.float64) - b.astype(np.float64)).mean()
    print(f"PSNR {psnr(held, noisy):.3f} -> {psnr(held, den):.3f} dB, MAE {mae(held, noisy):.3f} -> {mae(held, den):.3f}")
    assert psnr(held, den) > psnr(held, noisy) + GAIN_MARGIN_DB, (psnr(held, noisy), psnr(held, den))
    assert mae(held, den) < mae(held, noisy)
    assert model.risk_history == [] and not (tmp_path / "run" / "risk.jsonl").exists()


def test_the_regulariser_and_risk_validation_run_through_the_loop(tmp_path):
    """gamma 2, ramped over 10 epochs of 30 steps: from the second epoch on every step runs the full-resolution inference forward
    for the regulariser; SURE on two held-out NOISY batches after every epoch goes to risk.jsonl and model.risk_history"""
    directory = _write_noisy_training_image(tmp_path)
    held = _noisy_u8(_lena()[384:512], 0)
    batches = [np.stack([held[:, 0:128], held[:, 128:256]]), np.stack([held[:, 256:384], held[:, 384:512]])]
    cfg = _config(directory, 7, 2.0, 10, 30, {"every": 0, "sigma": None, "method": "mad", "probes": 1})
    model, hist = bf.train_loop(cfg, str(tmp_path / "run"), validation_noisy_batches=batches)
    assert len(hist) == 300 and np.isfinite(hist).all() and np.mean(hist[-20:]) < hist[0]
    records = [json.loads(line) for line in (tmp_path / "run" / "risk.jsonl").read_text().splitlines()]
    assert len(records) == 10 and len(model.risk_history) == 10
    assert [r["step"] for r in records] == [30 * (e + 1) for e in range(10)] and [r["epoch"] for r in records] == list(range(10))
    assert records[-1]["risk"]["images"] == 4 and len(records[-1]["risk"]["batches"]) == 2
    first, last = records[0]["risk"]["aggregate"]["psnr"], records[-1]["risk"]["aggregate"]["psnr"]
    print(f"estimated PSNR {first:.3f} -> {last:.3f} dB")
    assert np.isfinite([first, last]).all() and last > first
    assert bf.format_risk_report(model.risk_history[-1]["risk"]).count("\n") == 4


def test_validation_every_n_steps_and_unknown_type(tmp_path):
    directory = _write_noisy_training_image(tmp_path)
    held = _noisy_u8(_lena()[384:512], 0)
    cfg = _config(directory, 7, 0.0, 1, 20, {"every": 8, "sigma": 20.0})
    model, hist = bf.train_loop(cfg, str(tmp_path / "run"), validation_noisy_batches=[held[None, :, 0:128]])
    assert len(hist) == 20 and [r["step"] for r in model.risk_history] == [8, 16]
    assert model.risk_history[0]["risk"]["method"] == "given"
    cfg["train"]["self_supervised"]["type"] = "noise2void"
    with pytest.raises(ValueError, match="self_supervised"):
        bf.train_loop(cfg, str(tmp_path / "other"))


def test_the_training_tool_runs_a_directory_and_prints_the_risk_table(tmp_path, capsys):
    """tools/train_noisy.py: config + directory of noisy images + output directory -> the loop with the section, risk.jsonl as tables"""
    import sys
    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1] / "tools"))
    try:
        import train_noisy
    finally:
        sys.path.pop(0)
    directory = _write_noisy_training_image(tmp_path)
    cfg = _config("elsewhere", 7, 0.0, 1, 4)
    del cfg["train"]["self_supervised"]
    cfg["dataset"]["additional_noise"] = [20]                         # dropped by the tool: the images are noisy already
    (tmp_path / "pipeline.json").write_text(json.dumps(cfg))
    model, hist = train_noisy.main([str(tmp_path / "pipeline.json"), str(directory), str(tmp_path / "run"), "--gamma", "1", "--no-ramp",
                                    "--every", "2", "--sigma", "20"])
    out = capsys.readouterr().out
    assert len(hist) == 4 and [r["step"] for r in model.risk_history] == [2, 4]
    assert out.count("estimated psnr") == 2 and "step 2 (epoch 0)" in out and "step 4 (epoch 0)" in out
    assert (tmp_path / "run" / "final").exists()


def _family_run(tmp_path, model_section, train_optimizer):
    """50 steps of `train.self_supervised` on five fixed batches of noisy 64 x 64 crops, handed over as (junk, noisy) pairs"""
    noisy = _noisy_u8(_lena()[0:384], 1)
    rng = np.random.default_rng(4)
    data = []
    for _ in range(5):
        crops = [noisy[r:r + 64, c:c + 64] for r, c in zip(rng.integers(0, 320, 4), rng.integers(0, 448, 4))]
        data.append((None, _dev(np.stack(crops).astype(np.float32))))
    cfg = {"model": model_section,
           "loss": {"hinge": 0.0, "cutoff": 255.0, "mae_multiplier": 1.0, "ssim_multiplier": 0.0, "regularization": 0.01},
           "train": {"epochs": 10, "gpu_batches_per_step": 1, "seed": 7, "optimizer": train_optimizer,
                     "self_supervised": {"type": "neighbor2neighbor", "gamma": 1.0, "ramp": True}}}
    model, hist = bf.train_loop(cfg, str(tmp_path / "run"), dataset=data)
    print(f"loss {hist[0]:.3f} -> {np.mean(hist[-10:]):.3f}")
    assert len(hist) == 50 and np.isfinite(hist).all() and np.mean(hist[-10:]) < hist[0]
    return model


_ADAM = {"type": "Adam", "gradient_clipping_by_norm": 1.0,
         "schedule": {"type": "exponential_decay", "config": {"decay_rate": 0.9, "decay_steps": 10000, "learning_rate": 1e-3}}}


def test_the_pairs_feed_the_generic_resnet_family(tmp_path):
    model = _family_run(tmp_path, PM.resnet_generic_config(), _ADAM)
    assert type(model).__name__ == "GenericResnetHydra"


def test_the_pairs_feed_the_unet_laplacian_family(tmp_path):
    """depth 2: 32 x 32 pairs are the smallest the two-level pyramid trains on; output 0 of the hydra feeds the regulariser"""
    model = _family_run(tmp_path, PM.unet_laplacian_config(), _ADAM)
    assert type(model).__name__ == "UnetLaplacianHydra"
