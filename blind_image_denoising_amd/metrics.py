"""
Image-quality metrics on the device and the evaluation protocol built from them.

`image_metrics(a, b)` is ONE C-ABI call (bf_image_metrics, csrc/metrics.hip): per image the sum of squared differences, the sum
of absolute differences and the sum of the SSIM map of `tf.image.ssim` (TF 2.13, VALID windows) in one pass over both batches,
uint8 or float32, no float copy of the images.  PSNR (`tf.image.psnr`: infinite for identical images), SSIM, MAE and MSE per
image are formed from those sums in float64 and stay on the device; nothing synchronises.

`evaluate(module, clean_batches)` is the acceptance check the reference holds for trained weights
(tests/bfcnn/test_pretrained.py:41-78) as a report: corrupt with truncated-normal noise of a given standard deviation, round,
clip, cast to uint8, denoise, and measure noisy-vs-clean and denoised-vs-clean at every noise level.  `Evaluator` is the same
protocol on a fixed set of images and a fixed seed, called by `train_loop` between optimizer steps (`train.evaluation`).
"""
import json
import os
from collections import namedtuple
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import _args as A
from . import _native as N
from .custom_logger import logger
from .module_denoiser import DenoiserModule

ImageMetrics = namedtuple("ImageMetrics", ["psnr", "ssim", "mae", "mse"])

DEFAULT_NOISE_STD = (10, 15, 20, 25, 30)                 # tests/bfcnn/test_pretrained.py:30
DEFAULT_TRAIN_NOISE_STD = (0, 20, 40, 60, 80)            # bfcnn/train_loop.py:507-509
_DTYPES = {torch.uint8: N.BF_DTYPE_U8, torch.float32: N.BF_DTYPE_F32}
_FEATURE = "image_metrics"


def _checked_window(filter_size) -> int:
    if int(filter_size) < 3 or int(filter_size) > 11 or int(filter_size) % 2 == 0:
        raise ValueError(f"filter_size must be odd and in 3..11, got {filter_size}")
    return int(filter_size)


def _as_tensor_pair(a, b, filter_size: int):
    """argument checks shared by every entry point; returns (a, b, was_numpy) with NumPy inputs wrapped (not yet uploaded)"""
    if isinstance(a, np.ndarray) != isinstance(b, np.ndarray):
        raise ValueError("a and b must both be torch tensors or both be numpy arrays")
    filter_size = _checked_window(filter_size)
    (a, was_numpy), (b, _) = (A.host_or_device(t, what, tuple(_DTYPES), min_hw=filter_size) for t, what in ((a, "a"), (b, "b")))
    if a.dtype != b.dtype or a.shape != b.shape:
        raise ValueError(f"a and b differ in dtype or shape: {a.dtype} {tuple(a.shape)} and {b.dtype} {tuple(b.shape)}")
    return a, b, was_numpy


def image_metric_sums(a, b, max_val: float = 255.0, filter_size: int = 11, filter_sigma: float = 1.5, k1: float = 0.01,
                      k2: float = 0.03) -> torch.Tensor:
    """what bf_image_metrics writes: a float64 [B,4] device tensor of (sum (a-b)^2, sum |a-b|, sum of the SSIM map, number of
    SSIM terms) per image.  uint8 inputs: the first two are exact integers."""
    a, b, was_numpy = _as_tensor_pair(a, b, filter_size)
    if not (max_val > 0.0 and filter_sigma > 0.0 and k1 >= 0.0 and k2 >= 0.0):
        raise ValueError("max_val and filter_sigma must be positive, k1 and k2 non-negative")
    a, b = (A.to_device(t, was_numpy, None, what, _FEATURE).contiguous() for t, what in ((a, "a"), (b, "b")))
    if a.device != b.device:
        raise ValueError(f"a and b are on different devices: {a.device} and {b.device}")
    B, H, W, C = a.shape
    scratch, nbytes = N.scratch("bf_image_metrics", a.device, B, H, W, C, int(filter_size))
    out = torch.empty((B, 4), dtype=torch.float64, device=a.device)
    N.call("bf_image_metrics", N.ptr(a), N.ptr(b), _DTYPES[a.dtype], B, H, W, C, float(max_val), int(filter_size),
           float(filter_sigma), float(k1), float(k2), N.ptr(out), N.ptr(scratch), nbytes, N.stream_ptr(a))
    return out.cpu().numpy() if was_numpy else out


def image_metrics(a, b, max_val: float = 255.0, filter_size: int = 11, filter_sigma: float = 1.5, k1: float = 0.01,
                  k2: float = 0.03) -> ImageMetrics:
    """per-image (psnr, ssim, mae, mse) of two [B,H,W,C] batches, both uint8 or both float32: float64 tensors on the inputs'
    device (CUDA tensors: nothing synchronises) or NumPy arrays (NumPy inputs are uploaded).  psnr as tf.image.psnr (inf for
    identical images), ssim as tf.image.ssim with the given window."""
    was_numpy = isinstance(a, np.ndarray)
    sums = image_metric_sums(a, b, max_val, filter_size, filter_sigma, k1, k2)
    n = float(a.shape[1] * a.shape[2] * a.shape[3])
    if was_numpy:
        with np.errstate(divide="ignore"):
            mse = sums[:, 0] / n
            return ImageMetrics(20.0 * np.log10(float(max_val)) - 10.0 * np.log10(mse), sums[:, 2] / sums[:, 3], sums[:, 1] / n, mse)
    mse = sums[:, 0] / n
    return ImageMetrics(20.0 * float(np.log10(float(max_val))) - 10.0 * torch.log10(mse), sums[:, 2] / sums[:, 3], sums[:, 1] / n, mse)


def psnr(a, b, max_val: float = 255.0):
    """tf.image.psnr per image"""
    return image_metrics(a, b, max_val=max_val, filter_size=3).psnr


def ssim(a, b, max_val: float = 255.0, filter_size: int = 11, filter_sigma: float = 1.5, k1: float = 0.01, k2: float = 0.03):
    """tf.image.ssim per image"""
    return image_metrics(a, b, max_val, filter_size, filter_sigma, k1, k2).ssim


def mae(a, b):
    """mean absolute difference per image"""
    return image_metrics(a, b, filter_size=3).mae


# ---- the protocol of tests/bfcnn/test_pretrained.py ---------------------------------------------

def corrupt_u8(clean_u8: torch.Tensor, noise_std: float, seed: int) -> torch.Tensor:
    """test_pretrained.py:41-56 on the device: clean + truncated normal (bf_noise_augment, mult_std = 0), round, clip to 0..255,
    uint8.  noise_std <= 0: the clean batch itself."""
    if float(noise_std) <= 0.0:
        return clean_u8
    from .dataset import noise_augment
    _, noisy = noise_augment(clean_u8, mult_std=0.0, add_std=float(noise_std), seed=seed)
    return noisy.clamp_(0.0, 255.0).to(torch.uint8)


def _level_seed(seed: int, level: int, batch: int) -> int:
    return ((int(seed) * 1000003 + level) * 1000003 + batch) & 0x7FFFFFFFFFFFFFFF


def _check_noise_std(noise_std) -> List[float]:
    levels = [float(s) for s in noise_std]
    if not levels or any(s < 0.0 for s in levels):
        raise ValueError(f"noise_std must be a non-empty sequence of non-negative standard deviations, got {list(noise_std)}")
    return levels


def evaluate(module, clean_batches: Iterable, noise_std: Sequence[float] = DEFAULT_NOISE_STD, seed: int = 0,
             filter_size: int = 11) -> List[Dict]:
    """The reference's acceptance protocol as a report.  `module`: callable uint8 [B,H,W,C] -> uint8 of the same shape
    (DenoiserModule, GraphedDenoiserModule); `clean_batches`: an iterable of uint8 batches, host or device, of any shapes.  Per
    noise level one dict: noise_std, images, the means psnr_noisy / psnr_denoised, ssim_* and mae_*, and improved_psnr /
    improved_ssim / improved_mae = the number of images whose denoised version beats the noisy one (test_pretrained.py:62-78).
    Nothing is asserted.  Nothing crosses to the host before a level is finished; the module's deferred f16-range status is
    checked once per level."""
    if not callable(module):
        raise ValueError("module must be callable: uint8 [B,H,W,C] -> uint8 [B,H,W,C]")
    levels = _check_noise_std(noise_std)
    _checked_window(filter_size)
    batches = A.uint8_batches(clean_batches, "clean batches")
    dev = A.device_of(module, "evaluate")
    batches = [b.to(dev).contiguous() for b in batches]
    report = []
    for li, sigma in enumerate(levels):
        noisy_m, den_m = [], []
        for bi, clean in enumerate(batches):
            noisy = corrupt_u8(clean, sigma, _level_seed(seed, li, bi))
            denoised = A.module_result(module(noisy), torch.uint8, clean.shape)
            noisy_m.append(torch.stack(image_metrics(clean, noisy, filter_size=filter_size)))
            den_m.append(torch.stack(image_metrics(clean, denoised, filter_size=filter_size)))
        if hasattr(module, "check_status"):
            module.check_status()                       # an overflow of the split-f16 kernels is not averaged into a number
        n, d = torch.cat(noisy_m, dim=1).cpu().numpy(), torch.cat(den_m, dim=1).cpu().numpy()      # [4 = psnr ssim mae mse, images]
        report.append({"noise_std": sigma, "images": int(n.shape[1]),
                       "psnr_noisy": float(n[0].mean()), "psnr_denoised": float(d[0].mean()),
                       "ssim_noisy": float(n[1].mean()), "ssim_denoised": float(d[1].mean()),
                       "mae_noisy": float(n[2].mean()), "mae_denoised": float(d[2].mean()),
                       "improved_psnr": int((n[0] < d[0]).sum()), "improved_ssim": int((n[1] < d[1]).sum()),
                       "improved_mae": int((d[2] < n[2]).sum())})
    return report


def format_report(report: List[Dict]) -> str:
    """the table tools/evaluate.py prints and train_loop logs"""
    lines = ["sigma  images   psnr noisy -> denoised    ssim noisy -> denoised     mae noisy -> denoised   improved psnr/ssim/mae"]
    for r in report:
        lines.append(f"{r['noise_std']:5.1f}  {r['images']:6d}   {r['psnr_noisy']:10.3f} -> {r['psnr_denoised']:8.3f}    "
                     f"{r['ssim_noisy']:10.5f} -> {r['ssim_denoised']:8.5f}    {r['mae_noisy']:9.3f} -> {r['mae_denoised']:8.3f}   "
                     f"{r['improved_psnr']}/{r['improved_ssim']}/{r['improved_mae']}")
    return "\n".join(lines)


def json_safe(value):
    """strict JSON has no infinity or NaN (psnr of identical images): those become null"""
    if isinstance(value, dict):
        return {k: json_safe(v) for k, v in value.items()}
    if isinstance(value, (list, tuple)):
        return [json_safe(v) for v in value]
    if isinstance(value, float) and not np.isfinite(value):
        return None
    return value


def summarise(batches, per_batch_tensors, keys):
    """the end of every report over batches: (rows, aggregate) from one [len(keys), B] device tensor per batch -- per batch its
    shape, its number of images and the mean of every key over its images; `aggregate` the same over every image"""
    with np.errstate(invalid="ignore"):
        host = [p.cpu().numpy() for p in per_batch_tensors]
        rows = [{"shape": [int(v) for v in b.shape], "images": int(h.shape[1]), **{k: float(h[i].mean()) for i, k in enumerate(keys)}}
                for b, h in zip(batches, host)]
        every = np.concatenate(host, axis=1)
        aggregate = {"images": int(every.shape[1]), **{k: float(every[i].mean()) for i, k in enumerate(keys)}}
    return rows, aggregate


# ---- validation inside train_loop ---------------------------------------------------------------

EvaluationConfig = namedtuple("EvaluationConfig", ["every", "noise_std", "inputs", "no_images"])


def parse_evaluation_config(train_config: Dict) -> Optional[EvaluationConfig]:
    """the `evaluation` section of the train configuration; None when there is none (train_loop then does what it always did)"""
    section = train_config.get("evaluation")
    if section is None:
        return None
    if not isinstance(section, dict):
        raise ValueError("train.evaluation must be a dictionary")
    unknown = set(section) - {"every", "noise_std", "inputs", "no_images"}
    if unknown:
        raise ValueError(f"unknown keys in train.evaluation: {sorted(unknown)}")
    inputs = section.get("inputs", [])
    if isinstance(inputs, str):
        inputs = [inputs]
    no_images = int(section.get("no_images", 16))
    if no_images < 1:
        raise ValueError("train.evaluation.no_images must be at least 1")
    return EvaluationConfig(every=max(0, int(section.get("every", 0))),
                            noise_std=tuple(_check_noise_std(section.get("noise_std", DEFAULT_TRAIN_NOISE_STD))),
                            inputs=[str(i) for i in inputs], no_images=no_images)


def load_evaluation_batches(inputs: Sequence[str], no_images: int, input_shape: Sequence[int], num_channels: int = 3) -> List[np.ndarray]:
    """the first `no_images` image files under `inputs` (sorted), resized to the dataset's height and width as the dataset loads
    them, as one uint8 batch"""
    from .file_operations import image_filenames_generator, load_image
    names = sorted(image_filenames_generator(directory=list(inputs), verbose=False)())[:int(no_images)]
    if not names:
        raise ValueError(f"no images found under {list(inputs)}")
    size = (int(input_shape[0]), int(input_shape[1]))
    images = [load_image(path=p, image_size=size, num_channels=num_channels, expand_dims=False, normalize=False) for p in names]
    return [np.clip(np.round(np.stack(images)), 0, 255).astype(np.uint8)]


class PeriodicValidator:
    """A report on a fixed set of images with a fixed seed, so that successive records are comparable, called by `train_loop`
    between optimizer steps.  It runs the current weights through the inference path (DenoiserModule re-packs after an optimizer
    step) and touches nothing a training step reads: no BatchNorm statistics, no optimizer slot, no random stream of the dataset.
    A subclass names its file, its batches (what, min_hw, the message for none) and has `run(step, epoch)`."""
    FILE, BATCHES = None, None

    def __init__(self, model, config, batches: Iterable, model_dir: Optional[str] = None, seed: int = 0):
        self.config, self.seed = config, int(seed)
        self.module = DenoiserModule(model)
        self.batches = A.uint8_batches(batches, *self.BATCHES)
        if getattr(model, "device", None) is not None and torch.device(model.device).type == "cuda":
            self.batches = [b.to(model.device) for b in self.batches]          # loaded once, kept on the device as uint8
        self.path = None if model_dir is None else os.path.join(model_dir, self.FILE)
        self.history: List[Dict] = []

    def due(self, step: int) -> bool:
        return self.config.every > 0 and step > 0 and step % self.config.every == 0

    def _keep(self, record: Dict) -> Dict:
        """appends the record to the history and, as one line of strict JSON, to the file"""
        self.history.append(record)
        if self.path is not None:
            os.makedirs(os.path.dirname(self.path), exist_ok=True)
            with open(self.path, "a") as f:
                f.write(json.dumps(json_safe(record), allow_nan=False) + "\n")
        return record


class Evaluator(PeriodicValidator):
    """`evaluate` as a PeriodicValidator: what a run that has clean images validates with."""
    FILE = "evaluation.jsonl"
    BATCHES = ("clean batches", 1, "train.evaluation needs images: name `inputs` directories or pass evaluation_batches")

    def run(self, step: int, epoch: int) -> Dict:
        record = {"step": int(step), "epoch": int(epoch), "levels": evaluate(self.module, self.batches, self.config.noise_std, self.seed)}
        for r in record["levels"]:
            logger.info(f"evaluation step {step} sigma {r['noise_std']:g}: psnr {r['psnr_noisy']:.3f} -> {r['psnr_denoised']:.3f}, "
                        f"ssim {r['ssim_noisy']:.5f} -> {r['ssim_denoised']:.5f}, mae {r['mae_noisy']:.3f} -> {r['mae_denoised']:.3f}")
        return self._keep(record)


def build_evaluator(train_config: Dict, model, model_dir: Optional[str] = None, dataset_config: Optional[Dict] = None,
                    evaluation_batches: Optional[Iterable] = None) -> Optional[Evaluator]:
    """the evaluator of a train configuration, or None without a `train.evaluation` section"""
    config = parse_evaluation_config(train_config)
    if config is None:
        return None
    if evaluation_batches is None:
        if not config.inputs:
            raise ValueError("train.evaluation names no `inputs` directories and no evaluation_batches were given")
        shape = (dataset_config or {}).get("input_shape")
        if shape is None:
            raise ValueError("train.evaluation.inputs needs dataset.input_shape for the size the images are loaded at")
        evaluation_batches = load_evaluation_batches(config.inputs, config.no_images, shape, int(model.desc.in_channels))
    return Evaluator(model, config, evaluation_batches, model_dir)
