"""
No-reference noise estimation on the device, and the evaluation of a blind denoiser on images that have no clean counterpart.

`noise_statistics(images)` is ONE C-ABI call (bf_noise_estimate, csrc/noise_estimate.hip): one pass over a uint8 or float32
[B,H,W,C] batch that leaves, per image and channel, the Immerkaer sum S = sum |image (*) [[1,-2,1],[-2,4,-2],[1,-2,1]]| and
sigma_fast = sqrt(pi/2) / 6 * S / ((H-2)(W-2)) (Immerkaer, "Fast noise variance estimation", 1996), sigma_mad = the median of
the finest diagonal Haar band / 0.6745 (Donoho's MAD rule, from an exact histogram; uint8 only) and the number of saturated
samples (0 or 255; uint8 only).  Both estimators assume additive noise that is white at the pixel scale (correlated noise reads
low: pixel_shuffle.noise_correlation measures how far it reaches and the level beyond); saturation biases
both low, which is why the clipped fraction is reported next to them.  Nothing synchronises; there is no CPU execution path.

`evaluate_blind(module, noisy_batches)` answers, for photographs that are already noisy: how noisy is the frame (sigma_in), how
noisy is what the network returns (sigma_out), how much did it remove (removed_rms = sqrt(MSE(noisy, denoised))) and is that
the size of the noise that was there (ratio = removed_rms / sigma_in, near 1 when it is).
"""
from collections import namedtuple
from typing import Dict, Iterable

import torch

from . import _args as A
from . import _native as N
from .metrics import image_metric_sums, summarise

NoiseEstimate = namedtuple("NoiseEstimate", ["sigma_fast", "sigma_mad", "clipped_fraction"])

METHODS = ("mad", "immerkaer")
_DTYPES = {torch.uint8: N.BF_DTYPE_U8, torch.float32: N.BF_DTYPE_F32}
_FEATURE = "noise_statistics"


def _checked_images(images):
    """the argument checks of every entry point, before the GPU is touched: (images as a torch tensor, whether NumPy was given)"""
    return A.host_or_device(images, "images", tuple(_DTYPES), min_hw=3, allow_empty=True)


def _statistics(images: torch.Tensor, was_numpy: bool) -> torch.Tensor:
    B, H, W, C = images.shape
    if B == 0:                                                   # nothing to launch
        return torch.empty((0, C, 4), dtype=torch.float64, device=images.device)
    images = A.to_device(images, was_numpy, None, "images", _FEATURE).contiguous()
    scratch, nbytes = N.scratch("bf_noise_estimate", images.device, B, H, W, C)
    out = torch.empty((B, C, 4), dtype=torch.float64, device=images.device)
    N.call("bf_noise_estimate", N.ptr(images), _DTYPES[images.dtype], B, H, W, C, N.ptr(scratch), nbytes, N.ptr(out),
           N.stream_ptr(images))
    return out


def noise_statistics(images) -> torch.Tensor:
    """what bf_noise_estimate writes: a float64 [B,C,4] device tensor of (S, sigma_fast, sigma_mad, clipped count) per image and
    channel of a uint8 or float32 [B,H,W,C] batch (torch or NumPy; NumPy is uploaded).  uint8: S and the count are exact
    integers; float32: sigma_mad and the count are NaN.  An empty batch returns an empty tensor without a launch."""
    images, was_numpy = _checked_images(images)
    return _statistics(images, was_numpy)


def noise_summary(images) -> NoiseEstimate:
    """(sigma_fast, sigma_mad, clipped_fraction), each [B,C] float64: tensors on the images' device, NumPy arrays for NumPy images"""
    images, was_numpy = _checked_images(images)
    stats = _statistics(images, was_numpy)
    est = NoiseEstimate(stats[:, :, 1], stats[:, :, 2], stats[:, :, 3] / float(images.shape[1] * images.shape[2]))
    return NoiseEstimate(*(v.cpu().numpy() for v in est)) if was_numpy else est


def estimate_noise(images, method: str = "mad", per_channel: bool = False):
    """the noise standard deviation of every image of a [B,H,W,C] batch, in the images' own units: [B], or [B,C] with
    `per_channel`.  method "mad": the median of the finest diagonal Haar band / 0.6745 (uint8 images only: it needs the exact
    histogram); "immerkaer": the mean absolute response of the Laplacian-difference mask.  The channels are combined as the root
    mean square of their sigmas.  float64 tensors on the images' device, NumPy arrays for NumPy images."""
    method = A.one_of(method, "method", METHODS)
    images, was_numpy = _checked_images(images)
    if method == "mad" and images.dtype != torch.uint8:
        raise ValueError('method "mad" needs uint8 images (the exact histogram of the Haar band); use method="immerkaer" for float32')
    sigma = _statistics(images, was_numpy)[:, :, 2 if method == "mad" else 1]
    if not per_channel:
        sigma = torch.sqrt((sigma * sigma).mean(dim=1))
    return sigma.cpu().numpy() if was_numpy else sigma


# ---- evaluation without ground truth -------------------------------------------------------------

_KEYS = ("sigma_in", "sigma_out", "removed_rms", "ratio", "clipped_fraction")


def evaluate_blind(module, noisy_batches: Iterable, method: str = "mad") -> Dict:
    """A blind denoiser on images that are already noisy.  `module`: callable uint8 [B,H,W,C] -> uint8 of the same shape
    (DenoiserModule, GraphedDenoiserModule, SelfEnsembleDenoiserModule); `noisy_batches`: an iterable of uint8 batches, host or
    device, of any shapes.  Returns {"method", "images", "batches": [one dict per batch], "aggregate": the same keys over every
    image}: the means over the images of sigma_in = estimate_noise(noisy), sigma_out = estimate_noise(denoised), removed_rms =
    sqrt(MSE(noisy, denoised)), ratio = removed_rms / sigma_in per image, and clipped_fraction = the share of saturated input
    samples.  Nothing is asserted; the module's deferred f16-range status is checked once at the end."""
    if not callable(module):
        raise ValueError("module must be callable: uint8 [B,H,W,C] -> uint8 [B,H,W,C]")
    method = A.one_of(method, "method", METHODS)
    batches = A.uint8_batches(noisy_batches, "noisy batches", min_hw=3)
    dev = A.device_of(module, "evaluate_blind")
    per_image = []                                               # one [5, B] device tensor per batch, rows as _KEYS
    for noisy in batches:
        noisy = noisy.to(dev).contiguous()
        denoised = A.module_result(module(noisy), torch.uint8, noisy.shape)
        stats_in = noise_statistics(noisy)
        column = 2 if method == "mad" else 1
        sigma_in = torch.sqrt((stats_in[:, :, column] ** 2).mean(dim=1))
        sigma_out = estimate_noise(denoised.contiguous(), method)
        _, H, W, C = noisy.shape
        removed = torch.sqrt(image_metric_sums(noisy, denoised.contiguous(), filter_size=3)[:, 0] / float(H * W * C))
        clipped = stats_in[:, :, 3].sum(dim=1) / float(H * W * C)
        per_image.append(torch.stack([sigma_in, sigma_out, removed, removed / sigma_in, clipped]))
    if hasattr(module, "check_status"):
        module.check_status()                                    # an overflow of the split-f16 kernels is not averaged into a number
    rows, aggregate = summarise(batches, per_image, _KEYS)
    return {"method": method, "images": aggregate["images"], "batches": rows, "aggregate": aggregate}


def format_blind_report(report: Dict) -> str:
    """the table tools/evaluate_blind.py prints"""
    lines = [f"noise estimator: {report['method']}",
             "batch            shape  images   sigma in -> out    removed rms   removed / sigma in   clipped"]

    def line(name, shape, r):
        return (f"{name:>5}  {shape:>15}  {r['images']:6d}   {r['sigma_in']:8.3f} -> {r['sigma_out']:6.3f}   {r['removed_rms']:11.3f}   "
                f"{r['ratio']:18.3f}   {100.0 * r['clipped_fraction']:6.2f}%")
    for i, r in enumerate(report["batches"]):
        lines.append(line(str(i), "x".join(map(str, r["shape"])), r))
    lines.append(line("all", "", report["aggregate"]))
    return "\n".join(lines)
