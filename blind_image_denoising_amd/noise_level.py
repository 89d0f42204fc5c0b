"""
Signal-dependent (Poisson-Gaussian) noise on the device: measure it, and make it.

Camera noise is not one sigma per frame: shot noise makes the variance grow with the signal, var(y | x) ~ gain * x + offset.
`noise_level_statistics(images)` is ONE C-ABI call (bf_noise_level, csrc/noise_level.hip): one pass over a uint8 [B,H,W,C] batch
that conditions the MAD estimator of `noise_statistics` on the local intensity.  Every complete 2x2 cell gives q = |x00 - x01 -
x10 + x11| (twice the modulus of the Haar HH coefficient) and s = x00 + x01 + x10 + x11 (twice the LL coefficient, orthogonal to
HH: conditioning on s does not bias q under independent noise); a cell that holds a 0 or a 255 is excluded and counted; every
other cell belongs to level s >> 6, one of 16.  Per image, channel and level the kernel leaves the number of cells n, the exact
sum of s, and sigma_l = the grouped median of q / 2 / 0.6745.

`noise_level_function(images)` fits var = gain * x + offset to those levels: a weighted least squares of sigma_l^2 on the level
means m_l = sum_s / (4 n), weights n, over the levels with n >= `min_cells`, in fp64 torch ops on the device (16 numbers per
plane).  `camera_noise(clean, gain, read_sigma)` draws such noise (bf_op_camera_noise_u8, csrc/augment.hip).  What is exact and
what is approximate: DESIGN.md 7.10.  There is no CPU execution path.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _args as A
from . import _native as N
from .noise_estimate import noise_statistics

LEVELS = 16
_FEATURE = "the noise level code for the MI355X"

_Fields = namedtuple("NoiseLevelFunction", ["gain", "offset", "level_mean", "level_sigma", "level_count", "excluded_fraction"])


class NoiseLevelFunction(_Fields):
    """var(y | x) = gain * x + offset per image and channel.  gain, offset, excluded_fraction (the share of the 2x2 cells that
    hold a 0 or a 255): [B,C]; level_mean, level_sigma, level_count: [B,C,16], the cell mean, the MAD sigma and the cell count of
    every level, NaN (count 0) where a level holds no cell.  float64 tensors on the images' device, NumPy arrays for NumPy images."""
    __slots__ = ()

    def sigma_at(self, x):
        """the noise standard deviation at intensity x: sqrt(gain * x + offset), [B,C] for a scalar x (x broadcasts against [B,C])"""
        if isinstance(self.gain, np.ndarray):
            return np.sqrt(np.maximum(self.gain * np.asarray(x, np.float64) + self.offset, 0.0))
        x = torch.as_tensor(x, dtype=torch.float64, device=self.gain.device)
        return torch.sqrt((self.gain * x + self.offset).clamp_min(0.0))


def _checked_u8(images):
    """uint8 only: the levels are exact histograms of integers"""
    return A.host_or_device(images, "images", (torch.uint8,), min_hw=3, allow_empty=True)


def _statistics(images: torch.Tensor, was_numpy: bool):
    B, H, W, C = images.shape
    if B == 0:                                                   # nothing to launch
        return (torch.empty((0, C, LEVELS, 3), dtype=torch.float64, device=images.device),
                torch.empty((0, C), dtype=torch.float64, device=images.device))
    images = A.to_device(images, was_numpy, None, "images", _FEATURE).contiguous()
    scratch, nbytes = N.scratch("bf_noise_level", images.device, B, H, W, C)
    levels = torch.empty((B, C, LEVELS, 3), dtype=torch.float64, device=images.device)
    excluded = torch.empty((B, C), dtype=torch.float64, device=images.device)
    N.call("bf_noise_level", N.ptr(images), B, H, W, C, N.ptr(scratch), nbytes, N.ptr(levels), N.ptr(excluded), N.stream_ptr(images))
    return levels, excluded


def noise_level_statistics(images):
    """what bf_noise_level writes for a uint8 [B,H,W,C] batch (torch or NumPy; NumPy is uploaded): (levels, excluded), float64
    device tensors.  levels [B,C,16,3] = (n, sum of s, sigma_l) per level, excluded [B,C] = the number of excluded cells; n, the
    sums and the counts are exact integers.  An empty batch returns empty tensors without a launch."""
    images, was_numpy = _checked_u8(images)
    return _statistics(images, was_numpy)


def fit_noise_levels(levels: torch.Tensor, fallback_variance: torch.Tensor, min_cells: int = 64):
    """The affine fit on `levels` [B,C,16,3] (what noise_level_statistics returns): (gain [B,C], offset [B,C], usable [B,C,16]).
    Weighted least squares of v_l = sigma_l^2 on m_l = sum_s / (4 n) with weights w_l = n over the levels with n >= min_cells.
    Fewer than two usable levels, or a fitted gain < 0: gain = 0, offset = sum w v / sum w.  A fitted offset < 0: offset = 0,
    gain = sum w m v / sum w m^2.  No usable level: gain = 0, offset = `fallback_variance` [B,C]."""
    n, sum_s, sigma = levels[..., 0], levels[..., 1], levels[..., 2]
    usable = n >= float(min_cells)
    w = torch.where(usable, n, torch.zeros_like(n))
    m = torch.where(usable, sum_s / (4.0 * n.clamp_min(1.0)), torch.zeros_like(n))
    v = torch.where(usable, sigma * sigma, torch.zeros_like(n))
    sw, swm, swv = w.sum(dim=2), (w * m).sum(dim=2), (w * v).sum(dim=2)
    swmm, swmv = (w * m * m).sum(dim=2), (w * m * v).sum(dim=2)
    count = usable.sum(dim=2)
    one = torch.ones_like(sw)
    sw1 = torch.where(sw > 0, sw, one)
    mean_m, mean_v = swm / sw1, swv / sw1
    dm = m - mean_m.unsqueeze(2)                                 # w = 0 outside the usable levels
    sxx, sxy = (w * dm * dm).sum(dim=2), (w * dm * (v - mean_v.unsqueeze(2))).sum(dim=2)
    fitted = (count >= 2) & (sxx > 0)
    gain = torch.where(fitted, sxy / torch.where(fitted, sxx, one), torch.zeros_like(sw))
    offset = mean_v - gain * mean_m
    flat = ~fitted | (gain < 0)
    gain = torch.where(flat, torch.zeros_like(gain), gain)
    offset = torch.where(flat, mean_v, offset)
    through_zero = ~flat & (offset < 0)
    gain = torch.where(through_zero, swmv / torch.where(swmm > 0, swmm, one), gain)
    offset = torch.where(through_zero, torch.zeros_like(offset), offset)
    none = count == 0
    offset = torch.where(none, fallback_variance.to(offset.dtype), offset)
    return gain, offset, usable


def noise_level_function(images, min_cells: int = 64) -> NoiseLevelFunction:
    """The noise level function var(y | x) = gain * x + offset of every image and channel of a uint8 [B,H,W,C] batch (torch or
    NumPy): the fit of fit_noise_levels on noise_level_statistics(images); with no usable level at all the offset is
    noise_statistics' sigma_mad^2.  Clipping at 0 and 255 is not modelled: cells that touch either end are excluded, and levels
    next to the ends still see a one-sided tail."""
    min_cells = A.int_in(min_cells, "min_cells", 1)
    images, was_numpy = _checked_u8(images)
    levels, excluded = _statistics(images, was_numpy)
    B, H, W, C = images.shape
    if B == 0:
        fallback = torch.empty((0, C), dtype=torch.float64, device=levels.device)
    else:
        fallback = noise_statistics(images.to(levels.device))[:, :, 2] ** 2
    gain, offset, _ = fit_noise_levels(levels, fallback, min_cells)
    n, sum_s, sigma = levels[..., 0], levels[..., 1], levels[..., 2]
    used = n > 0
    nan = torch.full_like(n, float("nan"))
    nlf = NoiseLevelFunction(gain, offset, torch.where(used, sum_s / (4.0 * n.clamp_min(1.0)), nan), torch.where(used, sigma, nan), n,
                             excluded / float((H // 2) * (W // 2)))
    return NoiseLevelFunction(*(v.cpu().numpy() for v in nlf)) if was_numpy else nlf


def _checked_channel_parameter(value, C: int, what: str) -> np.ndarray:
    try:
        a = np.asarray(value.detach().cpu().numpy() if isinstance(value, torch.Tensor) else value, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a float or {C} floats, got {type(value)}") from None
    if a.ndim == 0:
        a = np.full(C, float(a))
    if a.shape != (C,):
        raise ValueError(f"{what} must be a float or {C} floats for {C} channels, got shape {a.shape}")
    if not np.all(np.isfinite(a)) or np.any(a < 0) or np.any(a > 1.0e6):
        raise ValueError(f"{what} must be finite, non-negative and at most 1e6, got {a.tolist()}")
    return a.astype(np.float32)


def camera_noise(clean_u8: torch.Tensor, gain, read_sigma, seed: int = 0) -> torch.Tensor:
    """bf_op_camera_noise_u8 on a uint8 device tensor [B,H,W,C] (C in 1..4): uint8 of the same shape,

        y = clip(rint(x + sqrt(gain_c x + read_sigma_c^2) z), 0, 255),    z ~ N(0, 1), not truncated,

    z from Box-Muller on Philox (seed, the sample's index inside its image): an image gets the same noise alone or inside a
    batch.  `gain` and `read_sigma`: a float or [C] each, in grey levels (as float32 in the kernel).  Negative or non-finite
    parameters and non-uint8 input raise ValueError before the GPU is touched."""
    B, H, W, C = A.image_batch(clean_u8, "clean_u8", (torch.uint8,)).shape
    g = _checked_channel_parameter(gain, C, "gain")
    r = _checked_channel_parameter(read_sigma, C, "read_sigma")
    seed = A.seed64(seed)
    clean_u8 = A.to_device(clean_u8, False, None, "clean_u8", _FEATURE).contiguous()
    out = torch.empty_like(clean_u8)
    N.call("bf_op_camera_noise_u8", N.ptr(clean_u8), N.ptr(out), B, H, W, C, g.ctypes.data, r.ctypes.data, seed,
           N.stream_ptr(clean_u8))
    return out
