"""
Denoise camera noise with a Gaussian denoiser: variance stabilisation around the call.

Every network here is trained on additive Gaussian noise of one sigma per frame; camera noise has var(y | x) = gain x + offset,
a sigma that changes by a factor of several between the shadows and the highlights of one frame.  The standard remedy needs no
retraining: the generalised Anscombe transform with the frame's (gain, offset) makes the noise Gaussian of one standard deviation
everywhere, the denoiser runs on that, and the exact unbiased inverse of Makitalo & Foi (IEEE TIP 2013, closed form) returns to
grey levels without the bias the algebraic inverse has.  Two kernels of csrc/vst.hip carry everything that is not the denoiser:
`bf_op_vst_forward_u8` (uint8 -> uint8 through a table per image, built in fp64; 0 -> 0, 255 -> 255, the identity for gain 0) and
`bf_op_vst_inverse` (float32 -> float32 or uint8).  Both read (gain, offset) as fp64 [B,C] DEVICE tensors, which is what
`noise_level_function` leaves there: the fit never comes to the host.  DESIGN.md 7.11 has the formulas and what was measured.
There is no CPU execution path.
"""
from typing import Dict, Iterable, Optional

import numpy as np
import torch

from . import _args as A
from . import _native as N
from .metrics import image_metrics, summarise
from .module_denoiser import DenoiserWrapper
from .noise_level import NoiseLevelFunction, camera_noise, noise_level_function

GAIN_MAX, OFFSET_MAX = 64.0, 65025.0
INVERSES = ("exact", "algebraic")
_FEATURE = "the stabilisation code"


def _checked_noise_level(noise_level):
    """(gain, offset) of a NoiseLevelFunction or a (gain, offset) pair.  Device tensors are passed on as they are (the kernels
    sanitise what they read); everything else is host-given: float64 NumPy arrays of at most two dimensions, finite, 0 <= gain <=
    64, 0 <= offset <= 65025, else ValueError."""
    pair = (noise_level.gain, noise_level.offset) if isinstance(noise_level, NoiseLevelFunction) else noise_level
    if not isinstance(pair, (tuple, list)) or len(pair) != 2 or pair[0] is None or pair[1] is None:
        raise ValueError("noise_level must be a NoiseLevelFunction or a (gain, offset) pair")
    out = []
    for value, what, top in ((pair[0], "gain", GAIN_MAX), (pair[1], "offset", OFFSET_MAX)):
        if isinstance(value, torch.Tensor) and value.is_cuda:
            if value.dim() > 2:
                raise ValueError(f"{what} must be a float, [C] or [B,C], got shape {tuple(value.shape)}")
            out.append(value)
            continue
        try:
            a = np.asarray(value.detach().numpy() if isinstance(value, torch.Tensor) else value, dtype=np.float64)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"{what} must be a float, a [C] or a [B,C] array, got {type(value)}") from None
        if a.ndim > 2:
            raise ValueError(f"{what} must be a float, [C] or [B,C], got shape {a.shape}")
        if not np.all(np.isfinite(a)) or np.any(a < 0) or np.any(a > top):
            raise ValueError(f"{what} must be finite and in 0..{top:g}, got {a.tolist()}")
        out.append(a)
    return out[0], out[1]


def _launch_arguments(images, dtype, what: str, noise_level):
    """the argument checks shared by both directions: (contiguous images, gain [B,C], offset [B,C]) on the images' device"""
    B, _, _, C = A.image_batch(images, what, (dtype,)).shape
    pair = _checked_noise_level(noise_level)                    # host-given values are refused before the GPU is touched
    for value, name in zip(pair, ("gain", "offset")):
        A.broadcasts_to(value.shape, B, C, name)
    images = A.to_device(images, False, None, what, _FEATURE)
    gain, offset = (torch.as_tensor(v).to(device=images.device, dtype=torch.float64).expand(B, C).contiguous() for v in pair)
    return images.contiguous(), gain, offset


def stabilise_u8(images_u8: torch.Tensor, noise_level) -> torch.Tensor:
    """bf_op_vst_forward_u8 on a uint8 device tensor [B,H,W,C] (C in 1..4): uint8 of the same shape, v = rint(s u(y)) with u(y) =
    2 y / (sqrt(a y + c) + rc), c = 3/8 a^2 + o, rc = sqrt(c), s = 255 / u(255), per image and channel.  The noise of variance
    a x + o has the standard deviation s everywhere in v; 0 stays 0, 255 stays 255, and a = 0 gives v = y.

    `noise_level`: a NoiseLevelFunction (noise_level_function's, device tensors or NumPy) or a (gain, offset) pair, each a float,
    [C] or [B,C].  Host-given values must be finite with 0 <= gain <= 64 and 0 <= offset <= 65025 (ValueError before the GPU is
    touched) and are uploaded as float64; device tensors are read as they are and sanitised by the kernel (gain not finite or not
    positive: 0, capped at 64; offset clamped to [1/12, 65025], 1/12 when not finite -- the variance rounding to grey levels gives
    any uint8 image)."""
    images_u8, gain, offset = _launch_arguments(images_u8, torch.uint8, "images_u8", noise_level)
    B, H, W, C = images_u8.shape
    out = torch.empty_like(images_u8)
    N.call("bf_op_vst_forward_u8", N.ptr(images_u8), N.ptr(out), B, H, W, C, N.ptr(gain), N.ptr(offset), N.stream_ptr(images_u8))
    return out


def unstabilise(stabilised_f32: torch.Tensor, noise_level, inverse: str = "exact", cast_to_uint8: bool = True) -> torch.Tensor:
    """bf_op_vst_inverse on a float32 device tensor [B,H,W,C] in the stabilised domain (what a denoiser returns for
    stabilise_u8's output): with w clamped to [0, 255] and u = w / s,

        algebraic   x = rc u + a u^2 / 4
        exact       x = algebraic + a / 4 + a (K1 d - K2 d^2 + K3 d^3),   d = a / (a u + 2 rc)

    K1 = sqrt(3/2) / 4, K2 = 11/8, K3 = 5 sqrt(3/2) / 8: the closed form of the exact unbiased inverse of Makitalo & Foi (2013)
    with the terms that diverge as a -> 0 cancelled.  x is clipped to [0, 255]: float32, or uint8 rounded half to even.
    `noise_level` as stabilise_u8 (the same one)."""
    A.one_of(inverse, "inverse", INVERSES)
    stabilised_f32, gain, offset = _launch_arguments(stabilised_f32, torch.float32, "stabilised_f32", noise_level)
    B, H, W, C = stabilised_f32.shape
    out = torch.empty((B, H, W, C), dtype=torch.uint8 if cast_to_uint8 else torch.float32, device=stabilised_f32.device)
    N.call("bf_op_vst_inverse", N.ptr(stabilised_f32), N.ptr(out), B, H, W, C, N.ptr(gain), N.ptr(offset), int(inverse == "exact"),
           int(bool(cast_to_uint8)), N.stream_ptr(stabilised_f32))
    return out


def parse_setting(stabilise) -> Optional[dict]:
    """load_model's `stabilise`: None | False -> None; True -> the fit per frame; a (gain, offset) pair -> that pair.  Everything
    is checked here, before anything is loaded."""
    if stabilise is not None and not isinstance(stabilise, (bool, tuple, list)):
        raise ValueError(f"stabilise must be None, a bool or a (gain, offset) pair, got {stabilise!r}")
    if stabilise is None or stabilise is False:
        return None
    if stabilise is True:
        return {}
    _checked_noise_level(stabilise)
    return {"noise_level": stabilise}


class StabilisedDenoiserModule(DenoiserWrapper):
    """A denoiser run between the variance-stabilising transform and its inverse: uint8 [B,H,W,C] -> uint8 [B,H,W,C] (float32,
    not rounded, with cast_to_uint8=False).  `module`, argument checks, input handling, return types, empty batches and f16-range
    status as every wrapper (DenoiserWrapper).

    A call is: with `noise_level=None` the fit
    noise_level_function(image, min_cells), per image of the batch given, on the device (needs H, W >= 3); stabilise_u8; the float
    module; unstabilise(inverse).  A fixed `noise_level` (a NoiseLevelFunction or a (gain, offset) pair, as stabilise_u8 takes it)
    of shape [B,C] must match the batch, else ValueError.  `last_noise_level` holds the fit of the last call (the
    NoiseLevelFunction, device tensors), or the fixed pair as it was given.  With gain 0 the forward map is the identity and the
    inverse x = rc (w / s) = w up to two float32 roundings: the wrapper then returns what the module returns to within those."""
    SETTINGS = ("noise_level", "inverse", "min_cells")

    def __init__(self, module, noise_level=None, inverse: str = "exact", cast_to_uint8: bool = True, min_cells: int = 64):
        if isinstance(module, StabilisedDenoiserModule):
            raise ValueError("module is already stabilised")
        self._wrap(module, cast_to_uint8)
        self._inverse, self._min_cells = A.one_of(inverse, "inverse", INVERSES), A.int_in(min_cells, "min_cells", 1)
        self._noise_level = None if noise_level is None else _checked_noise_level(noise_level)
        self.last_noise_level = None

    def __call__(self, image):
        image, was_numpy = self._checked_input(image)
        B, H, W, C = image.shape
        if self._noise_level is not None:
            for value, what in zip(self._noise_level, ("gain", "offset")):
                A.broadcasts_to(value.shape, B, C, what)
        if B == 0:
            return self._empty_output(image, was_numpy)
        image = self._place(image, was_numpy, "image", _FEATURE)
        if self._noise_level is None:
            level = noise_level_function(image, self._min_cells)
        else:
            level = self._noise_level
        self.last_noise_level = level
        result = self._run(stabilise_u8(image, level))
        if self._repeat_in_fp32(was_numpy):
            return self(image.cpu().numpy())
        return self._deliver(unstabilise(result.to(image.device), level, self._inverse, self._cast_to_uint8), was_numpy)


# ---- evaluation on synthetic camera noise --------------------------------------------------------

_ARMS = ("noisy", "direct", "stabilised_known", "stabilised_fitted")
_METRICS = ("psnr", "ssim", "mae")


def evaluate_camera(module, clean_batches: Iterable, gain: float, read_sigma: float, seed: int = 0) -> Dict:
    """What stabilisation is worth for `module` on camera noise of a known (gain, read_sigma): every clean uint8 batch (host or
    device, H and W >= 11 for the SSIM window) gets camera_noise(clean, gain, read_sigma, seed + k), and PSNR, SSIM and MAE
    (metrics.image_metrics) against the clean frames are taken of four things: the noisy frame, the module applied directly, the
    module stabilised with the known (gain, read_sigma^2 + 1/12), and the module stabilised with the frame's own fit.  `module`: a
    DenoiserModule or SelfEnsembleDenoiserModule (uint8 -> uint8).  Returns {"gain", "read_sigma", "images", "batches": [one dict per
    batch], "aggregate"}: per entry psnr_*, ssim_*, mae_* for the four arms (means over the images) and fitted_gain /
    fitted_offset (means over images and channels).  Nothing is asserted; the module's deferred f16-range status is checked once
    at the end."""
    gain, read_sigma = A.non_negative_float(gain, "gain"), A.non_negative_float(read_sigma, "read_sigma")
    known = (gain, read_sigma ** 2 + 1.0 / 12.0)
    arms = {"direct": module,
            "stabilised_known": StabilisedDenoiserModule(module, known),
            "stabilised_fitted": StabilisedDenoiserModule(module, None)}
    batches = A.uint8_batches(clean_batches, "clean batches")
    dev = A.device_of(module, "evaluate_camera")
    per_batch = []                                               # one [14, B] device tensor per batch
    for k, clean in enumerate(batches):
        clean = clean.to(dev).contiguous()
        noisy = camera_noise(clean, gain, read_sigma, (int(seed) + k) % 2 ** 64)
        rows = list(image_metrics(clean, noisy)[:3])
        for name in _ARMS[1:]:
            rows += list(image_metrics(clean, A.module_result(arms[name](noisy), torch.uint8, clean.shape))[:3])
        fit = arms["stabilised_fitted"].last_noise_level
        rows += [fit.gain.mean(dim=1), fit.offset.mean(dim=1)]
        per_batch.append(torch.stack(rows))
    if hasattr(module, "check_status"):
        module.check_status()                                    # an overflow of the split-f16 kernels is not averaged into a number
    keys = [f"{m}_{arm}" for arm in _ARMS for m in _METRICS] + ["fitted_gain", "fitted_offset"]
    rows, aggregate = summarise(batches, per_batch, keys)
    return {"gain": gain, "read_sigma": read_sigma, "images": aggregate["images"], "batches": rows,
            "aggregate": aggregate}


def format_camera_report(report: Dict) -> str:
    """the table tools/evaluate_camera.py prints"""
    lines = [f"camera noise: gain {report['gain']:g}, read sigma {report['read_sigma']:g}; fitted gain "
             f"{report['aggregate']['fitted_gain']:.3f}, offset {report['aggregate']['fitted_offset']:.3f}",
             "batch            shape  images  arm                    psnr      ssim       mae"]

    def block(name, shape, r):
        return [f"{name:>5}  {shape:>15}  {r['images']:6d}  {arm:<18} {r['psnr_' + arm]:8.3f}  {r['ssim_' + arm]:8.5f}  {r['mae_' + arm]:8.3f}"
                for arm in _ARMS]
    for i, r in enumerate(report["batches"]):
        lines += block(str(i), "x".join(map(str, r["shape"])), r)
    lines += block("all", "", report["aggregate"])
    return "\n".join(lines)
