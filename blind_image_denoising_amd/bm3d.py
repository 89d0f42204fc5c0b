"""BM3D: block matching and collaborative filtering (Dabov, Foi, Katkovnik, Egiazarian, "Image denoising by sparse 3-D
transform-domain collaborative filtering", IEEE TIP 2007), the baseline every denoising paper quotes: a denoiser without weights,
about 2 dB above non-local means (nlm.py).  Every 8 x 8 reference block gathers the blocks of its search window that look like it,
the group is transformed (Hadamard in the block, along the group and across the channels), shrunk and transformed back, and the
filtered blocks are averaged where they overlap.  Two steps: a hard threshold gives a basic estimate; the second step matches on
that estimate and shrinks with the Wiener gains it gives.  It takes any channel count 1..4 and any noise level.  Two entry points
of csrc/bm3d.hip carry it.

images = uint8 [B,H,W,C], H and W >= 8; search radius r in 1..12, step in 1..8; Hn the Sylvester Hadamard matrix; per C a forward
matrix A, its squared row norms n2 and a back matrix Bk with Bk A = s I (C = 3: A = [1,1,1], [1,0,-1], [1,-2,1], n2 = 3, 2, 6,
Bk = [2,3,1], [2,0,-2], [2,-3,1], s = 6; else A = Bk = HC, n2 = s = C).

    params    int64 [B,4] = (tau1, thr1, tau2, v1) per image, from sigma [B] in fp64: tau1 = floor((match[0] 64.0) C),
              thr1 = floor((((threshold threshold) sigma) sigma) 64.0), tau2 = floor((match[1] 64.0) C), v1 = floor((64.0 sigma) sigma)
    a step    (noisy, guide, wiener); the first has guide = noisy, the second guide = the uint8 result of the first and wiener
    blocks    reference blocks at 0, step, 2 step, ... <= n - 8 and at n - 8 along each axis; candidates (cy, cx) with
              max(0, y - r) <= cy <= min(H - 8, y + r), the same in x: wholly inside the frame
    match     D = the squared difference of the guide's blocks; a candidate counts if D <= tau (tau1, or tau2 with wiener), the
              reference always; key = (D << 10) | ((dy + r)(2 r + 1) + dx + r), the reference's -1; the group = the first K by
              ascending key, K the largest power of two <= min(count, 16)
    forward   t = H8 block H8 of the noisy blocks, HK along the group, A along the channels; with wiener tb = the same of the guide
    shrink    hard: t where t t > (thr1 K) n2[c], else 0; w = max(4096 // max(kept, 1), 1)
              wiener: S = tb tb, g = (S << 12) // max(S + (v1 K) n2[c], 1), t = (t g + 2048) >> 12;
              w = min(max(2^36 // max(sum g g, 1), 1), 2^14)
    back      Bk along the channels, HK along the group, H8 . H8 per block, times 16 // K: the scale 1024 s
    aggregate num[pixel, c] += w value, den[pixel] += w over the K blocks (int64)
    finish    d = den 1024 s: uint8 clip((2 max(num, 0) + d) // (2 d), 0, 255), or float32(float64(num) / float64(d)), not clipped;
              weights = den, int64 [B,H,W]

Integer arithmetic up to the one division, and integer sums are the same in any order: the results are those of NumPy bit for bit
(tests/bm3d_reference.py).  At sigma = 0 both steps return the image unchanged.

There is no CPU execution path for the kernels; `bm3d_params` is tensor arithmetic and runs where its sigma lives."""
from typing import Optional, Tuple

import numpy as np
import torch

from . import _args as A
from . import _native as N
from .module_denoiser import DenoiserWrapper
from .nlm import _checked_sigma, _per_image
from .noise_estimate import estimate_noise

_FEATURE = "BM3D"
BLOCK, GROUP = 8, 16
MAX_SEARCH, MAX_STEP = 12, 8
THRESHOLD, MATCH = 2.7, (2500.0, 400.0)
SETTINGS = ("sigma", "search", "step", "threshold", "wiener")
MODEL_NAME = "bm3d"


# ---- argument checks ---------------------------------------------------------------------------------------------------------

def _checked_geometry(search, step) -> Tuple[int, int]:
    return A.int_in(search, "search", 1, MAX_SEARCH), A.int_in(step, "step", 1, MAX_STEP)


def _checked_bool(value, what: str) -> bool:
    if not isinstance(value, (bool, np.bool_)):
        raise ValueError(f"{what} must be a bool, got {value!r}")
    return bool(value)


def _checked_match(match) -> Tuple[float, float]:
    if not isinstance(match, (tuple, list)) or len(match) != 2:
        raise ValueError(f"match must be a pair of floats (first step, second step), got {match!r}")
    return A.non_negative_float(match[0], "match"), A.non_negative_float(match[1], "match")


def checked_settings(sigma=None, search: int = 12, step: int = 4, threshold: float = THRESHOLD, wiener: bool = True):
    """the settings of Bm3dDenoiserModule, checked: (sigma, search, step, threshold, wiener)"""
    return (_checked_sigma(sigma),) + _checked_geometry(search, step) + (A.non_negative_float(threshold, "threshold"),
                                                                       _checked_bool(wiener, "wiener"))


def parse_setting(bm3d) -> dict:
    """load_model's `bm3d`: None -> the defaults; a dict of SETTINGS -> itself.  Everything is checked here, before anything is
    loaded."""
    return A.parse_setting(bm3d, "bm3d", "None or a dict of Bm3dDenoiserModule settings", SETTINGS, checked_settings, bools=False) or {}


def _checked_images(images, what: str = "images") -> Tuple[torch.Tensor, bool]:
    images, was_numpy = A.host_or_device(images, what, (torch.uint8,), min_hw=BLOCK, allow_empty=True)
    if images.numel() >= 2 ** 31:
        raise ValueError(f"{what} must hold fewer than 2^31 samples, got {tuple(images.shape)}")
    return images, was_numpy


def _checked_params(params, B: int):
    if not isinstance(params, torch.Tensor) or params.dtype != torch.int64 or tuple(params.shape) != (B, 4):
        raise ValueError(f"params must be an int64 tensor {(B, 4)} for this batch, got {A._got(params)}")


# ---- the operators -----------------------------------------------------------------------------------------------------------

def bm3d_params(sigma, C: int, threshold: float = THRESHOLD, match=MATCH) -> torch.Tensor:
    """the (tau1, thr1, tau2, v1) rows of noise levels sigma [B] (a tensor where it lives, else anything torch.as_tensor takes),
    int64 [B,4] on sigma's device, in fp64: tau1 = floor((match[0] 64.0) C), thr1 = floor((((threshold threshold) sigma) sigma) 64.0),
    tau2 = floor((match[1] 64.0) C), v1 = floor((64.0 sigma) sigma).  Tensor arithmetic: nothing synchronises."""
    C = A.int_in(C, "C", 1, 4)
    threshold = A.non_negative_float(threshold, "threshold")
    match = _checked_match(match)
    s = torch.as_tensor(sigma).to(torch.float64)
    if s.dim() != 1:
        raise ValueError(f"sigma must be a [B] array, got shape {tuple(s.shape)}")
    tau1 = torch.full_like(s, float(np.floor((match[0] * 64.0) * C)))
    thr1 = torch.floor((((threshold * threshold) * s) * s) * 64.0)
    tau2 = torch.full_like(s, float(np.floor((match[1] * 64.0) * C)))
    v1 = torch.floor((64.0 * s) * s)
    return torch.stack([tau1, thr1, tau2, v1], dim=1).to(torch.int64).contiguous()


def _accumulator(images: torch.Tensor) -> torch.Tensor:
    B, H, W, C = images.shape
    return torch.empty((B, H, W, C + 1), dtype=torch.int64, device=images.device)


def _launch_step(noisy: torch.Tensor, guide: torch.Tensor, params: torch.Tensor, search: int, step: int, wiener: bool,
                 acc: torch.Tensor, cast_to_uint8: bool, want_weights: bool):
    """one step into `acc` and its finish: (out, weights or None)"""
    B, H, W, C = noisy.shape
    N.call("bf_op_bm3d_step", N.ptr(noisy), N.ptr(guide), N.ptr(params), B, H, W, C, search, step, int(wiener), N.ptr(acc),
           N.stream_ptr(noisy))
    out = torch.empty((B, H, W, C), dtype=torch.uint8 if cast_to_uint8 else torch.float32, device=noisy.device)
    weights = torch.empty((B, H, W), dtype=torch.int64, device=noisy.device) if want_weights else None
    N.call("bf_op_bm3d_finish", N.ptr(acc), B, H, W, C, N.ptr(out), int(cast_to_uint8), N.ptr(weights), N.stream_ptr(noisy))
    return out, weights


def _launch(images: torch.Tensor, params: torch.Tensor, search: int, step: int, wiener: bool, cast_to_uint8: bool, want_weights: bool):
    """step one, and with `wiener` step two on its uint8 result; one accumulator serves both"""
    acc = _accumulator(images)
    if not wiener:
        return _launch_step(images, images, params, search, step, False, acc, cast_to_uint8, want_weights)
    basic = _launch_step(images, images, params, search, step, False, acc, True, False)[0]
    return _launch_step(images, basic, params, search, step, True, acc, cast_to_uint8, want_weights)


def _empty(images: torch.Tensor, cast_to_uint8: bool):
    _, H, W, C = images.shape
    return (torch.empty((0, H, W, C), dtype=torch.uint8 if cast_to_uint8 else torch.float32, device=images.device),
            torch.empty((0, H, W), dtype=torch.int64, device=images.device))


def _placed(images: torch.Tensor, was_numpy: bool, params: torch.Tensor, what: str) -> torch.Tensor:
    images = A.to_device(images, was_numpy, None, what, _FEATURE).contiguous()
    if params.device != images.device:
        raise ValueError(f"params must live on the images' device {images.device}, got {params.device}")
    return images


def _delivered(out, weights, was_numpy: bool, return_weights: bool):
    if was_numpy:
        out, weights = out.cpu().numpy(), weights.cpu().numpy() if return_weights else None
    return (out, weights) if return_weights else out


def bm3d_step(noisy, guide, params: torch.Tensor, wiener: bool, search: int = 12, step: int = 4, cast_to_uint8: bool = True,
              return_weights: bool = False):
    """bf_op_bm3d_step and bf_op_bm3d_finish: one step of BM3D on a uint8 [B,H,W,C] batch `noisy`, matching on `guide` (the same
    shape; both torch on the GPU, or both NumPy, which are uploaded and NumPy handed back) under `params` (int64 [B,4] on the
    images' device; bm3d_params makes them): the hard threshold, or with `wiener` the Wiener gains of the guide.  uint8 [B,H,W,C],
    or float32 before the rounding and not clipped; with `return_weights` (out, weights int64 [B,H,W] = den).  An empty batch
    returns an empty result without a launch."""
    wiener = _checked_bool(wiener, "wiener")
    search, step = _checked_geometry(search, step)
    noisy, was_numpy = _checked_images(noisy, "noisy")
    guide, guide_numpy = _checked_images(guide, "guide")
    if tuple(guide.shape) != tuple(noisy.shape) or guide_numpy != was_numpy:
        raise ValueError(f"guide must be a batch like noisy, {'NumPy' if was_numpy else 'torch'} uint8 {tuple(noisy.shape)}, got "
                         f"{'NumPy' if guide_numpy else 'torch'} {A._got(guide)}")
    _checked_params(params, noisy.shape[0])
    if noisy.shape[0] == 0:
        out, weights = _empty(noisy, cast_to_uint8)
    else:
        noisy = _placed(noisy, was_numpy, params, "noisy")
        guide = A.to_device(guide, guide_numpy, None, "guide", _FEATURE).contiguous()
        if guide.device != noisy.device:
            raise ValueError(f"guide must live on noisy's device {noisy.device}, got {guide.device}")
        out, weights = _launch_step(noisy, guide, params.contiguous(), search, step, wiener, _accumulator(noisy), bool(cast_to_uint8),
                                    bool(return_weights))
    return _delivered(out, weights, was_numpy, return_weights)


def bm3d(images, params: torch.Tensor, search: int = 12, step: int = 4, wiener: bool = True, cast_to_uint8: bool = True,
         return_weights: bool = False):
    """BM3D of a uint8 [B,H,W,C] batch (torch on the GPU, or NumPy, which is uploaded and NumPy handed back) under `params` (int64
    [B,4] on the images' device; bm3d_params makes them): step one (uint8), then step two on (images, the result of step one); with
    wiener=False step one alone.  uint8 [B,H,W,C], or float32 before the rounding; with `return_weights` (out, weights int64
    [B,H,W] = den of the last step).  An empty batch returns an empty result without a launch."""
    wiener = _checked_bool(wiener, "wiener")
    search, step = _checked_geometry(search, step)
    images, was_numpy = _checked_images(images)
    _checked_params(params, images.shape[0])
    if images.shape[0] == 0:
        out, weights = _empty(images, cast_to_uint8)
    else:
        images = _placed(images, was_numpy, params, "images")
        out, weights = _launch(images, params.contiguous(), search, step, wiener, bool(cast_to_uint8), bool(return_weights))
    return _delivered(out, weights, was_numpy, return_weights)


# ---- the module --------------------------------------------------------------------------------------------------------------

class Bm3dDenoiserModule(DenoiserWrapper):
    """BM3D as a denoiser module: uint8 [B,H,W,C] -> uint8 [B,H,W,C] (float32, not rounded, with cast_to_uint8=False), C in 1..4,
    H and W >= 8.  Input handling, return types and empty batches as every wrapper (DenoiserWrapper), around no module: there is no
    model (`model_hydra` is None) and, in integer arithmetic, no range to leave (`check_status()` is True).  It has a
    `float_form()`, so every wrapper (tiled, pixel-shuffled, stabilised, burst, video) and estimate_risk take it.

    `sigma`: the noise level the thresholds and the Wiener gains are made from; None estimates it per image (estimate_noise, "mad")
    on the device with no host read; a float or a [B] array is taken as given, a [B,C] array is reduced to the root mean square
    over the channels.  `threshold`: the hard threshold of the first step in units of sigma.  `wiener`: False stops after the
    first step.  With a device tensor and a fixed sigma nothing in a call synchronises: it can be captured into a HIP graph.

    `last_weights` is the int64 [B,H,W] = den of the last call of this module or of its float form: the sum of the weights of the
    groups that reached the pixel."""
    SETTINGS = SETTINGS

    def __init__(self, sigma=None, search: int = 12, step: int = 4, threshold: float = THRESHOLD, wiener: bool = True,
                 cast_to_uint8: bool = True):
        self._sigma, self._search, self._step, self._threshold, self._wiener = checked_settings(sigma, search, step, threshold, wiener)
        self._wrap(None, cast_to_uint8, allow_none=True)
        self._record = {"weights": None}

    def _twin(self, **settings):
        return type(self)(**settings)                             # no module to pass on

    @property
    def last_weights(self) -> Optional[torch.Tensor]:
        return self._record["weights"]

    def __call__(self, images):
        images, was_numpy = _checked_images(images, "image")
        B, H, W, C = images.shape
        if isinstance(self._sigma, torch.Tensor) and B > 0 and tuple(self._sigma.shape) != (B,):
            raise ValueError(f"sigma must be a float or a [{B}] array for this batch, got shape {tuple(self._sigma.shape)}")
        if B == 0:
            return self._empty_output(images, was_numpy)
        images = self._place(images, was_numpy, "image", _FEATURE)
        sigma = estimate_noise(images, "mad") if self._sigma is None else _per_image(self._sigma, B, images.device, "sigma")
        out, weights = _launch(images, bm3d_params(sigma, C, self._threshold), self._search, self._step, self._wiener,
                               self._cast_to_uint8, True)
        self._record["weights"] = weights
        return self._deliver(out, was_numpy)
