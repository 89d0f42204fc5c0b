"""Spatially correlated noise around a denoiser that was trained on white noise: how far the correlation reaches, pixel-shuffle
down-sampling (Zhou et al., "When AWGN-based denoiser meets real noises", AAAI 2020) and the random-replacing refinement (Lee et
al., AP-BSN, CVPR 2022).  Five entry points of csrc/pixel_shuffle.hip carry everything that is not the denoiser.

The dilated Haar statistic (`bf_noise_correlation`), for s = 1..S, per image and channel of a uint8 [B,H,W,C] batch:

    q_s(y,x) = |x(y,x) - x(y,x+s) - x(y+s,x) + x(y+s,x+s)|       at the (H - s)(W - s) positions with y + s < H and x + s < W
    sigma_s  = the grouped-data median of the exact 511-bin histogram of q_s / 2 / 0.6745        (the rule of noise_estimate.py)

q_s is zero on every image f(x) + g(y) and has variance 4 sigma^2 (1 - rho(0,s) - rho(s,0) + (rho(s,s) + rho(s,-s)) / 2) under noise
of autocorrelation rho: flat in s for white noise, rising with s to sigma where the correlation ends.  The stride rule on
sigma[b,s] = the root mean square over the channels of sigma_s:

    stride[b]      = the smallest s in 1..S-1 with sigma[b,s] >= threshold sigma[b,s+1], else S        (a curve of zeros: 1)
    sigma_white[b] = sigma[b, min(stride + 1, S)]

Pixel-shuffle (`bf_op_pd_split_u8`, `bf_op_pd_merge`), Hs = ceil(H / s), Ws = ceil(W / s), H, W >= 2 s unless s == 1:

    split  [B,H,W,C] -> [B s^2, Hs, Ws, C]: member b s^2 + i s + j at (u, v) = pixel (u s + i, v s + j); a coordinate past the frame
           is lowered by s (the last row / column of the same phase is repeated)
    merge  out(b, y, x) = src(b s^2 + (y mod s) s + (x mod s), y div s, x div s); float32, or clipped, rounded half to even, uint8

Refinement (`bf_op_pd_replace_u8`, `bf_op_pd_mean`): T copies of `base` in which the pixels whose Philox word is below
min(int(replace 2^32), 2^32 - 1) carry the `noisy` value (pixel p = y W + x takes word p & 3 of philox4x32_10(counter = (lo32 g,
hi32 g, t, 5), key = (lo32 seed, hi32 seed)), g = p >> 2; the same masks for every image of a batch), and the mean of T float
results: fp64 sum in ascending t, one division, cast.  There is no CPU execution path for the kernels."""
from typing import NamedTuple, Optional, Tuple, Union

import torch

from . import _args as A
from . import _native as N
from .module_denoiser import DenoiserWrapper

_FEATURE = "the pixel-shuffle code"
MAX_STRIDE = 8                  # of every kernel here
MAX_COPIES = 16
SETTINGS = ("stride", "max_stride", "threshold", "refine", "replace", "seed")


class NoiseCorrelation(NamedTuple):
    """sigma [B,S] float64: the root mean square over the channels of sigma_s, s = 1..S; stride [B] int64 and sigma_white [B]
    float64 by the stride rule (module docstring)"""
    sigma: object
    stride: object
    sigma_white: object


# ---- the correlation statistic -----------------------------------------------------------------------------------------------

def _checked_images(images, max_stride) -> Tuple[torch.Tensor, bool, int]:
    S = A.int_in(max_stride, "max_stride", 1, MAX_STRIDE)
    images, was_numpy = A.host_or_device(images, "images", (torch.uint8,), min_hw=S + 1, allow_empty=True)
    return images, was_numpy, S


def _statistics(images: torch.Tensor, was_numpy: bool, S: int) -> Tuple[torch.Tensor, torch.Tensor]:
    B, H, W, C = images.shape
    if B == 0:                                                   # nothing to launch
        return (torch.empty((0, C, S, 512), dtype=torch.int64, device=images.device),
                torch.empty((0, C, S), dtype=torch.float64, device=images.device))
    images = A.to_device(images, was_numpy, None, "images", _FEATURE).contiguous()
    scratch, nbytes = N.scratch("bf_noise_correlation", images.device, B, H, W, C, S)
    sigma = torch.empty((B, C, S), dtype=torch.float64, device=images.device)
    N.call("bf_noise_correlation", N.ptr(images), B, H, W, C, S, N.ptr(scratch), nbytes, N.ptr(sigma), N.stream_ptr(images))
    return scratch.view(torch.int64).view(B, C, S, 512), sigma


def noise_correlation_statistics(images, max_stride: int = 6) -> Tuple[torch.Tensor, torch.Tensor]:
    """what bf_noise_correlation writes for a uint8 [B,H,W,C] batch (torch or NumPy; NumPy is uploaded), H, W >= max_stride + 1:
    (the exact histograms of q_s, int64 [B,C,S,512] with bin 511 empty, sigma_s float64 [B,C,S]), device tensors.  An empty batch
    returns empty tensors without a launch."""
    images, was_numpy, S = _checked_images(images, max_stride)
    return _statistics(images, was_numpy, S)


def stride_rule(sigma: torch.Tensor, threshold: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(stride [B] int64, sigma_white [B]) of a [B,S] curve: a few tensor operations where the curve lives, nothing synchronises"""
    B, S = sigma.shape
    steps = torch.arange(1, S + 1, dtype=torch.int64, device=sigma.device)
    settled = torch.ones((B, S), dtype=torch.bool, device=sigma.device)
    settled[:, :S - 1] = sigma[:, :S - 1] >= threshold * sigma[:, 1:]
    stride = torch.where(settled, steps, torch.full_like(steps, S)).min(dim=1).values
    white = sigma.gather(1, torch.clamp(stride + 1, max=S).unsqueeze(1) - 1).squeeze(1)
    return stride, white


def _channel_rms(sigma_s: torch.Tensor) -> torch.Tensor:
    """[B,C,S] -> [B,S]; the squares are added in ascending channel order, so that the value does not depend on a reduction's
    order, and divided by a tensor (torch divides by a Python number as a product with its reciprocal: one rounding more)"""
    total = sigma_s[:, 0] * sigma_s[:, 0]
    for c in range(1, sigma_s.shape[1]):
        total = total + sigma_s[:, c] * sigma_s[:, c]
    return torch.sqrt(total / torch.full_like(total, float(sigma_s.shape[1])))


def _checked_threshold(threshold) -> float:
    threshold = A.non_negative_float(threshold, "threshold", 1.0)
    if threshold == 0.0:
        raise ValueError("threshold must be a finite float in 0..1 and above 0, got 0")
    return threshold


def noise_correlation(images, max_stride: int = 6, threshold: float = 0.8) -> NoiseCorrelation:
    """How far the noise of every image of a uint8 [B,H,W,C] batch is correlated: NoiseCorrelation(sigma [B,S], stride [B] int64,
    sigma_white [B]) by the stride rule of the module docstring; sigma_white is the level a white-noise estimator should have
    read.  Tensors on the images' device, NumPy arrays for NumPy images."""
    threshold = _checked_threshold(threshold)
    images, was_numpy, S = _checked_images(images, max_stride)
    sigma = _channel_rms(_statistics(images, was_numpy, S)[1])
    result = NoiseCorrelation(sigma, *stride_rule(sigma, threshold))
    return NoiseCorrelation(*(v.cpu().numpy() for v in result)) if was_numpy else result


# ---- the four data-movement kernels ------------------------------------------------------------------------------------------

def _checked_stride(stride, H: Optional[int] = None, W: Optional[int] = None) -> int:
    s = A.int_in(stride, "stride", 1, MAX_STRIDE)
    if s > 1 and H is not None and (H < 2 * s or W < 2 * s):
        raise ValueError(f"stride {s} needs H, W >= {2 * s}, got {H} x {W}")
    return s


def pd_split_u8(image_u8: torch.Tensor, stride: int) -> torch.Tensor:
    """bf_op_pd_split_u8 on a uint8 device tensor [B,H,W,C]: the s^2 sub-images of every s-th pixel, uint8 [B s^2, Hs, Ws, C],
    member b s^2 + i s + j = phase (i, j) of image b"""
    A.image_batch(image_u8, "image_u8", (torch.uint8,))
    B, H, W, C = image_u8.shape
    s = _checked_stride(stride, H, W)
    image_u8 = A.to_device(image_u8, False, None, "image_u8", _FEATURE).contiguous()
    out = torch.empty((B * s * s, -(H // -s), -(W // -s), C), dtype=torch.uint8, device=image_u8.device)
    N.call("bf_op_pd_split_u8", N.ptr(image_u8), N.ptr(out), B, H, W, C, s, N.stream_ptr(image_u8))
    return out


def pd_merge(members_f32: torch.Tensor, B: int, H: int, W: int, stride: int, cast_to_uint8: bool = True) -> torch.Tensor:
    """bf_op_pd_merge on the float32 device results of the s^2 sub-images of B frames of H x W, [B s^2, Hs, Ws, C] as pd_split_u8
    orders them: interleaved back to [B,H,W,C] float32, or clipped, rounded half to even and cast to uint8"""
    B, H, W = A.int_in(B, "B", 1), A.int_in(H, "H", 1), A.int_in(W, "W", 1)
    s = _checked_stride(stride, H, W)
    A.image_batch(members_f32, "members_f32", (torch.float32,))
    C = int(members_f32.shape[-1])
    want = (B * s * s, -(H // -s), -(W // -s), C)
    if tuple(members_f32.shape) != want:
        raise ValueError(f"members_f32 must be {want} for {B} frames of {H} x {W} at stride {s}, got {tuple(members_f32.shape)}")
    members_f32 = A.to_device(members_f32, False, None, "members_f32", _FEATURE).contiguous()
    out = torch.empty((B, H, W, C), dtype=torch.uint8 if cast_to_uint8 else torch.float32, device=members_f32.device)
    N.call("bf_op_pd_merge", N.ptr(members_f32), N.ptr(out), int(bool(cast_to_uint8)), B, H, W, C, s, N.stream_ptr(members_f32))
    return out


def replace_threshold(replace) -> int:
    """the uint32 a Philox word is compared with: min(int(replace 2^32), 2^32 - 1); 0 replaces nothing"""
    return min(int(A.non_negative_float(replace, "replace", 1.0) * 2.0 ** 32), 2 ** 32 - 1)


def pd_replace_u8(base_u8: torch.Tensor, noisy_u8: torch.Tensor, copies: int, replace: float = 0.16, seed: int = 0) -> torch.Tensor:
    """bf_op_pd_replace_u8 on two uint8 device tensors [B,H,W,C]: uint8 [B T, H, W, C], member b T + t = `base_u8` with a share
    `replace` of its pixels (all channels of a pixel) carrying the `noisy_u8` value; the masks depend on (seed, t, pixel) alone"""
    T, threshold, seed = A.int_in(copies, "copies", 1, MAX_COPIES), replace_threshold(replace), A.seed64(seed)
    A.image_batch(base_u8, "base_u8", (torch.uint8,))
    A.image_batch(noisy_u8, "noisy_u8", (torch.uint8,))
    if tuple(base_u8.shape) != tuple(noisy_u8.shape) or base_u8.device != noisy_u8.device:
        raise ValueError(f"base_u8 and noisy_u8 must have one shape and one device, got {tuple(base_u8.shape)} on {base_u8.device} "
                         f"and {tuple(noisy_u8.shape)} on {noisy_u8.device}")
    base_u8 = A.to_device(base_u8, False, None, "base_u8", _FEATURE).contiguous()
    noisy_u8 = noisy_u8.contiguous()
    B, H, W, C = base_u8.shape
    out = torch.empty((B * T, H, W, C), dtype=torch.uint8, device=base_u8.device)
    N.call("bf_op_pd_replace_u8", N.ptr(base_u8), N.ptr(noisy_u8), N.ptr(out), B, H, W, C, T, threshold, seed, N.stream_ptr(base_u8))
    return out


def pd_mean(members_f32: torch.Tensor, copies: int, cast_to_uint8: bool = True) -> torch.Tensor:
    """bf_op_pd_mean on a float32 device tensor [B T, H, W, C] as pd_replace_u8 orders it: the mean over t (fp64 sum in ascending t,
    one division), [B,H,W,C] float32, or clipped, rounded half to even and cast to uint8"""
    T = A.int_in(copies, "copies", 1, MAX_COPIES)
    A.image_batch(members_f32, "members_f32", (torch.float32,))
    N_, H, W, C = members_f32.shape
    if N_ % T:
        raise ValueError(f"members_f32 must hold a multiple of {T} images, got {tuple(members_f32.shape)}")
    members_f32 = A.to_device(members_f32, False, None, "members_f32", _FEATURE).contiguous()
    out = torch.empty((N_ // T, H, W, C), dtype=torch.uint8 if cast_to_uint8 else torch.float32, device=members_f32.device)
    N.call("bf_op_pd_mean", N.ptr(members_f32), N.ptr(out), int(bool(cast_to_uint8)), N_ // T, H, W, C, T, N.stream_ptr(members_f32))
    return out


# ---- the wrapper -------------------------------------------------------------------------------------------------------------

def checked_settings(stride: Union[int, str] = 2, max_stride: int = 4, threshold: float = 0.8, refine: int = 0, replace: float = 0.16,
                     seed: int = 0):
    """the settings of PixelShuffleDenoiserModule, checked: (stride or "auto", max_stride, threshold, refine, replace, seed)"""
    if not (isinstance(stride, str) and stride == "auto"):
        if isinstance(stride, str):
            raise ValueError(f'stride must be an int in 1..{MAX_STRIDE} or "auto", got {stride!r}')
        stride = _checked_stride(stride)
    replace_threshold(replace)
    return (stride, A.int_in(max_stride, "max_stride", 1, MAX_STRIDE), _checked_threshold(threshold),
            A.int_in(refine, "refine", 0, MAX_COPIES), float(replace), A.seed64(seed))


def parse_setting(pixel_shuffle) -> Optional[dict]:
    """load_model's `pixel_shuffle`: None | False -> None; True -> "auto"; an int or "auto" -> that stride; a dict of SETTINGS ->
    itself.  Everything is checked here, before anything is loaded."""
    def stride_of(value):
        return {"stride": "auto" if value is True else value} if isinstance(value, (int, str)) else None
    return A.parse_setting(pixel_shuffle, "pixel_shuffle", 'None, a bool, a stride, "auto" or a dict of PixelShuffleDenoiserModule settings',
                           SETTINGS, checked_settings, stride_of)


class PixelShuffleDenoiserModule(DenoiserWrapper):
    """A denoiser run on the s^2 sub-images of every s-th pixel, whose noise is correlated over 1 / s of the distance: uint8
    [B,H,W,C] -> uint8 [B,H,W,C] (float32, not rounded, with cast_to_uint8=False).  `module`, argument checks, input handling,
    return types, empty batches and f16-range status as every wrapper (DenoiserWrapper).

    A call is: pd_split_u8, ONE float denoiser call on [B s^2, Hs, Ws, C], pd_merge.  With `refine` = T > 0 the merged result is
    rounded to uint8, pd_replace_u8 makes T copies of it in which a share `replace` of the pixels carries the noisy input again
    (masks from `seed`), one more denoiser call runs on [B T, H, W, C] and pd_mean averages its results: the second stage sees the
    frame at full resolution and removes the aliasing the first one leaves, while the replaced pixels are too sparse to carry
    the correlation.

    `stride`: 1..8, or "auto": noise_correlation(image, max_stride, threshold) runs on the batch and the largest stride over its
    images is used, clamped to what H, W >= 2 s allows.  Reading that stride is the call's ONE host read (a synchronisation); a
    fixed stride has none.  The probe cannot tell correlated noise from fine texture of the image itself, which also rises with s:
    "auto" is for frames whose noise is well above their pixel-scale texture.  `last_stride` is what the last
    call of this module or of its float form used.  A stride of 1 with
    refine=0 returns exactly what the wrapped module returns."""
    SETTINGS = SETTINGS

    def __init__(self, module, stride: Union[int, str] = 2, max_stride: int = 4, threshold: float = 0.8, refine: int = 0,
                 replace: float = 0.16, seed: int = 0, cast_to_uint8: bool = True):
        if isinstance(module, PixelShuffleDenoiserModule):
            raise ValueError("module is already pixel-shuffled")
        self._wrap(module, cast_to_uint8)
        (self._stride, self._max_stride, self._threshold, self._refine, self._replace,
         self._seed) = checked_settings(stride, max_stride, threshold, refine, replace, seed)
        self._record = {"stride": None}

    @property
    def last_stride(self) -> Optional[int]:
        """the stride of the last call of this module or of its float form"""
        return self._record["stride"]

    def _stride_for(self, image: torch.Tensor) -> int:
        H, W = int(image.shape[1]), int(image.shape[2])
        if self._stride != "auto":
            return _checked_stride(self._stride, H, W)
        S = min(self._max_stride, H - 1, W - 1)
        if S < 1:
            return 1
        found = int(noise_correlation(image, S, self._threshold).stride.max())         # the one host read of a call
        return max(1, min(found, H // 2, W // 2))

    def __call__(self, image):
        image, was_numpy = self._checked_input(image)
        B, H, W, _ = image.shape
        if B == 0:
            return self._empty_output(image, was_numpy)
        if self._stride != "auto":
            _checked_stride(self._stride, H, W)                   # before the GPU is touched
        image = self._place(image, was_numpy, "image", _FEATURE)
        s = self._record["stride"] = self._stride_for(image)
        result = self._run(pd_split_u8(image, s))
        if self._repeat_in_fp32(was_numpy):
            return self(image.cpu().numpy())
        out = pd_merge(result.to(image.device), B, H, W, s, self._cast_to_uint8 or self._refine > 0)
        if self._refine > 0:
            result = self._run(pd_replace_u8(out, image, self._refine, self._replace, self._seed))
            if self._repeat_in_fp32(was_numpy):
                return self(image.cpu().numpy())
            out = pd_mean(result.to(image.device), self._refine, self._cast_to_uint8)
        return self._deliver(out, was_numpy)
