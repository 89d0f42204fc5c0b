"""Burst merge in front of a blind denoiser: the T frames of a burst are aligned to one of them by block matching on a luma
pyramid and averaged along the alignment with weights that drop what does not match (after Hasinoff et al., "Burst photography
for high dynamic range and low-light imaging on mobile cameras", SIGGRAPH Asia 2016, in the spatial domain).  Averaging N aligned
frames cuts the noise variance to 1 / N before any network runs; the merged frame's noise is lower and varies over the frame,
which a blind denoiser does not need to be told.  Two entry points of csrc/burst.hip carry everything that is not the denoiser.

frames = uint8 [B,T,H,W,C], 1 <= T <= 16, reference index `ref`; clamp(p) clips a coordinate to the frame.  All integers:

    luma      L_0 = (2 sum_c x_c + C) // (2 C) as uint8; level k + 1 is ceil(H_k / 2) x ceil(W_k / 2), each value (the sum of the
              2 x 2 cell at (2 y, 2 x), coordinates clamped, + 2) >> 2; `levels` K in 1..4
    align     (`bf_burst_align`) tiles of 16 x 16 at every level, grid gy_k x gx_k = ceil(H_k / 16) x ceil(W_k / 16), edge tiles cut
              by the frame; coarsest level first; tile (i, j) of level k starts from
              d0 = 2 d_{k+1}[min(i >> 1, gy_{k+1} - 1), min(j >> 1, gx_{k+1} - 1)] (0 at the coarsest level) and takes among
              d = d0 + (u, v), u, v in -R..R (`search` R in 1..7) the smallest key (cost, u u + v v, u, v), lexicographically,
              cost(d) = sum over the tile's pixels p of |L_ref(p) - L_alt(clamp(p + d))|.
              The field is int32 [B,T,gy_0,gx_0,2] as (dy, dx), zero for t == ref; the reach is R (2^K - 1) pixels.
    merge     (`bf_op_burst_merge`) pixel p in tile (p_y // 16, p_x // 16) with displacement d_t:
              D_t = sum over q in the 5 x 5 window around p (q clamped first), over channels, of (alt_t(clamp(q + d_t)) - ref(q))^2
              w_t = 256 if D_t <= lo; 0 if D_t >= hi; else ((hi - D_t) 256) // (hi - lo);  w_ref = 256  (lo < hi int64 per image)
              num_c = sum_t w_t alt_t,c(clamp(p + d_t)), den = sum_t w_t, sq = sum_t w_t^2
              out = float32(float64(num_c) / float64(den)), or that float32 rounded half to even to uint8;
              counts = int32 [B,H,W,2] = (den, sq): the merged pixel's noise is sigma sqrt(sq) / den
    thresholds  E = ((sigma sigma) 2.0) (25 C) in fp64, the expectation of D_t for an aligned static pixel under white noise of
              sigma; lo = floor(k_lo E), hi = floor(k_hi E) + 1.  sigma = 0: only identical windows merge.

There is no CPU execution path for the kernels; `burst_thresholds` is tensor arithmetic and runs where its sigma lives."""
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _args as A
from . import _native as N
from .module_denoiser import DenoiserWrapper
from .noise_estimate import estimate_noise
from .pixel_shuffle import pd_merge

_FEATURE = "the burst code"
TILE = 16
MAX_FRAMES = 16
MAX_LEVELS = 4
MAX_SEARCH = 7
SETTINGS = ("reference", "levels", "search", "sigma", "k")


# ---- argument checks ---------------------------------------------------------------------------------------------------------

def _checked_frames(frames, what: str = "frames") -> Tuple[torch.Tensor, bool]:
    """a uint8 [B,T,H,W,C] burst, torch or NumPy (wrapped, not uploaded): (the tensor, whether NumPy was given)"""
    was_numpy = isinstance(frames, np.ndarray)
    if was_numpy and frames.dtype == np.uint8:
        frames = torch.from_numpy(np.ascontiguousarray(frames))
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 5:
        raise ValueError(f"{what} must be a [B,T,H,W,C] burst of dtype torch.uint8, got {A._got(frames)}")
    B, T, H, W, C = frames.shape
    if not 1 <= T <= MAX_FRAMES:
        raise ValueError(f"{what} must hold 1..{MAX_FRAMES} frames per burst, got {tuple(frames.shape)}")
    if not 1 <= C <= 4 or H < 1 or W < 1:
        raise ValueError(f"{what} must have 1..4 channels and at least 1 x 1 pixels, got {tuple(frames.shape)}")
    return frames, was_numpy


def _checked_reference(reference, T: Optional[int] = None) -> int:
    ref = A.int_in(reference, "reference", 0, MAX_FRAMES - 1)
    if T is not None and ref >= T:
        raise ValueError(f"reference must be an int in 0..{T - 1} for bursts of {T} frames, got {ref}")
    return ref


def _checked_k(k) -> Tuple[float, float]:
    if not isinstance(k, (tuple, list)) or len(k) != 2:
        raise ValueError(f"k must be a pair (k_lo, k_hi), got {k!r}")
    k_lo, k_hi = A.non_negative_float(k[0], "k_lo"), A.non_negative_float(k[1], "k_hi")
    if not k_lo < k_hi:
        raise ValueError(f"k_lo < k_hi does not hold: k = ({k_lo}, {k_hi})")
    return k_lo, k_hi


def _checked_sigma(sigma):
    """None (estimate per call), a float, or a [B] array / tensor, finite and non-negative"""
    if sigma is None:
        return None
    if isinstance(sigma, (torch.Tensor, np.ndarray, list, tuple)):
        s = torch.as_tensor(sigma).to(torch.float64)
        if s.dim() != 1:
            raise ValueError(f"sigma must be None, a float or a [B] array, got shape {tuple(s.shape)}")
        return s
    return A.non_negative_float(sigma, "sigma")


def checked_settings(reference: int = 0, levels: int = 3, search: int = 4, sigma=None, k=(1.5, 3.0)):
    """the settings of BurstDenoiserModule, checked: (reference, levels, search, sigma, (k_lo, k_hi))"""
    return (_checked_reference(reference), A.int_in(levels, "levels", 1, MAX_LEVELS), A.int_in(search, "search", 1, MAX_SEARCH),
            _checked_sigma(sigma), _checked_k(k))


def parse_setting(burst) -> Optional[dict]:
    """load_model's `burst`: None | False -> None; True -> the defaults; a dict of SETTINGS -> itself.  Everything is checked
    here, before anything is loaded."""
    return A.parse_setting(burst, "burst", "None, a bool or a dict of BurstDenoiserModule settings", SETTINGS, checked_settings)


def _check_sigma_batch(sigma, B: int):
    if isinstance(sigma, torch.Tensor) and tuple(sigma.shape) != (B,):
        raise ValueError(f"sigma must be None, a float or a [{B}] array for this batch, got shape {tuple(sigma.shape)}")


# ---- the kernels -------------------------------------------------------------------------------------------------------------

def level_shapes(H: int, W: int, levels: int) -> List[Tuple[int, int]]:
    """(H_k, W_k) of the luma levels 0..levels-1"""
    shapes = [(H, W)]
    for _ in range(1, levels):
        shapes.append((-(shapes[-1][0] // -2), -(shapes[-1][1] // -2)))
    return shapes


def grid_shape(H: int, W: int) -> Tuple[int, int]:
    """(gy, gx) of the alignment field of an H x W frame"""
    return -(H // -TILE), -(W // -TILE)


def _on_device(frames: torch.Tensor, was_numpy: bool, what: str = "frames") -> torch.Tensor:
    return A.to_device(frames, was_numpy, None, what, _FEATURE).contiguous()


def _align(frames: torch.Tensor, ref: int, K: int, R: int) -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """bf_burst_align on a contiguous device burst: (the field, views of the luma levels in the call's scratch)"""
    B, T, H, W, C = frames.shape
    scratch, nbytes = N.scratch("bf_burst_align", frames.device, B, T, H, W, C, K)
    field = torch.empty((B, T) + grid_shape(H, W) + (2,), dtype=torch.int32, device=frames.device)
    N.call("bf_burst_align", N.ptr(frames), B, T, H, W, C, ref, K, R, N.ptr(scratch), nbytes, N.ptr(field), N.stream_ptr(frames))
    raw, views, offset = scratch.view(torch.uint8), [], 0
    for h, w in level_shapes(H, W, K):                           # the layout of include/bfcnn_hip.h: every part padded to 16 bytes
        views.append(raw[offset:offset + B * T * h * w].view(B, T, h, w))
        offset += -((B * T * h * w) // -16) * 16
    return field, views


def burst_pyramid(frames, levels: int = 3) -> List[torch.Tensor]:
    """the luma levels bf_burst_align works on, for a uint8 [B,T,H,W,C] burst (torch on the GPU, or NumPy, which is uploaded):
    uint8 device tensors [B,T,H_k,W_k], k = 0..levels-1, views of one scratch buffer"""
    K = A.int_in(levels, "levels", 1, MAX_LEVELS)
    frames, was_numpy = _checked_frames(frames)
    if frames.shape[0] == 0:
        return [torch.empty((0, frames.shape[1], h, w), dtype=torch.uint8, device=frames.device)
                for h, w in level_shapes(frames.shape[2], frames.shape[3], K)]
    return _align(_on_device(frames, was_numpy), 0, K, 1)[1]


def burst_align(frames, reference: int = 0, levels: int = 3, search: int = 4) -> torch.Tensor:
    """bf_burst_align: the alignment field of a uint8 [B,T,H,W,C] burst (torch on the GPU, or NumPy, which is uploaded) against
    its frame `reference`, int32 [B,T,ceil(H/16),ceil(W/16),2] as (dy, dx) on the device: frame t at p + d matches the reference
    at p.  Zero for t == reference.  Displacements up to search (2^levels - 1) pixels are within reach."""
    K, R = A.int_in(levels, "levels", 1, MAX_LEVELS), A.int_in(search, "search", 1, MAX_SEARCH)
    frames, was_numpy = _checked_frames(frames)
    ref = _checked_reference(reference, frames.shape[1])
    if frames.shape[0] == 0:
        return torch.empty((0, frames.shape[1]) + grid_shape(frames.shape[2], frames.shape[3]) + (2,), dtype=torch.int32,
                           device=frames.device)
    return _align(_on_device(frames, was_numpy), ref, K, R)[0]


def burst_thresholds(sigma, C: int, k_lo: float = 1.5, k_hi: float = 3.0) -> torch.Tensor:
    """the merge thresholds of noise levels sigma [B] (a tensor where it lives, else anything torch.as_tensor takes), int64 [B,2] =
    (lo, hi) on sigma's device: E = ((sigma sigma) 2.0) (25 C) in fp64, lo = floor(k_lo E), hi = floor(k_hi E) + 1.  Tensor
    arithmetic: nothing synchronises."""
    C = A.int_in(C, "C", 1, 4)
    k_lo, k_hi = _checked_k((k_lo, k_hi))
    s = torch.as_tensor(sigma).to(torch.float64)
    if s.dim() != 1:
        raise ValueError(f"sigma must be a [B] array, got shape {tuple(s.shape)}")
    E = ((s * s) * 2.0) * float(25 * C)
    return torch.stack([torch.floor(k_lo * E).to(torch.int64), torch.floor(k_hi * E).to(torch.int64) + 1], dim=1).contiguous()


def thresholds_of(sigma, k, frame: torch.Tensor) -> torch.Tensor:
    """burst_thresholds for a uint8 [B,H,W,C] device frame from a checked `sigma` setting: None estimates the level on that
    frame (estimate_noise, "mad"; no host read), a float is filled in, a [B] tensor is moved to the frame"""
    B, C = int(frame.shape[0]), int(frame.shape[3])
    if sigma is None:
        sigma = estimate_noise(frame.contiguous(), "mad")
    elif isinstance(sigma, torch.Tensor):
        _check_sigma_batch(sigma, B)
        sigma = sigma.to(frame.device)
    else:
        sigma = torch.full((B,), sigma, dtype=torch.float64, device=frame.device)
    return burst_thresholds(sigma, C, *k)


def _merge(frames: torch.Tensor, field: torch.Tensor, thresholds: torch.Tensor, ref: int, cast_to_uint8: bool, want_counts: bool):
    B, T, H, W, C = frames.shape
    out = torch.empty((B, H, W, C), dtype=torch.uint8 if cast_to_uint8 else torch.float32, device=frames.device)
    counts = torch.empty((B, H, W, 2), dtype=torch.int32, device=frames.device) if want_counts else None
    N.call("bf_op_burst_merge", N.ptr(frames), N.ptr(field), N.ptr(thresholds), B, T, H, W, C, ref, N.ptr(out), int(cast_to_uint8),
           N.ptr(counts), N.stream_ptr(frames))
    return out, counts


def burst_merge(frames, field: torch.Tensor, thresholds: torch.Tensor, reference: int = 0, cast_to_uint8: bool = True,
                return_counts: bool = False):
    """bf_op_burst_merge: the robust mean of a uint8 [B,T,H,W,C] burst (torch on the GPU, or NumPy, which is uploaded) along
    `field` (int32 [B,T,ceil(H/16),ceil(W/16),2], any displacements) under `thresholds` (int64 [B,2], lo < hi), both on the device:
    uint8 [B,H,W,C], or float32 before the rounding; with `return_counts` (out, counts int32 [B,H,W,2] = (den, sq))."""
    frames, was_numpy = _checked_frames(frames)
    B, T, H, W, C = frames.shape
    ref = _checked_reference(reference, T)
    want = (B, T) + grid_shape(H, W) + (2,)
    if not isinstance(field, torch.Tensor) or field.dtype != torch.int32 or tuple(field.shape) != want:
        raise ValueError(f"field must be an int32 tensor {want} for this burst, got {A._got(field)}")
    if not isinstance(thresholds, torch.Tensor) or thresholds.dtype != torch.int64 or tuple(thresholds.shape) != (B, 2):
        raise ValueError(f"thresholds must be an int64 tensor {(B, 2)} for this burst, got {A._got(thresholds)}")
    if B == 0:
        out = torch.empty((0, H, W, C), dtype=torch.uint8 if cast_to_uint8 else torch.float32, device=frames.device)
        return (out, torch.empty((0, H, W, 2), dtype=torch.int32, device=frames.device)) if return_counts else out
    frames = _on_device(frames, was_numpy)
    for t, what in ((field, "field"), (thresholds, "thresholds")):
        if t.device != frames.device:
            raise ValueError(f"{what} must live on the frames' device {frames.device}, got {t.device}")
    out, counts = _merge(frames, field.contiguous(), thresholds.contiguous(), ref, bool(cast_to_uint8), bool(return_counts))
    return (out, counts) if return_counts else out


# ---- the wrapper -------------------------------------------------------------------------------------------------------------

class BurstDenoiserModule(DenoiserWrapper):
    """A burst merged into one frame, then denoised: uint8 [B,T,H,W,C] -> uint8 [B,H,W,C] (float32, not rounded, with
    cast_to_uint8=False).  `module`: what every wrapper takes (DenoiserWrapper), or None for the merge alone.  Input handling,
    return types, empty batches and f16-range status as every wrapper.

    A call is: burst_align against frame `reference`, burst_merge to uint8, ONE float denoiser call on the merged [B,H,W,C],
    rounding.  A burst of one frame returns exactly what the wrapped module returns for that frame.  `sigma`: the noise level the
    thresholds are made from; None estimates it per image from the reference frames (estimate_noise, "mad") on the device with no
    host read; a float or a [B] array is taken as given.  `k` = (k_lo, k_hi) of burst_thresholds.  Nothing in a call with a
    device tensor synchronises: with a fixed sigma the whole call can be captured into a HIP graph.

    `last_counts` is the int32 [B,H,W,2] = (den, sq) of the last call of this module or of its float form (None after a burst of
    one frame): den / 256 frames went into a pixel, and its noise is sigma sqrt(sq) / den.  `last_field` is that call's alignment."""
    SETTINGS = SETTINGS

    def __init__(self, module, reference: int = 0, levels: int = 3, search: int = 4, sigma=None, k=(1.5, 3.0),
                 cast_to_uint8: bool = True):
        if isinstance(module, BurstDenoiserModule):
            raise ValueError("module already merges bursts")
        self._wrap(module, cast_to_uint8, allow_none=True)
        self._reference, self._levels, self._search, self._sigma, self._k = checked_settings(reference, levels, search, sigma, k)
        self._record = {"counts": None, "field": None}

    @property
    def last_counts(self) -> Optional[torch.Tensor]:
        return self._record["counts"]

    @property
    def last_field(self) -> Optional[torch.Tensor]:
        return self._record["field"]

    def __call__(self, frames):
        frames, was_numpy = _checked_frames(frames)
        B, T, H, W, C = frames.shape
        ref = _checked_reference(self._reference, T)
        if self._base is not None:
            self._base._checked_input(frames[:, ref])              # the model's channel count
        if B == 0:
            return self._empty_output(frames[:, ref], was_numpy)
        _check_sigma_batch(self._sigma, B)
        if T == 1 and self._cast_to_uint8 and callable(getattr(self._module, "float_form", None)):
            return self._module(frames[:, 0].numpy() if was_numpy else frames[:, 0])       # exactly the wrapped module
        frames = self._place(frames, was_numpy, "frames", _FEATURE)
        to_uint8 = self._cast_to_uint8 or self._module is not None               # the denoiser reads uint8
        if T == 1:
            field = counts = None
            merged = frames[:, 0].contiguous() if to_uint8 else frames[:, 0].float()
        else:
            field = _align(frames, ref, self._levels, self._search)[0]
            merged, counts = _merge(frames, field, thresholds_of(self._sigma, self._k, frames[:, ref]), ref, to_uint8, True)
        self._record["counts"], self._record["field"] = counts, field
        if self._module is None:
            return self._deliver(merged, was_numpy)
        result = self._run(merged)
        if self._repeat_in_fp32(was_numpy):
            return self(frames.cpu().numpy())
        out = pd_merge(result.to(frames.device), B, H, W, 1, True) if self._cast_to_uint8 else result       # stride 1: the rounding alone
        return self._deliver(out, was_numpy)
