"""Video in front of a blind denoiser: a recursive motion-compensated temporal filter.  Per stream it keeps one accumulated frame and
one per-pixel frame count; every new frame warps that state onto itself along a block-matched motion field (`bf_burst_align` on the
pair (frame, image of the state)), drops the history wherever the warped state does not match, and blends with the count as the
weight (`bf_op_video_update`, csrc/video.hip).  The cost per frame is constant, the temporal support goes up to `n_max` frames, and a
scene cut or a moving object resets itself pixel by pixel.  The spatial denoiser runs on the filtered frame; the filter accumulates
the noisy frames, never the network's outputs: nothing feeds back.

The state of B parallel streams (VideoState): acc = uint16 [B,H,W,C], the accumulated frame times 256, in 0..65280; cnt = uint16
[B,H,W], the frames in a pixel times 256, 0 = empty; image = uint8 (acc + 128) >> 8, written by the update for the next alignment.
For a frame x, a field d on the 16 x 16 tiles of burst.py, thresholds (lo, hi) and n_max in 1..64, all integers:

    D      = sum over q in the 5 x 5 window around p (q clamped first), over channels, of (image_in(clamp(q + d)) - x(q))^2
    w      = 256 if D <= lo; 0 if D >= hi; else ((hi - D) 256) // (hi - lo)          (the ramp of burst_merge)
    s      = clamp(p + d);  n = min(cnt_in(s), 256 (n_max - 1));  m = (w n) >> 8;  den = 256 + m
    acc_out(p, c) = (65536 x(p, c) + m acc_in(s, c) + (den >> 1)) // den;  cnt_out(p) = den
    out(p, c)     = uint8 (acc_out + 128) >> 8 (the new state's image), or float32 acc_out / 256 (exact)

An empty state passes the first frame through, n_max = 1 passes every frame through, identical frames keep acc = 256 x while cnt
climbs to 256 n_max, and in the steady state a new frame has weight 1 / n_max.  There is no CPU execution path for the kernels."""
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _args as A
from . import _native as N
from . import burst as BU
from .module_denoiser import DenoiserWrapper
from .pixel_shuffle import pd_merge

_FEATURE = "the video code"
MAX_N = 64
SETTINGS = ("n_max", "levels", "search", "sigma", "k")


class VideoState(NamedTuple):
    """the temporal filter's state of B streams; `image` is (acc + 128) >> 8, what the next frame is aligned against"""
    acc: torch.Tensor                                             # uint16 [B,H,W,C]
    cnt: torch.Tensor                                             # uint16 [B,H,W]
    image: torch.Tensor                                           # uint8 [B,H,W,C]


# ---- argument checks ---------------------------------------------------------------------------------------------------------

def checked_settings(n_max: int = 8, levels: int = 3, search: int = 4, sigma=None, k=(1.5, 3.0)):
    """the settings of VideoDenoiserModule, checked: (n_max, levels, search, sigma, (k_lo, k_hi))"""
    return (A.int_in(n_max, "n_max", 1, MAX_N), A.int_in(levels, "levels", 1, BU.MAX_LEVELS), A.int_in(search, "search", 1, BU.MAX_SEARCH),
            BU._checked_sigma(sigma), BU._checked_k(k))


def parse_setting(video) -> Optional[dict]:
    """load_model's `video`: None | False -> None; True -> the defaults; a dict of SETTINGS -> itself.  Everything is checked
    here, before anything is loaded."""
    return A.parse_setting(video, "video", "None, a bool or a dict of VideoDenoiserModule settings", SETTINGS, checked_settings)


def _checked_state(state, shape, device) -> VideoState:
    B, H, W, C = shape
    if not isinstance(state, tuple) or len(state) != 3 or not all(isinstance(t, torch.Tensor) for t in state):
        raise ValueError(f"state must be a VideoState (acc, cnt, image) of tensors, got {type(state)}")
    for t, what, dtype, want in ((state[0], "acc", torch.uint16, (B, H, W, C)), (state[1], "cnt", torch.uint16, (B, H, W)),
                                 (state[2], "image", torch.uint8, (B, H, W, C))):
        if t.dtype != dtype or tuple(t.shape) != want:
            raise ValueError(f"state.{what} must be a {dtype} tensor {want} for this frame, got {A._got(t)}")
        if device is not None and t.device != device:
            raise ValueError(f"state.{what} must live on the frame's device {device}, got {t.device}")
    return VideoState(*state)


# ---- the kernel --------------------------------------------------------------------------------------------------------------

def video_state(B: int, H: int, W: int, C: int, device=None) -> VideoState:
    """the empty state of B streams of H x W x C frames on `device` (None: the current GPU): the first frame passes through"""
    B, H, W, C = A.int_in(B, "B", 0), A.int_in(H, "H", 1), A.int_in(W, "W", 1), A.int_in(C, "C", 1, 4)
    device = A.device_of(None, _FEATURE) if device is None else torch.device(device)
    zeros16 = lambda *shape: torch.zeros(shape, dtype=torch.int16, device=device).view(torch.uint16)       # the same bits
    return VideoState(zeros16(B, H, W, C), zeros16(B, H, W), torch.zeros((B, H, W, C), dtype=torch.uint8, device=device))


def _update(x: torch.Tensor, state: VideoState, field: torch.Tensor, thresholds: torch.Tensor, n_max: int, cast_to_uint8: bool):
    B, H, W, C = x.shape
    acc, cnt, image = torch.empty_like(state.acc), torch.empty_like(state.cnt), torch.empty_like(x)
    out = None if cast_to_uint8 else torch.empty((B, H, W, C), dtype=torch.float32, device=x.device)
    N.call("bf_op_video_update", N.ptr(x), N.ptr(state.acc), N.ptr(state.cnt), N.ptr(field), N.ptr(thresholds), B, H, W, C, n_max,
           N.ptr(acc), N.ptr(cnt), N.ptr(image), N.ptr(out), N.stream_ptr(x))
    return (image if cast_to_uint8 else out), VideoState(acc, cnt, image)


def video_update(x, state: VideoState, field: torch.Tensor, thresholds: torch.Tensor, n_max: int = 8, cast_to_uint8: bool = True):
    """bf_op_video_update: one step of the filter.  `x`: the next frame of B streams, uint8 [B,H,W,C] (torch on the GPU, or NumPy,
    which is uploaded); `state`: a VideoState on the device (video_state, or what the last step returned; only acc and cnt are
    read: the image is derived from acc); `field`: int32 [B,ceil(H/16),ceil(W/16),2], any displacements; `thresholds`: int64 [B,2],
    lo < hi.  Returns (out, new_state): out is the new state's uint8 image, or float32 acc / 256.  Not in place: the state given
    stays as it was."""
    n_max = A.int_in(n_max, "n_max", 1, MAX_N)
    x, was_numpy = A.host_or_device(x, "x", (torch.uint8,), allow_empty=True)
    B, H, W, C = x.shape
    want = (B,) + BU.grid_shape(H, W) + (2,)
    if not isinstance(field, torch.Tensor) or field.dtype != torch.int32 or tuple(field.shape) != want:
        raise ValueError(f"field must be an int32 tensor {want} for this frame, got {A._got(field)}")
    if not isinstance(thresholds, torch.Tensor) or thresholds.dtype != torch.int64 or tuple(thresholds.shape) != (B, 2):
        raise ValueError(f"thresholds must be an int64 tensor {(B, 2)} for this frame, got {A._got(thresholds)}")
    state = _checked_state(state, (B, H, W, C), None)
    if B == 0:
        out = torch.empty((0, H, W, C), dtype=torch.uint8 if cast_to_uint8 else torch.float32, device=x.device)
        return out, state
    x = A.to_device(x, was_numpy, None, "x", _FEATURE).contiguous()
    for t, what in ((field, "field"), (thresholds, "thresholds"), (state.acc, "state.acc"), (state.cnt, "state.cnt")):
        if t.device != x.device:
            raise ValueError(f"{what} must live on the frame's device {x.device}, got {t.device}")
    state = VideoState(state.acc.contiguous(), state.cnt.contiguous(), state.image)
    return _update(x, state, field.contiguous(), thresholds.contiguous(), n_max, bool(cast_to_uint8))


# ---- the wrapper -------------------------------------------------------------------------------------------------------------

class VideoDenoiserModule(DenoiserWrapper):
    """The next frame of B parallel streams, temporally filtered, then denoised: uint8 [B,H,W,C] -> uint8 [B,H,W,C] (float32, not
    rounded, with cast_to_uint8=False).  `module`: what every wrapper takes (DenoiserWrapper), or None for the temporal filter
    alone; a burst or video wrapper is refused.  Input handling, return types and empty batches as every wrapper.

    A call is: burst_align of the state's image against the frame, video_update with thresholds from burst_thresholds, ONE float
    denoiser call on the new state's uint8 image, rounding.  The first frame after reset(), and every frame with n_max = 1, returns
    exactly what the wrapped module returns for it.  `sigma`: the noise level the thresholds are made from; None estimates it per
    frame (estimate_noise, "mad") on the device with no host read; a float or a [B] array is taken as given.  Nothing in a call
    with a device tensor synchronises; with a fixed sigma a call can be captured into a HIP graph (the step is not in place: a
    replay reads the state the capture read, and the module keeps that state alive for as long as it lives itself).

    The module holds the state: `reset()` empties it, and a frame of another shape, batch size or device raises ValueError until then.
    `last_counts` is the uint16 [B,H,W] cnt of the last call of this module or of its float form (cnt / 256 frames are in a
    pixel), `last_field` that call's alignment, `state` the VideoState.  `check_status` is the wrapped module's; a host-array call
    that hits the f16 range switches the model to the exact-fp32 kernels and repeats the denoiser on the same filtered frame: the
    state advances once."""
    SETTINGS = SETTINGS

    def __init__(self, module, n_max: int = 8, levels: int = 3, search: int = 4, sigma=None, k=(1.5, 3.0), cast_to_uint8: bool = True):
        if isinstance(module, (BU.BurstDenoiserModule, VideoDenoiserModule)):
            raise ValueError("module already merges frames: a burst or video wrapper goes outermost")
        self._wrap(module, cast_to_uint8, allow_none=True)
        self._n_max, self._levels, self._search, self._sigma, self._k = checked_settings(n_max, levels, search, sigma, k)
        self._record = {"state": None, "field": None, "captured": []}          # float_form() shares it: the STATE too

    @property
    def state(self) -> Optional[VideoState]:
        return self._record["state"]

    @property
    def last_counts(self) -> Optional[torch.Tensor]:
        return None if self._record["state"] is None else self._record["state"].cnt

    @property
    def last_field(self) -> Optional[torch.Tensor]:
        return self._record["field"]

    def reset(self) -> None:
        """empties the state: the next frame passes the temporal filter unchanged, and may have another shape"""
        self._record["state"] = self._record["field"] = None

    def _checked_frame(self, x, what: str = "frame"):
        x, was_numpy = A.host_or_device(x, what, (torch.uint8,), allow_empty=True)
        if self._base is not None:
            self._base._checked_input(x)                          # the model's channel count
        B = int(x.shape[0])
        if B > 0:
            BU._check_sigma_batch(self._sigma, B)
        state = self._record["state"]
        if state is not None and B > 0 and tuple(state.acc.shape) != tuple(x.shape):
            raise ValueError(f"the state holds streams of shape {tuple(state.acc.shape)}, got a {what} of {tuple(x.shape)}: reset() first")
        return x, was_numpy

    def _filter(self, x: torch.Tensor, to_uint8: bool) -> torch.Tensor:
        """the temporal step on a contiguous device frame: advances the state, returns the filtered frame"""
        B, H, W, C = x.shape
        state = self._record["state"]
        if state is None:
            state = video_state(B, H, W, C, x.device)
        elif state.acc.device != x.device:
            raise ValueError(f"the state lives on {state.acc.device}, got a frame on {x.device}: reset() first")
        if x.is_cuda and torch.cuda.is_current_stream_capturing():
            # a replay reads the state this call reads, by address, and nothing else may own it once the new state replaces it:
            # keep it for the life of the module (reset() does not drop it), or the allocator hands its memory to the next tensor
            self._record["captured"].append(state)
        field = BU._align(torch.stack([x, state.image], dim=1), 0, self._levels, self._search)[0][:, 1].contiguous()
        out, state = _update(x, state, field, BU.thresholds_of(self._sigma, self._k, x), self._n_max, to_uint8)
        self._record["state"], self._record["field"] = state, field
        return out

    def _denoise(self, filtered: torch.Tensor, wait: bool) -> torch.Tensor:
        """the float denoiser on the filtered uint8 frame; with `wait` the f16-range repeat of a host-array call"""
        result = self._run(filtered)
        if wait and not self.check_status(wait=True):
            # an activation left the f16 range: the model now runs the exact-fp32 kernels (check_status switched it).  Repeat the
            # denoiser on the same filtered frame, not the call: the state has advanced once
            result = self._run(filtered)
            self.check_status(wait=True)
        return result

    def __call__(self, frame):
        x, was_numpy = self._checked_frame(frame)
        B, H, W, C = x.shape
        if B == 0:
            return self._empty_output(x, was_numpy)
        x = self._place(x, was_numpy, "frame", _FEATURE)
        filtered = self._filter(x, self._cast_to_uint8 or self._module is not None)          # the denoiser reads uint8
        if self._module is None:
            return self._deliver(filtered, was_numpy)
        result = self._denoise(filtered, was_numpy)
        out = pd_merge(result.to(x.device), B, H, W, 1, True) if self._cast_to_uint8 else result        # stride 1: the rounding alone
        return self._deliver(out, was_numpy)

    def denoise_sequence(self, frames):
        """reset(), then the T frames of uint8 [B,T,H,W,C] (torch on the GPU, or NumPy, which is uploaded once) one after the other:
        [B,T,H,W,C] of the module's output type.  The state is left after the last frame."""
        was_numpy = isinstance(frames, np.ndarray)
        if was_numpy and frames.dtype == np.uint8:
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 5 or frames.shape[1] < 1:
            raise ValueError(f"frames must be a [B,T,H,W,C] sequence of dtype torch.uint8 with T >= 1, got {A._got(frames)}")
        self.reset()
        self._checked_frame(frames[:, 0], "frames")
        B, T, H, W, C = frames.shape
        if B == 0:
            out = torch.empty((0, T, H, W, C), dtype=torch.uint8 if self._cast_to_uint8 else torch.float32)
            return out.numpy() if was_numpy else out
        frames = self._place(frames, was_numpy, "frame", _FEATURE)
        outs = [self(frames[:, t].contiguous()) for t in range(T)]
        if was_numpy and not self.check_status(wait=True):
            # an activation left the f16 range somewhere in the sequence: the model now runs the exact-fp32 kernels; run the
            # sequence again from the empty state
            self.reset()
            outs = [self(frames[:, t].contiguous()) for t in range(T)]
            self.check_status(wait=True)
        return self._deliver(torch.stack(outs, dim=1), was_numpy)
