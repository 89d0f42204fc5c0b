"""
Blind degradations for training: what real photographs carry besides noise -- the 8x8 block artefacts of JPEG, lens or resampling
blur, coarse quantisation, missing pixels -- as three HIP kernels on the device (csrc/degrade.hip) behind an opt-in
`dataset.degradations` section.  The reference's dataset section names `random_blur`, `use_jpeg_noise`, `quantization` and
`inpaint_drop_rate` and its `prepare_data_fn` never uses them (dataset.py keeps that: PrepareData.ignored); this module is what a
user reaches for instead, and a configuration without the section yields exactly the batches it yielded before.

    degrade_jpeg(x, quality, subsampling)       an encode / decode round trip without entropy coding
    degrade_blur(x, sigma)                      a separable Gaussian with integer taps (gaussian_taps), borders clamped
    degrade_pointwise(x, step, drop_rate, seed) clip to 0..255, quantise to multiples of `step`, drop pixels at `drop_rate`

`x` is a uint8 or float32 device batch [B,H,W,C] of integer-valued samples, every parameter a number or one per image, the result
float32, integer-valued, in [0, 255].  The contracts (include/bfcnn_hip.h) are integer arithmetic, so a result is reproducible bit
for bit (tests/degrade_reference.py restates them in NumPy).  `Degradations` parses the configuration section and draws the
per-image parameters; `PrepareData` runs the stages.  DESIGN.md 7.14 has the contracts and the measurements.
"""
import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _args as A
from . import _native as N

_DTYPES = (torch.uint8, torch.float32)
_FEATURE = "the degradation kernels"
MAX_SIGMA, MAX_RADIUS, MAX_DROP_RATE, MAX_STEP = 4.0, 12, 0.9, 255
_TAPS = 2 * MAX_RADIUS + 1
_SUBSAMPLINGS = ("420", "444")


def gaussian_taps(sigma: float) -> np.ndarray:
    """the integer taps of the blur, int32 [2 r + 1]: r = max(1, int(3 sigma + 0.5)); g the normalised Gaussian in fp64;
    w = floor(65536 g + 0.5); the residual 65536 - sum w goes to the centre tap.  sigma = 0 is the single tap [65536]: the identity"""
    sigma = A.non_negative_float(sigma, "sigma", MAX_SIGMA)
    if sigma == 0.0:
        return np.array([65536], np.int32)
    r = max(1, int(3.0 * sigma + 0.5))
    k = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-(k * k) / (2.0 * sigma * sigma))
    g = g / g.sum()
    w = np.floor(65536.0 * g + 0.5).astype(np.int64)
    w[r] += 65536 - w.sum()
    return w.astype(np.int32)


def _per_image(value, B: int, what: str, lo, hi, integer: bool) -> np.ndarray:
    """a number or one per image, in lo..hi: int64 or float64 [B]"""
    if isinstance(value, torch.Tensor):
        value = value.detach().cpu().numpy()
    try:
        a = np.asarray(value)
    except (TypeError, ValueError):
        a = np.asarray(None)
    kinds = "iu" if integer else "iuf"
    if a.dtype.kind not in kinds or a.ndim > 1 or (a.ndim == 1 and a.shape[0] != B):
        raise ValueError(f"{what} must be {'an int' if integer else 'a number'} or one per image ({B}), got {value!r}")
    a = np.broadcast_to(a.astype(np.int64 if integer else np.float64), (B,))
    if not (np.isfinite(a) & (a >= lo) & (a <= hi)).all():
        raise ValueError(f"{what} must be in {lo}..{hi}, got {value!r}")
    return a


def _batch(x) -> torch.Tensor:
    A.image_batch(x, "x", _DTYPES)
    return A.to_device(x, False, None, "x", _FEATURE).contiguous()


def _upload(values: np.ndarray, device) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(values, dtype=np.int32)).to(device)


def _tap_table(sigma: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(int32 [B, 25] rows of taps, int32 [B] radii) of per-image sigmas"""
    taps, radius = np.zeros((len(sigma), _TAPS), np.int32), np.zeros(len(sigma), np.int32)
    cache = {}
    for b, s in enumerate(sigma):
        if float(s) not in cache:
            cache[float(s)] = gaussian_taps(float(s))
        w = cache[float(s)]
        taps[b, :len(w)], radius[b] = w, (len(w) - 1) // 2
    return taps, radius


# the launches on device parameter arrays (PrepareData uploads all of a batch's parameters at once)

def _launch_jpeg(x: torch.Tensor, quality: torch.Tensor, subsampling: int) -> torch.Tensor:
    B, H, W, C = x.shape
    if C not in (1, 3):
        raise ValueError(f"the JPEG round trip takes 1 or 3 channels, got {tuple(x.shape)}")
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    nbytes = N.lib().bf_op_degrade_jpeg_scratch_bytes(B, H, W, C, subsampling)
    if nbytes < 0:
        N.check(int(nbytes), None, "bf_op_degrade_jpeg_scratch_bytes")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=x.device) if nbytes else None
    N.call("bf_op_degrade_jpeg", N.ptr(x), int(x.dtype == torch.uint8), N.ptr(out), B, H, W, C, N.ptr(quality), subsampling,
           N.ptr(scratch), nbytes, N.stream_ptr(x))
    return out


def _launch_blur(x: torch.Tensor, taps: torch.Tensor, radius: torch.Tensor) -> torch.Tensor:
    B, H, W, C = x.shape
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    N.call("bf_op_degrade_blur", N.ptr(x), int(x.dtype == torch.uint8), N.ptr(out), B, H, W, C, N.ptr(taps), N.ptr(radius),
           N.stream_ptr(x))
    return out


def _launch_pointwise(x: torch.Tensor, step: torch.Tensor, threshold: torch.Tensor, seed: int, want_mask: bool = False):
    B, H, W, C = x.shape
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    mask = torch.empty((B, H, W), dtype=torch.uint8, device=x.device) if want_mask else None
    N.call("bf_op_degrade_pointwise", N.ptr(x), int(x.dtype == torch.uint8), N.ptr(out), N.ptr(mask), B, H, W, C, N.ptr(step),
           N.ptr(threshold), seed, N.stream_ptr(x))
    return out, mask


def _thresholds(rate: np.ndarray) -> np.ndarray:
    return np.floor(rate * 16777216.0).astype(np.int64)


def degrade_jpeg(x: torch.Tensor, quality, subsampling: str = "420") -> torch.Tensor:
    """bf_op_degrade_jpeg: the JPEG round trip of every image of `x` (1 or 3 channels) at `quality` 1..100 (a number or one per
    image; 0 leaves that image unencoded), chroma `subsampling` "420" or "444"; float32 [B,H,W,C]"""
    A.image_batch(x, "x", _DTYPES)
    quality = _per_image(quality, x.shape[0], "quality", 0, 100, True)
    subsampling = int(A.one_of(subsampling, "subsampling", _SUBSAMPLINGS))
    x = _batch(x)
    return _launch_jpeg(x, _upload(quality, x.device), subsampling)


def degrade_blur(x: torch.Tensor, sigma) -> torch.Tensor:
    """bf_op_degrade_blur: every image of `x` blurred by the Gaussian of `sigma` 0..4 grey-level-exact integer taps (a number or
    one per image; 0 passes that image through bit for bit); float32 [B,H,W,C]"""
    A.image_batch(x, "x", _DTYPES)
    taps, radius = _tap_table(_per_image(sigma, x.shape[0], "sigma", 0.0, MAX_SIGMA, False))
    x = _batch(x)
    params = _upload(np.concatenate([taps.reshape(-1), radius]), x.device)
    return _launch_blur(x, params[:taps.size], params[taps.size:])


def degrade_pointwise(x: torch.Tensor, step=1, drop_rate=0.0, seed: int = 0, return_mask: bool = False):
    """bf_op_degrade_pointwise: clip to 0..255, round to multiples of `step` 1..255 (255 at most), then drop pixels (all channels
    to 0) at `drop_rate` 0..0.9, drawn from Philox (seed, image, pixel); `step` and `drop_rate` a number or one per image.
    float32 [B,H,W,C], with `return_mask` also the uint8 [B,H,W] mask of the dropped pixels"""
    A.image_batch(x, "x", _DTYPES)
    B = x.shape[0]
    step = _per_image(step, B, "step", 1, MAX_STEP, True)
    rate = _per_image(drop_rate, B, "drop_rate", 0.0, MAX_DROP_RATE, False)
    seed = A.seed64(seed)
    x = _batch(x)
    params = _upload(np.concatenate([step, _thresholds(rate)]), x.device)
    out, mask = _launch_pointwise(x, params[:B], params[B:], seed, bool(return_mask))
    return (out, mask) if return_mask else out


# ---- the configuration section -------------------------------------------------------------------------------------------------

def _range(section: Dict, stage: str, key: str, lo, hi, integer: bool):
    """`key` of a stage as (min, max): a number or a list of numbers, each in lo..hi"""
    value = section[key]
    values = list(value) if isinstance(value, (list, tuple)) else [value]
    ok = (int, np.integer) if integer else (int, float, np.integer, np.floating)
    if not values or any(isinstance(v, bool) or not isinstance(v, ok) or not math.isfinite(v) or v < lo or v > hi for v in values):
        raise ValueError(f"degradations.{stage}.{key} must be {'ints' if integer else 'numbers'} in {lo}..{hi}, got {value!r}")
    return values


class Degradations:
    """The `dataset.degradations` section: up to four stages, each with a `probability` (per image, default 0.5) and its parameter --

        "blur":         {"sigma": [0.5, 3.0], "probability": 0.5}          sigma ~ U[min, max], 0..4
        "quantization": {"step": [2, 4, 8], "probability": 0.5}            one of the listed steps, 1..255
        "jpeg":         {"quality": [25, 75], "subsampling": "420", "probability": 0.5}     an integer of min..max, 1..100
        "drop":         {"rate": [0.0, 0.3], "probability": 0.5}           rate ~ U[min, max], 0..0.9

    Unknown keys and values out of range raise a ValueError that names the key.  `draw(B)` returns the parameters of B images from a
    generator of this object's own (PrepareData.draw keeps its keys and its sequence); an image a stage does not fire for gets the
    stage's neutral value (sigma 0, step 1, quality 0, rate 0)."""

    STAGES = {"blur": ("sigma",), "quantization": ("step",), "jpeg": ("quality", "subsampling"), "drop": ("rate",)}

    def __init__(self, config: Dict, seed: Optional[int] = None):
        if not isinstance(config, dict):
            raise ValueError(f"degradations must be a dict of stages, got {config!r}")
        for stage, section in config.items():
            if stage not in self.STAGES:
                raise ValueError(f"degradations.{stage}: unknown stage (known: {sorted(self.STAGES)})")
            if not isinstance(section, dict):
                raise ValueError(f"degradations.{stage} must be a dict, got {section!r}")
            for key in section:
                if key not in self.STAGES[stage] + ("probability",):
                    raise ValueError(f"degradations.{stage}.{key}: unknown key (known: {list(self.STAGES[stage]) + ['probability']})")
            for key in self.STAGES[stage]:
                if key not in section and key != "subsampling":
                    raise ValueError(f"degradations.{stage}.{key} is missing")
        self.probability = {}
        for stage in self.STAGES:
            p = config.get(stage, {}).get("probability", 0.5) if stage in config else 0.0
            if isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)) or not 0.0 <= p <= 1.0:
                raise ValueError(f"degradations.{stage}.probability must be a number in 0..1, got {p!r}")
            self.probability[stage] = float(p)
        self.sigma = self.steps = self.quality = self.rate = None
        self.subsampling = 420
        if "blur" in config:
            v = _range(config["blur"], "blur", "sigma", 0.0, MAX_SIGMA, False)
            self.sigma = (float(min(v)), float(max(v)))
        if "quantization" in config:
            self.steps = [int(s) for s in _range(config["quantization"], "quantization", "step", 1, MAX_STEP, True)]
        if "jpeg" in config:
            v = _range(config["jpeg"], "jpeg", "quality", 1, 100, True)
            self.quality = (int(min(v)), int(max(v)))
            sub = config["jpeg"].get("subsampling", "420")
            if not isinstance(sub, str) or sub not in _SUBSAMPLINGS:
                raise ValueError(f"degradations.jpeg.subsampling must be one of {list(_SUBSAMPLINGS)}, got {sub!r}")
            self.subsampling = int(sub)
        if "drop" in config:
            v = _range(config["drop"], "drop", "rate", 0.0, MAX_DROP_RATE, False)
            self.rate = (float(min(v)), float(max(v)))
        self.rng = np.random.default_rng(None if seed is None else [int(seed), 0x0DE6])

    def draw(self, B: int) -> Dict[str, np.ndarray]:
        """the parameters of B images: {"sigma": float64 [B], "step": int64 [B], "quality": int64 [B], "rate": float64 [B]}.  Every
        configured stage draws its coins and its values whether it fires or not, so the sequence does not depend on the outcome"""
        B = A.int_in(B, "B", 1)
        r = self.rng
        out = {"sigma": np.zeros(B), "step": np.ones(B, np.int64), "quality": np.zeros(B, np.int64), "rate": np.zeros(B)}
        if self.sigma is not None:
            fire, v = r.uniform(size=B) < self.probability["blur"], r.uniform(self.sigma[0], self.sigma[1], size=B)
            out["sigma"] = np.where(fire, v, 0.0)
        if self.steps is not None:
            fire, v = r.uniform(size=B) < self.probability["quantization"], r.choice(np.asarray(self.steps, np.int64), size=B)
            out["step"] = np.where(fire, v, 1)
        if self.quality is not None:
            fire, v = r.uniform(size=B) < self.probability["jpeg"], r.integers(self.quality[0], self.quality[1] + 1, size=B)
            out["quality"] = np.where(fire, v, 0)
        if self.rate is not None:
            fire, v = r.uniform(size=B) < self.probability["drop"], r.uniform(self.rate[0], self.rate[1], size=B)
            out["rate"] = np.where(fire, v, 0.0)
        return out

    def apply(self, noisy: torch.Tensor, params: Dict[str, np.ndarray], seed: int) -> torch.Tensor:
        """stages 4 to 6 on a noisy batch (the blur, stage 2, sits in front of the noise: PrepareData.__call__): clip and quantise,
        JPEG, drop -- one launch per stage that fires for some image of the batch, none for the others; quantisation and drop share
        a launch when no JPEG lies between them.  One upload carries the parameters of all of them"""
        B = noisy.shape[0]
        step, quality, thr = params["step"], params["quality"], _thresholds(params["rate"])
        quantise, jpeg, drop = bool((step > 1).any()), bool((quality > 0).any()), bool((thr > 0).any())
        if not (quantise or jpeg or drop):
            return noisy
        dev = _upload(np.concatenate([step, thr, np.ones(B, np.int64), np.zeros(B, np.int64), quality]), noisy.device)
        d_step, d_thr, d_one, d_zero, d_quality = (dev[i * B:(i + 1) * B] for i in range(5))
        if jpeg:
            if quantise:
                noisy, _ = _launch_pointwise(noisy, d_step, d_zero, 0)
            noisy = _launch_jpeg(noisy, d_quality, self.subsampling)
            if drop:
                noisy, _ = _launch_pointwise(noisy, d_one, d_thr, seed)
        else:
            noisy, _ = _launch_pointwise(noisy, d_step, d_thr, seed)
        return noisy

    def blur(self, clean: torch.Tensor, params: Dict[str, np.ndarray]) -> Optional[torch.Tensor]:
        """stage 2: the blurred batch, or None when the blur fires for no image of the batch (nothing is launched)"""
        if not (params["sigma"] > 0).any():
            return None
        taps, radius = _tap_table(params["sigma"])
        dev = _upload(np.concatenate([taps.reshape(-1), radius]), clean.device)
        return _launch_blur(clean, dev[:taps.size], dev[taps.size:])
