"""Non-local means: a denoiser without weights (Buades, Coll, Morel, "A non-local algorithm for image denoising", CVPR 2005; the
parameters follow their IPOL 2011 article).  Every pixel becomes the mean of the pixels of its search window, weighted by how
alike their patches are.  It takes any channel count 1..4 and any noise level, and its one parameter scales with the noise level
the package estimates on the device: the baseline to put a network's numbers next to, and something to call where no trained
network fits.  One entry point of csrc/nlm.hip carries it.

images = uint8 [B,H,W,C]; patch radius p in 1..3, search radius r in 1..10; n = C (2 p + 1)^2; P = the image with edge replication.

    table     TABLE[i] = rint(4096 exp(-(i + 0.5) 9 / 1024)) for i < 1023, TABLE[1023] = 0: int32 [1024], built here in fp64
    pixel x   for every offset d != 0, |dy|, |dx| <= r, with q = x + d inside the frame (candidates outside are left out):
              D = sum over c and |u|, |v| <= p of (P[x + (u,v), c] - P[q + (u,v), c])^2
              a = max(D - offset, 0);  idx = min((a mult) >> 32, 1023);  w = TABLE[idx]
              (mult == 2^32 - 1, the clamp: every w is 0 and the image comes back unchanged -- the filter is off when its
              bandwidth is below the table's resolution)
              w_c = max(1, max_q w);  num_c = sum_q w I[q,c] + w_c I[x,c];  den = sum_q w + w_c
              out = float32(float64(num_c) / float64(den)), or uint8 (2 num_c + den) // (2 den);  weights = den, int32 [B,H,W]
    params    int64 [B,2] = (offset, mult) per image, from sigma [B] in fp64: v = sigma sigma, offset = floor((v 2.0) n),
              g = ((strength strength) v) n, mult = floor(min((2^32 1024 / 9) / g, 2^32 - 1)) (g = 0 gives the clamp).

That is w = 4096 exp(-max(D / n - 2 sigma^2, 0) / (strength sigma)^2), cut off at exp(-9).  Integer arithmetic up to the one
division: the results are those of NumPy bit for bit (tests/nlm_reference.py).

There is no CPU execution path for the kernel; `nlm_params` is tensor arithmetic and runs where its sigma lives."""
from typing import Optional, Tuple

import numpy as np
import torch

from . import _args as A
from . import _native as N
from .module_denoiser import DenoiserWrapper
from .noise_estimate import estimate_noise
from .risk import estimate_risk

_FEATURE = "non-local means"
TABLE_SIZE, ONE, CUTOFF = 1024, 4096, 9.0
MAX_PATCH, MAX_SEARCH = 3, 10
MULT_OFF = 2 ** 32 - 1
_MULT_SCALE = (2.0 ** 32 * TABLE_SIZE) / CUTOFF
STRENGTHS = (0.25, 0.4, 0.55, 0.75, 1.0, 1.4)
SETTINGS = ("sigma", "patch", "search", "strength")
MODEL_NAME = "nlm"

_tables = {}                                                      # device -> the uploaded table


def nlm_table() -> np.ndarray:
    """the weight table, int32 [1024]"""
    i = np.arange(TABLE_SIZE, dtype=np.float64)
    table = np.rint(ONE * np.exp(-(i + 0.5) * CUTOFF / TABLE_SIZE)).astype(np.int32)
    table[-1] = 0
    return table


def _device_table(device: torch.device) -> torch.Tensor:
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _tables:
        _tables[key] = torch.from_numpy(nlm_table()).to(device)
    return _tables[key]


# ---- argument checks ---------------------------------------------------------------------------------------------------------

def _checked_sigma(sigma):
    """None (estimate per call), a float, or a [B] or [B,C] array / tensor (reduced to the root mean square over the channels)"""
    if sigma is None:
        return None
    if isinstance(sigma, (torch.Tensor, np.ndarray, list, tuple)):
        s = torch.as_tensor(sigma).to(torch.float64)
        if s.dim() == 2:
            s = torch.sqrt((s * s).mean(dim=1))
        if s.dim() != 1:
            raise ValueError(f"sigma must be None, a float, a [B] or a [B, C] array, got shape {tuple(s.shape)}")
        return s
    return A.non_negative_float(sigma, "sigma")


def _checked_strength(strength, auto: bool = False):
    """a float, a [B] array / tensor, or (with `auto`) "auto" """
    if auto and isinstance(strength, str) and strength == "auto":
        return strength
    if isinstance(strength, (torch.Tensor, np.ndarray, list, tuple)):
        s = torch.as_tensor(strength).to(torch.float64)
        if s.dim() != 1:
            raise ValueError(f"strength must be a float or a [B] array, got shape {tuple(s.shape)}")
        return s
    if isinstance(strength, str):
        raise ValueError(f"strength must be a float{', a [B] array or auto' if auto else ' or a [B] array'}, got {strength!r}")
    return A.non_negative_float(strength, "strength")


def _checked_radii(patch, search) -> Tuple[int, int]:
    return A.int_in(patch, "patch", 1, MAX_PATCH), A.int_in(search, "search", 1, MAX_SEARCH)


def checked_settings(sigma=None, patch: int = 1, search: int = 10, strength=0.55):
    """the settings of NlmDenoiserModule, checked: (sigma, patch, search, strength)"""
    return (_checked_sigma(sigma),) + _checked_radii(patch, search) + (_checked_strength(strength, auto=True),)


def parse_setting(nlm) -> dict:
    """load_model's `nlm`: None -> the defaults; a dict of SETTINGS -> itself.  Everything is checked here, before anything is
    loaded."""
    return A.parse_setting(nlm, "nlm", "None or a dict of NlmDenoiserModule settings", SETTINGS, checked_settings, bools=False) or {}


def _per_image(value, B: int, device, what: str) -> torch.Tensor:
    """a checked float or [B] tensor as a float64 [B] tensor on `device`"""
    if isinstance(value, torch.Tensor):
        if tuple(value.shape) != (B,):
            raise ValueError(f"{what} must be a float or a [{B}] array for this batch, got shape {tuple(value.shape)}")
        return value.to(device)
    return torch.full((B,), value, dtype=torch.float64, device=device)


# ---- the operator ------------------------------------------------------------------------------------------------------------

def nlm_params(sigma, C: int, patch: int = 1, strength=0.55) -> torch.Tensor:
    """the (offset, mult) pairs of noise levels sigma [B] (a tensor where it lives, else anything torch.as_tensor takes), int64 [B,2]
    on sigma's device; `strength`: a float or [B].  v = sigma sigma, n = C (2 patch + 1)^2 in fp64: offset = floor((v 2.0) n),
    g = ((strength strength) v) n, mult = floor(min((2^32 1024 / 9) / g, 2^32 - 1)).  sigma = 0 or strength = 0 give the clamp:
    the filter is off.  Tensor arithmetic: nothing synchronises."""
    C = A.int_in(C, "C", 1, 4)
    patch = A.int_in(patch, "patch", 1, MAX_PATCH)
    strength = _checked_strength(strength)
    s = torch.as_tensor(sigma).to(torch.float64)
    if s.dim() != 1:
        raise ValueError(f"sigma must be a [B] array, got shape {tuple(s.shape)}")
    if isinstance(strength, torch.Tensor):
        if tuple(strength.shape) != tuple(s.shape):
            raise ValueError(f"strength must be a float or a [{s.shape[0]}] array for this sigma, got shape {tuple(strength.shape)}")
        strength = strength.to(s.device)
    n = float(C * (2 * patch + 1) ** 2)
    v = s * s
    offset = torch.floor((v * 2.0) * n)
    g = ((strength * strength) * v) * n
    mult = torch.floor(torch.clamp(_MULT_SCALE / g, max=float(MULT_OFF)))
    return torch.stack([offset.to(torch.int64), mult.to(torch.int64)], dim=1).contiguous()


def _launch(images: torch.Tensor, params: torch.Tensor, patch: int, search: int, cast_to_uint8: bool, want_weights: bool):
    B, H, W, C = images.shape
    out = torch.empty((B, H, W, C), dtype=torch.uint8 if cast_to_uint8 else torch.float32, device=images.device)
    weights = torch.empty((B, H, W), dtype=torch.int32, device=images.device) if want_weights else None
    N.call("bf_op_nlm", N.ptr(images), N.ptr(params), N.ptr(_device_table(images.device)), B, H, W, C, patch, search, N.ptr(out),
           int(cast_to_uint8), N.ptr(weights), N.stream_ptr(images))
    return out, weights


def _checked_images(images, what: str = "images") -> Tuple[torch.Tensor, bool]:
    images, was_numpy = A.host_or_device(images, what, (torch.uint8,), allow_empty=True)
    if images.numel() >= 2 ** 31:
        raise ValueError(f"{what} must hold fewer than 2^31 samples, got {tuple(images.shape)}")
    return images, was_numpy


def nlm(images, params: torch.Tensor, patch: int = 1, search: int = 10, cast_to_uint8: bool = True, return_weights: bool = False):
    """bf_op_nlm: non-local means of a uint8 [B,H,W,C] batch (torch on the GPU, or NumPy, which is uploaded and NumPy handed back)
    under `params` (int64 [B,2] = (offset, mult) on the images' device; nlm_params makes them): uint8 [B,H,W,C], or float32 before
    the rounding; with `return_weights` (out, weights int32 [B,H,W] = den).  An empty batch returns an empty result without a
    launch."""
    patch, search = _checked_radii(patch, search)
    images, was_numpy = _checked_images(images)
    B, H, W, C = images.shape
    if not isinstance(params, torch.Tensor) or params.dtype != torch.int64 or tuple(params.shape) != (B, 2):
        raise ValueError(f"params must be an int64 tensor {(B, 2)} for this batch, got {A._got(params)}")
    if B == 0:
        out = torch.empty((0, H, W, C), dtype=torch.uint8 if cast_to_uint8 else torch.float32, device=images.device)
        weights = torch.empty((0, H, W), dtype=torch.int32, device=images.device)
    else:
        images = A.to_device(images, was_numpy, None, "images", _FEATURE).contiguous()
        if params.device != images.device:
            raise ValueError(f"params must live on the images' device {images.device}, got {params.device}")
        out, weights = _launch(images, params.contiguous(), patch, search, bool(cast_to_uint8), bool(return_weights))
    if was_numpy:
        out, weights = out.cpu().numpy(), weights.cpu().numpy() if return_weights else None
    return (out, weights) if return_weights else out


# ---- the strength from the noisy frame alone ---------------------------------------------------------------------------------

def _checked_strengths(strengths) -> Tuple[float, ...]:
    if not isinstance(strengths, (tuple, list)) or not strengths:
        raise ValueError(f"strengths must be a non-empty sequence of floats, got {strengths!r}")
    return tuple(A.non_negative_float(s, "strengths") for s in strengths)


def _tune(images: torch.Tensor, sigma: torch.Tensor, strengths, patch: int, search: int, probes: int, amplitude: int, seed: int):
    """nlm_tune on a non-empty device batch with sigma float64 [B] on its device"""
    B, _, _, C = images.shape
    per_channel = sigma.unsqueeze(1).expand(B, C)
    mse = []
    for strength in strengths:
        params = nlm_params(sigma, C, patch, strength)

        def run(stack, params=params):                            # the member-major stack of (1 + probes) B images
            return _launch(stack.contiguous(), params.repeat(stack.shape[0] // B, 1), patch, search, False, False)[0]
        mse.append(estimate_risk(run, images, sigma=per_channel, probes=probes, amplitude=amplitude, seed=seed).mse)
    mse = torch.stack(mse, dim=1)
    best = torch.as_tensor(strengths, dtype=torch.float64, device=images.device)[torch.argmin(mse, dim=1)]
    return best, mse


def nlm_tune(images, sigma=None, strengths=STRENGTHS, patch: int = 1, search: int = 10, probes: int = 2, amplitude: int = 1,
             seed: int = 0):
    """The strength of least estimated error per image of a uint8 [B,H,W,C] batch (torch on the GPU, or NumPy, which is uploaded
    and NumPy handed back), chosen on the noisy images alone: one estimate_risk call (SURE, risk.py) per strength.  `sigma`: None
    (estimate_noise, "mad", per image), a float, [B] or [B,C].  Returns (the argmin strength float64 [B], the estimated MSE
    float64 [B, len(strengths)]) on the images' device."""
    strengths = _checked_strengths(strengths)
    patch, search = _checked_radii(patch, search)
    sigma = _checked_sigma(sigma)
    images, was_numpy = _checked_images(images)
    B = images.shape[0]
    if isinstance(sigma, torch.Tensor) and tuple(sigma.shape) != (B,):
        raise ValueError(f"sigma must be None, a float, a [{B}] or a [{B}, C] array for this batch, got shape {tuple(sigma.shape)}")
    if B == 0:
        best = torch.empty((0,), dtype=torch.float64, device=images.device)
        mse = torch.empty((0, len(strengths)), dtype=torch.float64, device=images.device)
    else:
        images = A.to_device(images, was_numpy, None, "images", _FEATURE).contiguous()
        level = estimate_noise(images, "mad") if sigma is None else _per_image(sigma, B, images.device, "sigma")
        best, mse = _tune(images, level, strengths, patch, search, probes, amplitude, seed)
    return (best.cpu().numpy(), mse.cpu().numpy()) if was_numpy else (best, mse)


# ---- the module --------------------------------------------------------------------------------------------------------------

class NlmDenoiserModule(DenoiserWrapper):
    """Non-local means as a denoiser module: uint8 [B,H,W,C] -> uint8 [B,H,W,C] (float32, not rounded, with cast_to_uint8=False),
    C in 1..4.  Input handling, return types and empty batches as every wrapper (DenoiserWrapper), around no module: there is no
    model (`model_hydra` is None) and, in integer arithmetic, no range to leave (`check_status()` is True).  It has a
    `float_form()`, so every wrapper (self-ensemble, tiled, pixel-shuffled, stabilised, burst) and estimate_risk take it.

    `sigma`: the noise level the weights are made from; None estimates it per image (estimate_noise, "mad") on the device with
    no host read; a float or a [B] array is taken as given, a [B,C] array is reduced to the root mean square over the channels.
    `strength`: the filter's bandwidth in units of sigma, a float or a [B] array; "auto" runs nlm_tune on every call.  With a
    device tensor and a fixed sigma and strength nothing in a call synchronises: it can be captured into a HIP graph.

    `last_weights` is the int32 [B,H,W] = den of the last call of this module or of its float form: den / 4096 is about the
    number of pixels that were averaged, and 1 where the filter found nothing alike (or is off)."""
    SETTINGS = SETTINGS

    def __init__(self, sigma=None, patch: int = 1, search: int = 10, strength=0.55, cast_to_uint8: bool = True):
        self._sigma, self._patch, self._search, self._strength = checked_settings(sigma, patch, search, strength)
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
        for value, what in ((self._sigma, "sigma"), (self._strength, "strength")):
            if isinstance(value, torch.Tensor) and B > 0 and tuple(value.shape) != (B,):
                raise ValueError(f"{what} must be a float or a [{B}] array for this batch, got shape {tuple(value.shape)}")
        if B == 0:
            return self._empty_output(images, was_numpy)
        images = self._place(images, was_numpy, "image", _FEATURE)
        sigma = estimate_noise(images, "mad") if self._sigma is None else _per_image(self._sigma, B, images.device, "sigma")
        if isinstance(self._strength, str):
            strength = _tune(images, sigma, STRENGTHS, self._patch, self._search, 2, 1, 0)[0]
        else:
            strength = self._strength
        out, weights = _launch(images, nlm_params(sigma, C, self._patch, strength), self._patch, self._search, self._cast_to_uint8, True)
        self._record["weights"] = weights
        return self._deliver(out, was_numpy)
