"""
Inpaint, demosaic and super-resolve with the prior implicit in the denoiser.

A blind, bias-free denoiser works at every noise level, so its residual D(y) - y estimates the score of the image prior.
Kadkhodaie & Simoncelli ("Stochastic solutions for linear inverse problems using the prior implicit in a denoiser", NeurIPS 2021,
Algorithm 2) climb that prior in the subspace a linear measurement leaves open and pin the measured subspace to the data, coarse
to fine, with injected noise that shrinks as the residual shrinks.  Nothing is retrained.  Per image, n = H W C, on the 0..255
scale, with a projection P and an anchor a (the measurement embedded in image space):

    y_0 = 127.5 (1 - P 1) + a + sigma_0 z_0
    t = 1, 2, ..:   h_t = h0 t / (1 + h0 (t - 1));   D = denoiser(y);   d = D - y + a - P D;   sigma_t^2 = sum d^2 / n
                    sigma_t <= sigma_l: the image is frozen (y and its step count never change again); else
                    gamma_t^2 = ((1 - beta h_t)^2 - (1 - h_t)^2) sigma_t^2;   y += h_t d + gamma_t z_t
    result          x = D - P D + a  for D = denoiser(final y)

Two constraints: `mask_constraint` (P v = m v: inpainting, dropped pixels, a Bayer mosaic) and `block_constraint` (P v = the s x s
block means: super-resolution by s).  The state between two denoiser calls lives on the device: four entries of csrc/restore.hip
(`restore_init`, `restore_direction`, `restore_step`, `restore_finish` call them directly) write y_0, d and sum d^2, the update and
the result; sigma_t, the freezing and the step counts stay there, and `restore` reads them only every `check_every` iterations.
The noise is Philox, counter (element group, sample id, t, 6): a result depends on (seed, sample id) and on nothing else, so an
image gives the same bits alone or inside a batch.  beta = 1 is the deterministic variant (no noise after y_0, several times fewer
iterations); beta = 0.01 draws a sample from the posterior the prior and the measurement define.  DESIGN.md 7.19 has the
measurements.  There is no CPU execution path.

Frame sizes: the denoiser is called in float at the frame's own size, which is not padded to a power of two as the uint8 path
pads it.  The resnet family takes any size (odd ones included); the shipped unet_laplacian_v5.6 needs H and W to be multiples of
4 and raises ValueError otherwise, which is passed through.
"""
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _args as A
from . import _native as N
from .module_denoiser import DenoiserModule, GraphedDenoiserModule, _DeferredStatus

KINDS = ("mask", "block")
_FEATURE = "the restoration code"
_IMAGE_TYPES = (torch.uint8, torch.float32)


class RestoreConstraint(NamedTuple):
    """a projection P and the anchor a: `kind` "mask" (mask uint8 [B,H,W,1 or C], anchor = the measured image [B,H,W,C]) or "block"
    (factor s, anchor = the low-resolution image [B,H/s,W/s,C]); anchor uint8 or float32; `shape` = (B,H,W,C) of the restored
    batch; `was_numpy`: host arrays were given, host arrays are handed back"""
    kind: str
    anchor: torch.Tensor
    mask: Optional[torch.Tensor]
    factor: int
    shape: tuple
    was_numpy: bool


class RestoreResult(NamedTuple):
    """image [N,H,W,C] (uint8, or float32 with cast_to_uint8=False), iterations int32 [N] (the updates each image took), sigma
    float64 [N] (sigma_t of the last iteration run), converged bool [N] (the image froze: sigma_t <= sigma_l), trace float64
    [iterations run, N] of sigma_t or None"""
    image: object
    iterations: object
    sigma: object
    converged: object
    trace: object


# ---- constraints (no device is touched) ------------------------------------------------------------------------------------------

def mask_constraint(image, mask) -> RestoreConstraint:
    """P v = m v, a = m x: `image` = the measured image x, uint8 or float32 [B,H,W,C] (its values where m = 0 are never read);
    `mask` uint8 [B,H,W,1] (all channels) or [B,H,W,C] (per channel, e.g. a Bayer pattern), non-zero = measured."""
    image, was_numpy = A.host_or_device(image, "image", _IMAGE_TYPES)
    mask, mask_numpy = A.host_or_device(mask, "mask", (torch.uint8,))
    B, H, W, C = image.shape
    if tuple(mask.shape[:3]) != (B, H, W) or mask.shape[3] not in (1, C):
        raise ValueError(f"mask must be uint8 [{B},{H},{W},1] or [{B},{H},{W},{C}] for this image, got {tuple(mask.shape)}")
    if H * W * C >= 2 ** 31:
        raise ValueError(f"an image must hold fewer than 2^31 elements, got {tuple(image.shape)}")
    return RestoreConstraint("mask", image, mask, 1, (B, H, W, C), was_numpy or mask_numpy)


def block_constraint(low, factor, size=None) -> RestoreConstraint:
    """P v = every s x s block of every channel replaced by its mean, a = `low` repeated s x s: `low` = the low-resolution image,
    uint8 or float32 [B,h,w,C]; `factor` = s in 2..8.  `size` = (H, W) of the frame to restore, when the caller has one in mind:
    it must be (h s, w s), which is what None means."""
    factor = A.int_in(factor, "factor", 2, 8)
    low, was_numpy = A.host_or_device(low, "low", _IMAGE_TYPES)
    B, h, w, C = low.shape
    H, W = (h * factor, w * factor) if size is None else (A.int_in(size[0], "size[0]", 1), A.int_in(size[1], "size[1]", 1))
    if H % factor or W % factor or (H // factor, W // factor) != (h, w):
        raise ValueError(f"factor {factor} must divide the frame {H} x {W} into the {h} x {w} samples of low")
    if H * W * C >= 2 ** 31:
        raise ValueError(f"an image must hold fewer than 2^31 elements, got {(B, H, W, C)}")
    return RestoreConstraint("block", low, None, factor, (B, H, W, C), was_numpy)


def _checked_constraint(constraint) -> RestoreConstraint:
    if not isinstance(constraint, RestoreConstraint) or constraint.kind not in KINDS:
        raise ValueError("constraint must come from mask_constraint or block_constraint")
    return constraint


def _on_device(con: RestoreConstraint, device=None) -> RestoreConstraint:
    """the constraint with its tensors on the device (host arrays are uploaded, host tensors refused: _args.to_device)"""
    anchor = A.to_device(con.anchor, con.was_numpy, device, "the measurement", _FEATURE).contiguous()
    mask = None if con.mask is None else A.to_device(con.mask, con.was_numpy, anchor.device, "mask", _FEATURE).to(anchor.device).contiguous()
    return con._replace(anchor=anchor, mask=mask)


def _repeated(con: RestoreConstraint, K: int) -> RestoreConstraint:
    if K == 1:
        return con
    rep = lambda t: None if t is None else t.repeat_interleave(K, dim=0).contiguous()
    return con._replace(anchor=rep(con.anchor), mask=rep(con.mask), shape=(con.shape[0] * K,) + tuple(con.shape[1:]))


def _constraint_args(con: RestoreConstraint):
    """(kind, mask, mask_channels, factor, anchor, anchor_is_u8) as the entries take them"""
    return (KINDS.index(con.kind), N.ptr(con.mask), 0 if con.mask is None else int(con.mask.shape[3]), int(con.factor),
            N.ptr(con.anchor), int(con.anchor.dtype == torch.uint8))


def _state(t, what: str, dtype, shape) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} must be a {dtype} tensor of shape {tuple(shape)}, got {A._got(t)}")
    if not t.is_cuda:
        raise A._no_cpu_path(what, _FEATURE)
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    return t


def _sample_ids(sample_ids, count: int, device=None):
    """None, or the ids as an int64 host list checked to be `count` uint32 values; on `device` as the int32 bits the kernel reads"""
    if sample_ids is None:
        return None
    if isinstance(sample_ids, torch.Tensor):
        sample_ids = sample_ids.detach().cpu().tolist()
    ids = [A.int_in(v, "sample_ids", 0, 2 ** 32 - 1) for v in list(sample_ids)]
    if len(ids) != count:
        raise ValueError(f"sample_ids must hold one id per restored image ({count}), got {len(ids)}")
    if device is None:
        return ids
    return torch.from_numpy(np.asarray(ids, np.uint32).view(np.int32).copy()).to(device)


# ---- the four operators ----------------------------------------------------------------------------------------------------------

def restore_init(constraint: RestoreConstraint, sigma_0: float = 255.0, seed: int = 0, sample_ids=None) -> torch.Tensor:
    """bf_op_restore_init: y_0 = 127.5 (1 - P 1) + a + sigma_0 z_0, float32 [B,H,W,C] on the constraint's device.  `sample_ids`:
    one uint32 per image (default: its index)."""
    con = _checked_constraint(constraint)
    sigma_0, seed = A.non_negative_float(sigma_0, "sigma_0"), A.seed64(seed)
    ids = _sample_ids(sample_ids, con.shape[0])
    con = _on_device(con)
    ids = _sample_ids(ids, con.shape[0], con.anchor.device)
    B, H, W, C = con.shape
    y = torch.empty(con.shape, dtype=torch.float32, device=con.anchor.device)
    N.call("bf_op_restore_init", N.ptr(y), B, H, W, C, *_constraint_args(con), sigma_0, seed, N.ptr(ids), N.stream_ptr(y))
    return y


def _direction(y, denoised, con, d, sumsq, scratch):
    B, H, W, C = con.shape
    N.call("bf_op_restore_direction", N.ptr(y), N.ptr(denoised), B, H, W, C, *_constraint_args(con), N.ptr(d), N.ptr(scratch),
           scratch.numel() * 8, N.ptr(sumsq), N.stream_ptr(y))


def restore_direction(y: torch.Tensor, denoised: torch.Tensor, constraint: RestoreConstraint):
    """bf_op_restore_direction: (d, sumsq) = (D - y + a - P D as float32 [B,H,W,C], sum d^2 per image as float64 [B]) for the
    iterate y and D = `denoised`, float32 device tensors of the constraint's shape.  The sum has a fixed order: the same bits in
    two calls, and for an image alone or inside a batch."""
    con = _checked_constraint(constraint)
    y, denoised = _state(y, "y", torch.float32, con.shape), _state(denoised, "denoised", torch.float32, con.shape)
    con = _on_device(con, y.device)
    B, H, W, C = con.shape
    d = torch.empty_like(y)
    sumsq = torch.empty(B, dtype=torch.float64, device=y.device)
    scratch, _ = N.scratch("bf_op_restore", y.device, B, H, W, C)
    _direction(y, denoised, con, d, sumsq, scratch)
    return d, sumsq


def step_size(t: int, h0: float) -> float:
    """h_t = h0 t / (1 + h0 (t - 1))"""
    return h0 * t / (1.0 + h0 * (t - 1))


def _step(y, d, sumsq, steps, t, h_t, beta, sigma_l, seed, ids, trace):
    B, H, W, C = y.shape
    N.call("bf_op_restore_step", N.ptr(y), N.ptr(d), N.ptr(sumsq), B, H, W, C, float(h_t), float(beta), float(sigma_l), int(t), seed,
           N.ptr(ids), N.ptr(trace), 0 if trace is None else int(trace.shape[0]), N.ptr(steps), N.stream_ptr(y))


def restore_step(y: torch.Tensor, d: torch.Tensor, sumsq: torch.Tensor, steps: torch.Tensor, t: int, h_t: float, *, beta: float = 0.01,
                 sigma_l: float = 2.55, seed: int = 0, sample_ids=None, trace: Optional[torch.Tensor] = None) -> None:
    """bf_op_restore_step, iteration t >= 1, in place: sigma_t = sqrt(sumsq / n) goes to trace[t - 1] (float64 [rows >= t, B], or
    None); an image whose steps[b] == t - 1 (int32 [B], zeros before t = 1) and whose sigma_t > sigma_l moves -- y += h_t d +
    gamma_t z_t, steps[b] = t -- and every other image is frozen: its y and its count stay.  Nothing comes to the host."""
    B = A.image_batch(y, "y", (torch.float32,)).shape[0]
    _state(y, "y", torch.float32, y.shape)
    _state(d, "d", torch.float32, y.shape), _state(sumsq, "sumsq", torch.float64, (B,)), _state(steps, "steps", torch.int32, (B,))
    t = A.int_in(t, "t", 1, 2 ** 31 - 1)
    h_t, beta, sigma_l, seed = _unit(h_t, "h_t", False), _unit(beta, "beta", True), _positive(sigma_l, "sigma_l"), A.seed64(seed)
    if trace is not None:
        if not isinstance(trace, torch.Tensor) or trace.dim() != 2 or trace.shape[0] < t:
            raise ValueError(f"trace must be a float64 [rows >= {t}, {B}] tensor, got {A._got(trace)}")
        _state(trace, "trace", torch.float64, (trace.shape[0], B))
    ids = _sample_ids(_sample_ids(sample_ids, B), B, y.device)
    _step(y, d, sumsq, steps, t, h_t, beta, sigma_l, seed, ids, trace)


def restore_finish(denoised: torch.Tensor, constraint: RestoreConstraint, cast_to_uint8: bool = True) -> torch.Tensor:
    """bf_op_restore_finish: x = D - P D + a for D = `denoised` (the denoiser's output for the final y); the measured samples of a
    mask constraint are the measurement itself.  float32, or uint8 rounded half to even and clipped."""
    con = _checked_constraint(constraint)
    denoised = _state(denoised, "denoised", torch.float32, con.shape)
    con = _on_device(con, denoised.device)
    B, H, W, C = con.shape
    out = torch.empty(con.shape, dtype=torch.uint8 if cast_to_uint8 else torch.float32, device=denoised.device)
    N.call("bf_op_restore_finish", N.ptr(denoised), B, H, W, C, *_constraint_args(con), N.ptr(out), int(bool(cast_to_uint8)),
           N.stream_ptr(denoised))
    return out


# ---- the loop ------------------------------------------------------------------------------------------------------------------

def _unit(value, what: str, zero_allowed: bool) -> float:
    value = A.non_negative_float(value, what, 1.0)
    if value == 0.0 and not zero_allowed:
        raise ValueError(f"{what} must be in (0, 1], got {value!r}")
    return value


def _positive(value, what: str) -> float:
    value = A.non_negative_float(value, what)
    if value == 0.0:
        raise ValueError(f"{what} must be positive, got {value!r}")
    return value


def _float_denoiser(denoiser, channels: int):
    """(the float32 -> float32 call, the hydra whose f16-range status it sets or None)"""
    if isinstance(denoiser, (DenoiserModule, GraphedDenoiserModule)):
        hydra = denoiser.model_hydra
        desc = getattr(hydra, "desc", hydra)
        cin, cout = int(desc.in_channels), int(desc.out_channels)
        if cin != cout or cin != channels:
            raise ValueError(f"the denoiser maps {cin} to {cout} channels: restoring {channels}-channel images needs a model of "
                             f"{channels} channels in and out")

        def call(y):
            out = hydra(y)
            return out[0] if isinstance(out, (list, tuple)) else out     # a multi-output hydra: full resolution first
        return call, hydra
    if hasattr(denoiser, "float_form") or hasattr(denoiser, "model_hydra") or type(denoiser).__name__.endswith("DenoiserModule"):
        raise ValueError(f"{type(denoiser).__name__} takes uint8 only; restore needs a DenoiserModule, a GraphedDenoiserModule "
                         f"(their hydra is called in float) or a callable float32 [B,H,W,C] -> float32 [B,H,W,C]")
    if not callable(denoiser):
        raise ValueError("denoiser must be a DenoiserModule, a GraphedDenoiserModule or a callable float32 [B,H,W,C] -> float32 "
                         "[B,H,W,C] on device tensors")
    return denoiser, None


def restore(denoiser, constraint: RestoreConstraint, *, sigma_0: float = 255.0, sigma_l: float = 2.55, h0: float = 0.01,
            beta: float = 0.01, max_iterations: int = 2000, samples: int = 1, seed: int = 0, sample_ids=None, check_every: int = 16,
            cast_to_uint8: bool = True, trace: bool = False) -> RestoreResult:
    """The restoration loop of the module's header around `denoiser`: a DenoiserModule or GraphedDenoiserModule (its model_hydra is
    called in float; the first output of a multi-output hydra; in_channels == out_channels), or any callable from a float32 device
    tensor [N,H,W,C] to a float32 device tensor of that shape.  The wrappers that take uint8 only are refused.

    Defaults are the paper's on the 0..255 scale; beta in [0, 1] (1 = deterministic), h0 in (0, 1], 0 < sigma_l <= sigma_0.
    `samples` = K repeats every measurement K times with sample id K b + k and returns [B K, ..]; `sample_ids` gives the ids
    instead (one per returned image).  The host reads the step counts every `check_every` iterations and stops when every image is
    frozen; freezing happens on the device, so the result does not depend on `check_every`.  At those reads the hydra's f16-range
    status is checked: on a hit the model is switched to arith 0 and the run repeated from y_0 (auto_exact_fallback), else
    FloatingPointError.  Host arrays in, host arrays out."""
    con = _checked_constraint(constraint)
    sigma_0, sigma_l = _positive(sigma_0, "sigma_0"), _positive(sigma_l, "sigma_l")
    if sigma_l > sigma_0:
        raise ValueError(f"sigma_l must not exceed sigma_0, got {sigma_l} > {sigma_0}")
    h0, beta, seed = _unit(h0, "h0", False), _unit(beta, "beta", True), A.seed64(seed)
    max_iterations, samples = A.int_in(max_iterations, "max_iterations", 1, 2 ** 31 - 1), A.int_in(samples, "samples", 1)
    check_every = A.int_in(check_every, "check_every", 1)
    call, hydra = _float_denoiser(denoiser, con.shape[3])
    count = con.shape[0] * samples
    ids = _sample_ids(sample_ids, count)
    if ids is None and samples > 1:
        ids = list(range(count))                                 # K b + k
    device = torch.device(hydra.device) if hydra is not None else None
    if hydra is not None:
        hydra._require_gpu()
    elif not con.anchor.is_cuda:
        device = A.device_of(None, _FEATURE)                     # the "no CPU path" error without a GPU
    con = _repeated(_on_device(con, device), samples)
    device = con.anchor.device
    ids = _sample_ids(ids, count, device)
    B, H, W, C = con.shape

    y0 = torch.empty(con.shape, dtype=torch.float32, device=device)
    N.call("bf_op_restore_init", N.ptr(y0), B, H, W, C, *_constraint_args(con), sigma_0, seed, N.ptr(ids), N.stream_ptr(y0))
    d, sumsq = torch.empty_like(y0), torch.empty(B, dtype=torch.float64, device=device)
    scratch, _ = N.scratch("bf_op_restore", device, B, H, W, C)
    sigmas = torch.zeros((max_iterations, B), dtype=torch.float64, device=device)
    status = _DeferredStatus()
    status.SLOTS = max(status.SLOTS, check_every + 1)            # one slot per call between two reads: posting never waits

    def denoise(y):
        out = call(y)
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.shape != y.shape or out.device != y.device:
            raise ValueError(f"the denoiser returned {A._got(out)} for a float32 {tuple(y.shape)} device tensor; float32 of the same "
                             f"shape on the same device is needed")
        out = out.contiguous()
        if hydra is not None and hasattr(hydra, "status_tensor") and hydra.status_tensor() is not None:
            status.post(hydra.status_tensor())
        return out

    for attempt in range(2):
        y, steps, ran, overflow = y0.clone(), torch.zeros(B, dtype=torch.int32, device=device), 0, False
        for t in range(1, max_iterations + 1):
            _direction(y, denoise(y), con, d, sumsq, scratch)
            _step(y, d, sumsq, steps, t, step_size(t, h0), beta, sigma_l, seed, ids, sigmas)
            ran = t
            if t % check_every == 0 or t == max_iterations:
                moving = bool((steps.cpu() == t).any())          # the one read of the host (synchronises)
                overflow = bool(status.poll(wait=True) & N.BF_STATUS_F16_RANGE)
                if overflow or not moving:
                    break
        if not overflow:
            final = denoise(y)
            image = restore_finish(final, con, cast_to_uint8)
            overflow = bool(status.poll(wait=True) & N.BF_STATUS_F16_RANGE)      # waits for the last call's word, if there is one
        if not overflow:
            break
        if attempt or not getattr(hydra, "auto_exact_fallback", False):
            raise FloatingPointError("an activation left the f16 range inside the split-f16 kernels during the restoration: its "
                                     "result is not trustworthy; use set_option('arith', 0)")
        from .custom_logger import logger
        logger.warning("an activation left the f16 range inside the split-f16 kernels: switching this model to the exact-fp32 "
                       "kernels and restoring again from y_0")
        hydra.set_option("arith", 0)

    iterations, sigma = steps, sigmas[ran - 1]
    converged = iterations < ran
    history = sigmas[:ran] if trace else None
    if con.was_numpy:
        host = lambda t: None if t is None else t.cpu().numpy()
        return RestoreResult(host(image), host(iterations), host(sigma), host(converged), host(history))
    return RestoreResult(image, iterations, sigma.clone(), converged, None if history is None else history.clone())


def inpaint(denoiser, image, mask, **settings) -> RestoreResult:
    """restore(denoiser, mask_constraint(image, mask), **settings): fill what the mask leaves out"""
    return restore(denoiser, mask_constraint(image, mask), **settings)


def super_resolve(denoiser, low, factor, **settings) -> RestoreResult:
    """restore(denoiser, block_constraint(low, factor), **settings): an image `factor` times the size whose block means are `low`"""
    return restore(denoiser, block_constraint(low, factor), **settings)


def bayer_mask(B: int, H: int, W: int) -> np.ndarray:
    """uint8 [B,H,W,3], the RGGB mosaic: red at (even, even), green at (even, odd) and (odd, even), blue at (odd, odd)"""
    m = np.zeros((B, H, W, 3), np.uint8)
    m[:, 0::2, 0::2, 0] = 1
    m[:, 0::2, 1::2, 1] = 1
    m[:, 1::2, 0::2, 1] = 1
    m[:, 1::2, 1::2, 2] = 1
    return m
