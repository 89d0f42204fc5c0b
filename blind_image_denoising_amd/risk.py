"""
Stein's unbiased risk estimate (SURE): the mean squared error and PSNR of a denoiser on images that have no clean counterpart.

For y = x + n with n ~ N(0, sigma^2) and N samples,

    E |f(y) - x|^2 / N  =  E[ |f(y) - y|^2 / N  -  sigma^2  +  (2 sigma^2 / N) div f(y) ]

and the divergence comes from a Monte-Carlo probe (Ramani, Blu, Unser, "Monte-Carlo SURE", 2008): div f(y) ~ s . (f(y + a s) -
f(y)) / a with s = +-1 per sample.  Two kernels of csrc/risk.hip carry everything that is not the denoiser: `bf_op_risk_probe_u8`
(one read of the uint8 batch; member 0 = the batch, member p = the batch + a s_p) and `bf_op_risk_sums` (per image and channel
R = sum (f_0 - y)^2 and D_p = sum s_p (f_p - f_0), in fp64, in a fixed order).  Everything stays uint8 on the input side -- the
amplitude `a` is a whole number of grey levels -- so every model family runs its usual fused uint8 -> float32 forward, once, on
the [(1 + K) B, H, W, C] stack.

The estimate is only as good as its assumptions: the noise is additive, white and Gaussian, and sigma is right (by default it
comes from `noise_statistics`, an estimator).  Saturated samples violate both and are reflected, not perturbed, by the probe; the
clipped fraction is therefore reported next to the number (`evaluate_blind_risk`).  DESIGN.md 7.8 has the details.

`estimate_risk_affine` drops the "one sigma" assumption for noise whose variance grows with the signal, var(y | x) = gain x + offset
(camera noise): `bf_op_risk_sums_affine` adds Y = sum y and Dy_p = sum y s_p (f_p - f_0) to the sums, and the estimate is linear in
the four.
"""
from collections import namedtuple
from typing import Dict, Iterable

import numpy as np
import torch

from . import _args as A
from . import _native as N
from .metrics import summarise
from .module_denoiser import float_form
from .noise_estimate import METHODS, noise_statistics
from .noise_level import NoiseLevelFunction, noise_level_function

RiskEstimate = namedtuple("RiskEstimate", ["mse", "psnr", "sigma", "residual_rms", "divergence", "probe_spread", "sums"])

MAX_PROBES, MAX_AMPLITUDE = 8, 16
_FEATURE = "the risk estimate"


def _checked_probe(probes, amplitude, seed):
    return A.int_in(probes, "probes", 1, MAX_PROBES), A.int_in(amplitude, "amplitude", 1, MAX_AMPLITUDE), A.seed64(seed)


def risk_probe_stack_u8(image_u8: torch.Tensor, probes: int = 1, amplitude: int = 1, seed: int = 0) -> torch.Tensor:
    """bf_op_risk_probe_u8 on a uint8 device tensor [B,H,W,C] (C in 1..4): uint8 [(1 + probes) B, H, W, C], member-major; member 0
    is the image, member p = 1..probes the image + amplitude * s_p, s_p = +-1 per sample from Philox (seed, p, sample index),
    reflected where it would leave 0..255.  The signs of an image do not depend on its place in the batch."""
    probes, amplitude, seed = _checked_probe(probes, amplitude, seed)
    image_u8 = A.to_device(A.image_batch(image_u8, "image_u8", (torch.uint8,)), False, None, "image_u8", _FEATURE).contiguous()
    B, H, W, C = image_u8.shape
    stack = torch.empty(((1 + probes) * B, H, W, C), dtype=torch.uint8, device=image_u8.device)
    N.call("bf_op_risk_probe_u8", N.ptr(image_u8), N.ptr(stack), B, H, W, C, probes, amplitude, seed, N.stream_ptr(image_u8))
    return stack


def _launch_sums(affine: bool, image_u8, stack_f32, probes, amplitude, seed) -> torch.Tensor:
    """the argument checks and the call of bf_op_risk_sums (float64 [B, C, 1 + K]) or bf_op_risk_sums_affine ([B, C, 2 + 2 K])"""
    probes, amplitude, seed = _checked_probe(probes, amplitude, seed)
    entry, columns = ("bf_op_risk_sums_affine", 2 + 2 * probes) if affine else ("bf_op_risk_sums", 1 + probes)
    A.image_batch(image_u8, "image_u8", (torch.uint8,))
    A.image_batch(stack_f32, "stack_f32", (torch.float32,))
    image_u8 = A.to_device(image_u8, False, None, "image_u8", _FEATURE)
    B, H, W, C = image_u8.shape
    if tuple(stack_f32.shape) != ((1 + probes) * B, H, W, C) or stack_f32.device != image_u8.device:
        raise ValueError(f"stack_f32 must be {((1 + probes) * B, H, W, C)} on {image_u8.device} for {probes} probes of a "
                         f"{tuple(image_u8.shape)} batch, got {tuple(stack_f32.shape)} on {stack_f32.device}")
    image_u8, stack_f32 = image_u8.contiguous(), stack_f32.contiguous()
    scratch, nbytes = N.scratch(entry, image_u8.device, B, H, W, C, probes)
    out = torch.empty((B, C, columns), dtype=torch.float64, device=image_u8.device)
    N.call(entry, N.ptr(image_u8), N.ptr(stack_f32), B, H, W, C, probes, amplitude, seed, N.ptr(scratch), nbytes, N.ptr(out),
           N.stream_ptr(image_u8))
    return out


def risk_sums(image_u8: torch.Tensor, stack_f32: torch.Tensor, probes: int, amplitude: int, seed: int) -> torch.Tensor:
    """bf_op_risk_sums: float64 [B, C, 1 + probes] on the device.  [..., 0] = sum over the pixels of (f_0 - y)^2, [..., p] = sum of
    s_p (f_p - f_0), for y = image_u8 [B,H,W,C] and f = stack_f32, the float32 result [(1 + probes) B, H, W, C] for
    risk_probe_stack_u8(image_u8, probes, amplitude, seed); the signs are regenerated, not read.  fp64 terms, fixed order."""
    return _launch_sums(False, image_u8, stack_f32, probes, amplitude, seed)


def risk_from_sums(sums, sigma, height: int, width: int, amplitude: int) -> RiskEstimate:
    """The host formula, on what bf_op_risk_sums leaves.  `sums`: float64 [B, C, 1 + K] (R_c, D_1c .. D_Kc); `sigma`: float64
    [B, C].  torch tensors (any device) or NumPy arrays; the result is of the same kind.  With HW = height * width:

        div_c = mean_p(D_pc) / a                     mse_c = R_c / HW - sigma_c^2 + 2 sigma_c^2 (div_c / HW)
        mse = mean_c mse_c                           psnr = 10 log10(255^2 / mse), +inf where mse <= 0
        residual_rms = sqrt(mean_c R_c / HW)         divergence = mean_c div_c / HW
        probe_spread = the sample standard deviation (n - 1) over the probes of the mse each probe gives alone; NaN for K = 1"""
    was_numpy = isinstance(sums, np.ndarray)
    s = torch.as_tensor(sums, dtype=torch.float64)
    sg = torch.as_tensor(sigma, dtype=torch.float64).to(s.device)
    if s.dim() != 3 or s.shape[2] < 2 or tuple(sg.shape) != tuple(s.shape[:2]):
        raise ValueError(f"sums must be [B, C, 1 + K] and sigma [B, C], got {tuple(s.shape)} and {tuple(sg.shape)}")
    C, K = s.shape[1], s.shape[2] - 1
    hw, a = float(int(height) * int(width)), float(amplitude)
    var = sg * sg
    fit = s[:, :, 0] / hw                                             # [B, C]
    div_p = s[:, :, 1:] / a / hw                                      # [B, C, K] divergence per sample, per probe
    div_c = s[:, :, 1:].sum(dim=2) / float(K) / a / hw                # [B, C]
    return _risk_estimate(fit, var, 2.0 * var * div_c, 2.0 * var.unsqueeze(2) * div_p, sg, div_c.sum(dim=1) / float(C), s, was_numpy)


def _risk_estimate(fit, var, twice_wdiv_c, twice_wdiv_p, sigma, divergence, sums, was_numpy: bool) -> RiskEstimate:
    """the tail of both host formulas: fit = R / HW and var, the variance that is subtracted, [B, C]; twice the variance-weighted
    divergence per sample, over all probes [B, C] and per probe [B, C, K]; sigma [B, C] and the plain divergence [B] as reported"""
    C, K = fit.shape[1], twice_wdiv_p.shape[2]
    mse = (fit - var + twice_wdiv_c).sum(dim=1) / float(C)
    mse_p = (fit.unsqueeze(2) - var.unsqueeze(2) + twice_wdiv_p).sum(dim=1) / float(C)                         # [B, K]
    if K > 1:
        spread = torch.sqrt(((mse_p - mse_p.mean(dim=1, keepdim=True)) ** 2).sum(dim=1) / float(K - 1))
    else:
        spread = torch.full_like(mse, float("nan"))
    psnr = torch.where(mse > 0.0, 10.0 * torch.log10(255.0 ** 2 / mse.clamp_min(1e-300)), torch.full_like(mse, float("inf")))
    est = RiskEstimate(mse, psnr, sigma, torch.sqrt(fit.sum(dim=1) / float(C)), divergence, spread, sums)
    return RiskEstimate(*(v.cpu().numpy() for v in est)) if was_numpy else est


def _probed_forward(fn, noisy: torch.Tensor, probes: int, amplitude: int, seed: int) -> torch.Tensor:
    """the float32 result of the float form of the module on the probe stack of a checked, non-empty device batch"""
    stack = risk_probe_stack_u8(noisy, probes, amplitude, seed)
    result = fn(stack)                                           # ONE call on [(1 + K) B, H, W, C]
    return A.module_result(result, torch.float32, stack.shape, hint=" (a rounded uint8 output cannot carry the finite difference "
                           "of the probe: DenoiserModule(hydra, cast_to_uint8=False))").to(noisy.device)


def _estimate(fn, noisy: torch.Tensor, sigma, method: str, probes: int, amplitude: int, seed: int) -> RiskEstimate:
    """estimate_risk on a checked, non-empty device batch with the float form of the module"""
    B, H, W, C = noisy.shape
    sums = risk_sums(noisy, _probed_forward(fn, noisy, probes, amplitude, seed), probes, amplitude, seed)
    if sigma is None:
        sigma = noise_statistics(noisy)[:, :, 2 if method == "mad" else 1]
    return risk_from_sums(sums, sigma.to(noisy.device), H, W, amplitude)


def estimate_risk(module, noisy, sigma=None, method: str = "mad", probes: int = 1, amplitude: int = 1, seed: int = 0) -> RiskEstimate:
    """The SURE estimate of the mean squared error between module(noisy) and the clean images nobody has, per image of the uint8
    [B,H,W,C] batch `noisy` (torch or NumPy; NumPy is uploaded).  Returns RiskEstimate(mse [B], psnr [B], sigma [B,C], residual_rms
    [B], divergence [B], probe_spread [B], sums [B,C,1+probes]) -- the formulas are risk_from_sums' -- as float64 tensors on the
    batch's device, or NumPy arrays for a NumPy batch.

    `sigma`: the noise standard deviation in grey levels: a float, [C] or [B,C]; None takes noise_statistics(noisy), column
    `method` ("mad" or "immerkaer"; needs H, W >= 3).  `probes` (1..8) probes of `amplitude` (1..16) grey levels are averaged;
    `seed` selects their signs (an image gets the same signs alone or inside a batch).

    `module`: a DenoiserModule (run through DenoiserModule(hydra, cast_to_uint8=False), its status record shared, so that
    module.check_status() covers the call), a SelfEnsembleDenoiserModule (rebuilt with cast_to_uint8=False over the same module
    and transforms), a GraphedDenoiserModule (its wrapped module, called directly), or any callable that maps a uint8 device
    tensor [B,H,W,C] to float32 of the same shape; a uint8 result raises ValueError.  A call is: probe stack, ONE module call on
    [(1 + probes) B, H, W, C], sums.  An empty batch returns empty results without a launch.

    The estimate inherits the arithmetic of the module: D is a difference of two forwards that differ by `amplitude` grey levels,
    so forward rounding enters it relative to that difference (DESIGN.md 7.8 has the measured sizes for the split-f16 and the
    exact-fp32 kernels; on the case measured there the two paths agree on the estimated mse to well below 1 %)."""
    A.one_of(method, "method", METHODS)
    return _framed(module, noisy, (probes, amplitude, seed), lambda K: 1 + K,
                   lambda B, C: None if sigma is None else A.per_image_channel(sigma, B, C, "sigma"),
                   lambda fn, y, given, K, a, seed_: _estimate(fn, y, given, method, K, a, seed_))


def _framed(module, noisy, probe, columns, levels, run) -> RiskEstimate:
    """What estimate_risk and estimate_risk_affine share.  The checks, in the order the callers promise: `probe` = (probes,
    amplitude, seed), the module, the batch, then `levels(B, C)` for the noise level that was given; an empty batch returns empty
    results ([0, C, columns(probes)] sums) without a device; NumPy is uploaded to the module's device and NumPy comes back, a
    host tensor is refused.  `run(float form, device batch, levels' result, probes, amplitude, seed)` is the estimate itself."""
    probes, amplitude, seed = _checked_probe(*probe)
    fn = float_form(module)
    noisy, was_numpy = A.host_or_device(noisy, "noisy", (torch.uint8,), allow_empty=True)
    B, _, _, C = noisy.shape
    given = levels(B, C)
    if B == 0:
        empty = lambda *shape: torch.empty(shape, dtype=torch.float64, device=noisy.device)
        est = RiskEstimate(empty(0), empty(0), empty(0, C), empty(0), empty(0), empty(0), empty(0, C, columns(probes)))
    else:
        device = A.device_of(module, _FEATURE) if was_numpy else None
        est = run(fn, A.to_device(noisy, was_numpy, device, "noisy", _FEATURE).contiguous(), given, probes, amplitude, seed)
    return RiskEstimate(*(v.cpu().numpy() for v in est)) if was_numpy else est


# ---- noise whose variance is affine in the signal ------------------------------------------------

def risk_sums_affine(image_u8: torch.Tensor, stack_f32: torch.Tensor, probes: int, amplitude: int, seed: int) -> torch.Tensor:
    """bf_op_risk_sums_affine: float64 [B, C, 2 + 2 probes] on the device = (R, Y, D_1..D_K, Dy_1..Dy_K) per image and channel.  R =
    sum (f_0 - y)^2 and D_p = sum s_p (f_p - f_0) are risk_sums' columns, with their bits; Y = sum y is an exact integer; Dy_p =
    sum y s_p (f_p - f_0).  The arguments are risk_sums': y = image_u8 [B,H,W,C], f = stack_f32, the float32 result
    [(1 + probes) B, H, W, C] for risk_probe_stack_u8(image_u8, probes, amplitude, seed)."""
    return _launch_sums(True, image_u8, stack_f32, probes, amplitude, seed)


def risk_from_affine_sums(sums, gain, offset, height: int, width: int, amplitude: int) -> RiskEstimate:
    """The host formula for var_i = gain y_i + offset, on what bf_op_risk_sums_affine leaves.  `sums`: float64 [B, C, 2 + 2 K] =
    (R_c, Y_c, D_1c .. D_Kc, Dy_1c .. Dy_Kc); `gain`, `offset`: float64 [B, C].  torch tensors (any device) or NumPy arrays; the
    result is of the same kind.  With HW = height * width and a = amplitude:

        mse_c = (R_c - (gain_c Y_c + offset_c HW) + 2 (gain_c mean_p Dy_pc + offset_c mean_p D_pc) / a) / HW
        mse = mean_c mse_c                           psnr = 10 log10(255^2 / mse), +inf where mse <= 0
        sigma_c = sqrt(gain_c Y_c / HW + offset_c), the root of the frame's mean variance
        residual_rms = sqrt(mean_c R_c / HW)         divergence = mean_c mean_p D_pc / a / HW (not weighted)
        probe_spread = the sample standard deviation (n - 1) over the probes of the mse each probe gives alone; NaN for K = 1"""
    was_numpy = isinstance(sums, np.ndarray)
    s = torch.as_tensor(sums, dtype=torch.float64)
    g = torch.as_tensor(gain, dtype=torch.float64).to(s.device)
    o = torch.as_tensor(offset, dtype=torch.float64).to(s.device)
    if s.dim() != 3 or s.shape[2] < 4 or s.shape[2] % 2 or tuple(g.shape) != tuple(s.shape[:2]) or tuple(o.shape) != tuple(s.shape[:2]):
        raise ValueError(f"sums must be [B, C, 2 + 2 K] and gain and offset [B, C], got {tuple(s.shape)}, {tuple(g.shape)} and "
                         f"{tuple(o.shape)}")
    C, K = s.shape[1], (s.shape[2] - 2) // 2
    hw, a = float(int(height) * int(width)), float(amplitude)
    fit, var = s[:, :, 0] / hw, g * s[:, :, 1] / hw + o            # [B, C]: the residual and the mean variance per sample
    d, dy = s[:, :, 2:2 + K], s[:, :, 2 + K:]
    wdiv_p = (g.unsqueeze(2) * dy + o.unsqueeze(2) * d) / a / hw   # [B, C, K]: sum var_i df_i/dy_i per sample, per probe
    wdiv_c = wdiv_p.sum(dim=2) / float(K)
    div = d.sum(dim=2).sum(dim=1) / float(K) / a / hw / float(C)
    return _risk_estimate(fit, var, 2.0 * wdiv_c, 2.0 * wdiv_p, torch.sqrt(var.clamp_min(0.0)), div, s, was_numpy)


def estimate_risk_affine(module, noisy, nlf=None, probes: int = 1, amplitude: int = 1, seed: int = 0) -> RiskEstimate:
    """estimate_risk for noise whose variance grows with the signal, var(y_i | x_i) = gain x_i + offset (shot noise plus read noise):
    for independent Gaussian noise of variances v_i,  E |f(y) - x|^2 = E[ |f(y) - y|^2 - sum v_i + 2 sum v_i df_i/dy_i ], and with
    the plug-in v_i = gain y_i + offset everything is linear in the sums of bf_op_risk_sums_affine (risk_from_affine_sums has the
    formula).  Returns the RiskEstimate of estimate_risk; its `sigma` [B,C] is sqrt(gain mean(y) + offset) and its `sums` are
    [B,C,2+2 probes].

    `nlf`: a NoiseLevelFunction (noise_level.noise_level_function), a (gain, offset) pair -- each a float, [C] or [B,C], in grey
    levels and grey levels squared -- or None for noise_level_function(noisy) (needs H, W >= 3).  `module`, `noisy`, `probes`,
    `amplitude` and `seed` as estimate_risk; the same probe stack and ONE module call.

    A StabilisedDenoiserModule (vst.py) is scored as the whole pipeline -- transform, module, inverse -- in its cast_to_uint8=False
    form.  With its noise_level=None every member of the probe stack is fitted on its own: the fit is part of the function being
    scored, and its reaction to the probe enters the divergence.  A fixed noise level of shape [B,C] does not match the
    [(1 + probes) B] stack (ValueError): give [C] or floats.

    What is approximate: the plug-in weighs the divergence with v(y_i) where the identity has v(x_i).  Since E[(y_i - x_i) g(y)] =
    v_i E dg/dy_i, this adds 2 gain v_i E d2f_i/dy_i^2 per sample, a second-order term: the estimate is unbiased for every linear f
    and close for a smooth one; the noise is taken as Gaussian (shot noise is Poisson: good above a few tens of electrons) and
    clipping at 0 and 255 is not modelled.  DESIGN.md 7.10 has the measured sizes."""
    def levels(B, C):
        if nlf is None:
            return None
        pair = (nlf.gain, nlf.offset) if isinstance(nlf, NoiseLevelFunction) else nlf
        if not isinstance(pair, (tuple, list)) or len(pair) != 2 or pair[0] is None or pair[1] is None:
            raise ValueError("nlf must be None, a NoiseLevelFunction or a (gain, offset) pair")
        try:                                                     # Python floats as float64, not as torch's default float32
            pair = [v if isinstance(v, torch.Tensor) else np.asarray(v, dtype=np.float64) for v in pair]
        except (TypeError, ValueError):
            raise ValueError("gain and offset must each be a float, a [C] or a [B, C] array") from None
        return A.per_image_channel(pair[0], B, C, "gain"), A.per_image_channel(pair[1], B, C, "offset")

    def run(fn, y, pair, K, a, seed_):
        if pair is None:
            fitted = noise_level_function(y)
            pair = (fitted.gain, fitted.offset)
        sums = risk_sums_affine(y, _probed_forward(fn, y, K, a, seed_), K, a, seed_)
        return risk_from_affine_sums(sums, pair[0].to(y.device), pair[1].to(y.device), y.shape[1], y.shape[2], a)

    return _framed(module, noisy, (probes, amplitude, seed), lambda K: 2 + 2 * K, levels, run)


# ---- evaluation without ground truth -------------------------------------------------------------

_KEYS = ("mse", "psnr", "sigma_in", "divergence", "clipped_fraction")


def evaluate_blind_risk(module, noisy_batches: Iterable, sigma=None, method: str = "mad", probes: int = 1, amplitude: int = 1,
                        seed: int = 0) -> Dict:
    """evaluate_blind with a quality number: the SURE estimate of a denoiser on images that are already noisy.  `module` and the
    other arguments as estimate_risk (`sigma`: None or a float for every batch); `noisy_batches`: an iterable of uint8 batches,
    host or device, of any shapes (H, W >= 3).  Batch k is probed with seed + k.  Returns {"method", "probes", "amplitude",
    "images", "batches": [one dict per batch], "aggregate": the same keys over every image}: the means over the images of the
    estimated mse and psnr, sigma_in (the root mean square over the channels of the sigma that entered the estimate), divergence
    (per sample) and clipped_fraction, the share of saturated input samples -- those violate the assumptions of the estimate.
    Nothing is asserted; the module's deferred f16-range status is checked once at the end."""
    probes, amplitude, seed = _checked_probe(probes, amplitude, seed)
    method = A.one_of(method, "method", METHODS)
    fn = float_form(module)
    if sigma is not None:
        sigma = A.non_negative_float(sigma, "sigma")
    batches = A.uint8_batches(noisy_batches, "noisy batches", min_hw=3)
    dev = A.device_of(module, _FEATURE)
    per_image = []                                               # one [5, B] device tensor per batch, rows as _KEYS
    for k, noisy in enumerate(batches):
        noisy = noisy.to(dev).contiguous()
        B, H, W, C = noisy.shape
        stats = noise_statistics(noisy)
        sg = stats[:, :, 2 if method == "mad" else 1] if sigma is None else A.per_image_channel(sigma, B, C, "sigma")
        est = _estimate(fn, noisy, sg, method, probes, amplitude, (seed + k) % 2 ** 64)
        sigma_in = torch.sqrt((est.sigma * est.sigma).sum(dim=1) / float(C))
        per_image.append(torch.stack([est.mse, est.psnr, sigma_in, est.divergence, stats[:, :, 3].sum(dim=1) / float(H * W * C)]))
    if hasattr(module, "check_status"):
        module.check_status()                                    # an overflow of the split-f16 kernels is not averaged into a number
    rows, aggregate = summarise(batches, per_image, _KEYS)
    return {"method": method if sigma is None else "given", "probes": probes, "amplitude": amplitude, "images": aggregate["images"],
            "batches": rows, "aggregate": aggregate}


def format_risk_report(report: Dict) -> str:
    """the table tools/evaluate_risk.py prints"""
    lines = [f"sigma: {report['method']}; {report['probes']} probe(s) of amplitude {report['amplitude']}",
             "batch            shape  images   sigma in   estimated mse   estimated psnr   divergence   clipped"]

    def line(name, shape, r):
        return (f"{name:>5}  {shape:>15}  {r['images']:6d}   {r['sigma_in']:8.3f}   {r['mse']:13.3f}   {r['psnr']:11.2f} dB   "
                f"{r['divergence']:10.4f}   {100.0 * r['clipped_fraction']:6.2f}%")
    for i, r in enumerate(report["batches"]):
        lines.append(line(str(i), "x".join(map(str, r["shape"])), r))
    lines.append(line("all", "", report["aggregate"]))
    return "\n".join(lines)
