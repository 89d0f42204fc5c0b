"""
Training on noisy images alone: Neighbor2Neighbor (Huang, Li, Jia, Lu, Liu, "Neighbor2Neighbor: Self-Supervised Denoising from Single
Noisy Images", CVPR 2021) in front of the training step this package already has.

From one noisy image y the sampler draws two half-resolution sub-images g1(y) and g2(y): in every 2x2 cell two adjacent pixels at
random.  The network is trained to map g1(y) to g2(y); the paper's regulariser compares the difference of the two with the
difference the network itself makes, d = g1(f(y)) - g2(f(y)), f(y) under stop-gradient:

    L = |f(g1(y)) - g2(y)|^2 + gamma |f(g1(y)) - g2(y) - d|^2

Squared loss.  With p = f(g1(y)), L = (1 + gamma) |p - (g2(y) + lambda d)|^2 + const, lambda = gamma / (1 + gamma): the whole method
is the ordinary training step fed with (target, input) = (g2(y) + lambda d, g1(y)), and the gradient is the paper's divided by
1 + gamma (tests/test_neighbor.py checks the identity with fp64 autograd).  The identity is exact for the squared loss
(`mse_multiplier`); with `mae_multiplier` the same blended target is used as a variant of the method, not as the paper's loss.

Inference-mode regulariser.  f(y) here is ONE call of DenoiserModule(model, cast_to_uint8=False) on y rounded and clamped to uint8:
the inference path, on the MOVING BatchNorm statistics, where the paper's code runs the training-mode network under no-grad.

One kernel (`bf_op_neighbor_pairs`, csrc/neighbor.hip) builds both tensors from y and optionally f(y); `NeighborPairs` puts it in
front of `train_loop` (`train.self_supervised`), and `RiskValidator` validates such a run by SURE (risk.py), since nobody has clean
images to validate on.  DESIGN.md 7.9 has the contract and the measurements.
"""
import json
import math
import os
from collections import namedtuple
from typing import Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch

from . import _native as N
from .custom_logger import logger

_DTYPES = (torch.uint8, torch.float32)


def _checked_seed(seed) -> int:
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
        raise ValueError(f"seed must be an int in 0..2^64-1, got {seed!r}")
    return int(seed)


def _checked_batch(t, what: str):
    if not isinstance(t, torch.Tensor) or t.dtype not in _DTYPES or t.dim() != 4:
        raise ValueError(f"{what} must be a uint8 or float32 tensor of shape [B,H,W,C], got "
                         f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    B, H, W, C = t.shape
    if B < 1 or H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError(f"{what} must hold at least one image of even height and width (2x2 cells), got {tuple(t.shape)}")
    if not 1 <= C <= 4:
        raise ValueError(f"{what} must have 1..4 channels, got {tuple(t.shape)}")


def neighbor_pairs(noisy: torch.Tensor, seed: int = 0, denoised: Optional[torch.Tensor] = None,
                   weight: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """bf_op_neighbor_pairs on a device tensor `noisy` = y, uint8 or float32 [B,H,W,C] (H, W even, C in 1..4): (input, target),
    float32 [B,H/2,W/2,C].  In every 2x2 cell an ordered pair (p1, p2) of adjacent pixels is drawn from Philox (seed, image, cell):
    input = y[p1]; target = y[p2], or with `denoised` = f(y) (float32, the shape of y) fmaf(weight, f[p1] - f[p2], y[p2]), `weight` =
    lambda in [0, 1).  The same seed draws the same pairs for every tensor of the shape: neighbor_pairs(f, seed) is (g1(f), g2(f))."""
    seed = _checked_seed(seed)
    _checked_batch(noisy, "noisy")
    if isinstance(weight, bool) or not isinstance(weight, (int, float, np.integer, np.floating)) or not math.isfinite(weight) \
            or not 0.0 <= float(np.float32(weight)) < 1.0:
        raise ValueError(f"weight must be a float in [0, 1), got {weight!r}")
    if denoised is not None:
        if not isinstance(denoised, torch.Tensor) or denoised.dtype != torch.float32 or denoised.shape != noisy.shape:
            raise ValueError(f"denoised must be a float32 tensor of the shape of noisy {tuple(noisy.shape)}, got "
                             f"{getattr(denoised, 'dtype', type(denoised))} {tuple(getattr(denoised, 'shape', ()))}")
        if denoised.device != noisy.device:
            raise ValueError(f"denoised lives on {denoised.device}, noisy on {noisy.device}")
    if not noisy.is_cuda:
        raise RuntimeError("noisy must live on the GPU: the pair kernel has no CPU execution path")
    noisy = noisy.contiguous()
    denoised = None if denoised is None else denoised.contiguous()
    B, H, W, C = noisy.shape
    inp = torch.empty((B, H // 2, W // 2, C), dtype=torch.float32, device=noisy.device)
    tgt = torch.empty_like(inp)
    N.call("bf_op_neighbor_pairs", N.ptr(noisy), int(noisy.dtype == torch.uint8), N.ptr(denoised), float(weight), N.ptr(inp),
           N.ptr(tgt), B, H, W, C, seed, N.stream_ptr(noisy))
    return inp, tgt


def _float_forward(model):
    """uint8 [B,H,W,C] -> float32 of the same shape for `model`: DenoiserModule(model, cast_to_uint8=False) for a hydra; any other
    callable is taken as that function itself (tests put a counting stub here)"""
    if hasattr(model, "infer_u8"):
        from .module_denoiser import DenoiserModule
        return DenoiserModule(model, cast_to_uint8=False)
    if not callable(model):
        raise ValueError("model must be a hydra or a callable uint8 [B,H,W,C] -> float32 [B,H,W,C]")
    return model


class NeighborPairs:
    """A re-iterable that turns noisy batches into the (input_image_batch, noisy_image_batch) = (target, input) pairs `train_loop`
    consumes.  `batches`: a re-iterable of noisy batches (uint8 or float32 [B,H,W,C], H and W even), or of the (anything, noisy)
    pairs `dataset_builder` yields -- the first element is ignored and never read.  Per batch the seed of the draw comes from a host
    generator seeded with `seed`, as PrepareData.draw does it.

    `gamma`: the weight of the paper's regulariser; gamma_t = gamma * percentage_done with `ramp` (what the paper's code does; the
    loop sets `percentage_done`), else gamma; lambda = gamma_t / (1 + gamma_t) goes into the target (see the module docstring:
    exact for the squared loss, a variant with `mae_multiplier`).  With lambda > 0, f(y) is ONE inference-mode call per batch of
    DenoiserModule(model, cast_to_uint8=False) on y rounded and clamped to uint8 (output 0 of a multi-output hydra; the module
    re-packs the weights after an optimizer step; moving BatchNorm statistics, where the paper runs the training-mode network
    under no-grad); its f16-range status is the module's own (`check_status`).  With lambda = 0 no forward is run at all."""

    def __init__(self, batches: Iterable, model=None, gamma: float = 0.0, ramp: bool = True, seed: Optional[int] = None):
        if isinstance(gamma, bool) or not isinstance(gamma, (int, float, np.integer, np.floating)) or not math.isfinite(gamma) or gamma < 0:
            raise ValueError(f"gamma must be a finite float >= 0, got {gamma!r}")
        if batches is None or not hasattr(batches, "__iter__"):
            raise ValueError("batches must be an iterable of noisy batches or of (anything, noisy) pairs")
        if float(gamma) > 0.0 and model is None:
            raise ValueError("gamma > 0 needs the model whose output the regulariser compares")
        self.batches, self.gamma, self.ramp = batches, float(gamma), bool(ramp)
        self.forward = _float_forward(model) if float(gamma) > 0.0 else None
        self.device = getattr(model, "device", None)
        self.rng = np.random.default_rng(seed)
        self.percentage_done = 0.0

    def weight(self) -> float:
        """lambda = gamma_t / (1 + gamma_t) at the current `percentage_done`"""
        g = self.gamma * min(1.0, max(0.0, float(self.percentage_done))) if self.ramp else self.gamma
        return g / (1.0 + g)

    def check_status(self, wait: bool = True) -> bool:
        return self.forward.check_status(wait) if hasattr(self.forward, "check_status") else True

    def _noisy(self, item) -> torch.Tensor:
        if isinstance(item, (tuple, list)):
            if len(item) != 2:
                raise ValueError(f"a batch must be a noisy tensor or an (anything, noisy) pair, got a sequence of {len(item)}")
            item = item[1]
        t = torch.from_numpy(np.ascontiguousarray(item)) if isinstance(item, np.ndarray) else item
        _checked_batch(t, "a noisy batch")
        if not t.is_cuda:
            t = t.to(self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device()))
        return t

    def __iter__(self):
        for item in self.batches:
            y = self._noisy(item)
            seed, lam, f = int(self.rng.integers(0, 2 ** 63 - 1)), self.weight(), None
            if lam > 0.0:
                y_u8 = y if y.dtype == torch.uint8 else y.round().clamp_(0.0, 255.0).to(torch.uint8)
                f = self.forward(y_u8)
                if not isinstance(f, torch.Tensor) or f.dtype != torch.float32 or f.shape != y.shape:
                    raise ValueError(f"the model returned {getattr(f, 'dtype', type(f))} {tuple(getattr(f, 'shape', ()))} for a uint8 "
                                     f"{tuple(y.shape)} batch; float32 of the same shape is needed")
            inp, tgt = neighbor_pairs(y, seed, f, lam)
            yield tgt, inp
        self.check_status(wait=True)


# ---- train_loop: the `train.self_supervised` section and validation by SURE ----------------------

TYPES = ("neighbor2neighbor",)
RiskValidationConfig = namedtuple("RiskValidationConfig", ["every", "inputs", "sigma", "method", "probes"])
VALIDATION_IMAGES = 16          # of `inputs`: the first ones, sorted, as train.evaluation loads them by default
SelfSupervisedConfig = namedtuple("SelfSupervisedConfig", ["type", "gamma", "ramp", "validation"])


def _parse_validation(section) -> Optional[RiskValidationConfig]:
    if section is None:
        return None
    if not isinstance(section, dict):
        raise ValueError("train.self_supervised.validation must be a dictionary")
    unknown = set(section) - set(RiskValidationConfig._fields)
    if unknown:
        raise ValueError(f"unknown keys in train.self_supervised.validation: {sorted(unknown)}")
    from .risk import _checked_probe
    from .noise_estimate import _checked_method
    inputs = section.get("inputs", [])
    inputs = [inputs] if isinstance(inputs, str) else list(inputs)
    sigma = section.get("sigma")
    if sigma is not None and (isinstance(sigma, bool) or not isinstance(sigma, (int, float)) or not math.isfinite(sigma) or sigma < 0):
        raise ValueError(f"train.self_supervised.validation.sigma must be null or a non-negative float, got {sigma!r}")
    probes, _, _ = _checked_probe(section.get("probes", 1), 1, 0)
    return RiskValidationConfig(every=max(0, int(section.get("every", 0))), inputs=[str(i) for i in inputs],
                                sigma=None if sigma is None else float(sigma), method=_checked_method(section.get("method", "mad")),
                                probes=probes)


def parse_self_supervised_config(train_config: Dict) -> Optional[SelfSupervisedConfig]:
    """the `self_supervised` section of the train configuration -- {"type": "neighbor2neighbor", "gamma": 0.0, "ramp": true,
    "validation": {"every": 0, "inputs": [], "sigma": null, "method": "mad", "probes": 1}} -- or None when there is none
    (train_loop then does what it always did).  `inputs`: directories of noisy images, the first 16 files loaded at the dataset's
    input_shape; `every` <= 0: one record per epoch"""
    section = train_config.get("self_supervised")
    if section is None:
        return None
    if not isinstance(section, dict):
        raise ValueError("train.self_supervised must be a dictionary")
    kind = str(section.get("type", "")).strip().lower()
    if kind not in TYPES:
        raise ValueError(f"train.self_supervised.type must be one of {TYPES}, got {section.get('type')!r}")
    unknown = set(section) - set(SelfSupervisedConfig._fields)
    if unknown:
        raise ValueError(f"unknown keys in train.self_supervised: {sorted(unknown)}")
    gamma = section.get("gamma", 0.0)
    if isinstance(gamma, bool) or not isinstance(gamma, (int, float)) or not math.isfinite(gamma) or gamma < 0:
        raise ValueError(f"train.self_supervised.gamma must be a finite float >= 0, got {gamma!r}")
    ramp = section.get("ramp", True)
    if not isinstance(ramp, bool):
        raise ValueError(f"train.self_supervised.ramp must be true or false, got {ramp!r}")
    return SelfSupervisedConfig(kind, float(gamma), ramp, _parse_validation(section.get("validation")))


class RiskValidator:
    """`evaluate_blind_risk` on a fixed set of noisy images with a fixed seed, so that successive records are comparable: what
    metrics.Evaluator is to a run that has clean images.  It runs the current weights through the inference path and touches
    nothing a training step reads."""

    def __init__(self, model, config: RiskValidationConfig, batches: Iterable, model_dir: Optional[str] = None, seed: int = 0):
        from .module_denoiser import DenoiserModule
        from .noise_estimate import _check_noisy_batch
        self.config, self.seed = config, int(seed)
        self.module = DenoiserModule(model)
        self.batches = [_check_noisy_batch(b) for b in batches]
        if not self.batches:
            raise ValueError("train.self_supervised.validation needs images: name `inputs` directories or pass validation_noisy_batches")
        if getattr(model, "device", None) is not None and torch.device(model.device).type == "cuda":
            self.batches = [b.to(model.device) for b in self.batches]
        self.path = None if model_dir is None else os.path.join(model_dir, "risk.jsonl")
        self.history: List[Dict] = []

    def due(self, step: int) -> bool:
        return self.config.every > 0 and step > 0 and step % self.config.every == 0

    def run(self, step: int, epoch: int) -> Dict:
        from .metrics import json_safe
        from .risk import evaluate_blind_risk
        c = self.config
        report = evaluate_blind_risk(self.module, self.batches, sigma=c.sigma, method=c.method, probes=c.probes, seed=self.seed)
        record = {"step": int(step), "epoch": int(epoch), "risk": report}
        self.history.append(record)
        a = report["aggregate"]
        logger.info(f"risk step {step}: sigma in {a['sigma_in']:.3f}, estimated mse {a['mse']:.3f}, estimated psnr {a['psnr']:.3f}")
        if self.path is not None:
            os.makedirs(os.path.dirname(self.path), exist_ok=True)
            with open(self.path, "a") as f:
                f.write(json.dumps(json_safe(record), allow_nan=False) + "\n")
        return record


def build_risk_validator(config: Optional[SelfSupervisedConfig], model, model_dir: Optional[str] = None,
                         dataset_config: Optional[Dict] = None, validation_noisy_batches: Optional[Iterable] = None):
    """the validator of a `train.self_supervised` section, or None without a `validation` part"""
    if config is None or config.validation is None:
        if validation_noisy_batches is not None:
            raise ValueError("validation_noisy_batches were given but the configuration has no train.self_supervised.validation section")
        return None
    v = config.validation
    if validation_noisy_batches is None:
        if not v.inputs:
            raise ValueError("train.self_supervised.validation names no `inputs` directories and no validation_noisy_batches were given")
        shape = (dataset_config or {}).get("input_shape")
        if shape is None:
            raise ValueError("train.self_supervised.validation.inputs needs dataset.input_shape for the size the images are loaded at")
        from .metrics import load_evaluation_batches
        validation_noisy_batches = load_evaluation_batches(v.inputs, VALIDATION_IMAGES, shape, int(model.desc.in_channels))
    return RiskValidator(model, v, validation_noisy_batches, model_dir)
