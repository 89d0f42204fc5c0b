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
import math
from collections import namedtuple
from typing import Dict, Iterable, Optional, Tuple

import numpy as np
import torch

from . import _args as A
from . import _native as N
from .custom_logger import logger
from .metrics import PeriodicValidator, load_evaluation_batches
from .module_denoiser import DenoiserModule, float_form
from .noise_estimate import METHODS
from .risk import MAX_PROBES, evaluate_blind_risk

_DTYPES = (torch.uint8, torch.float32)
_FEATURE = "the pair kernel"


def neighbor_pairs(noisy: torch.Tensor, seed: int = 0, denoised: Optional[torch.Tensor] = None,
                   weight: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """bf_op_neighbor_pairs on a device tensor `noisy` = y, uint8 or float32 [B,H,W,C] (H, W even, C in 1..4): (input, target),
    float32 [B,H/2,W/2,C].  In every 2x2 cell an ordered pair (p1, p2) of adjacent pixels is drawn from Philox (seed, image, cell):
    input = y[p1]; target = y[p2], or with `denoised` = f(y) (float32, the shape of y) fmaf(weight, f[p1] - f[p2], y[p2]), `weight` =
    lambda in [0, 1).  The same seed draws the same pairs for every tensor of the shape: neighbor_pairs(f, seed) is (g1(f), g2(f))."""
    seed = A.seed64(seed)
    A.image_batch(noisy, "noisy", _DTYPES, min_hw=2, even=True)
    if isinstance(weight, bool) or not isinstance(weight, (int, float, np.integer, np.floating)) or not math.isfinite(weight) \
            or not 0.0 <= float(np.float32(weight)) < 1.0:
        raise ValueError(f"weight must be a float in [0, 1), got {weight!r}")
    if denoised is not None:
        if not isinstance(denoised, torch.Tensor) or denoised.dtype != torch.float32 or denoised.shape != noisy.shape:
            raise ValueError(f"denoised must be a float32 tensor of the shape of noisy {tuple(noisy.shape)}, got "
                             f"{getattr(denoised, 'dtype', type(denoised))} {tuple(getattr(denoised, 'shape', ()))}")
        if denoised.device != noisy.device:
            raise ValueError(f"denoised lives on {denoised.device}, noisy on {noisy.device}")
    noisy = A.to_device(noisy, False, None, "noisy", _FEATURE).contiguous()
    denoised = None if denoised is None else denoised.contiguous()
    B, H, W, C = noisy.shape
    inp = torch.empty((B, H // 2, W // 2, C), dtype=torch.float32, device=noisy.device)
    tgt = torch.empty_like(inp)
    N.call("bf_op_neighbor_pairs", N.ptr(noisy), int(noisy.dtype == torch.uint8), N.ptr(denoised), float(weight), N.ptr(inp),
           N.ptr(tgt), B, H, W, C, seed, N.stream_ptr(noisy))
    return inp, tgt


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
        gamma = A.non_negative_float(gamma, "gamma")
        if batches is None or not hasattr(batches, "__iter__"):
            raise ValueError("batches must be an iterable of noisy batches or of (anything, noisy) pairs")
        if gamma > 0.0 and model is None:
            raise ValueError("gamma > 0 needs the model whose output the regulariser compares")
        self.batches, self.gamma, self.ramp = batches, gamma, bool(ramp)
        # a hydra runs as DenoiserModule(model, cast_to_uint8=False); any other callable is that function itself (tests put a
        # counting stub here)
        self.forward = None
        if gamma > 0.0:
            self.forward = DenoiserModule(model, cast_to_uint8=False) if hasattr(model, "infer_u8") else float_form(model, "model")
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
        t, _ = A.host_or_device(item, "a noisy batch", _DTYPES, min_hw=2, even=True)
        if not t.is_cuda:
            t = t.to(self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device()))
        return t

    def __iter__(self):
        for item in self.batches:
            y = self._noisy(item)
            seed, lam, f = int(self.rng.integers(0, 2 ** 63 - 1)), self.weight(), None
            if lam > 0.0:
                y_u8 = y if y.dtype == torch.uint8 else y.round().clamp_(0.0, 255.0).to(torch.uint8)
                f = A.module_result(self.forward(y_u8), torch.float32, y.shape)
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
    inputs = section.get("inputs", [])
    inputs = [inputs] if isinstance(inputs, str) else list(inputs)
    sigma = section.get("sigma")
    if sigma is not None:
        sigma = A.non_negative_float(sigma, "train.self_supervised.validation.sigma")
    return RiskValidationConfig(every=max(0, int(section.get("every", 0))), inputs=[str(i) for i in inputs], sigma=sigma,
                                method=A.one_of(section.get("method", "mad"), "train.self_supervised.validation.method", METHODS),
                                probes=A.int_in(section.get("probes", 1), "train.self_supervised.validation.probes", 1, MAX_PROBES))


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
    gamma = A.non_negative_float(section.get("gamma", 0.0), "train.self_supervised.gamma")
    ramp = section.get("ramp", True)
    if not isinstance(ramp, bool):
        raise ValueError(f"train.self_supervised.ramp must be true or false, got {ramp!r}")
    return SelfSupervisedConfig(kind, gamma, ramp, _parse_validation(section.get("validation")))


class RiskValidator(PeriodicValidator):
    """`evaluate_blind_risk` as a PeriodicValidator: what metrics.Evaluator is to a run that has clean images."""
    FILE = "risk.jsonl"
    BATCHES = ("noisy batches", 3,
               "train.self_supervised.validation needs images: name `inputs` directories or pass validation_noisy_batches")

    def run(self, step: int, epoch: int) -> Dict:
        c = self.config
        report = evaluate_blind_risk(self.module, self.batches, sigma=c.sigma, method=c.method, probes=c.probes, seed=self.seed)
        a = report["aggregate"]
        logger.info(f"risk step {step}: sigma in {a['sigma_in']:.3f}, estimated mse {a['mse']:.3f}, estimated psnr {a['psnr']:.3f}")
        return self._keep({"step": int(step), "epoch": int(epoch), "risk": report})


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
        validation_noisy_batches = load_evaluation_batches(v.inputs, VALIDATION_IMAGES, shape, int(model.desc.in_channels))
    return RiskValidator(model, v, validation_noisy_batches, model_dir)
