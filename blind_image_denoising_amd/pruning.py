"""Weight pruning strategies (bfcnn/pruning.py) on the device.

Every model here keeps its trainable tensors in one flat float32 device vector (`model.params`), so a strategy is one launch of
`bf_op_prune_tensors` (csrc/prune.hip) on that vector, in place, on the model's stream, driven by a device table of the [begin, end)
ranges of the Conv2D / DepthwiseConv2D kernels -- the tensors the reference prunes (pruning.py:232-260); BatchNorm / LayerNorm gammas,
multipliers and dense gate weights lie outside every range and are never written.  The table is built once per model.

    prune = prune_function_builder({"type": "drop_bottom", "config": {"percentage": 0.5}})
    prune(model)                                  # in place; packed inference weights and captured graphs refresh on next use
    conv2d_sparsity(model)["fraction"]

MINIMUM_THRESHOLD, MINIMUM_THRESHOLD_SHRINKAGE and DROP_BOTTOM reproduce the reference's NumPy result bit for bit (fp32 comparisons
and products; DROP_BOTTOM finds the element of rank int(np.round(n * percentage)) exactly).  MINIMUM_THRESHOLD_BIFURCATE draws from
Philox4x32-10 instead of NumPy's global generator: same distribution, reproducible from `seed`.  PCA_PROJECTION is refused: it is a
host eigen-decomposition with scikit-learn semantics.  There is no CPU path: a model on the CPU raises RuntimeError."""
from enum import Enum
from typing import Callable, Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from . import _native as N
from .constants import CONFIG_STR, TYPE_STR


class PruneStrategy(Enum):
    NONE = 0                            # do nothing
    MINIMUM_THRESHOLD = 1               # every kernel weight below a threshold becomes zero
    MINIMUM_THRESHOLD_BIFURCATE = 2     # ... is drawn again from U(-2t, 2t), then thresholded
    MINIMUM_THRESHOLD_SHRINKAGE = 3     # weights below shrinkage_threshold shrink, then the threshold
    PCA_PROJECTION = 4                  # (refused here)
    DROP_BOTTOM = 5                     # per tensor, the bottom `percentage` of |w| becomes zero

    @staticmethod
    def from_string(type_str: str) -> "PruneStrategy":
        if type_str is None:
            raise ValueError("type_str must not be null")
        if not isinstance(type_str, str):
            raise ValueError("type_str must be string")
        type_str = type_str.strip().upper()
        if len(type_str) <= 0:
            raise ValueError("stripped type_str must not be empty")
        return PruneStrategy[type_str]

    def to_string(self) -> str:
        return self.name


_CONV_KINDS = (0, "conv", "depthwise")


# ---- the range table ---------------------------------------------------------------------------------------------------------

def _hydra_of(model):
    """the model that owns the flat vector: a hydra itself, or what a DenoiserModule / BuilderResults wraps"""
    for attr in ("model_hydra", "hydra"):
        inner = getattr(model, attr, None)
        if inner is not None and hasattr(inner, "params"):
            return inner
    if model is None or not hasattr(model, "params") or not hasattr(model, "trainable_variables"):
        raise ValueError("model must be a hydra built by model_builder (or a DenoiserModule of one)")
    return model


def conv2d_ranges(model) -> List[Tuple[str, int, int]]:
    """(name, begin, end) of every convolution kernel in the model's flat parameter vector, in variable order: tensors of kind 0 of
    the 16-filter engine model, of kind "conv" / "depthwise" of the operator-graph models."""
    out = []
    for v in _hydra_of(model).trainable_variables:
        name, shape, kind, offset = (v.name, v.shape, v.kind, v.offset) if hasattr(v, "kind") else v
        if kind in _CONV_KINDS:
            out.append((str(name), int(offset), int(offset) + int(np.prod(shape))))
    return out


class _Table:
    """host and device forms of a model's ranges, kept on the model"""

    def __init__(self, hydra):
        ranges = conv2d_ranges(hydra)
        self.names = [r[0] for r in ranges]
        self.host = np.array([[r[1], r[2]] for r in ranges], np.int64).reshape(-1, 2)
        self.sizes = self.host[:, 1] - self.host[:, 0]
        self.n_params = int(hydra.params.numel())
        self._device = {}                 # what lives on the GPU, made on first use: ranges, gather index, ranks per percentage

    def ranges(self, device) -> torch.Tensor:
        if "ranges" not in self._device:
            self._device["ranges"] = torch.from_numpy(self.host).to(device)
        return self._device["ranges"]

    def index(self, device) -> torch.Tensor:
        if "index" not in self._device:
            idx = np.concatenate([np.arange(b, e, dtype=np.int64) for b, e in self.host]) if len(self.host) else np.zeros(0, np.int64)
            self._device["index"] = torch.from_numpy(idx).to(device)
        return self._device["index"]

    def ranks(self, percentage: float) -> np.ndarray:
        """index of the threshold in each tensor's ascending |w| (pruning.py:199-201), with NumPy's indexing rules: a negative
        index counts from the end, one outside the tensor is an IndexError"""
        k = np.array([int(np.round(int(n) * percentage)) for n in self.sizes], np.int64)
        bad = (k >= self.sizes) | (k < -self.sizes)
        if bad.any():
            i = int(np.argmax(bad))
            raise IndexError(f"index {int(k[i])} is out of bounds for axis 0 with size {int(self.sizes[i])} "
                             f"(drop_bottom percentage {percentage} on [{self.names[i]}])")
        return np.where(k < 0, k + self.sizes, k)

    def ranks_device(self, percentage: float, device) -> torch.Tensor:
        key = ("kth", float(percentage))
        if key not in self._device:
            self._device[key] = torch.from_numpy(self.ranks(percentage)).to(device)
        return self._device[key]


def _table(hydra) -> _Table:
    t = getattr(hydra, "_prune_table", None)
    if t is None or t.n_params != int(hydra.params.numel()):
        t = _Table(hydra)
        hydra._prune_table = t
    return t


def _require_gpu(hydra, what: str):
    if hydra.params.device.type != "cuda":
        raise RuntimeError(f"{what} needs the GPU: this model lives on the CPU and there is no CPU execution path")


# ---- the two entry points of csrc/prune.hip on any flat vector ---------------------------------------------------------------

def prune_tensors(w: torch.Tensor, ranges: torch.Tensor, strategy: PruneStrategy, minimum_threshold: float = 0.0,
                  shrinkage: float = 1.0, shrinkage_threshold: float = 0.0, seed: int = 0, kth: Optional[torch.Tensor] = None,
                  thresholds: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """bf_op_prune_tensors on w (float32, device, pruned in place) with ranges = device int64 [T, 2].  DROP_BOTTOM takes kth = device
    int64 [T] (each 0 <= kth < size: the caller's check) and returns the thresholds it found (device float32 [T])."""
    if not (isinstance(w, torch.Tensor) and w.is_cuda and w.dtype == torch.float32 and w.dim() == 1):
        raise RuntimeError("prune_tensors needs a flat float32 tensor on the GPU: there is no CPU execution path")
    if not (ranges.is_cuda and ranges.dtype == torch.int64 and ranges.dim() == 2 and ranges.shape[1] == 2):
        raise ValueError("ranges must be a device int64 tensor of shape [T, 2]")
    T = int(ranges.shape[0])
    if T == 0 or w.numel() == 0:
        return thresholds
    if strategy == PruneStrategy.DROP_BOTTOM:
        if kth is None or not kth.is_cuda or kth.dtype != torch.int64 or kth.numel() != T:
            raise ValueError("DROP_BOTTOM needs kth: a device int64 tensor with one rank per tensor")
        if thresholds is None:
            thresholds = torch.empty(T, dtype=torch.float32, device=w.device)
        elif not thresholds.is_cuda or thresholds.dtype != torch.float32 or thresholds.numel() != T:
            raise ValueError("thresholds must be a device float32 tensor with one element per tensor")
    N.call("bf_op_prune_tensors", N.ptr(w), w.numel(), N.ptr(ranges), T, int(strategy.value), float(minimum_threshold),
           float(shrinkage), float(shrinkage_threshold), int(seed) & (2 ** 64 - 1),
           N.ptr(kth) if strategy == PruneStrategy.DROP_BOTTOM else None,
           N.ptr(thresholds) if strategy == PruneStrategy.DROP_BOTTOM else None, N.stream_ptr(w))
    return thresholds


def count_below(w: torch.Tensor, ranges: torch.Tensor, threshold: float = 0.0) -> torch.Tensor:
    """bf_op_count_below: per range the number of |w| <= threshold, as a device int64 [T] tensor"""
    if not (isinstance(w, torch.Tensor) and w.is_cuda and w.dtype == torch.float32 and w.dim() == 1):
        raise RuntimeError("count_below needs a flat float32 tensor on the GPU: there is no CPU execution path")
    T = int(ranges.shape[0])
    counts = torch.empty(T, dtype=torch.int64, device=w.device)
    if T and w.numel():
        N.call("bf_op_count_below", N.ptr(w), w.numel(), N.ptr(ranges), T, float(threshold), N.ptr(counts), N.stream_ptr(w))
    return counts


# ---- strategies -> steps -----------------------------------------------------------------------------------------------------

def _step(entry) -> Tuple[PruneStrategy, Dict]:
    """one {"type", "config"} entry -> (strategy, its arguments); everything that can be refused without a model is refused here"""
    strategy = PruneStrategy.from_string(entry[TYPE_STR])
    kwargs = entry[CONFIG_STR]
    if strategy == PruneStrategy.NONE:
        return strategy, {}
    if strategy == PruneStrategy.PCA_PROJECTION:
        raise NotImplementedError("prune strategy [PCA_PROJECTION] is not built: it is a host eigen-decomposition with "
                                  "scikit-learn semantics, outside the device path")
    if strategy == PruneStrategy.DROP_BOTTOM:
        percentage = float(kwargs["percentage"])
        if percentage >= 1.0:
            # int(np.round(n * percentage)) >= n for every tensor size n: NumPy's x_sorted[n] in the reference
            raise IndexError(f"drop_bottom percentage {percentage}: index n is out of bounds for axis 0 with size n")
        return strategy, {"percentage": percentage}
    if strategy == PruneStrategy.MINIMUM_THRESHOLD_SHRINKAGE:
        return strategy, {"shrinkage": float(kwargs["shrinkage"]), "minimum_threshold": float(kwargs["minimum_threshold"]),
                          "shrinkage_threshold": float(kwargs["shrinkage_threshold"])}
    return strategy, {"minimum_threshold": float(kwargs["minimum_threshold"])}


def prune_function_builder(config: Union[Dict, List[Dict]], seed: Optional[int] = None) -> Callable:
    """bfcnn/pruning.py:267-313: config = {"type": ..., "config": {...}} or a list of them, applied in order; returns
    prune(model) -> model, which prunes the model's convolution kernels in place on the GPU.  `seed` seeds the draws of
    MINIMUM_THRESHOLD_BIFURCATE (None: fresh entropy); every launch of that strategy takes the next 64-bit key of the sequence."""
    if config is None:
        raise ValueError("config cannot be None")
    if isinstance(config, list):
        steps = [_step(c) for c in config]
    elif isinstance(config, dict):
        steps = [_step(config)]
    else:
        raise ValueError(f"don't know how to handle [{config}]")
    rng = np.random.default_rng(seed)

    def prune(model):
        if model is None:
            raise ValueError("model cannot be None")
        hydra = _hydra_of(model)
        _require_gpu(hydra, "pruning")
        table = _table(hydra)
        launches = []
        for strategy, kw in steps:                          # every host-side refusal comes before the first launch
            if strategy == PruneStrategy.DROP_BOTTOM:
                launches.append((strategy, {"kth": table.ranks_device(kw["percentage"], hydra.params.device)}))
            elif strategy == PruneStrategy.MINIMUM_THRESHOLD_BIFURCATE:
                launches.append((strategy, dict(kw, seed=int(rng.integers(0, 2 ** 63)))))
            elif strategy != PruneStrategy.NONE:
                launches.append((strategy, kw))
        ranges = table.ranges(hydra.params.device)
        for strategy, kw in launches:
            prune_tensors(hydra.params, ranges, strategy, **kw)
        if launches:
            hydra.mark_dirty()
        return model

    prune.strategies = [s for s, _ in steps]
    return prune


# ---- reports -----------------------------------------------------------------------------------------------------------------

def get_conv2d_weights(model) -> np.ndarray:
    """bfcnn/pruning.py:319-352: the convolution kernels' weights concatenated into one vector, in variable order (one device gather,
    one copy)"""
    hydra = _hydra_of(model)
    table = _table(hydra)
    if len(table.names) == 0:
        return np.zeros(0, np.float32)
    return hydra.params.detach()[table.index(hydra.params.device)].cpu().numpy()


def conv2d_sparsity(model, threshold: float = 0.0) -> Dict:
    """{"tensors": {name: (count, size)}, "count", "size", "fraction"}: per convolution kernel and in total, the number of weights
    with |w| <= threshold (0: exact zeros) -- one launch of bf_op_count_below and one small copy"""
    hydra = _hydra_of(model)
    _require_gpu(hydra, "conv2d_sparsity")
    table = _table(hydra)
    counts = count_below(hydra.params, table.ranges(hydra.params.device), threshold).cpu().numpy()
    tensors = {n: (int(c), int(s)) for n, c, s in zip(table.names, counts, table.sizes)}
    count, size = int(counts.sum()), int(table.sizes.sum())
    return {"tensors": tensors, "count": count, "size": size, "fraction": count / size if size else 0.0}
