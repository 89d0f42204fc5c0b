"""The argument checks of the wrappers around the denoiser, once.  Everything here runs before the GPU is touched and raises
ValueError naming the offending argument; only `to_device` and `device_of` look for a device, and theirs is the one RuntimeError
every feature raises for data that is well-formed but on the host: "... must live on the GPU: ... has no CPU execution path"."""
import math

import numpy as np
import torch

_REAL = (int, float, np.integer, np.floating)


def _got(x) -> str:
    return f"{getattr(x, 'dtype', type(x))} {tuple(getattr(x, 'shape', ()))}"


def image_batch(t, what: str, dtypes, *, min_hw: int = 1, even: bool = False, allow_empty: bool = False, channels=(1, 4)):
    """`t` is a torch tensor [B,H,W,C] of one of `dtypes` with channels[0]..channels[1] channels, H and W >= min_hw (both even
    with `even`) and, unless `allow_empty`, at least one image; returns it"""
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or t.dim() != 4:
        raise ValueError(f"{what} must be a [B,H,W,C] batch of dtype {' or '.join(str(d) for d in dtypes)}, got {_got(t)}")
    B, H, W, C = t.shape
    if not channels[0] <= C <= channels[1]:
        raise ValueError(f"{what} must have {channels[0]}..{channels[1]} channels, got {tuple(t.shape)}")
    if H < min_hw or W < min_hw or (even and (H % 2 or W % 2)):
        raise ValueError(f"{what} must be at least {min_hw} x {min_hw}{' and of even height and width' if even else ''}, "
                         f"got {tuple(t.shape)}")
    if B < 1 and not allow_empty:
        raise ValueError(f"{what} must hold at least one image, got {tuple(t.shape)}")
    return t


def host_or_device(x, what: str, dtypes, **rules):
    """image_batch for a torch tensor or a NumPy array: (the tensor, whether NumPy was given).  An array is wrapped, not uploaded"""
    was_numpy = isinstance(x, np.ndarray)
    if was_numpy:
        try:
            x = torch.from_numpy(np.ascontiguousarray(x))
        except TypeError:                                        # a dtype torch does not have
            raise ValueError(f"{what} must be a [B,H,W,C] batch of dtype {' or '.join(str(d) for d in dtypes)}, got {_got(x)}") from None
    return image_batch(x, what, dtypes, **rules), was_numpy


def uint8_batches(batches, what: str, min_hw: int = 1, missing: str = ""):
    """every element of an iterable of uint8 batches, host or device, as a checked tensor; ValueError when there is none"""
    checked = [host_or_device(b, what, (torch.uint8,), min_hw=min_hw)[0] for b in batches]
    if not checked:
        raise ValueError(missing or f"no {what} to evaluate on")
    return checked


def _no_cpu_path(what: str, feature: str) -> RuntimeError:
    return RuntimeError(f"{what} must live on the GPU: {feature} has no CPU execution path")


def device_of(module=None, feature: str = "the engine") -> torch.device:
    """the CUDA device of the module's model, else the current one; the RuntimeError of to_device when there is neither"""
    dev = getattr(getattr(module, "model_hydra", None), "device", None)
    if dev is not None and torch.device(dev).type == "cuda":
        return torch.device(dev)
    if not torch.cuda.is_available():
        raise _no_cpu_path("images", feature)
    return torch.device("cuda", torch.cuda.current_device())


def to_device(t: torch.Tensor, was_numpy: bool, device, what: str, feature: str) -> torch.Tensor:
    """the upload rule: what came as NumPy is uploaded (to `device`, None = the current one); a host tensor is not"""
    if t.is_cuda:
        return t
    if not was_numpy:
        raise _no_cpu_path(what, feature)
    return t.to(device_of(None, feature) if device is None else device)


def int_in(value, what: str, lo: int, hi=None) -> int:
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or int(value) < lo or (hi is not None and int(value) > hi):
        raise ValueError(f"{what} must be an int {f'in {lo}..{hi}' if hi is not None else f'>= {lo}'}, got {value!r}")
    return int(value)


def seed64(value) -> int:
    return int_in(value, "seed", 0, 2 ** 64 - 1)


def non_negative_float(value, what: str, top=None) -> float:
    if isinstance(value, bool) or not isinstance(value, _REAL) or not math.isfinite(value) or value < 0 \
            or (top is not None and value > top):
        raise ValueError(f"{what} must be a finite float {'>= 0' if top is None else f'in 0..{top}'}, got {value!r}")
    return float(value)


def one_of(value, what: str, choices):
    if not isinstance(value, str) or value not in choices:
        raise ValueError(f"{what} must be one of {list(choices)}, got {value!r}")
    return value


def broadcasts_to(shape, B: int, C: int, what: str):
    """a float, [C] or [B,C]: the shapes a per-image, per-channel parameter may be given in"""
    if tuple(shape) not in ((), (C,), (B, C)):
        raise ValueError(f"{what} must be a float, [{C}] or [{B}, {C}] for this batch, got {tuple(shape)}")


def per_image_channel(value, B: int, C: int, what: str) -> torch.Tensor:
    """a float, [C] or [B,C], finite and non-negative, as a contiguous float64 [B,C] tensor where it was given (host or device)"""
    try:
        s = torch.as_tensor(value).to(torch.float64)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"{what} must be a float, a [C] or a [B, C] array, got {type(value)}") from None
    broadcasts_to(s.shape, B, C, what)
    s = s.expand(B, C)
    if s.numel() and not bool((torch.isfinite(s) & (s >= 0)).all()):
        raise ValueError(f"{what} must be finite and non-negative")
    return s.contiguous()


def parse_setting(value, option: str, expected: str, settings, check=None, shorthand=None, bools: bool = True):
    """load_model's `option` as the keyword arguments of its wrapper, None for no wrapper: None | False -> None; True -> {} (the
    defaults); a dict whose keys are among `settings` -> a copy of it, once check(**it) has passed (its ValueError is prefixed
    "<option>: ").  With `shorthand`, what is no dict, True included, stands for the dict shorthand(value), or for none where
    that is None; without `bools` a bool is a wrong type.  Every other value: ValueError "<option> must be <expected>, got ...".  Everything is
    checked here, before anything is loaded."""
    if value is None or (bools and value is False):
        return None
    given = value
    if shorthand is not None and not isinstance(value, dict):
        value = shorthand(value)
    elif bools and value is True:
        value = {}
    if not isinstance(value, dict):
        raise ValueError(f"{option} must be {expected}, got {given!r}")
    if set(value) - set(settings):
        raise ValueError(f"{option} may set {', '.join(settings)}, got {sorted(value)}")
    if check is not None:
        try:
            check(**value)
        except ValueError as e:
            raise ValueError(f"{option}: {e}") from None
    return dict(value)


def module_result(result, dtype, shape, *, hint: str = ""):
    """what a module handed back for a uint8 batch of `shape` is a tensor of `dtype` and that shape; returns it"""
    if not isinstance(result, torch.Tensor) or result.dtype != dtype or tuple(result.shape) != tuple(shape):
        raise ValueError(f"the module returned {_got(result)} for a uint8 {tuple(shape)} batch; {dtype} of the same shape is "
                         f"needed{hint}")
    return result
