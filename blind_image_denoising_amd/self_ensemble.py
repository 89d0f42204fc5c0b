"""Self-ensemble inference ("x8" test-time augmentation): the denoiser runs on flips and rotations of the image, every result is
transformed back and the results are averaged.  Two kernels of csrc/self_ensemble.hip carry everything that is not the denoiser:
`bf_op_dihedral_stack_u8` (one read of the uint8 input, one write per member) and `bf_op_dihedral_merge` (one read per float
result, inverse transform, sequential sum in ascending k, mean, round half to even, cast, one write).

Transform numbering (the same in the C ABI, here, in DESIGN and in the tests), for k = 0..7 on x[B,H,W,C]:

    T_k(x) = flipW^(k >> 2)(rot90^(k & 3)(x))        rot90 = np.rot90(x, 1, axes=(1, 2)),  flipW = x[:, :, ::-1]

Odd k swaps H and W.  Layout of a set of members: the even ones in one batch [n_even*B, H, W, C], the odd ones in another
[n_odd*B, W, H, C], each member-major in ascending k; for H == W there is also the joint layout, every member in one batch
[n*B, H, W, C], member-major in ascending k."""
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _args as A
from . import _native as N
from .module_denoiser import DenoiserModule, DenoiserWrapper

TRANSFORM_SETS = {"d4": (0, 1, 2, 3, 4, 5, 6, 7), "flips": (0, 2, 4, 6)}
_FEATURE = "the dihedral transform"


def parse_transforms(transforms) -> Tuple[int, ...]:
    """"d4", "flips" or a non-empty sequence of distinct ints in 0..7 -> the member numbers, sorted"""
    if isinstance(transforms, str):
        if transforms not in TRANSFORM_SETS:
            raise ValueError(f"transforms must be one of {sorted(TRANSFORM_SETS)} or a sequence of ints in 0..7, got {transforms!r}")
        return TRANSFORM_SETS[transforms]
    try:
        ks = list(transforms)
    except TypeError:
        raise ValueError(f"transforms must be 'd4', 'flips' or a sequence of ints in 0..7, got {transforms!r}") from None
    if not ks:
        raise ValueError("transforms must name at least one member")
    for k in ks:
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= int(k) <= 7:
            raise ValueError(f"transforms must be ints in 0..7, got {k!r}")
    ks = sorted(int(k) for k in ks)
    if len(set(ks)) != len(ks):
        raise ValueError(f"transforms must be distinct, got {list(transforms)}")
    return tuple(ks)


def _mask(ks: Sequence[int]) -> int:
    return sum(1 << k for k in ks)


def _device_batch(t, dtype, what: str):
    return A.to_device(A.image_batch(t, what, (dtype,)), False, None, what, _FEATURE)


def dihedral_stack_u8(image_u8: torch.Tensor, members, joint: bool = False) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """bf_op_dihedral_stack_u8 on a uint8 device tensor [B,H,W,C] (C = 1 or 3): (even batch [n_even*B,H,W,C] or None, odd batch
    [n_odd*B,W,H,C] or None), member-major in ascending k.  joint=True (H == W only): (all members [n*B,H,W,C], None)."""
    ks = parse_transforms(members)
    image_u8 = _device_batch(image_u8, torch.uint8, "image_u8").contiguous()
    B, H, W, C = image_u8.shape
    n_odd = sum(k & 1 for k in ks)
    n_even = len(ks) - n_odd
    new = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=image_u8.device)
    if joint:
        if H != W:
            raise ValueError(f"the joint layout needs H == W, got {H} x {W}")
        even, odd = new(len(ks) * B, H, W, C), None
    else:
        even = new(n_even * B, H, W, C) if n_even else None
        odd = new(n_odd * B, W, H, C) if n_odd else None
    N.call("bf_op_dihedral_stack_u8", N.ptr(image_u8), N.ptr(even), N.ptr(odd), B, H, W, C, _mask(ks), N.stream_ptr(image_u8))
    return even, odd


def dihedral_merge(even_f32: Optional[torch.Tensor], odd_f32: Optional[torch.Tensor], members, B: int, H: int, W: int,
                   cast_to_uint8: bool = True) -> torch.Tensor:
    """bf_op_dihedral_merge on the float32 device results of the members, laid out as dihedral_stack_u8 lays the members out (odd_f32
    = None while odd members are selected: the joint layout in even_f32): per element the sequential fp32 sum of the members at
    their inverse-transformed positions in ascending k, divided by their number; [B,H,W,C] float32, or rounded half to even and
    clipped to uint8."""
    ks = parse_transforms(members)
    B, H, W = int(B), int(H), int(W)
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"B, H, W must be at least 1, got {B}, {H}, {W}")
    n_odd = sum(k & 1 for k in ks)
    n_even = len(ks) - n_odd
    joint = n_odd > 0 and odd_f32 is None
    if joint and H != W:
        raise ValueError(f"the joint layout (odd members without an odd batch) needs H == W, got {H} x {W}")
    first = even_f32 if even_f32 is not None else odd_f32
    if first is None:
        raise ValueError("no member batch was given")
    _device_batch(first, torch.float32, "member batch")
    C = int(first.shape[-1])
    want_even = (len(ks) * B, H, W, C) if joint else (n_even * B, H, W, C) if n_even else None
    want_odd = (n_odd * B, W, H, C) if n_odd and not joint else None
    for t, want, what in ((even_f32, want_even, "even_f32"), (odd_f32, want_odd, "odd_f32")):
        if want is None:
            if t is not None:
                raise ValueError(f"{what} was given but members {list(ks)} put nothing there")
            continue
        if t is None:
            raise ValueError(f"{what} is missing for members {list(ks)}")
        _device_batch(t, torch.float32, what)
        if tuple(t.shape) != want or t.device != first.device:
            raise ValueError(f"{what} must be {want} on {first.device} for members {list(ks)}, got {tuple(t.shape)} on {t.device}")
    even_f32 = None if even_f32 is None else even_f32.contiguous()
    odd_f32 = None if odd_f32 is None else odd_f32.contiguous()
    out = torch.empty((B, H, W, C), dtype=torch.uint8 if cast_to_uint8 else torch.float32, device=first.device)
    N.call("bf_op_dihedral_merge", N.ptr(even_f32), N.ptr(odd_f32), N.ptr(out), B, H, W, C, _mask(ks), int(bool(cast_to_uint8)),
           N.stream_ptr(first))
    return out


def parse_setting(self_ensemble) -> Optional[dict]:
    """load_model's `self_ensemble`: None -> None; everything parse_transforms takes -> those transforms.  Checked here, before
    anything is loaded."""
    return None if self_ensemble is None else {"transforms": parse_transforms(self_ensemble)}


class SelfEnsembleDenoiserModule(DenoiserWrapper):
    """A DenoiserModule run on the members T_k of the image, k in `transforms`, and averaged: uint8 [B,H,W,C] -> uint8 [B,H,W,C]
    (float32, not rounded, with cast_to_uint8=False).  Argument checks, input handling, return types and f16-range status as
    every wrapper (DenoiserWrapper); the module itself must be a DenoiserModule.

    A call is: dihedral_stack_u8, one call of DenoiserModule(hydra, cast_to_uint8=False) per batch of members, dihedral_merge.
    Batching contract: for H == W every member goes through ONE hydra call on [n*B, H, W, C], member-major in ascending k;
    otherwise the even members go through one call on [n_even*B, H, W, C] and the odd ones through another on [n_odd*B, W, H, C]
    (a batch with no members is not called).  The merge adds the members' results in ascending k, sequentially in fp32, divides by
    their number and rounds half to even: `transforms=[0]` returns exactly what DenoiserModule(hydra, cast_to_uint8) returns."""
    SETTINGS = ("transforms",)

    def __init__(self, module: DenoiserModule, transforms="d4", cast_to_uint8: bool = True):
        if not isinstance(module, DenoiserModule):
            raise ValueError("module must be a DenoiserModule")
        self._transforms = parse_transforms(transforms)
        self._wrap(module, cast_to_uint8)
        self._inner = self._float                       # shares the status record: check_status() sees the inner calls

    def __call__(self, image):
        image, was_numpy = self._checked_input(image)
        if image.shape[0] == 0:
            return self._empty_output(image, was_numpy)
        image = self._place(image, was_numpy, "image", _FEATURE)
        B, H, W, _ = image.shape
        batches = dihedral_stack_u8(image, self._transforms, joint=H == W)
        results = []
        for batch in batches:
            results.append(None if batch is None else self._inner(batch))
            if batch is not None and self._repeat_in_fp32(was_numpy):
                return self(image.cpu().numpy())
        return self._deliver(dihedral_merge(results[0], results[1], self._transforms, B, H, W, self._cast_to_uint8), was_numpy)
