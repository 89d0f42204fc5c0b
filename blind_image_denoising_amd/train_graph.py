"""What the training graphs of the operator-graph models share (resnet_generic_train, unet_backbone_train, unet_train): the
backward primitives as tensor-in / tensor-out calls (`Ops`) and the parameter / state / gradient views with the step's epilogue
(`TrainGraph`)."""
import ctypes as C
from typing import Dict

import numpy as np
import torch

from . import _native as N
from . import unet_laplacian as UL
from ._native import call


def pack(w2d: torch.Tensor) -> torch.Tensor:
    """a [cin, cout] kernel as the operand of a 1x1 convolution"""
    return UL.pack_pointwise(w2d.contiguous())


class Ops:
    """the backward primitives as tensor-in / tensor-out calls sharing one scratch buffer"""

    def __init__(self, device, scratch_floats: int):
        self.device = device
        self.scratch = torch.empty(int(scratch_floats), dtype=torch.float32, device=device)

    def _s(self):
        return N.ptr(self.scratch), self.scratch.numel()

    def act_bwd(self, out, dy, act, pre=None):
        """dy * act'(.): from the activation's OUTPUT for the sign-preserving ones, from its input `pre` for GELU"""
        code, a = UL._act(act)
        if code == 0:
            return dy
        dx = torch.empty_like(dy)
        if code == 3:
            if pre is None:
                raise ValueError("the GELU derivative needs the pre-activation")
            call("bf_op_act_bwd", N.ptr(pre), N.ptr(dy), N.ptr(dx), dy.numel(), code, a, 0, N.stream_ptr(dy))
        else:
            call("bf_op_act_bwd", N.ptr(out), N.ptr(dy), N.ptr(dx), dy.numel(), code, a, 1, N.stream_ptr(dy))
        return dx

    def act_bwd_alpha(self, out, dy, alpha):
        dx = torch.empty_like(dy)
        call("bf_op_act_bwd", N.ptr(out), N.ptr(dy), N.ptr(dx), dy.numel(), 2, float(alpha), 1, N.stream_ptr(dy))
        return dx

    def matmul_wgrad(self, x, dy, dw):
        cin, cout = x.shape[-1], dy.shape[-1]
        sp, sn = self._s()
        call("bf_op_matmul_wgrad", N.ptr(x), N.ptr(dy), N.ptr(dw), x.numel() // cin, cin, cout, sp, sn, N.stream_ptr(x))

    def dwconv_wgrad(self, x, dy, dw, k):
        B, H, W, Cc = x.shape
        sp, sn = self._s()
        call("bf_op_dwconv_wgrad", N.ptr(x), N.ptr(dy), N.ptr(dw), B, H, W, Cc, k, sp, sn, N.stream_ptr(x))

    def layernorm_bwd(self, x, gamma, dy, dgamma):
        Cc = x.shape[-1]
        dx = torch.empty_like(x)
        sp, sn = self._s()
        call("bf_op_layernorm_bwd", N.ptr(x), N.ptr(gamma), N.ptr(dy), N.ptr(dx), N.ptr(dgamma), x.numel() // Cc, Cc, UL.LN_EPSILON,
             sp, sn, N.stream_ptr(x))
        return dx

    def scale_add(self, res, t, m, s):
        B = t.shape[0]
        Cc = t.shape[-1]
        out = torch.empty_like(t)
        call("bf_op_scale_add", N.ptr(res), N.ptr(t), N.ptr(m), N.ptr(s), N.ptr(out), B, t.numel() // (B * Cc), Cc, N.stream_ptr(t))
        return out

    def scale_add_bwd(self, t, m, s, dy, dm):
        B, Cc = t.shape[0], t.shape[-1]
        dt = torch.empty_like(t)
        sp, sn = self._s()
        call("bf_op_scale_add_bwd", N.ptr(t), N.ptr(m), N.ptr(s), N.ptr(dy), N.ptr(dt), N.ptr(dm), B, t.numel() // (B * Cc), Cc,
             sp, sn, N.stream_ptr(t))
        return dt

    def add(self, a, b):
        """a + b (new tensor)"""
        return self.scale_add(a, b, None, None)

    def transpose(self, w2d):
        a, b = w2d.shape
        out = torch.empty((b, a), dtype=torch.float32, device=w2d.device)
        call("bf_op_transpose2d", N.ptr(w2d), N.ptr(out), a, b, N.stream_ptr(w2d))
        return out


class TrainGraph:
    """train_step_single_gpu's graph walk for a model with flat `params` / `state`: W / S are views of a parameter / moving
    statistic by name, G the slice of the step's flat gradient (`grads`, laid out like model.params) its gradient is written to.
    While a step runs, `ops` (the primitives), `grads` and `ld` (the loss descriptor) live on the graph."""

    def __init__(self, model, loss_config: Dict):
        self.m = model
        self.loss_config = dict(loss_config)
        self.off = {name: (off, shape, kind) for name, shape, kind, off in model.trainable_variables}
        self.soff = {name: (off, shape) for name, shape, off in model.non_trainable_variables}
        self.f32 = dict(dtype=torch.float32, device=model.device)
        self.ops = None
        self.totals = None

    def _inputs(self, gt: torch.Tensor, noisy: torch.Tensor):
        """the batch on the model's device: gt float32, noisy uint8 or float32"""
        dev = self.m.device
        gt = gt.to(device=dev, dtype=torch.float32).contiguous()
        noisy = noisy.to(device=dev).contiguous()
        if noisy.dtype != torch.uint8:
            noisy = noisy.to(torch.float32)
        return gt, noisy

    def _begin(self, grads: torch.Tensor, scratch_floats: int) -> Ops:
        """a step starts: the primitives with at least `scratch_floats` of scratch, no staged gradients yet"""
        if self.ops is None or self.ops.scratch.numel() < scratch_floats:
            self.ops = Ops(self.m.device, scratch_floats)
        self._unaligned = []
        self.grads = grads
        return self.ops

    def _loss_desc(self, ssim_multiplier: float) -> N.LossDesc:
        """the denoiser loss of loss_config (ssim_multiplier: its default); depth_weight is set per output"""
        ld = N.LossDesc()
        ld.struct_size = C.sizeof(N.LossDesc)
        lc = self.loss_config
        ld.hinge, ld.cutoff = float(lc.get("hinge", 0.0)), float(lc.get("cutoff", 255.0))
        ld.mae_multiplier, ld.mse_multiplier = float(lc.get("mae_multiplier", 1.0)), float(lc.get("mse_multiplier", 0.0))
        ld.ssim_multiplier, ld.regularization = float(lc.get("ssim_multiplier", ssim_multiplier)), float(lc.get("regularization", 1.0))
        return ld

    # ---- parameters / state / gradients -------------------------------------------------------------------------------------
    def W(self, name) -> torch.Tensor:
        off, shape, _ = self.off[name]
        n = int(np.prod(shape))
        t = self.m.params[off:off + n]
        if off % 4:
            t = t.clone()
        return t.view(shape)

    def S(self, name) -> torch.Tensor:
        off, shape = self.soff[name]
        return self.m.state[off:off + int(np.prod(shape))]

    def G(self, name) -> torch.Tensor:
        """the slice of the flat gradient a tensor's gradient is written to (16-byte aligned staging when the slice is not)"""
        off, shape, _ = self.off[name]
        n = int(np.prod(shape))
        if off % 4:
            buf = torch.empty(n, dtype=torch.float32, device=self.grads.device)
            self._unaligned.append((buf, off, n))
            return buf
        return self.grads[off:off + n]

    def _grad_view(self, name):
        """a gradient written earlier in the step: its staging buffer, or its slice of the flat gradient"""
        off, shape, _ = self.off[name]
        for buf, o, nn in self._unaligned:
            if o == off:
                return buf
        return self.grads[off:off + int(np.prod(shape))]

    def _finish(self, total: torch.Tensor, reg: float):
        """the step's epilogue: staged gradients copied into place, total[2] = total[1] * regularization, total[0] += total[2]"""
        for buf, off, n in self._unaligned:
            self.grads[off:off + n].copy_(buf)
        call("bf_op_axpy", N.ptr(total[2:3]), N.ptr(total[1:2]), reg, 0, 1, N.stream_ptr(total))
        call("bf_op_axpy", N.ptr(total), N.ptr(total[2:3]), 1.0, 0, 1, N.stream_ptr(total))
        self.totals = total
