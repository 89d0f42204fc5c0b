"""What the training graphs of the operator-graph models share (resnet_generic_train, unet_backbone_train, unet_train): the
backward primitives as tensor-in / tensor-out calls (`Ops`), and on `TrainGraph` the parameter / state / gradient views, the
layers every family has -- activation, 1x1 / k x k / depthwise convolution, base convolution, denoiser head with its loss; each
a step returning (output, backward closure d output -> d input), its adjoint written once -- the regulariser loop and the
step's epilogue."""
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


def push(chain, step):
    """a step's output, its backward closure appended to chain"""
    chain.append(step[1])
    return step[0]


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

    def conv2d_wgrad(self, x, dy, dw, k, image_range=None):
        """the kernel gradient of a k x k convolution into dw; image_range (v_min, v_max): x is the image (uint8 or float32)
        that the base convolution normalises on its way in"""
        B, H, W, cin = x.shape
        sp, sn = self._s()
        v_min, v_max = image_range or (0.0, 0.0)
        call("bf_op_conv2d_wgrad", N.ptr(x), int(x.dtype == torch.uint8), N.ptr(dy), N.ptr(dw), B, H, W, cin, dy.shape[-1], k,
             int(image_range is not None), v_min, v_max, sp, sn, N.stream_ptr(dy))

    def flip_hw(self, w):
        """a [k, k, ...] kernel with its taps flipped in both directions"""
        k = w.shape[0]
        out = torch.empty_like(w)
        call("bf_op_flip_hw", N.ptr(w), N.ptr(out), k, w.numel() // (k * k), N.stream_ptr(w))
        return out

    def conv_kernel_t(self, w):
        """the kernel of a k x k convolution's data gradient: [k, k, cin, cout] with the taps flipped and every tap transposed"""
        k, _, cin, cout = w.shape
        wf = self.flip_hw(w).view(k * k, cin, cout)
        wt = torch.empty((k, k, cout, cin), dtype=torch.float32, device=w.device)
        for t in range(k * k):
            call("bf_op_transpose2d", N.ptr(wf[t]), N.ptr(wt.view(k * k, cout, cin)[t]), cin, cout, N.stream_ptr(wf))
        return wt

    def slice_channels(self, x, off, c, out=None):
        """x[..., off:off + c] (into out when given)"""
        ctot = x.shape[-1]
        if out is None:
            out = torch.empty(x.shape[:-1] + (c,), dtype=torch.float32, device=x.device)
        call("bf_op_slice_channels", N.ptr(x), N.ptr(out), x.numel() // ctot, ctot, off, c, N.stream_ptr(x))
        return out

    def concat_channels(self, a, b, c=None):
        """two or three tensors joined along their last axis"""
        ca, cb, cc = a.shape[-1], b.shape[-1], 0 if c is None else c.shape[-1]
        out = torch.empty(a.shape[:-1] + (ca + cb + cc,), dtype=torch.float32, device=a.device)
        call("bf_op_concat_channels", N.ptr(a), N.ptr(b), N.ptr(c), N.ptr(out), a.numel() // ca, ca, cb, cc, N.stream_ptr(a))
        return out

    def upsample2x_bwd(self, dy, bilinear):
        """the adjoint of the nearest / bilinear 2x up-sampling"""
        B, H, W, Cc = dy.shape
        out = torch.empty((B, H // 2, W // 2, Cc), dtype=torch.float32, device=dy.device)
        call("bf_op_upsample2x_bwd", N.ptr(dy), N.ptr(out), B, H // 2, W // 2, Cc, int(bilinear), N.stream_ptr(dy))
        return out

    def resize_bilinear_bwd(self, dy, h, w):
        """the adjoint of the bilinear resize of a [B, h, w, C] tensor to dy's size"""
        B, H, W, Cc = dy.shape
        out = torch.empty((B, h, w, Cc), dtype=torch.float32, device=dy.device)
        call("bf_op_resize_bilinear_bwd", N.ptr(dy), N.ptr(out), B, h, w, Cc, H, W, N.ptr(self.scratch), N.stream_ptr(dy))
        return out

    def maxpool2_bwd(self, x, dy):
        """the adjoint of MaxPooling2D(2, 2, same) on x: the gradient goes to each window's first maximum"""
        B, H, W, Cc = x.shape
        dx = torch.empty_like(x)
        call("bf_op_maxpool2_bwd", N.ptr(x), N.ptr(dy), N.ptr(dx), B, H, W, Cc, N.stream_ptr(dy))
        return dx


class TrainGraph:
    """train_step_single_gpu's graph walk for a model with flat `params` / `state`: W / S are views of a parameter / moving
    statistic by name, G the slice of the step's flat gradient (`grads`, laid out like model.params) its gradient is written to
    (`off` / `soff` / `numel`: offsets, shapes and sizes by name).  While a step runs, `ops` (the primitives), `grads` and `ld`
    (the loss descriptor) live on the graph."""

    def __init__(self, model, loss_config: Dict):
        self.m = model
        self.loss_config = dict(loss_config)
        self.off = {name: (off, shape, kind) for name, shape, kind, off in model.trainable_variables}
        self.soff = {name: (off, shape) for name, shape, off in model.non_trainable_variables}
        self.numel = {name: int(np.prod(shape)) for name, shape, *_ in list(model.trainable_variables) + list(model.non_trainable_variables)}
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
        t = self.m.params[off:off + self.numel[name]]
        if off % 4:
            t = t.clone()
        return t.view(shape)

    def S(self, name) -> torch.Tensor:
        off = self.soff[name][0]
        return self.m.state[off:off + self.numel[name]]

    def G(self, name) -> torch.Tensor:
        """the slice of the flat gradient a tensor's gradient is written to (16-byte aligned staging when the slice is not)"""
        off, n = self.off[name][0], self.numel[name]
        if off % 4:
            buf = torch.empty(n, dtype=torch.float32, device=self.grads.device)
            self._unaligned.append((buf, off, n))
            return buf
        return self.grads[off:off + n]

    def _grad_view(self, name):
        """a gradient written earlier in the step: its staging buffer, or its slice of the flat gradient"""
        off = self.off[name][0]
        for buf, o, nn in self._unaligned:
            if o == off:
                return buf
        return self.grads[off:off + self.numel[name]]

    # ---- the layers every family has: each returns (output, backward closure d output -> d input) ----------------------------
    def act_step(self, x, act: str, alpha=None):
        """the activation of x: a pre-activation tensor, the activation then its own pass, or a callable a -> tensor that runs an
        operator with the activation a fused into its epilogue.  The one home of the GELU rule: the sign-preserving activations
        stay fused and are differentiated from their output; GELU's derivative needs the pre-activation, so the operator runs
        linear, its result is kept and the activation is its own pass.  alpha: the slope the caller gave a fused leaky ReLU."""
        code = UL._act(act)[0]
        if callable(x) and code != 3:
            pre, y = None, x(act)
        else:
            pre = x("linear") if callable(x) else x
            y = pre if code == 0 else UL.dwconv_ln(pre.view(1, 1, -1, 32), None, None, act).view(pre.shape)
        if alpha is not None:
            return y, lambda dy: self.ops.act_bwd_alpha(y, dy, alpha)
        return y, lambda dy: self.ops.act_bwd(y, dy, act, pre)

    def conv1x1_step(self, name: str, x: torch.Tensor, cout: int, act: str, w2d=None, unpack=None, alpha=None):
        """1x1 convolution + activation.  w2d: the dense [cin, cout] kernel where the caller expanded a grouped kernel or padded
        one with zero rows; `unpack(dense gradient, G(name))` then maps its gradient back."""
        ops, cin = self.ops, x.shape[-1]
        w = self.W(name).view(cin, cout) if w2d is None else w2d
        y, b_act = self.act_step(lambda a: UL.pointwise(x, pack(w), cout, a, alpha=alpha), act, alpha)

        def bwd(dy):
            dp, g = b_act(dy), self.G(name)
            dense = g if unpack is None else torch.empty(w.numel(), **self.f32)
            ops.matmul_wgrad(x, dp, dense)
            if unpack is not None:
                unpack(dense, g)
            return UL.pointwise(dp, pack(ops.transpose(w)), cin)
        return y, bwd

    def conv_step(self, name: str, x: torch.Tensor, act: str, w=None, unpack=None):
        """k x k convolution, stride 1, same padding, + activation; w / unpack: the dense [k, k, cin, cout] kernel of a grouped
        convolution and the way back for its gradient, as in conv1x1_step.  The data gradient is the convolution with
        Ops.conv_kernel_t of the kernel."""
        ops = self.ops
        w = self.W(name) if w is None else w
        k, _, cin, cout = w.shape
        y, b_act = self.act_step(lambda a: UL.conv2d(x, UL.pack_conv(w.contiguous()), cout, k, 1, a), act)

        def bwd(dy):
            dp, g = b_act(dy), self.G(name)
            dense = g if unpack is None else torch.empty_like(w)
            ops.conv2d_wgrad(x, dp, dense, k)
            if unpack is not None:
                unpack(dense, g)
            return UL.conv2d(dp, UL.pack_conv(ops.conv_kernel_t(w)), cin, k, 1, "linear")
        return y, bwd

    def depthwise_step(self, name: str, x: torch.Tensor, k: int, dm: int = 1):
        """DepthwiseConv2D k x k (kernel [k, k, C, dm]).  With a depth multiplier the adjoint is the plain depthwise one of the
        channel-repeated input: [k, k, C * dm] and [k, k, C, dm] are the same memory, the data gradient is summed per group."""
        ops = self.ops
        B, H, Wd, Cc = x.shape
        w = self.W(name)
        y = UL.dwconv_mult(x, w, None)

        def bwd(dy):
            xr = x
            if dm != 1:
                xr = torch.empty((B, H, Wd, Cc * dm), **self.f32)
                call("bf_op_channel_repeat", N.ptr(x), N.ptr(xr), B * H * Wd, Cc, dm, N.stream_ptr(x))
            ops.dwconv_wgrad(xr, dy, self.G(name), k)
            dxr = UL.dwconv_mult(dy, ops.flip_hw(w).view(k, k, Cc * dm, 1), None)
            if dm == 1:
                return dxr
            dx = torch.empty_like(x)
            call("bf_op_channel_group_sum", N.ptr(dxr), N.ptr(dx), B * H * Wd, Cc, dm, N.stream_ptr(dxr))
            return dx
        return y, bwd

    def base_step(self, noisy: torch.Tensor, k: int, act: str):
        """the k x k base convolution + activation on the normalised image: (f, backward d f -> None: the kernel's gradient)"""
        m = self.m
        _, H, Wd, _ = noisy.shape
        wb = self.W("base/kernel")
        f, b_act = self.act_step(lambda a: UL.first_conv(noisy, wb, H, Wd, a, True, m.v_min, m.v_max, arith=0), act)
        return f, lambda df: self.ops.conv2d_wgrad(noisy, b_act(df), self.G("base/kernel"), k, (m.v_min, m.v_max))

    def head_step(self, prefix: str, f: torch.Tensor, gt: torch.Tensor, depth_weight: float, total: torch.Tensor):
        """the denoiser head `prefix` on f, its loss (self.ld) against gt times depth_weight added to total[0], and the head's
        backward: (prediction, loss slots, d f).  Where f is wider than the head's first kernel (the zero channels behind
        add_concat_input) the kernel gets zero rows, and their gradient is dropped."""
        m, ops = self.m, self.ops
        B, H, Wd, Ch = f.shape
        n0, hf = f"{prefix}/conv0/kernel", m.head_filters
        w0, unpack = self.W(n0).view(-1, hf), None
        if Ch != w0.shape[0]:
            w0 = ops.concat_channels(w0.view(-1), torch.zeros((Ch - w0.shape[0]) * hf, **self.f32)).view(Ch, hf)
            unpack = lambda dense, g: ops.slice_channels(dense, 0, g.numel(), out=g)
        w1 = self.W(f"{prefix}/conv1/kernel").view(hf, m.out_channels).contiguous()
        h0, b_conv0 = self.conv1x1_step(n0, f, hf, m.head_activation, w0, unpack)
        pred = UL.head_out(h0, w1, H, Wd, False, True, m.v_min, m.v_max)
        losses = torch.zeros(N.BF_LOSS_COUNT, **self.f32)
        dpred, dh0 = torch.empty_like(pred), torch.empty_like(h0)
        self.ld.depth_weight = float(depth_weight)
        sp, sn = ops._s()
        call("bf_op_denoiser_loss", N.ptr(pred), N.ptr(gt), B, H, Wd, m.out_channels, C.byref(self.ld), N.ptr(dpred), N.ptr(losses),
             sp, sn, N.stream_ptr(pred))
        call("bf_op_axpy", N.ptr(total), N.ptr(losses[N.BF_LOSS_TOTAL:N.BF_LOSS_TOTAL + 1]), 1.0, 0, 1, N.stream_ptr(total))
        call("bf_op_head_out_bwd", N.ptr(h0), N.ptr(w1), N.ptr(dpred), N.ptr(dh0), N.ptr(self.G(f"{prefix}/conv1/kernel")),
             B * H * Wd, hf, m.out_channels, 1, m.v_min, m.v_max, sp, sn, N.stream_ptr(h0))
        return pred, losses, b_conv0(dh0)

    # ---- regularisers and epilogue ------------------------------------------------------------------------------------------
    def regularizer(self, name: str, kind: str):
        """a graph's policy: ("l1" | "l2", coefficient) or ("soft_orthonormal", (lambda, l1, l2)) for a trainable tensor, None
        for one without a regulariser"""
        raise NotImplementedError

    def regularize(self, total: torch.Tensor) -> float:
        """the regularisers in inventory order: value into total[1], gradients added times `regularization` (returned)"""
        reg = float(self.ld.regularization)
        sob = None
        for name, shape, kind, off in self.m.trainable_variables:
            rule = self.regularizer(name, kind)
            if rule is None:
                continue
            w, g = self.W(name), self._grad_view(name)
            if rule[0] == "soft_orthonormal":
                sob = torch.empty(2 * 512 * 512, **self.f32) if sob is None else sob
                call("bf_op_reg_soft_orthonormal", N.ptr(w), N.ptr(g), shape[2], shape[3], *rule[1], reg, N.ptr(total[1:2]),
                     N.ptr(sob), N.stream_ptr(w))
            else:
                call("bf_op_reg_elementwise", N.ptr(w), N.ptr(g), self.numel[name], N.BF_REG_L1 if rule[0] == "l1" else N.BF_REG_L2,
                     rule[1], reg, N.ptr(total[1:2]), N.stream_ptr(w))
        return reg

    def _finish(self, total: torch.Tensor, reg: float):
        """the step's epilogue: staged gradients copied into place, total[2] = total[1] * regularization, total[0] += total[2]"""
        for buf, off, n in self._unaligned:
            self.grads[off:off + n].copy_(buf)
        call("bf_op_axpy", N.ptr(total[2:3]), N.ptr(total[1:2]), reg, 0, 1, N.stream_ptr(total))
        call("bf_op_axpy", N.ptr(total), N.ptr(total[2:3]), 1.0, 0, 1, N.stream_ptr(total))
        self.totals = total
