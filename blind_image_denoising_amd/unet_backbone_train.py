"""
Training of the plain U-Net backbone (`UnetHydra`, bfcnn/backbone_unet.py:18-268): bfcnn/train_loop.py:259-312 -- training-mode
forward (BatchNormalization on batch statistics, moving statistics updated), denoiser loss, the builder's regularisers and the
gradient of the total for every trainable tensor -- as an explicit forward / backward walk over the operator library, with the
parameter / state / gradient views of GenericResnetTrainGraph and the same backward primitives.  What the unet adds to the resnet
walk: the entry convolutions, MaxPooling2D (bf_op_maxpool2_bwd: the gradient goes to each window's first maximum in row-major
order, as TF and torch do), the nearest upsampling (bf_op_upsample2x_bwd) and the concat.  The training forward materialises the
concat (the entry's kernel gradient reads it); its data gradient is one convolution C -> 2C with the flipped, transposed kernel,
sliced into the upsampled half and the skip half.  A skip's gradient is the sum of the decoder's and the pooling's.

Exact fp32.  Gradients are compared with the torch-autograd oracle (tests/unet_backbone_torch.py) in
tests/test_gpu_unet_backbone.py.
"""
import ctypes as C
from typing import Dict

import numpy as np
import torch

from . import _native as N
from . import unet_laplacian as UL
from .resnet_generic import BN_EPSILON
from .resnet_generic_train import BN_MOMENTUM, CHANNELWISE_L1, MULTIPLIER_L1, REG_COEF, GenericResnetTrainGraph
from .unet_backbone import UnetHydra, upsample_concat
from .unet_train import _Ops, _call


class UnetTrainGraph(GenericResnetTrainGraph):
    """train_step_single_gpu for a UnetHydra: `step(gt, noisy, grads)` returns (prediction, loss slots, totals[3]) and fills `grads`
    (flat, laid out like model.params); model.state (moving statistics) is updated in place."""

    def __init__(self, model: UnetHydra, loss_config: Dict):
        super().__init__(model, loss_config)
        for a in model.block_activation + [model.base_activation, model.head_activation]:
            if UL._act(a)[0] == 3:
                raise NotImplementedError("unet training: GELU activations are outside the built graph")

    def regularizer(self, name: str, kind: str):
        """backbone_unet.py:108-125 (kernel_regularizer on every backbone convolution), backbone_blocks.py:146-160 (l2 on the gate),
        the denoiser's on the head, the multipliers' own L1 (backbone_unet.py:152-164)"""
        if kind == "bn_gamma":
            return None
        if kind in ("channelwise", "multiplier"):
            return kind
        if name.startswith("head/"):
            return self.m.config["denoiser"].get("kernel_regularizer", "l2")
        if "/gate/" in name:
            return "l2"
        return self.m.kernel_regularizer

    def step(self, gt: torch.Tensor, noisy: torch.Tensor, grads: torch.Tensor, depth_weight: float = 1.0, drop_scale=None):
        """drop_scale: {(group, block index): per-sample factor [B] on the device} = RandomOnOff's draw (0 or 1 / (1 - rate))"""
        m = self.m
        drop_scale = drop_scale or {}
        dev = m.device
        gt = gt.to(device=dev, dtype=torch.float32).contiguous()
        noisy = noisy.to(device=dev).contiguous()
        if noisy.dtype != torch.uint8:
            noisy = noisy.to(torch.float32)
        B, H, Wd, _ = noisy.shape
        m._check_size(H, Wd)
        npix = B * H * Wd
        L = N.lib()
        cmax = 2 * max([m.filters] + m.block_filters)
        need = max(8 * 1024 * 1024, int(L.bf_op_denoiser_loss_scratch_floats(B, H, Wd, m.out_channels)) + 1024, npix * 4,
                   int(L.bf_op_gate_scratch_floats(B, cmax)) + 64, int(L.bf_op_bn_train_scratch_floats(cmax)) + 64)
        if self.ops is None or self.ops.scratch.numel() < need:
            self.ops = _Ops(dev, need)
        ops = self.ops
        self._unaligned = []
        f32 = dict(dtype=torch.float32, device=dev)

        def pack(w2d):
            return UL.pack_pointwise(w2d.contiguous())

        def conv(name, x, act, bn=None):
            """k x k convolution (+ BatchNorm on batch statistics) + activation: (y, backward dy -> dx)"""
            w = self.W(name)
            kk, _, cin, cf = w.shape
            if bn is None:
                y = UL.conv2d(x, UL.pack_conv(w.contiguous()), cf, kk, 1, act)
            else:
                c = UL.conv2d(x, UL.pack_conv(w.contiguous()), cf, kk, 1, "linear")
                code, alpha = UL._act(act)
                gamma = self.W(bn + "/gamma")
                save = torch.empty(2 * cf, **f32)
                y = torch.empty_like(c)
                sp, sn = ops._s()
                _call("bf_op_bn_train_fwd", N.ptr(c), N.ptr(gamma), N.ptr(y), N.ptr(save), N.ptr(self.S(bn + "/moving_mean")),
                      N.ptr(self.S(bn + "/moving_variance")), c.numel() // cf, cf, BN_EPSILON, BN_MOMENTUM, code, alpha, sp, sn,
                      N.stream_ptr(c))

            def bwd(dy):
                g = ops.act_bwd(y, dy, act)
                if bn is not None:
                    dc = torch.empty_like(c)
                    sp, sn = ops._s()
                    _call("bf_op_bn_train_bwd", N.ptr(c), N.ptr(gamma), N.ptr(save), N.ptr(g), N.ptr(dc), N.ptr(self.G(bn + "/gamma", grads)),
                          c.numel() // cf, cf, sp, sn, N.stream_ptr(c))
                    g = dc
                Bc, Hc, Wc, _ = x.shape
                sp, sn = ops._s()
                _call("bf_op_conv2d_wgrad", N.ptr(x), 0, N.ptr(g), N.ptr(self.G(name, grads)), Bc, Hc, Wc, cin, cf, kk, 0, 0.0, 0.0,
                      sp, sn, N.stream_ptr(g))
                # data gradient = convolution with the taps flipped and every tap transposed
                wf = torch.empty_like(w)
                _call("bf_op_flip_hw", N.ptr(w), N.ptr(wf), kk, cin * cf, N.stream_ptr(w))
                wt = torch.empty((kk, kk, cf, cin), **f32)
                for t_ in range(kk * kk):
                    _call("bf_op_transpose2d", N.ptr(wf.view(kk * kk, cin, cf)[t_]), N.ptr(wt.view(kk * kk, cf, cin)[t_]), cin, cf,
                          N.stream_ptr(wf))
                return UL.conv2d(g, UL.pack_conv(wt), cin, kk, 1, "linear")
            return y, bwd

        def bn_step(base, x):
            """a standalone BatchNormalization (initial / final): (y, backward)"""
            Cc = x.shape[-1]
            gamma = self.W(base + "/gamma")
            save = torch.empty(2 * Cc, **f32)
            y = torch.empty_like(x)
            sp, sn = ops._s()
            _call("bf_op_bn_train_fwd", N.ptr(x), N.ptr(gamma), N.ptr(y), N.ptr(save), N.ptr(self.S(base + "/moving_mean")),
                  N.ptr(self.S(base + "/moving_variance")), x.numel() // Cc, Cc, BN_EPSILON, BN_MOMENTUM, 0, 0.0, sp, sn, N.stream_ptr(x))

            def bwd(dy):
                dx = torch.empty_like(x)
                sp, sn = ops._s()
                _call("bf_op_bn_train_bwd", N.ptr(x), N.ptr(gamma), N.ptr(save), N.ptr(dy), N.ptr(dx), N.ptr(self.G(base + "/gamma", grads)),
                      x.numel() // Cc, Cc, sp, sn, N.stream_ptr(x))
                return dx
            return y, bwd

        def mult_step(name, t, s_=None, pad_to=None):
            """Multiplier / ChannelwiseMultiplier t * relu(w0 + 1) [* RandomOnOff's per-sample factor]; name None: the factor alone.
            pad_to: the factor for the first entries of a zero-padded tensor, ones behind them"""
            Cc = t.shape[-1]
            cf = Cc if pad_to is None else pad_to
            mvec = None
            if name is not None:
                w0 = self.W(name)
                nw = w0.numel()
                mv = torch.empty(cf, **f32)
                _call("bf_op_relu_shift", N.ptr(w0), nw, 1.0, N.ptr(mv), cf, N.stream_ptr(mv))
                mvec = mv
                if cf < Cc:
                    ones = torch.ones(Cc - cf, **f32)
                    mvec = torch.empty(Cc, **f32)
                    _call("bf_op_concat_channels", N.ptr(mv), N.ptr(ones), None, N.ptr(mvec), 1, cf, Cc - cf, 0, N.stream_ptr(mv))
            y = ops.scale_add(None, t, mvec, s_)

            def bwd(dy):
                dm = torch.empty(Cc, **f32) if name is not None else None
                dt = ops.scale_add_bwd(t, mvec, s_, dy, dm)
                if name is not None:
                    _call("bf_op_relu_shift_bwd", N.ptr(w0), nw, 1.0, N.ptr(dm), N.ptr(self.G(name, grads)), cf, N.stream_ptr(dm))
                return dt
            return y, bwd

        nb = len(m.block_kernels)

        def blocks(f, pre):
            """resnet_blocks_full (backbone_blocks.py:163-246): (output, backward)"""
            back = []
            for i in range(m.no_layers):
                b = f"{pre}/block{i}"
                t, steps = f, []
                for j in range(nb):
                    t, b_ = conv(f"{b}/conv{j}/kernel", t, m.block_activation[j], f"{b}/bn{j}" if j >= 1 and m.use_bn else None)
                    steps.append(b_)
                    if j == 1 and m.add_gates:
                        w0, w1 = self.W(f"{b}/gate/dense0/kernel"), self.W(f"{b}/gate/dense1/kernel")
                        Cc, C8 = t.shape[-1], w0.shape[1]
                        gsave = torch.empty(int(L.bf_op_gate_save_floats(B, Cc, C8)), **f32)
                        gout = torch.empty_like(t)
                        hw = t.shape[1] * t.shape[2]
                        sp, sn = ops._s()
                        _call("bf_op_gate_fwd", N.ptr(t), N.ptr(w0), N.ptr(w1), None, N.ptr(gout), N.ptr(gsave), B, hw, Cc, C8, sp, sn,
                              N.stream_ptr(t))

                        def b_gate(dy, t=t, w0=w0, w1=w1, gsave=gsave, Cc=Cc, C8=C8, hw=hw, b=b):
                            dx = torch.empty_like(t)
                            sp, sn = ops._s()
                            _call("bf_op_gate_bwd", N.ptr(t), N.ptr(w0), N.ptr(w1), N.ptr(gsave), N.ptr(dy), N.ptr(dx),
                                  N.ptr(self.G(f"{b}/gate/dense0/kernel", grads)), N.ptr(self.G(f"{b}/gate/dense1/kernel", grads)),
                                  B, hw, Cc, C8, sp, sn, N.stream_ptr(t))
                            return dx
                        steps.append(b_gate)
                        t = gout
                ds_ = drop_scale.get((pre, i))
                if m.add_multiplier or ds_ is not None:                  # Multiplier, RandomOnOff in front of the Add (:219-225)
                    t, b_ = mult_step(f"{b}/multiplier/w0" if m.add_multiplier else None, t, ds_)
                    steps.append(b_)
                f = ops.add(f, t)

                def b_block(dout, steps=steps):
                    g = dout
                    for b_ in reversed(steps):
                        g = b_(g)
                    return ops.add(dout, g)
                back.append(b_block)

            def bwd(dout):
                for b_ in reversed(back):
                    dout = b_(dout)
                return dout
            return f, bwd

        # -- forward -------------------------------------------------------------------------------------------------------------
        Lv = m.no_levels
        ea = m.entry_activation
        f0 = UL.first_conv(noisy, self.W("base/kernel"), H, Wd, m.base_activation, True, m.v_min, m.v_max, arith=0)
        f, b_init = f0, None
        if m.add_initial_bn:
            f, b_init = bn_step("initial_bn", f)
        skips, enc = [], []
        for lv in range(Lv):
            b_entry, pooled_from = None, None
            if lv > 0:
                pooled_from = f
                f, b_entry = conv(f"enc{lv}/entry/kernel", UL.maxpool2(f), ea)
            f, b_blocks = blocks(f, f"enc{lv}")
            skips.append(f)
            enc.append((pooled_from, b_entry, b_blocks))
        dec = {}
        f = None
        for lv in reversed(range(Lv)):
            s = skips[lv]
            x_in = s if f is None else upsample_concat(f, s)
            small = None if f is None else f.shape
            f, b_entry = conv(f"dec{lv}/entry/kernel", x_in, ea)
            f, b_blocks = blocks(f, f"dec{lv}")
            dec[lv] = (small, b_entry, b_blocks)
        chain = []                                                   # closing layers: closures d(out) -> d(in)
        if m.add_final_bn:
            f, b_ = bn_step("final_bn", f)
            chain.append(b_)
        Cf = f.shape[-1]
        cf = Cf + (m.in_channels if m.add_concat_input else 0)
        Cp = next(c for c in (32, 64, 128, 256) if c >= cf)
        if m.add_concat_input:                                       # zero-padded to the width the head's matrix kernel takes
            cat = torch.empty((B, H, Wd, Cp), **f32)
            _call("bf_op_concat_input", N.ptr(f), N.ptr(noisy), int(noisy.dtype == torch.uint8), N.ptr(cat), B, H, Wd, H, Wd, Cf,
                  m.in_channels, Cp, m.v_min, m.v_max, N.stream_ptr(f))

            def b_cat(dcat):
                df = torch.empty((B, H, Wd, Cf), **f32)
                _call("bf_op_slice_channels", N.ptr(dcat), N.ptr(df), npix, Cp, 0, Cf, N.stream_ptr(dcat))
                return df
            chain.append(b_cat)
            f = cat
        for name_ in (["channelwise/w0"] if m.add_channelwise else []) + (["multiplier/w0"] if m.add_multiplier else []):
            f, b_ = mult_step(name_, f, None, cf)
            chain.append(b_)
        if m.add_clip:
            fin = f
            f = torch.empty_like(fin)
            v = fin.view(1, 1, -1, 32)
            _call("bf_op_dwconv_ln", N.ptr(v), N.ptr(f), None, None, 1, 1, v.shape[2], 32, 0, UL.LN_EPSILON, 4, 0.0, N.stream_ptr(fin))

            def b_clip(dy, y=f):
                dx = torch.empty_like(dy)
                _call("bf_op_act_bwd", N.ptr(y), N.ptr(dy), N.ptr(dx), dy.numel(), 4, 0.0, 1, N.stream_ptr(dy))
                return dx
            chain.append(b_clip)

        # -- head + loss (as GenericResnetTrainGraph) -----------------------------------------------------------------------------
        ld = N.LossDesc()
        ld.struct_size = C.sizeof(N.LossDesc)
        lc = self.loss_config
        ld.hinge, ld.cutoff = float(lc.get("hinge", 0.0)), float(lc.get("cutoff", 255.0))
        ld.mae_multiplier, ld.mse_multiplier = float(lc.get("mae_multiplier", 1.0)), float(lc.get("mse_multiplier", 0.0))
        ld.ssim_multiplier, ld.regularization = float(lc.get("ssim_multiplier", 0.0)), float(lc.get("regularization", 1.0))
        ld.depth_weight = float(depth_weight)
        w0 = self.W("head/conv0/kernel").view(-1, m.head_filters)
        Ch = int(f.shape[-1])
        if Ch != w0.shape[0]:                                        # zero rows for the padding channels
            w0p = torch.empty((Ch, m.head_filters), **f32)
            zrows = torch.zeros((Ch - w0.shape[0]) * m.head_filters, **f32)
            _call("bf_op_concat_channels", N.ptr(w0), N.ptr(zrows), None, N.ptr(w0p), 1, w0.numel(), zrows.numel(), 0, N.stream_ptr(w0))
            w0 = w0p
        w1 = self.W("head/conv1/kernel").view(m.head_filters, m.out_channels).contiguous()
        h0 = UL.pointwise(f, pack(w0), m.head_filters, m.head_activation)
        pred = UL.head_out(h0, w1, H, Wd, False, True, m.v_min, m.v_max)
        losses = torch.zeros(N.BF_LOSS_COUNT, **f32)
        dpred = torch.empty_like(pred)
        total = torch.zeros(3, **f32)
        sp, sn = ops._s()
        _call("bf_op_denoiser_loss", N.ptr(pred), N.ptr(gt), B, H, Wd, m.out_channels, C.byref(ld), N.ptr(dpred), N.ptr(losses), sp, sn,
              N.stream_ptr(pred))
        _call("bf_op_axpy", N.ptr(total), N.ptr(losses[N.BF_LOSS_TOTAL:N.BF_LOSS_TOTAL + 1]), 1.0, 0, 1, N.stream_ptr(total))
        dh0 = torch.empty_like(h0)
        sp, sn = ops._s()
        _call("bf_op_head_out_bwd", N.ptr(h0), N.ptr(w1), N.ptr(dpred), N.ptr(dh0), N.ptr(self.G("head/conv1/kernel", grads)), npix,
              m.head_filters, m.out_channels, 1, m.v_min, m.v_max, sp, sn, N.stream_ptr(h0))
        dh0p = ops.act_bwd(h0, dh0, m.head_activation)
        g0 = self.G("head/conv0/kernel", grads)
        if Ch * m.head_filters != g0.numel():                        # the padded rows' gradient is dropped
            gp = torch.empty(Ch * m.head_filters, **f32)
            ops.matmul_wgrad(f, dh0p, gp)
            _call("bf_op_slice_channels", N.ptr(gp), N.ptr(g0), 1, gp.numel(), 0, g0.numel(), N.stream_ptr(gp))
        else:
            ops.matmul_wgrad(f, dh0p, g0)
        g = UL.pointwise(dh0p, pack(ops.transpose(w0)), Ch)

        # -- backward ------------------------------------------------------------------------------------------------------------
        for b_ in reversed(chain):
            g = b_(g)
        dskip = {}
        for lv in range(Lv):                                         # decoder, shallowest first
            small, b_entry, b_blocks = dec[lv]
            g = b_entry(b_blocks(g))
            if small is None:                                        # the deepest level: the entry read the skip alone
                dskip[lv] = g
                break
            Bs, hs, ws, cu = small
            cs = skips[lv].shape[-1]
            dup, ds_ = torch.empty((Bs, 2 * hs, 2 * ws, cu), **f32), torch.empty_like(skips[lv])
            rows = Bs * 4 * hs * ws
            _call("bf_op_slice_channels", N.ptr(g), N.ptr(dup), rows, cu + cs, 0, cu, N.stream_ptr(g))
            _call("bf_op_slice_channels", N.ptr(g), N.ptr(ds_), rows, cu + cs, cu, cs, N.stream_ptr(g))
            dskip[lv] = ds_
            g = torch.empty(small, **f32)
            _call("bf_op_upsample2x_bwd", N.ptr(dup), N.ptr(g), Bs, hs, ws, cu, 0, N.stream_ptr(dup))
        g = dskip[Lv - 1]
        for lv in reversed(range(Lv)):                               # encoder, deepest first
            pooled_from, b_entry, b_blocks = enc[lv]
            g = b_blocks(g)
            if lv == 0:
                break
            g = b_entry(g)                                           # d pooled
            dx = torch.empty_like(pooled_from)
            Bq, Hq, Wq, Cq = pooled_from.shape
            _call("bf_op_maxpool2_bwd", N.ptr(pooled_from), N.ptr(g), N.ptr(dx), Bq, Hq, Wq, Cq, N.stream_ptr(g))
            g = ops.add(dx, dskip[lv - 1])                           # the skip's two consumers
        if b_init is not None:
            g = b_init(g)
        dpre = ops.act_bwd(f0, g, m.base_activation)
        sp, sn = ops._s()
        _call("bf_op_conv2d_wgrad", N.ptr(noisy), int(noisy.dtype == torch.uint8), N.ptr(dpre), N.ptr(self.G("base/kernel", grads)),
              B, H, Wd, m.in_channels, m.filters, m.kernel_size, 1, m.v_min, m.v_max, sp, sn, N.stream_ptr(dpre))

        # -- regularisers: value into total[1], gradients added times `regularization` ------------------------------------------
        reg = float(ld.regularization)
        n_mult = 0
        for name, shape, kind, off in m.trainable_variables:
            rk = self.regularizer(name, kind)
            if rk in (None, "none"):
                continue
            w = self.W(name)
            if rk in ("channelwise", "multiplier"):
                _call("bf_op_reg_elementwise", N.ptr(w), N.ptr(self._grad_view(name, grads)), int(np.prod(shape)), N.BF_REG_L1,
                      CHANNELWISE_L1 if rk == "channelwise" else MULTIPLIER_L1, reg, N.ptr(total[1:2]), N.stream_ptr(w))
                n_mult += rk == "multiplier"
                continue
            if rk not in ("l1", "l2"):
                raise NotImplementedError(f"regularizer {rk}")
            _call("bf_op_reg_elementwise", N.ptr(w), N.ptr(self._grad_view(name, grads)), int(np.prod(shape)),
                  N.BF_REG_L1 if rk == "l1" else N.BF_REG_L2, REG_COEF, reg, N.ptr(total[1:2]), N.stream_ptr(w))
        if n_mult:                                                   # L1(1.0) of each Multiplier's constant w1 = 1.0, no gradient
            ones = torch.ones(n_mult, **f32)
            _call("bf_op_reg_elementwise", N.ptr(ones), None, n_mult, N.BF_REG_L1, MULTIPLIER_L1, reg, N.ptr(total[1:2]), N.stream_ptr(ones))
        for buf, off, n in self._unaligned:
            grads[off:off + n].copy_(buf)
        _call("bf_op_axpy", N.ptr(total[2:3]), N.ptr(total[1:2]), reg, 0, 1, N.stream_ptr(total))
        _call("bf_op_axpy", N.ptr(total), N.ptr(total[2:3]), 1.0, 0, 1, N.stream_ptr(total))
        m.mark_dirty()                                               # the folded inference weights no longer match the state
        self.totals = total
        return pred, losses, total
