"""
Training of the plain U-Net backbone (`UnetHydra`, bfcnn/backbone_unet.py:18-268): bfcnn/train_loop.py:259-312 -- training-mode
forward (BatchNormalization on batch statistics, moving statistics updated), denoiser loss, the builder's regularisers and the
gradient of the total for every trainable tensor -- as an explicit forward / backward walk over the operator library, with the
parameter / state / gradient views and the shared steps of train_graph.TrainGraph (k x k convolution, base, head and loss,
regulariser loop) and those of GenericResnetTrainGraph (BatchNorm, multipliers, gate, closing layers).  What the unet adds to the
resnet walk: the entry convolutions, MaxPooling2D (Ops.maxpool2_bwd: the gradient goes to each window's first maximum in row-major
order, as TF and torch do), the nearest upsampling (Ops.upsample2x_bwd) and the concat.  The training forward materialises the
concat (the entry's kernel gradient reads it); its data gradient is one convolution C -> 2C with the flipped, transposed kernel,
sliced into the upsampled half and the skip half.  A skip's gradient is the sum of the decoder's and the pooling's.

Exact fp32.  Gradients are compared with the torch-autograd oracle (tests/unet_backbone_torch.py) in
tests/test_gpu_unet_backbone.py.
"""
from typing import Dict

import torch

from . import _native as N
from . import unet_laplacian as UL
from ._native import call
from .resnet_generic_train import GenericResnetTrainGraph
from .train_graph import push
from .unet_backbone import UnetHydra, upsample_concat


class UnetBackboneTrainGraph(GenericResnetTrainGraph):
    """train_step_single_gpu for a UnetHydra: `step(gt, noisy, grads)` returns (prediction, loss slots, totals[3]) and fills `grads`
    (flat, laid out like model.params); model.state (moving statistics) is updated in place."""

    def __init__(self, model: UnetHydra, loss_config: Dict):
        super().__init__(model, loss_config)
        for a in model.block_activation + [model.base_activation, model.head_activation]:
            if UL._act(a)[0] == 3:
                raise NotImplementedError("unet training: GELU activations are outside the built graph")

    def kernel_regularizer(self, name: str):
        """backbone_unet.py:108-125 (kernel_regularizer on every backbone convolution), backbone_blocks.py:146-160 (l2 on the gate),
        the denoiser's on the head"""
        if name.startswith("head/"):
            return self.m.config["denoiser"].get("kernel_regularizer", "l2")
        return "l2" if "/gate/" in name else self.m.kernel_regularizer

    def conv(self, name: str, x: torch.Tensor, act: str, bn=None):
        """k x k convolution (+ BatchNorm on batch statistics) + activation: (y, backward dy -> dx)"""
        if bn is None:
            return self.conv_step(name, x, act)
        c, b_conv = self.conv_step(name, x, "linear")
        y, b_bn = self.bn_step(bn, c, act)
        return y, lambda dy: b_conv(b_bn(dy))

    def blocks(self, f: torch.Tensor, pre: str, drop_scale):
        """resnet_blocks_full (backbone_blocks.py:163-246): (output, backward)"""
        m, ops = self.m, self.ops
        back = []
        for i in range(m.no_layers):
            b = f"{pre}/block{i}"
            t, steps = f, []
            for j in range(len(m.block_kernels)):
                t = push(steps, self.conv(f"{b}/conv{j}/kernel", t, m.block_activation[j], f"{b}/bn{j}" if j >= 1 and m.use_bn else None))
                if j == 1 and m.add_gates:
                    t = push(steps, self.gate_step(b, t))
            ds_ = drop_scale.get((pre, i))
            if m.add_multiplier or ds_ is not None:                  # Multiplier, RandomOnOff in front of the Add (:219-225)
                t = push(steps, self.mult_step(f"{b}/multiplier/w0" if m.add_multiplier else None, t, ds_))
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

    def step(self, gt: torch.Tensor, noisy: torch.Tensor, grads: torch.Tensor, depth_weight: float = 1.0, drop_scale=None):
        """drop_scale: {(group, block index): per-sample factor [B] on the device} = RandomOnOff's draw (0 or 1 / (1 - rate))"""
        m = self.m
        drop_scale = drop_scale or {}
        gt, noisy = self._inputs(gt, noisy)
        B, H, Wd, _ = noisy.shape
        m._check_size(H, Wd)
        npix = B * H * Wd
        L = N.lib()
        cmax = 2 * max([m.filters] + m.block_filters)
        ops = self._begin(grads, max(8 * 1024 * 1024, int(L.bf_op_denoiser_loss_scratch_floats(B, H, Wd, m.out_channels)) + 1024,
                                     npix * 4, int(L.bf_op_gate_scratch_floats(B, cmax)) + 64, int(L.bf_op_bn_train_scratch_floats(cmax)) + 64))

        # -- forward -------------------------------------------------------------------------------------------------------------
        Lv = m.no_levels
        ea = m.entry_activation
        f, b_base = self.base_step(noisy, m.kernel_size, m.base_activation)
        b_init = None
        if m.add_initial_bn:
            f, b_init = self.bn_step("initial_bn", f, "linear")
        skips, enc = [], []
        for lv in range(Lv):
            b_entry, pooled_from = None, None
            if lv > 0:
                pooled_from = f
                f, b_entry = self.conv(f"enc{lv}/entry/kernel", UL.maxpool2(f), ea)
            f, b_blocks = self.blocks(f, f"enc{lv}", drop_scale)
            skips.append(f)
            enc.append((pooled_from, b_entry, b_blocks))
        dec = {}
        f = None
        for lv in reversed(range(Lv)):
            s = skips[lv]
            x_in = s if f is None else upsample_concat(f, s)
            small = None if f is None else f.shape
            f, b_entry = self.conv(f"dec{lv}/entry/kernel", x_in, ea)
            f, b_blocks = self.blocks(f, f"dec{lv}", drop_scale)
            dec[lv] = (small, b_entry, b_blocks)
        chain = []                                                   # closing layers: closures d(out) -> d(in)
        f = self.closing_layers(f, noisy, chain)
        if m.add_clip:
            fin = f
            f = torch.empty_like(fin)
            v = fin.view(1, 1, -1, 32)
            call("bf_op_dwconv_ln", N.ptr(v), N.ptr(f), None, None, 1, 1, v.shape[2], 32, 0, UL.LN_EPSILON, 4, 0.0, N.stream_ptr(fin))

            def b_clip(dy, y=f):
                dx = torch.empty_like(dy)
                call("bf_op_act_bwd", N.ptr(y), N.ptr(dy), N.ptr(dx), dy.numel(), 4, 0.0, 1, N.stream_ptr(dy))
                return dx
            chain.append(b_clip)
        pred, losses, total, g = self.head_loss(f, gt, depth_weight)

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
            cu = small[-1]
            dup, dskip[lv] = ops.slice_channels(g, 0, cu), ops.slice_channels(g, cu, g.shape[-1] - cu)
            g = ops.upsample2x_bwd(dup, False)
        g = dskip[Lv - 1]
        for lv in reversed(range(Lv)):                               # encoder, deepest first
            pooled_from, b_entry, b_blocks = enc[lv]
            g = b_blocks(g)
            if lv == 0:
                break
            g = b_entry(g)                                           # d pooled
            g = ops.add(ops.maxpool2_bwd(pooled_from, g), dskip[lv - 1])     # the skip's two consumers
        if b_init is not None:
            g = b_init(g)
        b_base(g)
        self.finish_step(total)
        return pred, losses, total
