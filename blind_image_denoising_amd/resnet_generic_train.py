"""
Training of the resnet backbones outside the 16-filter 3x3 engine (`GenericResnetHydra`: the shipped bottleneck / depthwise
config `resnet_color_1x6_bn_32x128x32_1x3x1_..._depthwise`, per-position kernels / filters / groups, `add_gates`):
bfcnn/train_loop.py:259-312 -- training-mode forward (BatchNormalization on batch statistics, moving statistics updated),
denoiser loss, the builder's regularisers, and the gradient of the total for every trainable tensor -- as an explicit
forward / backward walk of the graph of bfcnn/backbone_resnet.py:36-298 + backbone_blocks.py:163-246 over the operator
library's C-ABI entry points (forward operators of unet_ops.hip, backward primitives of train_prims.hip, BatchNorm / gate /
layout operators of train_generic.hip).  PyTorch holds the tensors; it computes nothing.

Exact fp32.  Gradients are compared with the torch-autograd oracle (oracle/resnet_generic_torch.py) in
tests/test_gpu_resnet_generic_train.py.
"""
import torch

from . import _native as N
from . import unet_laplacian as UL
from ._native import call
from .op_graph import BN_EPSILON, concat_input
from .resnet_generic import SELECTOR_EPSILON, SELECTOR_GLOBAL_LEAKY
from .train_graph import TrainGraph, push

BN_MOMENTUM = 0.995                # DEFAULT_BN_MOMENTUM (bfcnn/constants.py:10)
REG_COEF = 0.01                    # keras "l1" / "l2" string regularisers
CHANNELWISE_L1 = 0.1               # DEFAULT_CHANNELWISE_MULTIPLIER_L1 (bfcnn/constants.py:13)
MULTIPLIER_L1 = 1.0                # DEFAULT_MULTIPLIER_L1 (:12)


class GenericResnetTrainGraph(TrainGraph):
    """train_step_single_gpu for a GenericResnetHydra: `step(gt, noisy, grads)` returns (prediction, loss slots, totals[3]) and
    fills `grads` (flat, laid out like model.params); model.state (moving statistics) is updated in place.  The steps the plain
    U-Net's graph (unet_backbone_train) shares, and the selector pair, are methods: each returns (output, backward closure
    d output -> d input); the convolutions, the base and the head are the shared steps of train_graph.TrainGraph."""

    def regularizer(self, name: str, kind: str):
        """the multipliers' own L1, the string regulariser kernel_regularizer names on every kernel, none on the BatchNorm gammas"""
        if kind == "bn_gamma":
            return None
        if kind in ("channelwise", "multiplier"):
            return "l1", CHANNELWISE_L1 if kind == "channelwise" else MULTIPLIER_L1
        rk = self.kernel_regularizer(name)
        if rk in (None, "none"):
            return None
        if rk not in ("l1", "l2"):
            raise NotImplementedError(f"regularizer {rk}")
        return rk, REG_COEF

    def kernel_regularizer(self, name: str):
        """backbone_resnet.py:128-176, backbone_blocks.py:146-160, model.py:297-342"""
        bb, dn = self.m.config["backbone"], self.m.config["denoiser"]
        if name.startswith("base/"):
            return bb.get("kernel_regularizer", "l1")
        if name.startswith("head/"):
            return dn.get("kernel_regularizer", "l2")
        if "/gate/" in name:
            return "l2"
        if "/selector/" in name:                                   # custom_layers_selector.py:88
            return (bb.get("selector_params") or {}).get("kernel_regularizer", "l1")
        j = int(name.split("/")[1][4:])
        br = bb.get("block_regularizer") or [bb.get("kernel_regularizer", "l1")] * len(self.m.block_kernels)
        return br[j]

    # ---- the steps the plain U-Net's graph shares ---------------------------------------------------------------------------
    def bn_step(self, base: str, c: torch.Tensor, a: str):
        """BatchNormalization on batch statistics (+ activation a), moving statistics updated: (y, backward dy -> dc)"""
        ops = self.ops
        Cc = c.shape[-1]
        gamma = self.W(base + "/gamma")
        save = torch.empty(2 * Cc, **self.f32)

        def fwd(a_):
            y_ = torch.empty_like(c)
            sp, sn = ops._s()
            call("bf_op_bn_train_fwd", N.ptr(c), N.ptr(gamma), N.ptr(y_), N.ptr(save), N.ptr(self.S(base + "/moving_mean")),
                 N.ptr(self.S(base + "/moving_variance")), c.numel() // Cc, Cc, BN_EPSILON, BN_MOMENTUM, *UL._act(a_), sp, sn, N.stream_ptr(c))
            return y_
        y, b_act = self.act_step(fwd, a)

        def bwd(dy):
            dpre = b_act(dy)
            dx = torch.empty_like(c)
            sp, sn = ops._s()
            call("bf_op_bn_train_bwd", N.ptr(c), N.ptr(gamma), N.ptr(save), N.ptr(dpre), N.ptr(dx), N.ptr(self.G(base + "/gamma")),
                 c.numel() // Cc, Cc, sp, sn, N.stream_ptr(c))
            return dx
        return y, bwd

    def mult_step(self, name, t: torch.Tensor, s_=None, pad_to=None):
        """ChannelwiseMultiplier / Multiplier: t * relu(w0 + 1) [* the per-sample RandomOnOff factor]; name None: the factor alone.
        pad_to: the factor for the first entries of a zero-padded tensor, ones behind them"""
        ops, f32 = self.ops, self.f32
        Cc = t.shape[-1]
        cf = Cc if pad_to is None else pad_to
        mvec = None
        if name is not None:
            w0 = self.W(name)
            nw = w0.numel()
            mv = torch.empty(cf, **f32)
            call("bf_op_relu_shift", N.ptr(w0), nw, 1.0, N.ptr(mv), cf, N.stream_ptr(mv))
            mvec = mv
            if cf < Cc:
                mvec = ops.concat_channels(mv, torch.ones(Cc - cf, **f32))
        y = ops.scale_add(None, t, mvec, s_)

        def bwd(dy):
            dm = torch.empty(Cc, **f32) if name is not None else None
            dt = ops.scale_add_bwd(t, mvec, s_, dy, dm)
            if name is not None:
                call("bf_op_relu_shift_bwd", N.ptr(w0), nw, 1.0, N.ptr(dm), N.ptr(self.G(name)), cf, N.stream_ptr(dm))
            return dt
        return y, bwd

    def gate_step(self, prefix: str, t: torch.Tensor):
        """the channel gate of `add_gates` behind a block's second convolution (backbone_blocks.py:199-208): (y, backward)"""
        ops = self.ops
        w0, w1 = self.W(f"{prefix}/gate/dense0/kernel"), self.W(f"{prefix}/gate/dense1/kernel")
        B, hw, Cc, C8 = t.shape[0], t.shape[1] * t.shape[2], t.shape[-1], w0.shape[1]
        gsave = torch.empty(int(N.lib().bf_op_gate_save_floats(B, Cc, C8)), **self.f32)
        gout = torch.empty_like(t)
        sp, sn = ops._s()
        call("bf_op_gate_fwd", N.ptr(t), N.ptr(w0), N.ptr(w1), None, N.ptr(gout), N.ptr(gsave), B, hw, Cc, C8, sp, sn, N.stream_ptr(t))

        def bwd(dy):
            dx = torch.empty_like(t)
            sp, sn = ops._s()
            call("bf_op_gate_bwd", N.ptr(t), N.ptr(w0), N.ptr(w1), N.ptr(gsave), N.ptr(dy), N.ptr(dx),
                 N.ptr(self.G(f"{prefix}/gate/dense0/kernel")), N.ptr(self.G(f"{prefix}/gate/dense1/kernel")), B, hw, Cc, C8, sp, sn,
                 N.stream_ptr(t))
            return dx
        return gout, bwd

    def closing_layers(self, f: torch.Tensor, noisy: torch.Tensor, chain) -> torch.Tensor:
        """final BatchNorm, Concatenate([features, the normalised input]), the closing multipliers (backbone_resnet.py:274-287,
        backbone_unet.py:226-252); their backward closures appended to chain.  The concatenation is padded with zero channels to the
        width the head's matrix kernel takes, as the inference path runs it; the multipliers and the head's first kernel are padded
        likewise (factor 1 / zero rows) and their gradients sliced back.  The image carries no gradient."""
        m = self.m
        if m.add_final_bn:
            f, b_ = self.bn_step("final_bn", f, "linear")
            chain.append(b_)
        B, H, Wd, Cf = f.shape
        cf = Cf + (m.in_channels if m.add_concat_input else 0)
        if m.add_concat_input:
            Cp = next(c for c in (32, 64, 128, 256) if c >= cf)
            f = concat_input(f, noisy, H, Wd, Cp, m.v_min, m.v_max)
            chain.append(lambda dcat: self.ops.slice_channels(dcat, 0, Cf))
        for name_ in (["channelwise/w0"] if m.add_channelwise else []) + (["multiplier/w0"] if m.add_multiplier else []):
            f, b_ = self.mult_step(name_, f, None, cf)
            chain.append(b_)
        return f

    def regularize(self, total: torch.Tensor) -> float:
        reg = super().regularize(total)
        n_mult = sum(kind == "multiplier" for _, _, kind, _ in self.m.trainable_variables)
        if n_mult:
            # Multiplier hands its regulariser to the non-trainable w1 (= 1.0) as well (custom_layers.py:1067-1074): L1(1.0) of a
            # constant 1.0 per layer in model.losses, no gradient
            ones = torch.ones(n_mult, **self.f32)
            call("bf_op_reg_elementwise", N.ptr(ones), None, n_mult, N.BF_REG_L1, MULTIPLIER_L1, reg, N.ptr(total[1:2]), N.stream_ptr(ones))
        return reg

    def finish_step(self, total: torch.Tensor):
        """regularisers, epilogue; the folded inference weights no longer match the state"""
        self._finish(total, self.regularize(total))
        self.m.mark_dirty()

    def head_loss(self, f: torch.Tensor, gt: torch.Tensor, depth_weight: float):
        """the denoiser head on f, the loss against gt and the head's backward: (prediction, loss slots, totals[3], d f)"""
        self.ld = self._loss_desc(0.0)
        total = torch.zeros(3, **self.f32)                           # [0] total loss, [1] regularisation value, [2] [1] * regularization
        pred, losses, df = self.head_step("head", f, gt, depth_weight, total)
        return pred, losses, total, df

    # ---- the resnet's own steps ---------------------------------------------------------------------------------------------
    def conv_op(self, name: str, x: torch.Tensor, j: int):
        """convolution j of a block (no normalisation / activation).  Conv2D(groups = g) runs as the block-diagonal dense one, tap
        by tap (keras kernel [k][k][cin / g][cf]): the kernel gradient is taken dense and its diagonal blocks are written back
        (backbone_blocks.py:196-205, conv2d groups)"""
        m = self.m
        kk, cf, dm, g = m.block_kernels[j], m.block_filters[j], m.block_depthwise[j], m.block_groups[j]
        if dm != -1:
            return self.depthwise_step(name, x, kk, dm)
        if g == 1:
            return self.conv1x1_step(name, x, cf, "linear") if kk == 1 else self.conv_step(name, x, "linear")
        cin, taps = x.shape[-1], kk * kk

        def group_kernel(grouped, dense, back):
            for t_ in range(taps):
                call("bf_op_group_kernel", N.ptr(grouped.view(taps, cin // g, cf)[t_]), N.ptr(dense.view(taps, cin, cf)[t_]), cin, cf, g,
                     back, N.stream_ptr(dense))
        wd = torch.empty((kk, kk, cin, cf), **self.f32)
        group_kernel(self.W(name), wd, 0)
        unpack = lambda dense, gw: group_kernel(gw, dense, 1)
        return self.conv1x1_step(name, x, cf, "linear", wd.view(cin, cf), unpack) if kk == 1 else self.conv_step(name, x, "linear", wd, unpack)

    def prefilter_step(self, i: int, x: torch.Tensor, pre, pool, Ct: int, chain):
        """the selector's optional pre-filters (custom_layers_selector.py:160-185) forward, their adjoints appended to chain"""
        ops, f32 = self.ops, self.f32
        if pre.get("conv1x1"):
            x = push(chain, self.conv1x1_step(f"block{i}/selector/pre/kernel", x, Ct, "linear"))
        Bx, Hx, Wx, Cx = x.shape
        if pre.get("gn"):                                    # per sample: BatchNorm's batch-statistics forward / backward with gamma 1
            xin = x
            ones, mm, mv = (torch.ones(Cx, **f32) for _ in range(3))
            saves = torch.empty((Bx, 2 * Cx), **f32)
            x = torch.empty_like(xin)
            for b in range(Bx):
                sp, sn = ops._s()
                call("bf_op_bn_train_fwd", N.ptr(xin[b]), N.ptr(ones), N.ptr(x[b]), N.ptr(saves[b]), N.ptr(mm), N.ptr(mv), Hx * Wx, Cx,
                     SELECTOR_EPSILON, 0.0, 0, 0.0, sp, sn, N.stream_ptr(xin))

            def b_gn(dy, xin=xin):
                dx = torch.empty_like(xin)
                dgamma = torch.empty(Cx, **f32)
                for b in range(Bx):
                    sp, sn = ops._s()
                    call("bf_op_bn_train_bwd", N.ptr(xin[b]), N.ptr(ones), N.ptr(saves[b]), N.ptr(dy[b]), N.ptr(dx[b]), N.ptr(dgamma),
                         Hx * Wx, Cx, sp, sn, N.stream_ptr(xin))
                return dx
            chain.append(b_gn)
        if pre.get("ln"):
            xin = x

            def pooled(t, entry="bf_op_avgpool_same", *tail):    # the pooling; with "..._bwd", 0: its adjoint
                o = torch.empty_like(t)
                call(entry, N.ptr(t), N.ptr(o), Bx, Hx, Wx, Cx, pool[0], pool[1], 1, 1, *tail, N.stream_ptr(t))
                return o
            mean = pooled(xin)
            sq = torch.empty_like(xin)
            call("bf_op_center_scale", N.ptr(xin), N.ptr(mean), None, N.ptr(sq), xin.numel(), SELECTOR_EPSILON, N.stream_ptr(xin))
            var = pooled(sq)
            x = torch.empty_like(xin)
            call("bf_op_center_scale", N.ptr(xin), N.ptr(mean), N.ptr(var), N.ptr(x), xin.numel(), SELECTOR_EPSILON, N.stream_ptr(xin))

            def b_ln(dy, xin=xin):
                dd, dv = torch.empty_like(xin), torch.empty_like(xin)
                call("bf_op_center_scale_bwd", N.ptr(xin), N.ptr(mean), N.ptr(var), N.ptr(dy), N.ptr(dd), N.ptr(dv), xin.numel(),
                     SELECTOR_EPSILON, N.stream_ptr(dy))
                t = pooled(dv, "bf_op_avgpool_same_bwd", 0)
                tot = torch.empty_like(xin)
                call("bf_op_center_sq_bwd", N.ptr(xin), N.ptr(mean), N.ptr(t), N.ptr(dd), N.ptr(tot), xin.numel(), N.stream_ptr(dd))
                back = pooled(tot, "bf_op_avgpool_same_bwd", 0)
                call("bf_op_axpy", N.ptr(tot), N.ptr(back), -1.0, 0, tot.numel(), N.stream_ptr(tot))     # d (x - pool x)
                return tot
            chain.append(b_ln)
        for key, high in (("lp", 0), ("hp", 1)):
            if pre.get(key):
                xin = x
                x = torch.empty_like(xin)
                call("bf_op_pass_filter", N.ptr(xin), N.ptr(x), xin.numel(), 4.0, 4, high, N.stream_ptr(xin))

                def b_pf(dy, xin=xin, high=high):
                    dx = torch.empty_like(xin)
                    call("bf_op_pass_filter_bwd", N.ptr(xin), N.ptr(dy), N.ptr(dx), xin.numel(), 4.0, 4, high, N.stream_ptr(dy))
                    return dx
                chain.append(b_pf)
        return x

    def selector_step(self, i: int, x1: torch.Tensor, x2: torch.Tensor, sel: torch.Tensor):
        """selector_block (custom_layers_selector.py:81-330) in place of the skip Add: out = x1 s + x2 (1 - s), s = F(2.5 - u),
        u = up(relu(leaky(pool(sel) W0) W1)).  scale_type GLOBAL is the same chain with one window over the whole image
        (Dense layers, slope SELECTOR_GLOBAL_LEAKY).  Returns (out, backward: d out -> (d x1, d x2, d sel))."""
        ops, f32, sp = self.ops, self.f32, self.m.selector
        st, soft = sp["scale_type"], int(sp["activation_type"] == "soft")
        Ct = x1.shape[-1]
        pre_chain = []                                       # adjoints of the optional pre-filters, in forward order
        if sp.get("pre"):
            sel = self.prefilter_step(i, sel, sp["pre"], sp["pool"], Ct, pre_chain)
        Bs, Hs, Ws, Cs = sel.shape
        if st == "global":
            stride, pools, alpha0, kind = (Hs, Ws), [(Hs, Ws)], SELECTOR_GLOBAL_LEAKY, "dense"
        else:
            stride, pool, alpha0, kind = sp["stride"], sp["pool"], 0.3, "conv"
            if Hs % stride[0] or Ws % stride[1]:
                raise ValueError(f"selector_block: the image ({Hs}x{Ws}) must be a multiple of the strides {stride}")
            pools = [(pool[0] // 2, pool[1] // 2), pool, (pool[0] * 2, pool[1] * 2)] if st == "multiscale" else [pool]
        OH, OW = Hs // stride[0], Ws // stride[1]
        rows = Bs * OH * OW
        parts = []
        for ph, pw in pools:
            pm = torch.empty((Bs, OH, OW, Cs), **f32)
            call("bf_op_avgpool_same", N.ptr(sel), N.ptr(pm), Bs, Hs, Ws, Cs, ph, pw, stride[0], stride[1], N.stream_ptr(sel))
            parts.append(pm)
        if st == "mixed":                                    # local means next to the image's global mean on the same grid
            gm = torch.empty((Bs, OH, OW, Cs), **f32)
            sp_, sn_ = ops._s()
            call("bf_op_channel_mean_broadcast", N.ptr(sel), N.ptr(gm), Bs, Hs * Ws, Cs, OH * OW, sp_, sn_, N.stream_ptr(sel))
            parts.append(gm)
        cat = ops.concat_channels(*parts) if len(parts) > 1 else parts[0]
        Cc = cat.shape[-1]
        n0, n1 = f"block{i}/selector/{kind}0/kernel", f"block{i}/selector/{kind}1/kernel"
        w0, w1 = self.W(n0), self.W(n1)
        C8 = int(w0.shape[-1])
        u = torch.empty((Bs, OH, OW, Ct), **f32)
        call("bf_op_dense2", N.ptr(cat), N.ptr(w0), None, N.ptr(w1), None, N.ptr(u), rows, Cc, Ct, C8, 2, alpha0, 4, N.stream_ptr(cat))
        up = UL.resize_bilinear(u, Hs, Ws)
        out = torch.empty_like(x1)
        call("bf_op_selector_mix", N.ptr(x1), N.ptr(x2), N.ptr(up), N.ptr(out), x1.numel(), soft, N.stream_ptr(x1))

        def bwd(dout):
            dx1, dx2, dup = torch.empty_like(x1), torch.empty_like(x1), torch.empty_like(x1)
            call("bf_op_selector_mix_bwd", N.ptr(x1), N.ptr(x2), N.ptr(up), N.ptr(dout), N.ptr(dx1), N.ptr(dx2), N.ptr(dup), x1.numel(),
                 soft, N.stream_ptr(dout))
            du = ops.resize_bilinear_bwd(dup, OH, OW)
            dcat = torch.empty_like(cat)
            sp_, sn_ = ops._s()
            call("bf_op_dense2_bwd", N.ptr(cat), N.ptr(w0), N.ptr(w1), N.ptr(du), N.ptr(dcat), N.ptr(self.G(n0)),
                 N.ptr(self.G(n1)), rows, Cc, Ct, C8, alpha0, sp_, sn_, N.stream_ptr(du))
            dsel = torch.empty_like(sel)
            for k_, (ph, pw) in enumerate(pools):
                dpart = ops.slice_channels(dcat, k_ * Cs, Cs) if len(parts) > 1 else dcat
                call("bf_op_avgpool_same_bwd", N.ptr(dpart), N.ptr(dsel), Bs, Hs, Ws, Cs, ph, pw, stride[0], stride[1], int(k_ > 0),
                     N.stream_ptr(dpart))
            if st == "mixed":                                # d mean: the column sums of its gradient, spread over the image
                dgm = ops.slice_channels(dcat, Cs, Cs)
                spread = torch.empty_like(sel)
                call("bf_op_channel_mean_broadcast", N.ptr(dgm), N.ptr(spread), Bs, OH * OW, Cs, Hs * Ws, sp_, sn_, N.stream_ptr(dgm))
                call("bf_op_axpy", N.ptr(dsel), N.ptr(spread), float(OH * OW) / float(Hs * Ws), 0, dsel.numel(), N.stream_ptr(dsel))
            for b_pre in reversed(pre_chain):
                dsel = b_pre(dsel)
            return dx1, dx2, dsel
        return out, bwd

    def block(self, i: int, f: torch.Tensor, ds_):
        """resnet block i and the skip Add -- or the selector, which reads the first convolution's output -- behind it; ds_: the
        block's RandomOnOff factor or None"""
        m, ops = self.m, self.ops
        t, steps = f, []
        for j in range(len(m.block_kernels)):
            t = push(steps, self.conv_op(f"block{i}/conv{j}/kernel", t, j))
            a = m.block_activation[j]
            t = push(steps, self.bn_step(f"block{i}/bn{j}", t, a) if j >= 1 and m.use_bn else self.act_step(t, a))
            if j == 0:
                first, n_first = t, len(steps)                    # x_1st_conv: the selector layer; steps[:n_first] produce it
            if j == 1 and m.add_gates:
                t = push(steps, self.gate_step(f"block{i}", t))
        # backbone_blocks.py:215-225: ChannelwiseMultiplier, Multiplier, RandomOnOff in front of the Add
        tails = ([f"block{i}/channelwise/w0"] if m.add_channelwise else []) + ([f"block{i}/multiplier/w0"] if m.add_multiplier else [])
        if ds_ is not None and not tails:
            tails = [None]
        for q_, name_ in enumerate(tails):
            t = push(steps, self.mult_step(name_, t, ds_ if q_ == len(tails) - 1 else None))
        if m.selector:                                            # selector_block instead of the Add (backbone_blocks.py:227-239)
            out, b_sel = self.selector_step(i, f, t, first)
        else:
            out, b_sel = ops.add(f, t), None                      # Add()([x, previous_layer]) (backbone_blocks.py:242)

        def bwd(dout):
            dskip, g, dsel = b_sel(dout) if b_sel is not None else (dout, dout, None)
            for idx in range(len(steps) - 1, -1, -1):
                if dsel is not None and idx == n_first - 1:       # g is the gradient at the first convolution's output here
                    g = ops.add(g, dsel)
                g = steps[idx](g)
            return ops.add(dskip, g)
        return out, bwd

    # ---- one training step -------------------------------------------------------------------------------------------------
    def step(self, gt: torch.Tensor, noisy: torch.Tensor, grads: torch.Tensor, depth_weight: float = 1.0, drop_scale=None):
        """drop_scale: {block index: per-sample factor [B] on the device} = RandomOnOff's draw (0 or 1 / (1 - rate))"""
        m = self.m
        drop_scale = drop_scale or {}
        gt, noisy = self._inputs(gt, noisy)
        B, H, Wd, _ = noisy.shape
        npix = B * H * Wd
        L = N.lib()
        cmax = max([m.filters] + [c for c in self._channels()])
        self._begin(grads, max(8 * 1024 * 1024, int(L.bf_op_denoiser_loss_scratch_floats(B, H, Wd, m.out_channels)) + 1024,
                               npix * 4, int(L.bf_op_gate_scratch_floats(B, cmax)) + 64, int(L.bf_op_bn_train_scratch_floats(cmax)) + 64,
                               npix * m.filters if m.selector else 0))   # the selector's resize / dense adjoints (one row set per pixel)
        f, b_base = self.base_step(noisy, m.kernel_size, m.base_activation)
        chain = []                                   # closures d(output) -> d(input), in forward order
        if m.add_initial_bn:
            f = push(chain, self.bn_step("initial_bn", f, "linear"))
        for i in range(m.no_layers):
            f = push(chain, self.block(i, f, drop_scale.get(i)))
        f = self.closing_layers(f, noisy, chain)
        pred, losses, total, g = self.head_loss(f, gt, depth_weight)
        for b_ in reversed(chain):
            g = b_(g)
        b_base(g)
        self.finish_step(total)
        return pred, losses, total

    def _channels(self):
        m = self.m
        cin = m.filters
        for cf, dm in zip(m.block_filters, m.block_depthwise):
            cin = cin * dm if dm != -1 else cf
            yield cin
