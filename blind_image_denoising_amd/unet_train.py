"""
Training of the `unet_laplacian` hydra (bfcnn/train_loop.py:259-321 with a multi-output model): the
training-mode forward, one denoiser loss per output scale times its depth weight, the model's regularisers, and the gradient
of the total with respect to every trainable tensor -- what `tf.GradientTape` does in the reference -- as an explicit walk of
the graph of bfcnn/backbone_unet_laplacian.py:281-606 over the operator library's C-ABI entry points (`bf_op_*`: forward
operators of unet_ops.hip, backward primitives of train_prims.hip).  PyTorch holds the tensors; it computes nothing.

Scope: the graph family of configs/unet_laplacian_v5.json and v6.json -- ConvNext blocks (depthwise k x k, LayerNorm, 1x1 C->4C + activation,
1x1 4C->C, ChannelLearnableMultiplier, StochasticDepth, Add), self-attention blocks on the deepest level (resize to 16x16,
LayerNorm, query / key / value, dot-product attention with dropout, resize back, output convolution, multiplier), level
LayerNorm + activation, the averaging / Gaussian Laplacian split, strided down-sampling + 1x1 or 2x2 stride-2 convolution, `upsample_laplacian_conv2d` / nearest or bilinear + 3x3 convolution,
per-scale denoiser heads, AdditiveAttentionGate in front of the decoder Add (v3 / v4) -- with any depth / width / filters.
The graph revision of the reference's trained archive (tests/golden/unet_v56.npz: GELU in the MLP and on query / key / value,
row-wise full-resolution attention with a second LayerNorm, no level activation, 1x1-then-resize up-sampling, the output
LayerNorms in front of the heads) trains as well, so the shipped network can be fine-tuned.  So do mix projections, maxpool
down-sampling and plain bilinear / nearest up-sampling; conv2d_transpose up-sampling raises NotImplementedError (as in inference).

Every layer is a method returning (output, backward closure); the convolutions, the base and the heads are the shared steps of
train_graph.TrainGraph.  The gradient forks in two places only: a Laplacian `split`'s backward takes (d lap, d down) and returns
d x, an `upsample` join's takes d x and returns (d lap, d low).  `step` reads encoder, decoder, heads, backward, regularisers.

Exact fp32 throughout (the split-f16 inference operators are not used here): gradients are compared with the torch-autograd
oracle (oracle/unet_torch.py) in tests/test_gpu_unet_train.py.
"""
from typing import Dict, Optional, Sequence

import torch

from . import _native as N
from . import unet_laplacian as UL
from ._native import call
from .pyramid import avg_pool2_valid, upsample_2x
from .train_graph import TrainGraph, pack, push

SOFTORTHONORMAL = (0.01, 0.0, 1e-4)        # bfcnn/constants.py:19-21: lambda, l1, l2
MULTIPLIER_L1 = 1e-6                        # ChannelLearnableMultiplier's regulariser (custom_layers.py:267)
KERNEL_L2 = 0.01                            # keras "l2" string regulariser
GATE_L2 = 1e-4                              # AdditiveAttentionGate's default kernel regulariser (custom_layers.py:726)


class UnetTrainGraph(TrainGraph):
    """train_step_single_gpu for a UnetLaplacianHydra: `step(gt, noisy, depth_weights, ...)` returns the per-scale predictions
    and fills `grads` (flat, laid out like model.params) and the loss slots.  While a step runs, `depth_scale` / `attn_scale`
    (the StochasticDepth and attention-dropout draws by block prefix) live on the graph."""

    def __init__(self, model: "UL.UnetLaplacianHydra", loss_config: Dict, soft_orthonormal: Optional[bool] = None):
        bad = []
        if model.downsample_type not in ("strides", "conv2d", "maxpool"): bad.append(f"downsample_type {model.downsample_type}")
        if model.upsample_type not in ("upsample_laplacian_conv2d", "upsample_nearest_conv2d", "upsample_bilinear_conv2d", "bilinear",
                                       "nn", "nearest"):
            bad.append(f"upsample_type {model.upsample_type}")
        if model.activation == "gelu": bad.append("gelu outside the convnext MLP / the attention projections")
        if model.activation == "linear": bad.append("linear activation")
        if getattr(model, "use_concat", False) and not model.use_mix_project and model.dec_k not in (1, 3, 5):
            bad.append(f"use_concat without use_mix_project and decoder_kernel_size {model.dec_k}")
        if getattr(model, "use_concat", False) and model.use_attention_gates:       # the gate replaces the join: nothing is concatenated
            bad.append("use_concat with use_attention_gates")
        if any(model.level_filters(d) == 256 and not model._is_attention(d) for d in range(model.depth)):
            bad.append("a 256-channel ConvNext level (runs at inference only)")
        if bad:
            raise NotImplementedError("unet_laplacian training is built for the configs/unet_laplacian_v5.json graph family: " + ", ".join(bad))
        super().__init__(model, loss_config)
        bb = model.config["backbone"]
        self.soft_orthonormal = bool(bb.get("use_soft_orthonormal_regularization", False)) if soft_orthonormal is None else soft_orthonormal
        self.gauss = None if model.use_laplacian_averaging else \
            torch.from_numpy(UL.gaussian_kernel((model.gauss_k, model.gauss_k))).to(model.device)

    def regularizer(self, name: str, kind: str):
        """l1 on the multipliers, soft-orthonormal on the attention projections (with the flag: on the MLP and gate convolutions
        too), l2 on every other kernel (the gate's own coefficient), none on the LayerNorm gammas"""
        if kind == "ln_gamma":
            return None
        if kind == "multiplier":
            return "l1", MULTIPLIER_L1
        leaf, is_gate = name.split("/")[1], name.startswith("gate")
        if leaf in ("key", "query", "value", "out") or (self.soft_orthonormal and (leaf in ("pw1", "pw2") or (is_gate and kind == "conv"))):
            return "soft_orthonormal", SOFTORTHONORMAL
        return "l2", GATE_L2 if is_gate else KERNEL_L2

    def _multiplier_bwd(self, name: str, wm: torch.Tensor, dm: torch.Tensor):
        call("bf_op_multiplier_bwd", N.ptr(wm), N.ptr(dm), N.ptr(self.G(name)), dm.numel(), N.stream_ptr(dm))

    # ---- blocks -------------------------------------------------------------------------------------------------------------
    def convnext(self, prefix: str, x: torch.Tensor, k: int):
        """ConvNextBlock + the residual Add (+ depth scale).  The first decoder block behind a Concatenate without mix projection
        maps 2 C -> C channels: no Add, no StochasticDepth there (backbone_unet_laplacian.py:557-560)"""
        m, ops = self.m, self.ops
        Cin = x.shape[-1]
        Hh = int(self.off[f"{prefix}/pw1/kernel"][1][-1])
        Cc = int(self.off[f"{prefix}/pw2/kernel"][1][-1])
        skip = Cin == Cc
        w1, w2 = self.W(f"{prefix}/pw1/kernel").view(Cin, Hh), self.W(f"{prefix}/pw2/kernel").view(Hh, Cc)
        t1, b_dw = self.depthwise_step(f"{prefix}/dw/kernel", x, k)
        gamma = self.W(f"{prefix}/ln/gamma") if m.use_ln else None
        t2 = UL.dwconv_ln(t1, None, gamma) if m.use_ln else t1
        # the hidden layer in chunks of at most 256 units (the widest 1x1 convolution of the operator library): one chunk up
        # to 64 channels, two for the 128-channel levels of the 4-level models
        Hc = min(Hh, 256)
        chunks = range(Hh // Hc)
        w1c = [w1 if Hc == Hh else w1[:, j * Hc:(j + 1) * Hc].contiguous() for j in chunks]
        w2c = [w2[j * Hc:(j + 1) * Hc] for j in chunks]
        t3, b_act = zip(*[self.act_step(lambda a, j=j: UL.pointwise(t2, pack(w1c[j]), Hc, a), m.mlp_activation) for j in chunks])
        t4 = None
        for j in chunks:
            t4 = UL.pointwise(t3[j], pack(w2c[j]), Cc, res=t4)
        wm = self.W(f"{prefix}/gamma/w") if m.use_gamma else None
        mult = UL.channel_multiplier(wm) if m.use_gamma else None
        s = self.depth_scale.get(prefix) if skip else None
        out = ops.scale_add(x if skip else None, t4, mult, s)

        def bwd(dout):
            dm = torch.empty(Cc, **self.f32) if m.use_gamma else None
            dt4 = ops.scale_add_bwd(t4, mult, s, dout, dm)
            if m.use_gamma:
                self._multiplier_bwd(f"{prefix}/gamma/w", wm, dm)
            gw2, gw1 = self.G(f"{prefix}/pw2/kernel").view(Hh, Cc), self.G(f"{prefix}/pw1/kernel").view(Cin, Hh)
            dt2 = None
            for j in chunks:
                ops.matmul_wgrad(t3[j], dt4, gw2[j * Hc:(j + 1) * Hc])
                dt3 = b_act[j](UL.pointwise(dt4, pack(ops.transpose(w2c[j].contiguous())), Hc))
                if Hc == Hh:
                    ops.matmul_wgrad(t2, dt3, gw1)
                else:                                          # a column block of the kernel gradient: staged, then copied in
                    blk = torch.empty((Cin, Hc), **self.f32)
                    ops.matmul_wgrad(t2, dt3, blk)
                    gw1[:, j * Hc:(j + 1) * Hc].copy_(blk)
                dt2 = UL.pointwise(dt3, pack(ops.transpose(w1c[j])), Cin, res=dt2)
            dx = b_dw(ops.layernorm_bwd(t1, gamma, dt2, self.G(f"{prefix}/ln/gamma")) if m.use_ln else dt2)
            return ops.add(dout, dx) if skip else dx
        return out, bwd

    def attention(self, prefix: str, x: torch.Tensor):
        m, ops, f32 = self.m, self.ops, self.f32
        Bc, Hc, Wc, Cc = x.shape
        A = m.filters
        rows = m.attention_rows                  # the trained archive's graph: no resize, one sequence per image row
        rh, rw = (Hc, Wc) if rows else m.attention_resolution
        NB, T = (Bc * rh, rw) if rows else (Bc, rh * rw)
        r = x if rows else UL.resize_bilinear(x, rh, rw)
        gamma = self.W(f"{prefix}/ln/gamma") if m.use_ln else None
        n_ = UL.dwconv_ln(r, None, gamma) if m.use_ln else r
        qact, alpha = (m.attention_activation, None) if m.attention_activation else ("leaky_relu", m.attention_alpha)
        # keras reads [query, value, key]; the archive's graph hands the key convolution over as the value and the value
        # convolution as the key (unet_laplacian._attention)
        order = ("query", "key", "value") if rows else ("query", "value", "key")
        (q, v, k_), b_qvk = zip(*[self.conv1x1_step(f"{prefix}/{n}/kernel", n_, A, qact, alpha=alpha) for n in order])
        q, v, k_ = (z.view(NB, T, A) for z in (q, v, k_))
        ps = self.attn_scale.get(prefix)
        o = torch.empty((NB, T, A), **f32)
        P = torch.empty((NB, T, T), **f32)
        call("bf_op_attention_train", N.ptr(q), N.ptr(v), N.ptr(k_), N.ptr(ps), N.ptr(o), N.ptr(P), NB, T, A, N.stream_ptr(q))
        o4 = o.view(Bc, rh, rw, A)
        gamma1 = self.W(f"{prefix}/ln1/gamma") if (rows and m.use_ln) else None
        if rows:
            u = UL.dwconv_ln(o4, None, gamma1) if m.use_ln else o4
        else:
            u = UL.resize_bilinear(o4, Hc, Wc)
        t, b_out = self.conv1x1_step(f"{prefix}/out/kernel", u, Cc, "linear")
        wm = self.W(f"{prefix}/gamma/w")
        mult = UL.channel_multiplier(wm)
        s = self.depth_scale.get(prefix)
        out = ops.scale_add(x, t, mult, s)

        def bwd(dout):
            dm = torch.empty(Cc, **f32)
            dt = ops.scale_add_bwd(t, mult, s, dout, dm)
            self._multiplier_bwd(f"{prefix}/gamma/w", wm, dm)
            du = b_out(dt)
            if rows:
                do = ops.layernorm_bwd(o4, gamma1, du, self.G(f"{prefix}/ln1/gamma")) if m.use_ln else du
            else:
                do = ops.resize_bilinear_bwd(du, rh, rw)
            dq, dv, dk = (torch.empty((NB, T, A), **f32) for _ in range(3))
            dS = torch.empty((NB, T, T), **f32)
            call("bf_op_attention_bwd", N.ptr(q), N.ptr(v), N.ptr(k_), N.ptr(ps), N.ptr(P), N.ptr(do), N.ptr(dq), N.ptr(dv),
                 N.ptr(dk), N.ptr(dS), NB, T, A, N.stream_ptr(q))
            dn = None
            for b_, dy in zip(b_qvk, (dq, dv, dk)):
                part = b_(dy.view(Bc, rh, rw, A))
                dn = part if dn is None else ops.add(dn, part)
            dr = ops.layernorm_bwd(r, gamma, dn, self.G(f"{prefix}/ln/gamma")) if m.use_ln else dn
            return ops.add(dout, dr if rows else ops.resize_bilinear_bwd(dr, Hc, Wc))
        return out, bwd

    def norm_act(self, name: str, x: torch.Tensor, act: str):
        """y = act(LayerNorm(x) * gamma)"""
        gamma = self.W(name)
        y = UL.dwconv_ln(x, None, gamma, act)
        return y, lambda dy: self.ops.layernorm_bwd(x, gamma, self.ops.act_bwd(y, dy, act), self.G(name))

    def split(self, x: torch.Tensor):
        """the Laplacian split of a level: (lap, down, backward (d lap, d down) -> d x); conv2d / maxpool down-sampling take the
        full-resolution smooth map, strides its ::2 slice"""
        m = self.m
        ds = 2 if m.downsample_type == "strides" else 1
        lp, down = UL.smooth_split(x, m.gauss_k, self.gauss, ds)
        B, H, Wd, Cc = x.shape

        def bwd(dlap, ddown):
            dx = torch.empty_like(x)
            call("bf_op_smooth_split_bwd_ex", N.ptr(dlap), N.ptr(ddown), N.ptr(self.gauss), N.ptr(dx), B, H, Wd, Cc, m.gauss_k, ds,
                 N.stream_ptr(ddown))
            return dx
        return lp, down, bwd

    def downsample(self, d: int, down: torch.Tensor):
        """the convolution to level d + 1 behind the split: 1x1 on the strided map, MaxPooling2D(2, 2, same) + 1x1
        (downsampling.py:56-68), or Conv2D 2 x 2, strides 2, same (downsample_type "conv2d", downsampling.py:45-55).  The last,
        on even sizes: no padding, every output sees its own 2 x 2 block, so the weight gradient is four 1 x 1 weight gradients on
        the strided slices of x and the data gradient the transposed convolution with the same kernel array"""
        m, ops = self.m, self.ops
        name, cout, act = f"down{d}/kernel", m.level_filters(d + 1), m.activation
        if m.downsample_type == "strides":
            return self.conv1x1_step(name, down, cout, act)
        if m.downsample_type == "maxpool":
            y, b_conv = self.conv1x1_step(name, UL.maxpool2(down), cout, act)
            return y, lambda dy: ops.maxpool2_bwd(down, b_conv(dy))
        Bc, Hc, Wc, cin = down.shape
        if Hc % 2 or Wc % 2:
            raise ValueError(f"conv2d down-sampling in training needs even sizes (got {Hc}x{Wc})")
        w = self.W(name)                                                      # [2,2,cin,cout]
        y, b_act = self.act_step(lambda a: UL.conv2d(down, UL.pack_conv(w.contiguous()), cout, 2, 2, a), act)

        def bwd(dy):
            dp = b_act(dy)
            gw = self.G(name).view(4, cin * cout)
            xs = torch.empty((Bc, Hc // 2, Wc // 2, cin), **self.f32)
            flat = down.reshape(-1)
            for t_ in range(4):
                src = flat[(t_ // 2 * Wc + t_ % 2) * cin:]                    # x[:, ky::2, kx::2, :] as a strided slice from a shifted base
                call("bf_strided_slice2", N.ptr(src), N.ptr(xs), Bc, Hc, Wc, cin, N.stream_ptr(down))
                ops.matmul_wgrad(xs, dp, gw[t_])
            return UL.conv2d_transpose(dp, w.contiguous(), 2, "linear")     # keras Conv2D kernel [k,k,cin,cout] = Conv2DTranspose's [k,k,out,in]
        return y, bwd

    def attention_gate(self, d: int, enc: torch.Tensor, up: torch.Tensor):
        """AdditiveAttentionGate (custom_layers.py:805-832) and the Add behind it (backbone_unet_laplacian.py:497-519):
        x = enc * sigmoid(4 * scale(conv_o(leaky_relu_0.1(conv_x(LN up) + conv_y(LN enc))))) + up.
        Returns (x, backward: dx -> (d enc, d up))."""
        m, ops = self.m, self.ops
        Cc = enc.shape[-1]
        pre = f"gate{d}"
        gx = self.W(f"{pre}/x_ln/gamma") if m.use_ln else None
        gy = self.W(f"{pre}/y_ln/gamma") if m.use_ln else None
        wx, wy = (self.W(f"{pre}/{n_}/kernel").view(Cc, Cc) for n_ in ("x", "y"))
        lx = UL.dwconv_ln(up, None, gx) if m.use_ln else up
        ly = UL.dwconv_ln(enc, None, gy) if m.use_ln else enc
        z = ops.add(UL.pointwise(lx, pack(wx), Cc), UL.pointwise(ly, pack(wy), Cc))
        sact = UL.dwconv_ln(z, None, None, "leaky_relu_01")
        o_raw, b_o = self.conv1x1_step(f"{pre}/o/kernel", sact, Cc, "linear")
        wm = self.W(f"{pre}/scale/w")
        mult = UL.channel_multiplier(wm)
        o = ops.scale_add(None, o_raw, mult, None)
        out = torch.empty_like(enc)
        call("bf_op_sigmoid_gate", N.ptr(enc), N.ptr(o), N.ptr(up), N.ptr(out), enc.numel(), N.stream_ptr(enc))

        def bwd(dout):
            denc, do = torch.empty_like(enc), torch.empty_like(enc)
            call("bf_op_sigmoid_gate_bwd", N.ptr(enc), N.ptr(o), N.ptr(dout), N.ptr(denc), N.ptr(do), enc.numel(), N.stream_ptr(enc))
            dm = torch.empty(Cc, **self.f32)
            do_raw = ops.scale_add_bwd(o_raw, mult, None, do, dm)
            self._multiplier_bwd(f"{pre}/scale/w", wm, dm)
            dz = ops.act_bwd(sact, b_o(do_raw), "leaky_relu_01")
            ops.matmul_wgrad(lx, dz, self.G(f"{pre}/x/kernel"))
            ops.matmul_wgrad(ly, dz, self.G(f"{pre}/y/kernel"))
            dlx = UL.pointwise(dz, pack(ops.transpose(wx)), Cc)
            dly = UL.pointwise(dz, pack(ops.transpose(wy)), Cc)
            dup = ops.layernorm_bwd(up, gx, dlx, self.G(f"{pre}/x_ln/gamma")) if m.use_ln else dlx
            dency = ops.layernorm_bwd(enc, gy, dly, self.G(f"{pre}/y_ln/gamma")) if m.use_ln else dly
            return ops.add(denc, dency), ops.add(dout, dup)
        return out, bwd

    def upsample(self, d: int, low: torch.Tensor, lap: torch.Tensor):
        """level d + 1's output brought up to level d and joined with the level's Laplacian -- the gate, the Concatenate
        (backbone_unet_laplacian.py:516-517) or the Add: (x, backward d x -> (d lap, d low))"""
        m, ops, a = self.m, self.ops, self.m.activation
        Cc, ut, name = m.level_filters(d), m.upsample_type, f"up{d}/kernel"
        bil = ut != "upsample_nearest_conv2d"
        conv_first = ut == "upsample_laplacian_conv2d" and m.upsample_linear      # upsampling.py:80-90: 1x1, then resize
        if ut in ("bilinear", "nn", "nearest"):                                   # UpSampling2D alone (upsampling.py:103-116)
            if low.shape[-1] != Cc:
                raise ValueError(f"Add of [{Cc}] and [{low.shape[-1]}] channels: upsample_type [{ut}] needs equal filters on both levels")
            bil = ut == "bilinear"
            up, b_conv = upsample_2x(low, bilinear=bil), (lambda g: g)
        elif conv_first:
            c_, b_conv = self.conv1x1_step(name, low, Cc, "linear")
            up = upsample_2x(c_, bilinear=True)
        elif ut == "upsample_laplacian_conv2d":
            up, b_conv = self.conv1x1_step(name, upsample_2x(low, bilinear=bil), Cc, a)
        else:                                                                     # Conv2D 3 x 3 behind an UpSampling2D (upsampling.py:52-76)
            up, b_conv = self.conv_step(name, upsample_2x(low, bilinear=bil), a)
        if m.use_attention_gates:
            x, b_join = self.attention_gate(d, lap, up)
        elif m.use_concat:
            x, b_join = ops.concat_channels(lap, up), lambda g: (ops.slice_channels(g, 0, Cc), ops.slice_channels(g, Cc, Cc))
        else:
            x, b_join = ops.add(lap, up), lambda g: (g, g)

        def bwd(dx):
            dlap, dup = b_join(dx)
            return dlap, (b_conv(ops.upsample2x_bwd(dup, bil)) if conv_first else ops.upsample2x_bwd(b_conv(dup), bil))
        return x, bwd

    # ---- one training step ----------------------------------------------------------------------------------------------------
    def step(self, gt: torch.Tensor, noisy: torch.Tensor, depth_weights: Sequence[float], grads: torch.Tensor,
             depth_scale: Optional[Dict[str, torch.Tensor]] = None, attn_scale: Optional[Dict[str, torch.Tensor]] = None):
        m = self.m
        gt, noisy = self._inputs(gt, noisy)
        B, H, Wd, _ = noisy.shape
        if H % (1 << (m.depth - 1)) or Wd % (1 << (m.depth - 1)):
            raise ValueError(f"training needs sizes divisible by {1 << (m.depth - 1)} (got {H}x{Wd})")
        self.depth_scale, self.attn_scale = depth_scale or {}, attn_scale or {}
        ops = self._begin(grads, max(8 * 1024 * 1024, int(N.lib().bf_op_denoiser_loss_scratch_floats(B, H, Wd, m.out_channels)) + 1024,
                                     B * 256 * 256 + 1024, B * H * Wd * 4))
        a = m.activation
        la = a if m.level_activation else "linear"
        level_norm = m.use_output_normalization and m.use_ln and not m.output_norm_at_heads
        last = m.depth - 1

        # -- encoder: a chain of closures on the gradient of its running value; a split's takes the gradient of the level's
        # Laplacian next to it, which the decoder's backward has put into dlap by then
        x, b_base = self.base_step(noisy, 5, a)
        enc, lap, dlap = [], {}, {}
        for d in range(m.depth):
            for w_ in range(m.width):
                pre = f"enc{d}_{w_}"
                x = push(enc, self.attention(pre, x) if m._is_attention(d) else self.convnext(pre, x, m.enc_k))
            if level_norm:
                x = push(enc, self.norm_act(f"enc{d}/out_ln/gamma", x, la))
            elif la != "linear":
                y = UL.dwconv_ln(x, None, None, la)
                x = push(enc, (y, lambda dy, y=y: ops.act_bwd(y, dy, la)))
            if d != last:
                lap[d], down, b_split = self.split(x)
                enc.append(lambda g, d=d, b_split=b_split: b_split(dlap[d], g))
                x = push(enc, self.downsample(d, down))

        # -- decoder: per level the join and a chain behind it
        outs, dec = {last: x}, {}
        for d in reversed(range(last)):
            chain = []
            x, b_join = self.upsample(d, outs[d + 1], lap[d])
            if m.use_mix_project:                                             # backbone_unet_laplacian.py:521-527
                x = push(chain, self.conv1x1_step(f"mix{d}/kernel", x, m.level_filters(d), a))
            for w_ in range(m.width):
                x = push(chain, self.convnext(f"dec{d}_{w_}", x, m.dec_k))
            if level_norm:
                x = push(chain, self.norm_act(f"dec{d}/out_ln/gamma", x, "linear"))
            outs[d], dec[d] = x, (chain, b_join)

        # -- heads + losses: df[i], the gradient of level i's output from its head
        self.ld = self._loss_desc(1.0)
        gts = [gt]
        for _ in range(last):
            gts.append(avg_pool2_valid(gts[-1], clip_values=True, round_values=True))       # multiscales_generator_fn
        preds, scale_losses, df = [], [], {}
        total = torch.zeros(3, **self.f32)                            # [0] total loss, [1] regularisation value, [2] [1] * regularization
        for i in range(m.depth):
            f, b_ln = outs[i], None
            if m.use_output_normalization and m.use_ln and m.output_norm_at_heads:     # the archive's graph: only the heads read the
                f, b_ln = self.norm_act(m._out_ln_name(i), f, "linear")                # normalised maps, the decoder the raw ones
            pred, losses, df[i] = self.head_step(f"head{i}", f, gts[i], depth_weights[i], total)
            preds.append(pred)
            scale_losses.append(losses)
            if b_ln is not None:
                df[i] = b_ln(df[i])

        # -- backward: decoder levels top (d = 0) to bottom, each yields the gradient of its Laplacian skip and of the level below
        dlow = {}
        for d in range(m.depth):
            g = df[d] if d not in dlow else ops.add(df[d], dlow[d])
            if d == last:
                break
            chain, b_join = dec[d]
            for b_ in reversed(chain):
                g = b_(g)
            dlap[d], dlow[d + 1] = b_join(g)
        for b_ in reversed(enc):
            g = b_(g)
        b_base(g)
        self._finish(total, self.regularize(total))
        return preds, scale_losses, total
