"""The plain U-Net backbone, `"type": "unet"` (bfcnn/backbone_unet.py:18-268 + unet_blocks, bfcnn/backbone_blocks.py:319-403):
base convolution, `no_levels` encoder levels (entry convolution from level 1 on, `no_layers` residual blocks, MaxPooling2D(2, 2,
same)), the decoder over the skips from the deepest up (Concatenate([UpSampling2D(2, nearest)(x), skip]) from the second level on,
entry convolution, the blocks again), then the closing layers and the usual denoiser head.  Inference here, training in
unet_backbone_train.py.

The residual blocks are those of the generic resnet (`GenericResnetHydra`): the first convolution without BatchNorm, the second /
third with it, the channel gate behind the second (`add_gates`), the per-block Multiplier (`add_learnable_multiplier`) and
RandomOnOff (`dropout_rate`, identity at inference).  `unet_blocks` forwards only bn / gate / dropout / multiplier parameters to the
blocks (backbone_blocks.py:322-333), so the per-block ChannelwiseMultiplier, the selector, sparsity and mean / sigma normalisation
are not part of the graph.  Exact fp32 throughout: every convolution is bf_op_conv2d (BatchNorm folded: scale into the weights at
pack time, shift as the epilogue bias), the base convolution and the head run their exact fp32 kernels (arith 0).  The decoder
entries read the upsampled tensor and the skip directly (bf_op_upcat_conv2d); neither the upsampled tensor nor the concat is
written."""
import copy
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _native as N
from . import unet_laplacian as UL
from ._native import call
from .custom_logger import logger
from .op_graph import OpGraphModel, concat_input
from .resnet_generic import channel_gate, scale_add

# channel pairs of the bf_op_conv2d instances (any odd k): the entries, the block convolutions and the unfused decoder entries
CONV_PAIRS = {(32, 32), (32, 64), (64, 32), (64, 64), (64, 128), (128, 64), (128, 128), (256, 128), (128, 256)}
UPCAT_KERNELS = (1, 3, 5)           # bf_op_upcat_conv2d: c_up = c_skip = cout in {32, 64, 128}
FILTERS = (32, 64, 128)
# options the reference unet accepts and does not use: the builder turns add_selector / add_sparsity /
# add_mean_sigma_normalization into block parameters that unet_blocks drops into **kwargs (backbone_blocks.py:319-333); the
# block_* lists are not arguments of the unet builder and land in its own **kwargs (backbone_unet.py:44, logged at :83)
IGNORED = ("add_selector", "add_sparsity", "add_mean_sigma_normalization", "block_depthwise", "block_groups", "block_activation",
           "block_regularizer")


def upcat_conv2d(up: torch.Tensor, skip: torch.Tensor, wp: torch.Tensor, cout: int, k: int, act: str = "linear",
                 res: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """res + act(conv_kxk(Concatenate([UpSampling2D(2, nearest)(up), skip])) + bias), one kernel; wp = pack_conv of the
    (c_up + c_skip) -> cout kernel"""
    B, H, W, cs = skip.shape
    cu = up.shape[-1]
    if tuple(up.shape[:3]) != (B, H // 2, W // 2) or H % 2 or W % 2:
        raise ValueError(f"upcat_conv2d: up {tuple(up.shape)} is not the half-resolution of skip {tuple(skip.shape)}")
    out = torch.empty((B, H, W, cout), dtype=torch.float32, device=skip.device)
    code, a = UL._act(act)
    call("bf_op_upcat_conv2d", N.ptr(up), N.ptr(skip), N.ptr(out), N.ptr(wp), N.ptr(res), N.ptr(bias), B, H, W, cu, cs, cout, k,
         code, a, N.stream_ptr(skip))
    return out


def upsample_concat(up: torch.Tensor, skip: torch.Tensor) -> torch.Tensor:
    """Concatenate([UpSampling2D(2, nearest)(up), skip]) materialised (bf_upsample2x + bf_op_concat_channels)"""
    B, h, w, cu = up.shape
    cs = skip.shape[-1]
    u = torch.empty((B, 2 * h, 2 * w, cu), dtype=torch.float32, device=up.device)
    call("bf_upsample2x", N.ptr(up), None, N.ptr(u), B, h, w, cu, 0, 1.0, 0.0, N.stream_ptr(up))
    cat = torch.empty((B, 2 * h, 2 * w, cu + cs), dtype=torch.float32, device=up.device)
    call("bf_op_concat_channels", N.ptr(u), N.ptr(skip), None, N.ptr(cat), B * 4 * h * w, cu, cs, 0, N.stream_ptr(up))
    return cat


def tanh_(t: torch.Tensor) -> torch.Tensor:
    """tf.tanh (add_clip) as an activation-only pass"""
    out = torch.empty_like(t)
    v = t.view(1, 1, -1, 32)
    call("bf_op_dwconv_ln", N.ptr(v), N.ptr(out), None, None, 1, 1, v.shape[2], 32, 0, UL.LN_EPSILON, 4, 0.0, N.stream_ptr(t))
    return out


class UnetHydra(OpGraphModel):
    FAMILY = "unet"
    # fuse_upcat: 1 (default) the decoder entries read the upsampled tensor and the skip directly (bf_op_upcat_conv2d);
    # 0: bf_upsample2x + bf_op_concat_channels + bf_op_conv2d (the same result, bit for bit).
    OPTIONS = ("fuse_upcat",)
    arith = 0                           # exact fp32 throughout (not an option here)

    def __init__(self, config: Dict, device=None, seed: Optional[int] = None):
        bb, dn = config["backbone"], config["denoiser"]
        self.config = copy.deepcopy(config)
        # --- refused: options the graph here does not build
        for key in ("add_sparse_features", "use_bias"):                          # backbone_unet.py:236-242; use_bias: BN center, conv bias
            if bb.get(key, False):
                raise NotImplementedError(f"unet: {key} is outside the built graph")
        for key in ("use_bias", "use_bn", "use_ln"):
            if dn.get(key, False):
                raise NotImplementedError(f"unet denoiser head: {key} is outside the built graph")
        ignored = [k for k in IGNORED if bb.get(k)]
        if ignored:
            logger.info(f"unet options without effect (as in the reference): {ignored}")
        # --- arguments (backbone_unet.py:18-45 defaults, :86-95 checks)
        self.no_levels = int(bb["no_levels"])
        self.no_layers = int(bb["no_layers"])
        if self.no_levels < 1:
            raise ValueError("no_levels must be >= 1")
        if self.no_layers < 0:
            raise ValueError("no_layers must be >= 0")                           # backbone_blocks.py:341-342
        self.kernel_size = int(bb.get("kernel_size", 3))
        self.filters = int(bb.get("filters", 32))
        self.block_kernels = [int(k) for k in bb.get("block_kernels", [3, 3])]
        self.block_filters = [int(f) for f in bb.get("block_filters", [32, 32])]
        nb = len(self.block_kernels)
        self._check_block_count(nb)
        if len(self.block_filters) <= 0:
            raise ValueError("len(block_filters) must be >= 0 ")
        if nb != len(self.block_filters):
            raise ValueError("len(block_filters) must == len(block_kernels)")
        self.activation = bb.get("activation", "relu")
        self.base_activation = bb.get("base_activation", "linear")
        # convs_params[j]: `activation`, the last one `base_activation` (:127); the entry convolutions use convs_params[0]
        self.block_activation = [self.activation] * nb
        self.block_activation[-1] = self.base_activation
        self.entry_activation = self.block_activation[0]
        self._parse_bn_gates(bb, nb)
        self._parse_dropout(bb)
        self.add_multiplier = bool(bb.get("add_learnable_multiplier", False))  # per block (unet_blocks forwards it) and final
        self.add_channelwise = bool(bb.get("add_channelwise_scaling", False))  # final only (unet_blocks drops channelwise_params)
        self.add_initial_bn = bool(bb.get("add_initial_bn", False))            # :216-217
        self.add_final_bn = bool(bb.get("add_final_bn", False))                # :226-228
        self.add_concat_input = bool(bb.get("add_concat_input", False))        # :230-234
        self.add_clip = bool(bb.get("add_clip", False))                        # :254-256
        self.kernel_regularizer = bb.get("kernel_regularizer", "l1")
        self._parse_io(bb, dn)
        for a in self.block_activation + [self.activation, self.base_activation, self.head_activation]:
            UL._act(a)
        self._check_channels()
        self._init_storage(device, seed)
        self.fuse_upcat = 1                     # see OPTIONS

    @staticmethod
    def train_graph_class():
        from .unet_backbone_train import UnetBackboneTrainGraph
        return UnetBackboneTrainGraph

    # -- graph bookkeeping -------------------------------------------------------------------
    def _check_channels(self):
        """walks the graph's channel counts: what Keras rejects is a ValueError (the residual Add), what the operators do not
        cover a NotImplementedError naming the pair"""
        C, bf, nb = self.filters, self.block_filters, len(self.block_kernels)
        if C not in (32, 64):                  # the exact fp32 base convolution (bf_op_first_conv) writes 16 / 32 / 64 channels
            raise NotImplementedError(f"unet: filters={C} (32 / 64 are built; 16 filters has its own whole-image engine, 128 no base "
                                      f"convolution)")
        if self.head_filters != 32 or self.kernel_size > 7 or self.kernel_size % 2 == 0:
            raise NotImplementedError("unet: head filters must be 32 and the base kernel odd and at most 7x7")

        def conv(cin, cout, what):
            if (cin, cout) not in CONV_PAIRS:
                raise NotImplementedError(f"unet: {what} convolution {cin}->{cout} is outside the built operators")

        def blocks(cin, where):
            if self.no_layers == 0:
                return cin
            c = cin
            for j in range(nb):
                conv(c, bf[j], f"{where} block conv{j}")
                c = bf[j]
            if c != cin:
                raise ValueError(f"unet {where}: the residual Add needs the last block convolution to produce {cin} channels (got {c})")
            return cin

        skips, c = [], C
        for lv in range(self.no_levels):
            if lv > 0:
                conv(c, bf[0], f"encoder level {lv} entry")
                c = bf[0]
            c = blocks(c, f"encoder level {lv}")
            skips.append(c)
        x = None
        for lv in reversed(range(self.no_levels)):
            s = skips[lv]
            if x is None:
                conv(s, bf[0], f"decoder level {lv} entry")
            else:
                if not (x == s == bf[0] and x in FILTERS and self.block_kernels[0] in UPCAT_KERNELS):
                    raise NotImplementedError(f"unet: decoder level {lv} entry (upsampled {x}, skip {s}) -> {bf[0]}, k={self.block_kernels[0]} "
                                              f"is outside bf_op_upcat_conv2d (c_up = c_skip = cout in {FILTERS}, k in {UPCAT_KERNELS})")
            x = blocks(bf[0], f"decoder level {lv}")
        self.out_features = x
        self.level_channels = skips

    def _block_inventory(self, prefix, cin, out, state):
        for i in range(self.no_layers):
            c = cin
            for j, (kk, cf) in enumerate(zip(self.block_kernels, self.block_filters)):
                out.append((f"{prefix}/block{i}/conv{j}/kernel", (kk, kk, c, cf), "conv"))
                if j >= 1 and self.use_bn:                # the first convolution of a block has no BN (backbone_blocks.py:174-179)
                    out.append((f"{prefix}/block{i}/bn{j}/gamma", (cf,), "bn_gamma"))
                    state += [(f"{prefix}/block{i}/bn{j}/moving_mean", (cf,)), (f"{prefix}/block{i}/bn{j}/moving_variance", (cf,))]
                if j == 1 and self.add_gates:             # the two bias-free Dense layers of the gate (:146-160)
                    c8 = max(int(cf / 8), 2)
                    out.append((f"{prefix}/block{i}/gate/dense0/kernel", (cf, c8), "dense"))
                    out.append((f"{prefix}/block{i}/gate/dense1/kernel", (c8, cf), "dense"))
                c = cf
            if self.add_multiplier:
                out.append((f"{prefix}/block{i}/multiplier/w0", (1,), "multiplier"))

    def _build_inventory(self):
        k, C, bf0, k0 = self.kernel_size, self.filters, self.block_filters[0], self.block_kernels[0]
        out = [("base/kernel", (k, k, self.in_channels, C), "conv")]
        state = []
        if self.add_initial_bn:
            out.append(("initial_bn/gamma", (C,), "bn_gamma"))
            state += [("initial_bn/moving_mean", (C,)), ("initial_bn/moving_variance", (C,))]
        c = C
        for lv in range(self.no_levels):
            if lv > 0:
                out.append((f"enc{lv}/entry/kernel", (k0, k0, c, bf0), "conv"))
                c = bf0
            self._block_inventory(f"enc{lv}", c, out, state)
        x = None
        for lv in reversed(range(self.no_levels)):
            s = self.level_channels[lv]
            out.append((f"dec{lv}/entry/kernel", (k0, k0, s if x is None else x + s, bf0), "conv"))
            x = bf0
            self._block_inventory(f"dec{lv}", x, out, state)
        cf = x
        if self.add_final_bn:
            out.append(("final_bn/gamma", (cf,), "bn_gamma"))
            state += [("final_bn/moving_mean", (cf,)), ("final_bn/moving_variance", (cf,))]
        if self.add_concat_input:
            cf += self.in_channels
        if self.add_channelwise:
            out.append(("channelwise/w0", (cf,), "channelwise"))
        if self.add_multiplier:
            out.append(("multiplier/w0", (1,), "multiplier"))
        out.append(("head/conv0/kernel", (1, 1, cf, self.head_filters), "conv"))
        out.append(("head/conv1/kernel", (1, 1, self.head_filters, self.out_channels), "conv"))
        return out, state

    def block_prefixes(self) -> List[str]:
        """the `no_layers` block groups in graph order: enc0 .. enc{L-1}, dec{L-1} .. dec0"""
        return [f"enc{lv}" for lv in range(self.no_levels)] + [f"dec{lv}" for lv in reversed(range(self.no_levels))]

    def dropout_blocks(self) -> List:
        """the keys of RandomOnOff's per-step draw (one per residual block): (group, block index)"""
        return [(pre, i) for pre in self.block_prefixes() for i in range(self.no_layers)]

    # -- packing (host arithmetic on the weights only: BatchNorm folding) ------------------------------------------------------
    def _pack(self):
        if self._packed is not None:
            return self._packed
        W, S, dev, bn_affine = self._host_weights()
        homogeneous = lambda a: UL._act(a)[0] in (0, 1, 2)                 # act(s z) = s act(z) for s >= 0
        nb = len(self.block_kernels)
        P = {"base": dev(W["base/kernel"])}
        if self.add_initial_bn:
            sc, sh = bn_affine("initial_bn")
            P["initial_bn"] = (dev(sc.reshape(1, 1, -1, 1)), dev(sh))
        for lv in range(self.no_levels):
            P[f"enc{lv}/entry"] = UL.pack_conv(dev(W[f"enc{lv}/entry/kernel"])) if lv > 0 else None
            P[f"dec{lv}/entry"] = UL.pack_conv(dev(W[f"dec{lv}/entry/kernel"]))
        for pre in self.block_prefixes():
            for i in range(self.no_layers):
                b = f"{pre}/block{i}"
                for j in range(nb):
                    k = W[f"{b}/conv{j}/kernel"]
                    scale, shift = np.ones(k.shape[-1]), None
                    if j >= 1 and self.use_bn:               # inference BN folded: gamma (x - mean) / sqrt(var + eps), center=False
                        scale, shift = bn_affine(f"{b}/bn{j}")
                    if j == nb - 1 and self.add_multiplier:
                        # the block's Multiplier (relu(w0 + 1) >= 0) rides on the last convolution when its activation commutes
                        # with a non-negative factor and no gate sits between, else it is its own pass carrying the Add
                        es = max(float(W[f"{b}/multiplier/w0"][0]) + 1.0, 0.0)
                        if homogeneous(self.block_activation[j]) and not (self.add_gates and j == 1):
                            scale, shift = scale * es, (None if shift is None else shift * es)
                        else:
                            P[f"{b}/scale"] = dev(np.full(k.shape[-1], es))
                    P[f"{b}/conv{j}"] = (UL.pack_conv(dev(k * scale[None, None, None, :])), None if shift is None else dev(shift))
                    if j == 1 and self.add_gates:
                        P[f"{b}/gate"] = (dev(W[f"{b}/gate/dense0/kernel"]), dev(W[f"{b}/gate/dense1/kernel"]))
        if self.add_final_bn:
            sc, sh = bn_affine("final_bn")
            P["final_bn"] = (dev(sc.reshape(1, 1, -1, 1)), dev(sh))
        w_head0 = W["head/conv0/kernel"][0, 0]
        cf = w_head0.shape[0]
        es = np.ones(cf)
        if self.add_channelwise:
            es = es * np.maximum(W["channelwise/w0"] + 1.0, 0.0)
        if self.add_multiplier:
            es = es * np.maximum(W["multiplier/w0"] + 1.0, 0.0)
        self._head_cin = next(c for c in (32, 64, 128, 256) if c >= cf)
        if self.add_clip:                                  # tanh sits between the multipliers and the head: their own pass
            if self.add_channelwise or self.add_multiplier:
                P["final_scale"] = dev(np.concatenate([es, np.ones(self._head_cin - cf)]))
        else:                                              # no shift: the head's first 1x1 absorbs the factor (rows of W)
            w_head0 = w_head0 * es[:, None]
        w_head0 = np.concatenate([w_head0, np.zeros((self._head_cin - cf, w_head0.shape[1]))], axis=0)   # zero rows for padding
        P["head0"] = UL.pack_pointwise(dev(w_head0))
        P["head1"] = dev(W["head/conv1/kernel"])
        self._packed = P
        return P

    # -- forward -----------------------------------------------------------------------------
    def _blocks(self, f: torch.Tensor, pre: str, P) -> torch.Tensor:
        nb = len(self.block_kernels)
        for i in range(self.no_layers):
            b = f"{pre}/block{i}"
            tail = P.get(f"{b}/scale")
            t = f
            for j in range(nb):
                wp, shift = P[f"{b}/conv{j}"]
                gate_here = self.add_gates and j == 1
                last = j == nb - 1
                res = f if last and not gate_here and tail is None else None          # Add()([x, previous_layer]) (:242)
                t = UL.conv2d(t, wp, self.block_filters[j], self.block_kernels[j], 1, self.block_activation[j], res=res, bias=shift)
                if gate_here:
                    t = channel_gate(t, *P[f"{b}/gate"], res=f if last and tail is None else None)
            if tail is not None:
                t = scale_add(f, t, tail)
            f = t
        return f

    def _check_size(self, H: int, W: int):
        m = 1 << (self.no_levels - 1)
        if H % m or W % m:
            raise ValueError(f"unet with {self.no_levels} levels: H and W ({H}x{W}) must be multiples of {m}")

    def _features(self, x: torch.Tensor, H: int, W: int) -> torch.Tensor:
        L = self.no_levels
        self._check_size(H, W)
        P = self._pack()
        bf0, k0, ea = self.block_filters[0], self.block_kernels[0], self.entry_activation
        f = UL.first_conv(x, P["base"], H, W, self.base_activation, True, self.v_min, self.v_max, arith=0)
        if self.add_initial_bn:
            f = UL.dwconv_mult(f, *P["initial_bn"])
        skips = []
        for lv in range(L):
            if lv > 0:
                f = UL.conv2d(UL.maxpool2(f), P[f"enc{lv}/entry"], bf0, k0, 1, ea)   # the last level's pooled output is never used
            f = self._blocks(f, f"enc{lv}", P)
            skips.append(f)
        f = None
        for lv in reversed(range(L)):
            s = skips[lv]
            if f is None:
                f = UL.conv2d(s, P[f"dec{lv}/entry"], bf0, k0, 1, ea)
            elif self.fuse_upcat:
                f = upcat_conv2d(f, s, P[f"dec{lv}/entry"], bf0, k0, ea)
            else:
                f = UL.conv2d(upsample_concat(f, s), P[f"dec{lv}/entry"], bf0, k0, 1, ea)
            f = self._blocks(f, f"dec{lv}", P)
        if self.add_final_bn:
            f = UL.dwconv_mult(f, *P["final_bn"])
        if self.add_concat_input:
            f = concat_input(f, x, H, W, self._head_cin, self.v_min, self.v_max)
        if self.add_clip:
            if "final_scale" in P:
                f = scale_add(None, f, P["final_scale"])
            f = tanh_(f)
        return f

    def __call__(self, x, training: bool = False):
        if not training:
            self._check_size(int(x.shape[1]), int(x.shape[2]))
        return super().__call__(x, training)
