"""The ConvNeXt backbone, `"type": "convnext"` (bfcnn/backbone_convnext.py:103-375 + convnext_blocks_full / resnet_blocks_full with
ln_after_first_conv_params=True, bfcnn/backbone_blocks.py:51-68, 163-246): base convolution (`base_activation`), BatchNorm
(`add_initial_bn`, default True here), `no_layers` blocks, [final BatchNorm], [Concatenate input], [ChannelwiseMultiplier],
[Multiplier], then the usual denoiser head.  Inference here, training in convnext_backbone_train.py.

A block: conv0 (depthwise k x k, its activation) -> LayerNormalization(center=False, scale=True, epsilon 1e-3) -> conv1 (1x1 C -> E,
its activation) -> [channel gate on the E-wide tensor, `add_gates`] -> conv2 (1x1 E -> C, `base_activation`) ->
[ChannelwiseMultiplier] -> [Multiplier] -> [RandomOnOff: identity at inference] -> Add.  The builder forces bn_params to None inside
the blocks, so `use_bn` changes nothing; the initial / final BatchNorm exist regardless of it.

Built: filters 32 / 64; blocks of exactly three convolutions -- depthwise (multiplier 1, k in {1, 3, 5, 7}), 1x1 C -> E, 1x1 E -> C
with (C, E), (E, C) instances of bf_op_pointwise; head filters 32; base kernel odd and at most 7.  The reference's own default width
(96 / 384) is refused: the LayerNorm and pointwise kernels are built for power-of-two channel groups.  Importing a Keras archive of
a convnext model is not built.

Forward paths (set_option, each 0 / 1):
  arith 0 (default): exact fp32.  conv0 + LN is one bf_op_dwconv_ln launch when conv0's activation is linear, else
      bf_op_dwconv_mult (with the activation) then bf_op_dwconv_ln with k = 0; then bf_op_convnext_mlp where E = 4C, there is no
      gate and conv2 is linear, else two bf_op_pointwise_ex calls.  The block's closing multipliers are folded into conv2's
      kernel when `base_activation` commutes with a non-negative factor, else a scale_add pass carries them and the Add.
  arith 1: the MLP on the f16 matrix cores with split-f16 operands (bf_op_convnext_mlp_h3; |activation| < 65504, as documented
      for GenericResnetHydra); with fuse_block 1 (default) the whole block in bf_op_convnext_block_h3 where that kernel exists
      (C = 32, k in {3, 5}, linear conv0 activation, no gate).  The base convolution and the head stay exact fp32."""
import copy
from typing import Dict, Optional

import numpy as np
import torch

from . import unet_laplacian as UL
from .custom_logger import logger
from .op_graph import OpGraphModel, concat_input
from .resnet_generic import channel_gate, scale_add

FILTERS = (32, 64)
BLOCK_KERNELS = (1, 3, 5, 7)                   # bf_op_dwconv_ln / bf_op_dwconv_wgrad
EXPANSIONS = (32, 64, 128, 256)                # (C, E) and (E, C) are instances of bf_op_pointwise for C in FILTERS
# options the reference convnext builder accepts and its blocks never read: mean_sigma_params / gradient dropout are not used by
# resnet_blocks_full's body (backbone_blocks.py:164-243), bn_params is overwritten with None (:64)
IGNORED = ("add_mean_sigma_normalization", "add_gradient_dropout", "use_bn")


class ConvnextHydra(OpGraphModel):
    FAMILY = "convnext"
    OPTIONS = ("arith", "fuse_block")

    def __init__(self, config: Dict, device=None, seed: Optional[int] = None):
        """What the reference rejects with a ValueError is one here, with one exception: a block that is not three convolutions
        is a NotImplementedError, checked before the list-length checks (the reference would raise ValueError for lists of
        unequal length there)."""
        bb, dn = config["backbone"], config["denoiser"]
        self.config = copy.deepcopy(config)
        # --- refused: options the graph here does not build
        if bb.get("use_bias", False):
            raise NotImplementedError("convnext: use_bias is outside the built graph")
        for key in ("selector_params", "base_conv_params"):
            if bb.get(key) is not None:
                raise NotImplementedError(f"convnext: {key} is outside the built graph")
        for key in ("use_bias", "use_bn", "use_ln"):
            if dn.get(key, False):
                raise NotImplementedError(f"convnext denoiser head: {key} is outside the built graph")
        ignored = [k for k in IGNORED if bb.get(k)]
        if ignored:
            logger.info(f"convnext options without effect (as in the reference): {ignored}")
        # --- arguments (backbone_convnext.py:103-133 defaults, :175-208 fixing and checks)
        self.no_layers = int(bb["no_layers"])
        if self.no_layers < 0:
            raise ValueError("no_layers must be >= 0")                           # backbone_blocks.py:120-121
        self.kernel_size = int(bb.get("kernel_size", 3))
        self.filters = int(bb.get("filters", 32))
        self.block_kernels = [int(k) for k in bb.get("block_kernels", [7, 1, 1])]
        self.block_filters = [int(f) for f in bb.get("block_filters", [96, 384, 96])]
        nb = len(self.block_kernels)
        if nb != 3:
            raise NotImplementedError(f"convnext: a block of {nb} convolutions is outside the built graph (exactly three: depthwise, "
                                      f"1x1 C -> E, 1x1 E -> C)")
        self.block_depthwise = [int(d) for d in (bb.get("block_depthwise", [1, -1, -1]) or [-1] * nb)]
        self.block_groups = [int(g) for g in (bb.get("block_groups", [1, 1, 1]) or [1] * nb)]
        self.activation = bb.get("activation", "linear")
        self.block_activation = list(bb.get("block_activation", ["linear", "gelu", "linear"]) or [self.activation] * nb)
        self.kernel_regularizer = bb.get("kernel_regularizer", "l1")
        block_regularizer = bb.get("block_regularizer") or [self.kernel_regularizer] * nb
        if len(self.block_filters) != nb:
            raise ValueError("len(block_filters) must == len(block_kernels)")
        if len(self.block_groups) != nb:
            raise ValueError("len(block_filters) must == len(block_groups)")
        if len(block_regularizer) != nb:
            raise ValueError("len(block_regularizer) must == len(block_groups)")
        if len(self.block_activation) != nb:
            raise ValueError("len(block_activation) must == len(block_groups)")
        if len(self.block_depthwise) != nb:
            raise ValueError("len(block_depthwise) must == len(block_kernels)")
        self.base_activation = bb.get("base_activation", "linear")
        self.block_activation[-1] = self.base_activation                      # :260
        self.use_bn = False                                                    # bn_params = None inside the blocks (backbone_blocks.py:64)
        self.add_gates = bool(bb.get("add_gates", False))
        self._parse_dropout(bb)
        self.add_initial_bn = bool(bb.get("add_initial_bn", True))             # :124, 341-342
        self.add_final_bn = bool(bb.get("add_final_bn", False))                # :351-352
        self.add_concat_input = bool(bb.get("add_concat_input", False))        # :355-356
        self.add_channelwise = bool(bb.get("add_channelwise_scaling", False))  # per block (:316-318) and final (:359-360)
        self.add_multiplier = bool(bb.get("add_learnable_multiplier", False))  # per block (:320-322) and final (:363-364)
        self.selector = None
        self._parse_io(bb, dn)
        for a in self.block_activation + [self.base_activation, self.head_activation]:
            UL._act(a)
        self._check_scope()
        self._init_storage(device, seed)
        self.arith = 0                          # see OPTIONS
        self.fuse_block = 1

    @staticmethod
    def train_graph_class():
        from .convnext_backbone_train import ConvnextTrainGraph
        return ConvnextTrainGraph

    def _check_scope(self):
        C, (k0, k1, k2), (_, E, c2) = self.filters, self.block_kernels, self.block_filters
        if C not in FILTERS:
            raise NotImplementedError(f"convnext: filters={C} (32 / 64 are built; the reference's default width 96 / 384 is not: the "
                                      f"LayerNorm and pointwise kernels are built for power-of-two channel groups)")
        if self.head_filters != 32 or self.kernel_size > 7 or self.kernel_size % 2 == 0:
            raise NotImplementedError("convnext: head filters must be 32 and the base kernel odd and at most 7x7")
        if self.block_depthwise != [1, -1, -1] or k0 not in BLOCK_KERNELS or k1 != 1 or k2 != 1:
            raise NotImplementedError(f"convnext: block_kernels={self.block_kernels}, block_depthwise={self.block_depthwise} is outside "
                                      f"the built blocks (depthwise k in {BLOCK_KERNELS} with multiplier 1, then two 1x1 convolutions)")
        if self.block_groups != [1, 1, 1]:
            raise NotImplementedError(f"convnext: block_groups={self.block_groups} (grouped block convolutions are outside the built graph)")
        if c2 != C:
            raise ValueError(f"the last block convolution must produce {C} channels for the residual Add (got {c2})")
        if E not in EXPANSIONS:
            raise NotImplementedError(f"convnext: block convolutions {C}->{E}->{C} are outside bf_op_pointwise (the middle width must be "
                                      f"one of {EXPANSIONS}; power-of-two channel groups)")
        if self.add_gates and (256 % E or max(E // 8, 2) > 32):
            raise NotImplementedError(f"convnext: add_gates on {E} channels is outside bf_op_gate_fwd")
        self.expansion = E

    # -- inventory (Keras creation order) ------------------------------------------------------------------------------------------
    def _build_inventory(self):
        k, C, E, k0 = self.kernel_size, self.filters, self.expansion, self.block_kernels[0]
        out = [("base/kernel", (k, k, self.in_channels, C), "conv")]
        state = []
        if self.add_initial_bn:
            out.append(("initial_bn/gamma", (C,), "bn_gamma"))
            state += [("initial_bn/moving_mean", (C,)), ("initial_bn/moving_variance", (C,))]
        for i in range(self.no_layers):
            out.append((f"block{i}/conv0/kernel", (k0, k0, C, 1), "depthwise"))
            out.append((f"block{i}/ln/gamma", (C,), "ln_gamma"))
            out.append((f"block{i}/conv1/kernel", (1, 1, C, E), "conv"))
            if self.add_gates:                         # the two bias-free Dense layers of the gate (backbone_blocks.py:136-161)
                c8 = max(int(E / 8), 2)
                out.append((f"block{i}/gate/dense0/kernel", (E, c8), "dense"))
                out.append((f"block{i}/gate/dense1/kernel", (c8, E), "dense"))
            out.append((f"block{i}/conv2/kernel", (1, 1, E, C), "conv"))
            if self.add_channelwise:
                out.append((f"block{i}/channelwise/w0", (C,), "channelwise"))
            if self.add_multiplier:
                out.append((f"block{i}/multiplier/w0", (1,), "multiplier"))
        if self.add_final_bn:
            out.append(("final_bn/gamma", (C,), "bn_gamma"))
            state += [("final_bn/moving_mean", (C,)), ("final_bn/moving_variance", (C,))]
        cf = C + (self.in_channels if self.add_concat_input else 0)
        if self.add_channelwise:
            out.append(("channelwise/w0", (cf,), "channelwise"))
        if self.add_multiplier:
            out.append(("multiplier/w0", (1,), "multiplier"))
        out.append(("head/conv0/kernel", (1, 1, cf, self.head_filters), "conv"))
        out.append(("head/conv1/kernel", (1, 1, self.head_filters, self.out_channels), "conv"))
        return out, state

    def _initial_value(self, shape, kind: str, rng) -> np.ndarray:
        if kind == "ln_gamma":                         # LayerNormalization's gamma: ones, no regulariser
            return np.ones(shape)
        return super()._initial_value(shape, kind, rng)

    # -- packing (host arithmetic on the weights only) -----------------------------------------------------------------------------
    def _mlp_fused(self) -> bool:
        """conv1 -> activation -> conv2 -> Add as one MLP kernel: E = 4C, nothing between the two convolutions, conv2 linear"""
        return self.expansion == 4 * self.filters and not self.add_gates and UL._act(self.base_activation)[0] == 0

    def _pack(self):
        if self._packed is not None:
            return self._packed
        W, S, dev, bn_affine = self._host_weights()
        C, k0 = self.filters, self.block_kernels[0]
        homogeneous = UL._act(self.base_activation)[0] in (0, 1, 2)           # act(s z) = s act(z) for s >= 0

        def end_scale(prefix, n):
            sc = np.ones(n)
            if self.add_channelwise:
                sc = sc * np.maximum(W[prefix + "channelwise/w0"] + 1.0, 0.0)
            if self.add_multiplier:
                sc = sc * np.maximum(W[prefix + "multiplier/w0"] + 1.0, 0.0)
            return sc
        P = {"base": dev(W["base/kernel"])}
        for base in (["initial_bn"] if self.add_initial_bn else []) + (["final_bn"] if self.add_final_bn else []):
            sc, sh = bn_affine(base)
            P[base] = (dev(sc.reshape(1, 1, -1, 1)), dev(sh))
        for i in range(self.no_layers):
            b = f"block{i}"
            w1, w2 = W[f"{b}/conv1/kernel"][0, 0], W[f"{b}/conv2/kernel"][0, 0]
            if self.add_channelwise or self.add_multiplier:
                es = end_scale(f"{b}/", C)
                if homogeneous:                        # rides on conv2's output channels
                    w2 = w2 * es[None, :]
                else:                                  # its own pass, which carries the Add
                    P[f"{b}/scale"] = dev(es)
            P[f"{b}/dw"] = dev(W[f"{b}/conv0/kernel"])                        # [k, k, C, 1]
            P[f"{b}/ln"] = dev(W[f"{b}/ln/gamma"])
            P[f"{b}/pw"] = (UL.pack_pointwise(dev(w1)), UL.pack_pointwise(dev(w2)))
            if self.add_gates:
                P[f"{b}/gate"] = (dev(W[f"{b}/gate/dense0/kernel"]), dev(W[f"{b}/gate/dense1/kernel"]))
            if self._mlp_fused():
                P[f"{b}/mlp_h3"] = UL.pack_mlp_h3(dev(w1), dev(w2))
        w_head0 = W["head/conv0/kernel"][0, 0]
        cf = w_head0.shape[0]
        if self.add_channelwise or self.add_multiplier:                       # no shift behind them: rows of the head's first kernel
            w_head0 = w_head0 * end_scale("", cf)[:, None]
        self._head_cin = next(c for c in (32, 64, 128, 256) if c >= cf)
        w_head0 = np.concatenate([w_head0, np.zeros((self._head_cin - cf, w_head0.shape[1]))], axis=0)   # zero rows for padding
        P["head0"] = UL.pack_pointwise(dev(w_head0))
        P["head1"] = dev(W["head/conv1/kernel"])
        self._packed = P
        return P

    # -- forward -------------------------------------------------------------------------------------------------------------------
    def _block(self, f: torch.Tensor, i: int, P) -> torch.Tensor:
        b = f"block{i}"
        C, E, k0 = self.filters, self.expansion, self.block_kernels[0]
        a0, a1, a2 = self.block_activation
        dw, gamma = P[f"{b}/dw"], P[f"{b}/ln"]
        linear0 = UL._act(a0)[0] == 0
        h3 = self.arith == 1 and f"{b}/mlp_h3" in P
        if h3 and self.fuse_block and C == 32 and k0 in (3, 5) and linear0:
            return UL.convnext_block_h3(f, dw.view(k0, k0, C), gamma, P[f"{b}/mlp_h3"], None, a1)
        if linear0:
            t = UL.dwconv_ln(f, dw, gamma)
        else:                                          # the activation sits between the convolution and the LayerNorm
            t = UL.dwconv_ln(UL.dwconv_mult(f, dw, None, a0), None, gamma)
        if h3:
            return UL.convnext_mlp_h3(t, f, P[f"{b}/mlp_h3"], None, a1)
        w1p, w2p = P[f"{b}/pw"]
        if self._mlp_fused():
            return UL.convnext_mlp(t, f, w1p, w2p, None, a1)
        tail = P.get(f"{b}/scale")
        t = UL.pointwise_ex(t, w1p, E, 0, a1)
        if self.add_gates:
            t = channel_gate(t, *P[f"{b}/gate"])
        t = UL.pointwise_ex(t, w2p, C, 0, a2, res=f if tail is None else None)      # Add()([x, previous_layer]) (backbone_blocks.py:242)
        return t if tail is None else scale_add(f, t, tail)

    def _features(self, x: torch.Tensor, H: int, W: int) -> torch.Tensor:
        P = self._pack()
        f = UL.first_conv(x, P["base"], H, W, self.base_activation, True, self.v_min, self.v_max, arith=0)
        if self.add_initial_bn:
            f = UL.dwconv_mult(f, *P["initial_bn"])
        for i in range(self.no_layers):
            f = self._block(f, i, P)
        if self.add_final_bn:
            f = UL.dwconv_mult(f, *P["final_bn"])
        if self.add_concat_input:
            f = concat_input(f, x, H, W, self._head_cin, self.v_min, self.v_max)
        return f

    def _outputs(self, x: torch.Tensor, H: int, W: int, crop=None, as_uint8: bool = False):
        """the head in exact fp32 whatever `arith` says (the option covers the blocks' MLP)"""
        P = self._pack()
        Ho, Wo = crop or (H, W)
        return UL.head_fused(self._features(x, H, W), None, P["head0"], self.head_activation, P["head1"], Ho, Wo, as_uint8, True,
                             self.v_min, self.v_max, arith=0)
