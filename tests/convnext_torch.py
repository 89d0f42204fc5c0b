"""torch oracle of the ConvNeXt backbone (`"type": "convnext"`; bfcnn/backbone_convnext.py:103-375, convnext_blocks_full /
resnet_blocks_full with ln_after_first_conv_params=True of bfcnn/backbone_blocks.py:51-68, 163-246) for the tests: its own spec and
parameter inventory (read from the reference builder, not from blind_image_denoising_amd.convnext_backbone), the inference and
training forward with torch ops (float64 by default; float32 for the check of the +-1 LSB cap), and autograd for the gradients.
Test infrastructure only.

Keras creation order of the variables: base conv, [initial BN gamma], per block conv0 (depthwise), LN gamma, conv1, [gate dense0,
dense1], conv2, [ChannelwiseMultiplier w0], [Multiplier w0]; [final BN gamma], [ChannelwiseMultiplier], [Multiplier], head conv0,
head conv1.  Inside the blocks bn_params is None whatever use_bn says.
"""
from typing import Dict, List, Tuple

import numpy as np
import torch

from oracle import bfcnn_oracle as O
from oracle import resnet_generic_torch as RT
from oracle import unet_torch as UT

DT = torch.float64
LN_EPS = 1e-3              # keras LayerNormalization default


class ConvnextSpec:
    def __init__(self, model_config: Dict):
        bb, dn = model_config["backbone"], model_config["denoiser"]
        self.no_layers = int(bb["no_layers"])
        self.kernel_size, self.filters = int(bb.get("kernel_size", 3)), int(bb.get("filters", 32))
        self.block_kernels = [int(k) for k in bb.get("block_kernels", [7, 1, 1])]                 # backbone_convnext.py:108-113
        self.block_filters = [int(f) for f in bb.get("block_filters", [96, 384, 96])]
        nb = len(self.block_kernels)
        self.block_depthwise = list(bb.get("block_depthwise", [1, -1, -1]) or [-1] * nb)
        self.block_groups = list(bb.get("block_groups", [1, 1, 1]) or [1] * nb)
        self.activation = bb.get("activation", "linear")
        self.base_activation = bb.get("base_activation", "linear")
        self.block_activation = list(bb.get("block_activation", ["linear", "gelu", "linear"]) or [self.activation] * nb)
        self.block_activation[-1] = self.base_activation                                          # :260
        self.kernel_regularizer = bb.get("kernel_regularizer", "l1")
        self.block_regularizer = list(bb.get("block_regularizer") or [self.kernel_regularizer] * nb)
        self.head_regularizer = dn.get("kernel_regularizer", "l2")
        self.add_gates = bool(bb.get("add_gates", False))
        self.dropout_rate = float(bb.get("dropout_rate", -1))
        self.initial_bn, self.final_bn = bool(bb.get("add_initial_bn", True)), bool(bb.get("add_final_bn", False))
        self.concat_input = bool(bb.get("add_concat_input", False))
        self.channelwise = bool(bb.get("add_channelwise_scaling", False))
        self.multiplier = bool(bb.get("add_learnable_multiplier", False))
        self.in_channels = int(bb["input_shape"][-1])
        vr = bb.get("value_range", [0, 255])
        self.v_min, self.v_max = float(vr[0]), float(vr[1])
        self.head_filters, self.head_activation = int(dn.get("filters", 32)), dn.get("activation", "linear")
        self.out_channels = int(dn.get("output_channels", 3))

    def _inventory(self):
        C = self.filters
        out, state = [("base/kernel", (self.kernel_size, self.kernel_size, self.in_channels, C), "conv")], []
        if self.initial_bn:
            out.append(("initial_bn/gamma", (C,), "bn_gamma"))
            state += [("initial_bn/moving_mean", (C,)), ("initial_bn/moving_variance", (C,))]
        for i in range(self.no_layers):
            c = C
            for j, (k, f, dm) in enumerate(zip(self.block_kernels, self.block_filters, self.block_depthwise)):
                if dm != -1:
                    out.append((f"block{i}/conv{j}/kernel", (k, k, c, dm), "depthwise"))
                    c = c * dm
                else:
                    out.append((f"block{i}/conv{j}/kernel", (k, k, c, f), "conv"))
                    c = f
                if j == 0:                                        # ln_after_first_conv_params (backbone_blocks.py:187-189)
                    out.append((f"block{i}/ln/gamma", (c,), "ln_gamma"))
                if j == 1 and self.add_gates:                     # gate_no_filters = second_conv_params["filters"] (:136-161)
                    out.append((f"block{i}/gate/dense0/kernel", (c, max(c // 8, 2)), "dense"))
                    out.append((f"block{i}/gate/dense1/kernel", (max(c // 8, 2), c), "dense"))
            if self.channelwise:
                out.append((f"block{i}/channelwise/w0", (c,), "channelwise"))
            if self.multiplier:
                out.append((f"block{i}/multiplier/w0", (1,), "multiplier"))
        if self.final_bn:
            out.append(("final_bn/gamma", (C,), "bn_gamma"))
            state += [("final_bn/moving_mean", (C,)), ("final_bn/moving_variance", (C,))]
        cf = C + (self.in_channels if self.concat_input else 0)
        if self.channelwise:
            out.append(("channelwise/w0", (cf,), "channelwise"))
        if self.multiplier:
            out.append(("multiplier/w0", (1,), "multiplier"))
        out += [("head/conv0/kernel", (1, 1, cf, self.head_filters), "conv"),
                ("head/conv1/kernel", (1, 1, self.head_filters, self.out_channels), "conv")]
        return out, state

    def tensors(self) -> List[Tuple[str, Tuple[int, ...], str]]:
        return self._inventory()[0]

    def state_tensors(self) -> List[Tuple[str, Tuple[int, ...]]]:
        return self._inventory()[1]


def init_params(spec: ConvnextSpec, seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """random weights away from the creation values (so every BN, LN, multiplier and gate is exercised), glorot-scaled kernels"""
    r = np.random.default_rng(seed)
    out = []
    for name, shape, kind in spec.tensors():
        if kind in ("bn_gamma", "ln_gamma"):
            v = r.uniform(0.6, 1.4, shape)
        elif kind in ("channelwise", "multiplier"):
            v = r.uniform(-0.3, 0.3, shape)
        elif kind == "depthwise":                                 # fan in = fan out = k * k per channel
            v = r.normal(size=shape) * np.sqrt(1.0 / (shape[0] * shape[1]))
        else:
            fan = int(np.prod(shape[:-1])) if kind == "conv" else shape[0]
            v = r.normal(size=shape) * np.sqrt(2.0 / (fan + shape[-1]))
        out.append(np.asarray(v, np.float32).ravel())
    st = []
    for name, shape in spec.state_tensors():
        st.append((r.normal(size=shape) * 0.1 if name.endswith("mean") else r.uniform(0.5, 1.5, shape)).astype(np.float32).ravel())
    return np.concatenate(out), (np.concatenate(st) if st else np.zeros(0, np.float32))


def _views(items, flat):
    out, o = {}, 0
    for it in items:
        n = int(np.prod(it[1]))
        out[it[0]] = flat[o:o + n].reshape(it[1])
        o += n
    return out


def layer_norm(t, gamma):
    """keras LayerNormalization(center=False, scale=True) over the last axis"""
    mu = t.mean(dim=-1, keepdim=True)
    var = ((t - mu) ** 2).mean(dim=-1, keepdim=True)
    return (t - mu) / torch.sqrt(var + LN_EPS) * gamma


def hydra(spec: ConvnextSpec, P, S, x, training: bool, drop_scale=None):
    """returns (prediction, new state).  drop_scale: {block index: [B] factor} = RandomOnOff's draw, training only"""
    new_state = dict(S)
    drop_scale = drop_scale or {}
    scaled = lambda t, name: t * torch.relu(P[name] + 1.0)
    xn = (torch.clamp(x, spec.v_min, spec.v_max) - spec.v_min) / (spec.v_max - spec.v_min) - 0.5
    f = RT._act(RT.conv_same(xn, P["base/kernel"]), spec.base_activation)
    if spec.initial_bn:
        f = RT._batch_norm(f, "initial_bn", P, S, new_state, training)
    for i in range(spec.no_layers):
        t = f
        for j, (dm, g, a) in enumerate(zip(spec.block_depthwise, spec.block_groups, spec.block_activation)):
            w = P[f"block{i}/conv{j}/kernel"]
            t = RT._act(RT.depthwise_mult_same(t, w) if dm != -1 else RT.conv_same(t, w, g), a)
            if j == 0:
                t = layer_norm(t, P[f"block{i}/ln/gamma"])
            if j == 1 and spec.add_gates:
                y = torch.relu(t.mean(dim=(1, 2)) @ P[f"block{i}/gate/dense0/kernel"])
                y = torch.clamp(0.2 * (y @ P[f"block{i}/gate/dense1/kernel"]) + 0.5, 0.0, 1.0)
                t = t * y[:, None, None, :]
        if spec.channelwise:
            t = scaled(t, f"block{i}/channelwise/w0")
        if spec.multiplier:
            t = scaled(t, f"block{i}/multiplier/w0")
        if training and i in drop_scale:
            t = t * drop_scale[i].reshape(-1, 1, 1, 1)
        f = t + f
    if spec.final_bn:
        f = RT._batch_norm(f, "final_bn", P, S, new_state, training)
    if spec.concat_input:
        f = torch.cat([f, xn], dim=-1)
    if spec.channelwise:
        f = scaled(f, "channelwise/w0")
    if spec.multiplier:
        f = scaled(f, "multiplier/w0")
    h = RT._act(RT.conv_same(f, P["head/conv0/kernel"]), spec.head_activation)
    p = torch.tanh(2.0 * RT.conv_same(h, P["head/conv1/kernel"])) * 0.51
    return (torch.clamp(p, -0.5, 0.5) + 0.5) * (spec.v_max - spec.v_min) + spec.v_min, new_state


def regularization(spec: ConvnextSpec, P):
    """block_regularizer[j] on block convolution j, kernel_regularizer on the base, the denoiser's on the head, "l2" on the gate Dense
    kernels, L1(0.1) on ChannelwiseMultiplier, L1(1.0) on Multiplier (+ 1.0 for its constant w1), none on the BN / LN gammas;
    keras strings: 0.01"""
    total = torch.zeros((), dtype=DT)
    for name, _, kind in spec.tensors():
        if kind in ("bn_gamma", "ln_gamma"):
            continue
        if kind == "channelwise":
            total = total + 0.1 * P[name].abs().sum()
            continue
        if kind == "multiplier":
            total = total + P[name].abs().sum() + 1.0
            continue
        if name.startswith("base/"):
            rk = spec.kernel_regularizer
        elif name.startswith("head/"):
            rk = spec.head_regularizer
        elif "/gate/" in name:
            rk = "l2"
        else:
            rk = spec.block_regularizer[int(name.split("/")[1][4:])]
        if rk in (None, "none"):
            continue
        total = total + 0.01 * (P[name].abs().sum() if rk == "l1" else (P[name] ** 2).sum())
    return total


def train_step(spec: ConvnextSpec, ls: O.LossSpec, params, state, gt, noisy, drop_scale=None):
    """(total, regularisation, denoiser loss dict, prediction, flat gradient, new flat state)"""
    flat = torch.tensor(np.asarray(params, np.float64), dtype=DT, requires_grad=True)
    P = _views(spec.tensors(), flat)
    S = _views(spec.state_tensors(), torch.tensor(np.asarray(state, np.float64), dtype=DT))
    ds = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in (drop_scale or {}).items()}
    pred, new_state = hydra(spec, P, S, torch.from_numpy(np.asarray(noisy, np.float64)), True, ds)
    dl = UT.denoiser_loss(ls, torch.from_numpy(np.asarray(gt, np.float64)), pred)
    reg = regularization(spec, P)
    total = dl["total_loss"] + reg * ls.regularization
    total.backward()
    st = np.concatenate([new_state[n].numpy().ravel() for n, _ in spec.state_tensors()]) if spec.state_tensors() else np.zeros(0)
    return (float(total.detach()), float(reg.detach()), {k: float(v.detach()) for k, v in dl.items()}, pred.detach().numpy(),
            flat.grad.numpy().copy(), st)


def infer(spec: ConvnextSpec, params, state, x, dtype=DT) -> np.ndarray:
    """the inference forward; dtype torch.float32 runs the same arithmetic in single precision"""
    npd = np.float64 if dtype == torch.float64 else np.float32
    P = _views(spec.tensors(), torch.tensor(np.asarray(params, npd), dtype=dtype))
    S = _views(spec.state_tensors(), torch.tensor(np.asarray(state, npd), dtype=dtype))
    with torch.no_grad():
        return hydra(spec, P, S, torch.from_numpy(np.asarray(x, npd)), False)[0].numpy().astype(np.float64)


def denoiser_module_call(spec: ConvnextSpec, params, state, image_u8: np.ndarray, dtype=DT) -> np.ndarray:
    """DenoiserModule.__call__: pad to powers of two, hydra, crop, round half to even, uint8"""
    xp, ph, pw = O.pad_to_power_of_2(image_u8.astype(np.float64))
    y = O.remove_padding(infer(spec, params, state, xp, dtype), ph, pw)
    return np.clip(O.round_half_even(y), 0, 255).astype(np.uint8)


def config(**bb) -> Dict:
    """model section of a convnext pipeline JSON (3 colour channels in and out): the default block at 32 filters"""
    backbone = dict(type="convnext", value_range=[0, 255], input_shape=[None, None, 3], no_layers=2, kernel_size=3, filters=32,
                    block_kernels=[7, 1, 1], block_filters=[32, 128, 32], kernel_regularizer="l1", kernel_initializer="glorot_normal")
    backbone.update(bb)
    return {"backbone": backbone, "denoiser": {"filters": 32, "output_channels": 3, "kernel_regularizer": "l2",
                                               "kernel_initializer": "glorot_normal"}}


# the configurations of the GPU inference test and of the CPU check of its +-1 LSB cap: (backbone keys, (B, H, W))
INFER = [
    (dict(), (2, 64, 64)),
    (dict(filters=64, block_filters=[64, 256, 64], add_gates=True, add_learnable_multiplier=True, add_concat_input=True,
          dropout_rate=0.1), (1, 50, 70)),
    (dict(block_kernels=[5, 1, 1], block_activation=["relu", "gelu", "linear"], add_initial_bn=False, add_final_bn=True,
          add_channelwise_scaling=True, base_activation="relu"), (2, 32, 48)),
    (dict(block_kernels=[3, 1, 1], block_filters=[32, 64, 32]), (1, 40, 24)),
    (dict(block_kernels=[1, 1, 1], no_layers=0), (2, 32, 32)),
]
INFER_SEEDS = dict(params=11, image=3)
