"""fp64 torch oracle of the plain U-Net backbone (`"type": "unet"`; bfcnn/backbone_unet.py:18-268, unet_blocks and
resnet_blocks_full of bfcnn/backbone_blocks.py:319-403 / 163-246) for the tests: its own spec and parameter inventory (read from
the reference builder, not from blind_image_denoising_amd.unet_backbone), the inference and training forward with torch ops, and
autograd for the gradients.  Test infrastructure only.

Keras creation order of the variables: base conv, [initial BN], per encoder level [entry conv (level > 0)] + blocks, per decoder
level from the deepest up entry conv + blocks, [final BN], [ChannelwiseMultiplier], [Multiplier], head conv0, head conv1; inside a
block conv0, conv1, [bn1], [gate dense0, dense1], conv2, [bn2], [Multiplier].
"""
from typing import Dict, List, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import bfcnn_oracle as O
from oracle import resnet_generic_torch as RT
from oracle import unet_torch as UT

DT = torch.float64
BN_EPS = 1e-3


class UnetSpec:
    def __init__(self, model_config: Dict):
        bb, dn = model_config["backbone"], model_config["denoiser"]
        self.no_levels, self.no_layers = int(bb["no_levels"]), int(bb["no_layers"])
        self.kernel_size, self.filters = int(bb.get("kernel_size", 3)), int(bb.get("filters", 32))
        self.block_kernels = [int(k) for k in bb.get("block_kernels", [3, 3])]
        self.block_filters = [int(f) for f in bb.get("block_filters", [32, 32])]
        nb = len(self.block_kernels)
        act, base = bb.get("activation", "relu"), bb.get("base_activation", "linear")
        self.conv_acts = [act] * (nb - 1) + [base]             # convs_params[-1] takes base_activation (backbone_unet.py:127)
        self.base_activation = base
        self.use_bn = bool(bb.get("use_bn", True))
        self.add_gates = bool(bb.get("add_gates", False))
        self.dropout_rate = float(bb.get("dropout_rate", -1))
        self.multiplier = bool(bb.get("add_learnable_multiplier", False))
        self.channelwise = bool(bb.get("add_channelwise_scaling", False))
        self.initial_bn, self.final_bn = bool(bb.get("add_initial_bn", False)), bool(bb.get("add_final_bn", False))
        self.concat_input, self.clip = bool(bb.get("add_concat_input", False)), bool(bb.get("add_clip", False))
        self.kernel_regularizer = bb.get("kernel_regularizer", "l1")
        self.head_regularizer = dn.get("kernel_regularizer", "l2")
        self.in_channels = int(bb["input_shape"][-1])
        vr = bb.get("value_range", [0, 255])
        self.v_min, self.v_max = float(vr[0]), float(vr[1])
        self.head_filters, self.head_activation = int(dn.get("filters", 32)), dn.get("activation", "linear")
        self.out_channels = int(dn.get("output_channels", 3))

    def groups(self) -> List[str]:
        """the block groups in graph order"""
        return [f"enc{l}" for l in range(self.no_levels)] + [f"dec{l}" for l in reversed(range(self.no_levels))]

    def _blocks(self, prefix, cin, out, state):
        for i in range(self.no_layers):
            c = cin
            for j, (k, f) in enumerate(zip(self.block_kernels, self.block_filters)):
                out.append((f"{prefix}/block{i}/conv{j}/kernel", (k, k, c, f), "conv"))
                if j >= 1 and self.use_bn:
                    out.append((f"{prefix}/block{i}/bn{j}/gamma", (f,), "bn_gamma"))
                    state += [(f"{prefix}/block{i}/bn{j}/moving_mean", (f,)), (f"{prefix}/block{i}/bn{j}/moving_variance", (f,))]
                if j == 1 and self.add_gates:
                    out.append((f"{prefix}/block{i}/gate/dense0/kernel", (f, max(f // 8, 2)), "dense"))
                    out.append((f"{prefix}/block{i}/gate/dense1/kernel", (max(f // 8, 2), f), "dense"))
                c = f
            if self.multiplier:
                out.append((f"{prefix}/block{i}/multiplier/w0", (1,), "multiplier"))

    def _inventory(self):
        C, k0, f0 = self.filters, self.block_kernels[0], self.block_filters[0]
        out, state = [("base/kernel", (self.kernel_size, self.kernel_size, self.in_channels, C), "conv")], []
        if self.initial_bn:
            out.append(("initial_bn/gamma", (C,), "bn_gamma"))
            state += [("initial_bn/moving_mean", (C,)), ("initial_bn/moving_variance", (C,))]
        skips, c = [], C
        for l in range(self.no_levels):
            if l > 0:
                out.append((f"enc{l}/entry/kernel", (k0, k0, c, f0), "conv"))
                c = f0
            self._blocks(f"enc{l}", c, out, state)
            skips.append(c)
        x = None
        for l in reversed(range(self.no_levels)):
            out.append((f"dec{l}/entry/kernel", (k0, k0, skips[l] + (x or 0), f0), "conv"))
            x = f0
            self._blocks(f"dec{l}", x, out, state)
        if self.final_bn:
            out.append(("final_bn/gamma", (x,), "bn_gamma"))
            state += [("final_bn/moving_mean", (x,)), ("final_bn/moving_variance", (x,))]
        cf = x + (self.in_channels if self.concat_input else 0)
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


def init_params(spec: UnetSpec, seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """random weights away from the creation values (so every BN, multiplier and gate is exercised), glorot-scaled kernels"""
    r = np.random.default_rng(seed)
    out = []
    for name, shape, kind in spec.tensors():
        if kind == "bn_gamma":
            v = r.uniform(0.6, 1.4, shape)
        elif kind in ("channelwise", "multiplier"):
            v = r.uniform(-0.3, 0.3, shape)
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


def _blocks(spec: UnetSpec, prefix, x, P, S, new_state, training, drop_scale):
    scaled = lambda t, name: t * torch.relu(P[name] + 1.0)
    for i in range(spec.no_layers):
        t = x
        for j, a in enumerate(spec.conv_acts):
            t = RT.conv_same(t, P[f"{prefix}/block{i}/conv{j}/kernel"])
            if j >= 1 and spec.use_bn:
                t = RT._batch_norm(t, f"{prefix}/block{i}/bn{j}", P, S, new_state, training)
            t = RT._act(t, a)
            if j == 1 and spec.add_gates:
                y = torch.relu(t.mean(dim=(1, 2)) @ P[f"{prefix}/block{i}/gate/dense0/kernel"])
                y = torch.clamp(0.2 * (y @ P[f"{prefix}/block{i}/gate/dense1/kernel"]) + 0.5, 0.0, 1.0)
                t = t * y[:, None, None, :]
        if spec.multiplier:
            t = scaled(t, f"{prefix}/block{i}/multiplier/w0")
        if training and (prefix, i) in drop_scale:
            t = t * drop_scale[(prefix, i)].reshape(-1, 1, 1, 1)
        x = t + x
    return x


def maxpool2(x):
    return RT._nhwc(F.max_pool2d(RT._nchw(x), 2, 2))


def upsample2(x):
    return RT._nhwc(F.interpolate(RT._nchw(x), scale_factor=2, mode="nearest"))


def hydra(spec: UnetSpec, P, S, x, training: bool, drop_scale=None):
    """returns (prediction, new state).  drop_scale: {(group, block): [B] factor} = RandomOnOff's draw, training only"""
    new_state = dict(S)
    drop_scale = drop_scale or {}
    xn = (torch.clamp(x, spec.v_min, spec.v_max) - spec.v_min) / (spec.v_max - spec.v_min) - 0.5
    f = RT._act(RT.conv_same(xn, P["base/kernel"]), spec.base_activation)
    if spec.initial_bn:
        f = RT._batch_norm(f, "initial_bn", P, S, new_state, training)
    ea = spec.conv_acts[0]
    skips = []
    for l in range(spec.no_levels):
        if l > 0:
            f = RT._act(RT.conv_same(maxpool2(f), P[f"enc{l}/entry/kernel"]), ea)
        f = _blocks(spec, f"enc{l}", f, P, S, new_state, training, drop_scale)
        skips.append(f)
    f = None
    for l in reversed(range(spec.no_levels)):
        f = skips[l] if f is None else torch.cat([upsample2(f), skips[l]], dim=-1)       # the upsampled tensor first
        f = RT._act(RT.conv_same(f, P[f"dec{l}/entry/kernel"]), ea)
        f = _blocks(spec, f"dec{l}", f, P, S, new_state, training, drop_scale)
    if spec.final_bn:
        f = RT._batch_norm(f, "final_bn", P, S, new_state, training)
    if spec.concat_input:
        f = torch.cat([f, xn], dim=-1)
    if spec.channelwise:
        f = f * torch.relu(P["channelwise/w0"] + 1.0)
    if spec.multiplier:
        f = f * torch.relu(P["multiplier/w0"] + 1.0)
    if spec.clip:
        f = torch.tanh(f)
    h = RT._act(RT.conv_same(f, P["head/conv0/kernel"]), spec.head_activation)
    p = torch.tanh(2.0 * RT.conv_same(h, P["head/conv1/kernel"])) * 0.51
    return (torch.clamp(p, -0.5, 0.5) + 0.5) * (spec.v_max - spec.v_min) + spec.v_min, new_state


def regularization(spec: UnetSpec, P):
    """the builder's regularisers: kernel_regularizer on every backbone convolution, "l2" on the gate Dense kernels, the denoiser's
    on the head, L1(0.1) on ChannelwiseMultiplier, L1(1.0) on Multiplier (+ 1.0 for its constant w1); keras strings: 0.01"""
    total = torch.zeros((), dtype=DT)
    coef = {"l1": (0.01, 1), "l2": (0.01, 2)}
    for name, _, kind in spec.tensors():
        if kind == "bn_gamma":
            continue
        if kind == "channelwise":
            total = total + 0.1 * P[name].abs().sum()
            continue
        if kind == "multiplier":
            total = total + P[name].abs().sum() + 1.0
            continue
        rk = "l2" if "/gate/" in name else (spec.head_regularizer if name.startswith("head/") else spec.kernel_regularizer)
        if rk in (None, "none"):
            continue
        c, pw = coef[rk]
        total = total + c * (P[name].abs().sum() if pw == 1 else (P[name] ** 2).sum())
    return total


def train_step(spec: UnetSpec, ls: O.LossSpec, params, state, gt, noisy, drop_scale=None):
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


def infer(spec: UnetSpec, params, state, x) -> np.ndarray:
    P = _views(spec.tensors(), torch.tensor(np.asarray(params, np.float64), dtype=DT))
    S = _views(spec.state_tensors(), torch.tensor(np.asarray(state, np.float64), dtype=DT))
    with torch.no_grad():
        return hydra(spec, P, S, torch.from_numpy(np.asarray(x, np.float64)), False)[0].numpy()


def denoiser_module_call(spec: UnetSpec, params, state, image_u8: np.ndarray) -> np.ndarray:
    """DenoiserModule.__call__: pad to powers of two, hydra, crop, round half to even, uint8"""
    xp, ph, pw = O.pad_to_power_of_2(image_u8.astype(np.float64))
    y = O.remove_padding(infer(spec, params, state, xp), ph, pw)
    return np.clip(O.round_half_even(y), 0, 255).astype(np.uint8)


def config(**bb) -> Dict:
    """model section of a unet pipeline JSON (3 colour channels in and out)"""
    backbone = dict(type="unet", value_range=[0, 255], input_shape=[None, None, 3], no_levels=2, no_layers=1, kernel_size=3,
                    filters=32, block_kernels=[3, 3], block_filters=[32, 32], activation="relu", base_activation="linear",
                    use_bn=True, kernel_regularizer="l1", kernel_initializer="glorot_normal")
    backbone.update(bb)
    return {"backbone": backbone, "denoiser": {"filters": 32, "output_channels": 3, "kernel_regularizer": "l2",
                                               "kernel_initializer": "glorot_normal"}}
