"""
Training of the ConvNeXt backbone (`ConvnextHydra`, bfcnn/backbone_convnext.py:103-375): bfcnn/train_loop.py:259-312 -- training-mode
forward (the initial / final BatchNormalization on batch statistics, moving statistics updated), denoiser loss, the builder's
regularisers and the gradient of the total for every trainable tensor -- as the forward / backward walk of GenericResnetTrainGraph
with the ConvNeXt block in place of the resnet one.  BatchNorm, multipliers, gate, RandomOnOff, closing layers and the regulariser
rules are that graph's; the depthwise and 1x1 convolutions, the base and the head are the shared steps of train_graph.TrainGraph.
What the block adds is the LayerNormalization behind its first convolution: forward bf_op_dwconv_ln with k = 0, backward
Ops.layernorm_bwd (bf_op_layernorm_bwd).  The depthwise kernel gradient is bf_op_dwconv_wgrad (k up to 7).

Regularisers: block_regularizer[j] / kernel_regularizer on the kernels, l2 on the gate's Dense kernels, the multipliers' own L1,
none on the BatchNorm and LayerNorm gammas.  Exact fp32; PyTorch holds the tensors and computes nothing.  Gradients are compared
with the torch-autograd oracle (tests/convnext_torch.py) in tests/test_gpu_convnext_backbone.py.
"""
import torch

from . import unet_laplacian as UL
from .resnet_generic_train import GenericResnetTrainGraph
from .train_graph import push


class ConvnextTrainGraph(GenericResnetTrainGraph):
    """train_step_single_gpu for a ConvnextHydra: `step(gt, noisy, grads)` as GenericResnetTrainGraph.step"""

    def regularizer(self, name: str, kind: str):
        if kind == "ln_gamma":
            return None
        return super().regularizer(name, kind)

    def ln_step(self, name: str, x: torch.Tensor):
        """LayerNormalization(center=False, scale=True) over the channels: (y, backward dy -> dx; the gamma gradient is written)"""
        gamma = self.W(name)
        y = UL.dwconv_ln(x, None, gamma)
        return y, lambda dy: self.ops.layernorm_bwd(x, gamma, dy, self.G(name))

    def block(self, i: int, f: torch.Tensor, ds_):
        """ConvNeXt block i and the skip Add behind it (backbone_blocks.py:174-242 with ln_after_first_conv_params); ds_: the block's
        RandomOnOff factor or None"""
        m, ops = self.m, self.ops
        b = f"block{i}"
        a0, a1, a2 = m.block_activation
        steps = []
        t = push(steps, self.depthwise_step(f"{b}/conv0/kernel", f, m.block_kernels[0]))
        t = push(steps, self.act_step(t, a0))
        t = push(steps, self.ln_step(f"{b}/ln/gamma", t))
        t = push(steps, self.conv1x1_step(f"{b}/conv1/kernel", t, m.expansion, a1))
        if m.add_gates:
            t = push(steps, self.gate_step(b, t))
        t = push(steps, self.conv1x1_step(f"{b}/conv2/kernel", t, m.filters, a2))
        # ChannelwiseMultiplier, Multiplier, RandomOnOff in front of the Add (:215-225)
        tails = ([f"{b}/channelwise/w0"] if m.add_channelwise else []) + ([f"{b}/multiplier/w0"] if m.add_multiplier else [])
        if ds_ is not None and not tails:
            tails = [None]
        for q_, name_ in enumerate(tails):
            t = push(steps, self.mult_step(name_, t, ds_ if q_ == len(tails) - 1 else None))
        out = ops.add(f, t)

        def bwd(dout):
            g = dout
            for b_ in reversed(steps):
                g = b_(g)
            return ops.add(dout, g)
        return out, bwd
