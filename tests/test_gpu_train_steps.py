"""The steps the three training graphs share (blind_image_denoising_amd/train_graph.py: conv_step, conv1x1_step, depthwise_step,
base_step, head_step), each called on its own against torch autograd on the CPU in float64.  The graph object is a
GenericResnetTrainGraph on a small model whose inventory holds kernels of the wanted shapes; a step reads its kernel by name and
takes any input of matching width.  Bars as the primitive tests': forwards 2e-5 of the reference's largest entry (`_close` in
test_gpu_unet_train.py), backward results 5e-5 (test_gpu_resnet_generic_train.py)."""
import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import _native as N
from oracle import bfcnn_oracle as O
from oracle import resnet_generic_oracle as R
from oracle import unet_torch as T

pytestmark = pytest.mark.gpu

LOSS = {"hinge": 0.0, "cutoff": 255.0, "mae_multiplier": 1.0, "mse_multiplier": 0.5, "ssim_multiplier": 1.0, "regularization": 0.01}
# small models (a block holds at most three convolutions) whose inventories hold the kernels the cases need
BACKBONES = {
    "conv128": dict(filters=32, kernel_size=3, no_layers=1, block_kernels=[1, 1], block_filters=[128, 32], block_depthwise=[-1, -1],
                    block_groups=[1, 1], block_activation=["relu", "relu"], block_regularizer=["l1", "l1"]),    # conv0: 1x1 32 -> 128
    # block0: depthwise 5x5 and 3x3 on 32 channels; base 5x5; the head reads 35 = 32 + 3 channels, padded to 64
    "depthwise": dict(filters=32, kernel_size=5, base_activation="relu", no_layers=1, block_kernels=[5, 3, 1], block_filters=[32, 32, 32],
                      block_depthwise=[1, 1, -1], block_groups=[1, 1, 1], block_activation=["relu", "relu", "linear"],
                      block_regularizer=["l1"] * 3, add_concat_input=True),
    "conv32": dict(filters=32, kernel_size=3, no_layers=1, block_kernels=[3, 3], block_filters=[64, 32], block_depthwise=[-1, -1],
                   block_groups=[1, 1], block_activation=["relu", "relu"], block_regularizer=["l1", "l1"]),     # conv0: 3x3 32 -> 64
    "conv64": dict(filters=64, kernel_size=3, no_layers=1, block_kernels=[3, 1], block_filters=[64, 64], block_depthwise=[-1, -1],
                   block_groups=[1, 1], block_activation=["relu", "relu"], block_regularizer=["l1", "l1"]),     # 3x3 and 1x1 64 -> 64
}


def _close(got, ref, rel, what):
    got, ref = np.asarray(got.detach().cpu(), np.float64), np.asarray(ref.detach(), np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, scale = np.abs(got - ref).max(), max(1e-6, np.abs(ref).max())
    print(f"{what}: error {err:.3e}, bar {rel * scale:.3e}")
    assert err <= rel * scale, f"{what}: {err:.3e} vs {scale:.3e}"


@pytest.fixture(scope="module")
def graphs():
    made = {}

    def graph(key):
        if key not in made:
            cfg = R.shipped_config()
            cfg["backbone"].update(BACKBONES[key])
            model = bf.model_builder(cfg, device="cuda").hydra
            g = model.train_graph_class()(model, LOSS)
            g.grad_buffer = torch.zeros(model.n_params, dtype=torch.float32, device="cuda")
            made[key] = g
        g = made[key]
        g._begin(g.grad_buffer, 1 << 22)
        g.ld = g._loss_desc(0.0)
        return g
    return graph


def _set(g, name, rng, scale):
    """a random kernel into the model's parameters: its float64 copy with requires_grad"""
    off, shape, _ = g.off[name]
    w = (rng.standard_normal(shape) * scale).astype(np.float32)
    g.m.params[off:off + w.size].copy_(torch.from_numpy(w.reshape(-1)))
    return torch.tensor(w.astype(np.float64), requires_grad=True)


def _pair(a, requires_grad=True):
    """a float32 array on the GPU and as a float64 torch tensor"""
    a = np.ascontiguousarray(a, np.float32)
    return torch.from_numpy(a).cuda(), torch.tensor(a.astype(np.float64), requires_grad=requires_grad)


def _check(g, name, step, ref, x, w, seed):
    """step / ref: x -> y on the GPU / in float64; forward, data gradient and kernel gradient"""
    xd, xt = _pair(x)
    y, bwd = step(xd)
    yr = ref(xt)
    _close(y, yr, 2e-5, "forward")
    dyd, dyt = _pair(np.random.default_rng(seed).standard_normal(tuple(yr.shape)), False)
    dx = bwd(dyd)
    torch.cuda.synchronize()
    (yr * dyt).sum().backward()
    _close(dx, xt.grad, 5e-5, "data gradient")
    _close(g._grad_view(name).view(w.shape), w.grad, 5e-5, "kernel gradient")


@pytest.mark.parametrize("backbone,shape,act", [("conv32", (2, 9, 7, 32), "relu"), ("conv64", (1, 8, 8, 64), "linear")],
                         ids=["3x3-32-64-relu", "3x3-64-64-linear"])
def test_conv_step(graphs, backbone, shape, act):
    g, rng, name = graphs(backbone), np.random.default_rng(1), "block0/conv0/kernel"
    w = _set(g, name, rng, 0.1)
    assert tuple(w.shape) == (3, 3, shape[-1], 64)
    _check(g, name, lambda x: g.conv_step(name, x, act), lambda x: T._act(T._conv(x, w), act), rng.standard_normal(shape), w, 2)


@pytest.mark.parametrize("backbone,name,cin,cout,act", [("conv128", "block0/conv0/kernel", 32, 128, "relu"),
                                                        ("conv64", "block0/conv1/kernel", 64, 64, "gelu")], ids=["32-128-relu", "64-64-gelu"])
def test_conv1x1_step(graphs, backbone, name, cin, cout, act):
    """gelu: the product is kept and the activation runs as its own pass, its derivative from the kept product"""
    g, rng = graphs(backbone), np.random.default_rng(3)
    w = _set(g, name, rng, 0.2)
    _check(g, name, lambda x: g.conv1x1_step(name, x, cout, act), lambda x: T._act(T._conv(x, w), act),
           rng.standard_normal((1, 7, 11, cin)), w, 4)


@pytest.mark.parametrize("name,k,shape", [("block0/conv0/kernel", 5, (2, 17, 23, 32)), ("block0/conv1/kernel", 3, (1, 6, 5, 32))],
                         ids=["k5", "k3"])
def test_depthwise_step(graphs, name, k, shape):
    g, rng = graphs("depthwise"), np.random.default_rng(5)
    w = _set(g, name, rng, 0.3)
    _check(g, name, lambda x: g.depthwise_step(name, x, k), lambda x: T._depthwise(x, w), rng.standard_normal(shape), w, 6)


def test_base_step(graphs):
    """5 x 5 on the normalised uint8 image, 3 -> 32, relu: the forward and the kernel's gradient (the image carries none)"""
    g, rng = graphs("depthwise"), np.random.default_rng(7)
    w = _set(g, "base/kernel", rng, 0.3)
    img = rng.integers(0, 256, (2, 9, 7, 3)).astype(np.uint8)
    f, bwd = g.base_step(torch.from_numpy(img).cuda(), 5, "relu")
    fr = torch.relu(T._conv(torch.from_numpy(img.astype(np.float64)) / 255.0 - 0.5, w))
    _close(f, fr, 2e-5, "forward")
    dfd, dft = _pair(rng.standard_normal(tuple(fr.shape)), False)
    assert bwd(dfd) is None
    torch.cuda.synchronize()
    (fr * dft).sum().backward()
    _close(g._grad_view("base/kernel").view(w.shape), w.grad, 5e-5, "kernel gradient")


@pytest.mark.parametrize("backbone,width", [("conv128", 32), ("depthwise", 64)], ids=["32-rows", "35-rows-padded-to-64"])
def test_head_step(graphs, backbone, width):
    """head, loss and head backward on 2 x 8 x 8; padded: 35 real rows of head/conv0/kernel in a 64-row kernel, the features
    zero behind channel 35 as Concatenate + padding leaves them; total[0] accumulates over two calls"""
    g, rng = graphs(backbone), np.random.default_rng(8)
    w0, w1 = _set(g, "head/conv0/kernel", rng, 0.2), _set(g, "head/conv1/kernel", rng, 0.2)
    rows = w0.shape[2]
    assert rows == (32 if width == 32 else 35)
    f = rng.standard_normal((2, 8, 8, width))
    f[..., rows:] = 0.0
    clean, _ = O.synthetic_batch(2, 8, 8, seed=9)
    gt = torch.from_numpy(clean.astype(np.float64))
    ls = O.LossSpec.from_config(LOSS)
    total = torch.zeros(3, dtype=torch.float32, device="cuda")
    expected = 0.0
    for depth_weight in (1.0, 0.5):
        g._begin(g.grad_buffer, 1 << 22)                  # a step of its own: no staged gradient of the call before
        fd, ft = _pair(f)
        pred, losses, df = g.head_step("head", fd, torch.from_numpy(clean.astype(np.float32)).cuda(), depth_weight, total)
        torch.cuda.synchronize()
        h = T._conv(T._act(T._conv(ft[..., :rows], w0), g.m.head_activation), w1)
        pr = (torch.clamp(torch.tanh(2.0 * h) * 0.51, -0.5, 0.5) + 0.5) * 255.0
        dl = T.denoiser_loss(ls, gt, pr)["total_loss"]
        w0.grad = w1.grad = None
        (dl * depth_weight).backward()
        expected += float(dl.detach()) * depth_weight
        _close(pred, pr, 2e-5, "prediction")
        _close(losses[N.BF_LOSS_DENOISER_TOTAL], dl, 2e-5, "loss")
        _close(total[0], torch.tensor(expected), 2e-5, f"total[0] after weight {depth_weight}")
        _close(df[..., :rows], ft.grad[..., :rows], 5e-5, "d f")
        _close(g._grad_view("head/conv0/kernel").view(w0.shape), w0.grad, 5e-5, "conv0 kernel gradient")
        _close(g._grad_view("head/conv1/kernel").view(w1.shape), w1.grad, 5e-5, "conv1 kernel gradient")
