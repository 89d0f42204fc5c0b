"""GPU tests of the plain U-Net backbone (`"type": "unet"`): the fused decoder-entry kernel bf_op_upcat_conv2d against the operators
it replaces (bitwise) and fp64; inference through DenoiserModule against the fp64 torch oracle (tests/unet_backbone_torch.py); the
training step against torch autograd; one Adam step through train_loop; a save / load round trip.
Bars as tests/test_resnet_generic.py (inference) and tests/test_gpu_resnet_generic_train.py (training)."""
import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import _native as N
from blind_image_denoising_amd import unet_laplacian as UL
from blind_image_denoising_amd.unet_backbone import upcat_conv2d, upsample_concat
from oracle import bfcnn_oracle as O
import unet_backbone_torch as UB

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("C", [32, 64, 128])
@pytest.mark.parametrize("k", [1, 3, 5])
def test_upcat_conv2d_is_bitwise_the_composed_operators(C, k):
    r = np.random.default_rng(C * 10 + k)
    B, H, W = 2, 6, 10                                                     # W / 2 = 5: odd
    up = torch.from_numpy(r.normal(size=(B, H // 2, W // 2, C)).astype(np.float32)).cuda()
    skip = torch.from_numpy(r.normal(size=(B, H, W, C)).astype(np.float32)).cuda()
    w = r.normal(size=(k, k, 2 * C, C)) / np.sqrt(k * k * 2 * C)
    wp = UL.pack_conv(torch.from_numpy(w.astype(np.float32)).cuda())
    res = torch.from_numpy(r.normal(size=(B, H, W, C)).astype(np.float32)).cuda()
    bias = torch.from_numpy(r.normal(size=C).astype(np.float32)).cuda()
    cat = upsample_concat(up, skip)
    ref64 = UB.RT.conv_same(torch.from_numpy(cat.cpu().numpy().astype(np.float64)), torch.from_numpy(w.astype(np.float32).astype(np.float64)))
    for rr, bb, act in ((None, None, "linear"), (res, None, "linear"), (None, bias, "relu"), (res, bias, "leaky_relu")):
        got = upcat_conv2d(up, skip, wp, C, k, act, res=rr, bias=bb)
        want = UL.conv2d(cat, wp, C, k, 1, act, res=rr, bias=bb)
        torch.cuda.synchronize()
        assert torch.equal(got, want), (C, k, rr is None, bb is None, act)
        if rr is None and bb is None:
            # fp32 accumulation over K = k*k*2C products: the rounding error grows like sqrt(K), so 1e-6 of the tensor max at
            # K = 256 and proportionally more above (measured: 1.5e-6 at K = 2304)
            d = np.abs(got.cpu().numpy() - ref64.numpy()).max()
            assert d <= 1e-6 * max(1.0, np.sqrt(k * k * 2 * C / 256.0)) * np.abs(ref64.numpy()).max(), d


def test_upcat_conv2d_refuses_what_it_does_not_build():
    L = N.lib()
    t = torch.zeros(4096, device="cuda")
    call = lambda cu, cs, co, k, H=4, W=4: L.bf_op_upcat_conv2d(N.ptr(t), N.ptr(t), N.ptr(t), N.ptr(t), None, None, 1, H, W, cu, cs, co, k,
                                                                0, 0.0, N.stream_ptr(t))
    assert call(32, 64, 32, 3) == N.BF_EUNSUPPORTED and call(32, 32, 32, 7) == N.BF_EUNSUPPORTED
    assert call(16, 16, 16, 3) == N.BF_EUNSUPPORTED and call(32, 32, 32, 3, H=5) == N.BF_EINVAL
    torch.cuda.synchronize()


INFER = [
    (dict(), (2, 64, 64)),
    (dict(no_levels=3, add_gates=True, add_learnable_multiplier=True, add_concat_input=True, dropout_rate=0.1), (1, 50, 70)),
    (dict(no_levels=3, no_layers=2, filters=64, block_kernels=[1, 3, 1], block_filters=[64, 128, 64], add_initial_bn=True,
          add_final_bn=True, add_channelwise_scaling=True, add_clip=True), (2, 32, 48)),
    (dict(no_levels=1, block_kernels=[5], block_filters=[32], activation="linear", base_activation="relu"), (1, 40, 24)),
    (dict(no_levels=4, no_layers=0, filters=64, block_kernels=[3], block_filters=[64], kernel_size=5), (2, 32, 32)),
    (dict(use_bn=False, activation="leaky_relu_01", add_learnable_multiplier=True, add_clip=True, add_concat_input=True,
          add_channelwise_scaling=True), (1, 50, 70)),
]


@pytest.mark.parametrize("bb,shape", INFER)
def test_inference_matches_the_oracle(bb, shape):
    cfg = UB.config(**bb)
    spec = UB.UnetSpec(cfg)
    params, state = UB.init_params(spec, seed=11)
    m = bf.model_builder(cfg, device="cuda").hydra
    m.set_weights(params, state)
    _, noisy = O.synthetic_batch(*shape, seed=3)
    mult = 1 << (spec.no_levels - 1)
    if shape[1] % mult == 0 and shape[2] % mult == 0:                     # hydra(x) directly on the float image
        x = noisy.astype(np.float32)
        got, ref = np.asarray(m(x), np.float64), UB.infer(spec, params, state, x)
        assert got.shape == ref.shape and np.isfinite(got).all()
        assert np.abs(got - ref).mean() / 255.0 <= 1e-4 and np.abs(got - ref).max() <= 0.05
    u8, want = bf.DenoiserModule(m)(noisy), UB.denoiser_module_call(spec, params, state, noisy)
    d = np.abs(u8.astype(np.int32) - want.astype(np.int32))
    assert u8.shape == noisy.shape[:3] + (3,) and u8.dtype == np.uint8 and d.max() <= 1 and (d > 0).mean() < 0.01
    # float output of the padded path (infer_u8 without the cast) against the oracle's, at the bar of the float parity
    flt = m.infer_u8(torch.from_numpy(noisy).cuda(), cast_to_uint8=False).cpu().numpy().astype(np.float64)
    xp, ph, pw = O.pad_to_power_of_2(noisy.astype(np.float64))
    ref_f = O.remove_padding(UB.infer(spec, params, state, xp), ph, pw)
    assert np.abs(flt - ref_f).mean() / 255.0 <= 1e-4


@pytest.mark.parametrize("bb", [dict(), dict(no_levels=3, no_layers=2, filters=64, block_filters=[64, 64], block_kernels=[5, 5]),
                                dict(no_levels=3, filters=64, block_filters=[64, 64], block_kernels=[1, 1])])
def test_fused_and_unfused_decoder_entries_are_identical(bb):
    cfg = UB.config(**bb)
    spec = UB.UnetSpec(cfg)
    params, state = UB.init_params(spec, seed=2)
    m = bf.model_builder(cfg, device="cuda").hydra
    m.set_weights(params, state)
    _, noisy = O.synthetic_batch(2, 64, 48, seed=9)
    x = torch.from_numpy(noisy.astype(np.float32)).cuda()
    a = m(x)
    m.set_option("fuse_upcat", 0)
    b = m(x)
    m.set_option("fuse_upcat", 1)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


TRAIN = [
    dict(),
    dict(no_levels=3, add_gates=True, dropout_rate=0.3, add_learnable_multiplier=True, add_concat_input=True),
    dict(no_levels=2, no_layers=1, filters=64, block_kernels=[1, 3, 1], block_filters=[64, 128, 64], add_initial_bn=True,
         add_final_bn=True, add_channelwise_scaling=True, add_clip=True, activation="leaky_relu"),
    dict(no_levels=3, no_layers=0, block_kernels=[5], block_filters=[32], base_activation="relu", kernel_regularizer="l2"),
]


def _train_parity(bb, shape=(2, 32, 32), seed=5):
    cfg = UB.config(**bb)
    spec = UB.UnetSpec(cfg)
    params, state = UB.init_params(spec, seed=seed)
    m = bf.model_builder(cfg, device="cuda").hydra
    m.set_weights(params, state)
    clean, noisy = O.synthetic_batch(*shape, seed=seed)
    gt, x = clean.astype(np.float32), noisy.astype(np.float32)
    loss_cfg = {"hinge": 0.0, "cutoff": 255.0, "mae_multiplier": 1.0, "mse_multiplier": 0.5, "regularization": 0.01}
    fns = bf.build_train_functions(m, bf.loss_function_builder(loss_cfg))
    r = np.random.default_rng(seed)
    ds = None
    if spec.dropout_rate > 0:
        ds = {key: (r.uniform(size=shape[0]) >= spec.dropout_rate).astype(np.float32) / np.float32(1 - spec.dropout_rate)
              for key in m.dropout_blocks()}
        ds[next(iter(ds))][:] = 0.0                                       # one block off for sure, the rest as drawn
        ds[list(ds)[-1]][:] = 1.0 / np.float32(1 - spec.dropout_rate)
        fns.train_step_single_gpu.drop_scale = {k: torch.from_numpy(v).cuda() for k, v in ds.items()}
    total, model_loss, [dl], pred, grads = fns.train_step_single_gpu(torch.from_numpy(gt), torch.from_numpy(x))
    r_total, r_reg, r_dl, r_pred, r_grads, r_state = UB.train_step(spec, O.LossSpec.from_config(loss_cfg), params, state,
                                                                   gt.astype(np.float64), x.astype(np.float64), ds)
    torch.cuda.synchronize()
    assert abs(total.item() - r_total) <= 1e-5 * abs(r_total), (total.item(), r_total)
    assert abs(model_loss["regularization_loss"].item() - r_reg) <= 1e-5 * abs(r_reg)
    assert abs(dl["total_loss"].item() - r_dl["total_loss"]) <= 1e-5 * abs(r_dl["total_loss"])
    assert np.abs(pred.cpu().numpy() - r_pred).max() <= 1e-2                # on the 0..255 scale
    g = grads.cpu().numpy()
    for name, shp, kind, off in m.trainable_variables:
        n = int(np.prod(shp))
        a, b = g[off:off + n], r_grads[off:off + n]
        assert np.abs(a - b).max() <= 5e-4 * max(np.abs(b).max(), 1e-12), (name, np.abs(a - b).max(), np.abs(b).max())
    st = m.get_weights()[1]
    assert np.abs(st - r_state).max() <= 1e-5 * max(1.0, np.abs(r_state).max()) if st.size else True
    return m, fns, loss_cfg, (gt, x)


@pytest.mark.parametrize("bb", TRAIN)
def test_training_step_matches_autograd(bb):
    _train_parity(bb)


def test_one_adam_step_through_train_loop():
    m, fns, loss_cfg, (gt, x) = _train_parity(dict(add_learnable_multiplier=True))
    before = m.get_weights()[0].copy()
    opt, _ = bf.optimizer_builder({"type": "Adam", "schedule": {"type": "exponential_decay", "config": {"decay_rate": 0.9,
                                   "decay_steps": 100, "learning_rate": 1e-3}}})
    total, _, _, _, grads = fns.train_step_single_gpu(torch.from_numpy(gt), torch.from_numpy(x))
    fns.apply_grads(opt, grads, None)
    torch.cuda.synchronize()
    after = m.get_weights()[0]
    assert np.isfinite(after).all() and np.abs(after - before).max() > 0
    # the step moved every tensor with a gradient by at most the learning rate (Adam's first step: |update| <= lr)
    assert np.abs(after - before).max() <= 1e-3 * 1.01
    total2, _, _, _, _ = fns.train_step_single_gpu(torch.from_numpy(gt), torch.from_numpy(x))
    torch.cuda.synchronize()
    assert np.isfinite(total2.item())
    m.set_option("fuse_upcat", 1)
    _, noisy = O.synthetic_batch(1, 32, 32, seed=1)
    assert bf.DenoiserModule(m)(noisy).dtype == np.uint8                  # the folded weights follow the step


def test_save_and_load_round_trip(tmp_path):
    cfg = UB.config(no_levels=3, add_gates=True, add_final_bn=True, add_concat_input=True)
    spec = UB.UnetSpec(cfg)
    params, state = UB.init_params(spec, seed=4)
    m = bf.model_builder(cfg, device="cuda").hydra
    m.set_weights(params, state)
    _, noisy = O.synthetic_batch(2, 50, 70, seed=6)
    a = bf.DenoiserModule(m)(noisy)
    bf.save_model(m, str(tmp_path / "unet"))
    b = bf.load_model(str(tmp_path / "unet"))(noisy)
    assert np.array_equal(a, b)
