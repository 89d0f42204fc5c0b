"""GPU tests of the ConvNeXt backbone (`"type": "convnext"`): the 7 x 7 depthwise + LayerNorm kernel (bf_op_dwconv_ln, k = 7) against
fp64; inference through DenoiserModule against the fp64 torch oracle (tests/convnext_torch.py) on every forward path; the training
step against torch autograd; an Adam step, a checkpoint round trip, the wrappers, and a seeded sweep over the built option space.
Bars as tests/test_gpu_unet.py ("dw+ln"), tests/test_gpu_unet_backbone.py (inference, training)."""
import os

import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import _native as N
from blind_image_denoising_amd import unet_laplacian as UL
from oracle import bfcnn_oracle as O
from oracle import resnet_generic_torch as RT
import convnext_torch as CT
from helpers import host, assert_close
from guarded import dev as dev_raw, dev_f32 as dev, guard_bands

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guard_bands")]

# bf_op_dwconv_ln at k = 7 walks strips of 8 rows, or of 32 rows once 32-row strips give at least 512 workgroups
STRIP_SMALL, STRIP_LARGE = 8, 32


def _dw7_reference(x, w, g, act):
    t = RT.depthwise_mult_same(torch.from_numpy(x), torch.from_numpy(w))
    if g is not None:
        t = CT.layer_norm(t, torch.from_numpy(g))
    return RT._act(t, act).numpy()


@pytest.mark.parametrize("C", [32, 64, 128])
@pytest.mark.parametrize("shape", [(1, 2, 3), (2, 7, 33), (1, 9, 37), (1, STRIP_SMALL + 1, 16), (1, STRIP_SMALL - 1, 16),
                                   (1, STRIP_LARGE + 1, 16), (1, STRIP_LARGE - 1, 16)])
def test_dwconv7_layernorm(C, shape):
    r = np.random.default_rng(C * 10 + 7 + shape[1])
    x = r.normal(size=shape + (C,)) * 2 + 0.5
    w = r.normal(size=(7, 7, C, 1))
    g = r.uniform(0.5, 1.5, C)
    x, w, g = (a.astype(np.float32).astype(np.float64) for a in (x, w, g))
    xd, wd, gd = dev(x), dev(w.reshape(7, 7, C)), dev(g)
    for gamma in (g, None):
        for act in ("linear", "leaky_relu_01"):
            got = UL.dwconv_ln(xd, wd, gd if gamma is not None else None, act)
            again = UL.dwconv_ln(xd, wd, gd if gamma is not None else None, act)
            assert_close(host(got), _dw7_reference(x, w, gamma, act), rel=5e-5, what=f"dw7 ln={gamma is not None} {act}")
            assert torch.equal(got, again), "two runs differ"


def test_dwconv7_layernorm_on_32_row_strips():
    """large enough for the 32-row strips (16 images x 16 column groups x 2 strips = 512 workgroups), H one more than the strip
    height; the same rows through 8-row strips (one image of the batch alone) must give the same bits: the summation order does
    not depend on the strip an output row falls in"""
    C, shape = 32, (16, STRIP_LARGE + 1, 1024)
    r = np.random.default_rng(99)
    x = (r.normal(size=shape + (C,)) * 2 + 0.5).astype(np.float32)
    w = r.normal(size=(7, 7, C, 1)).astype(np.float32)
    g = r.uniform(0.5, 1.5, C).astype(np.float32)
    xd, wd, gd = dev(x), dev(w.reshape(7, 7, C)), dev(g)
    got = UL.dwconv_ln(xd, wd, gd)
    assert torch.equal(got, UL.dwconv_ln(xd, wd, gd))
    assert torch.equal(got[3:4], UL.dwconv_ln(xd[3:4].contiguous(), wd, gd))
    assert_close(host(got[:2]), _dw7_reference(x[:2].astype(np.float64), w.astype(np.float64), g.astype(np.float64), "linear"), rel=5e-5,
                 what="dw7 32-row strips")


def test_dwconv_ln_refuses_what_it_does_not_build():
    L = N.lib()
    t = torch.zeros(1 << 16, device="cuda")
    call = lambda C, k: L.bf_op_dwconv_ln(N.ptr(t), N.ptr(t[32768:]), N.ptr(t), N.ptr(t), 1, 4, 4, C, k, 1e-3, 0, 0.0, N.stream_ptr(t))
    assert call(32, 9) == N.BF_EUNSUPPORTED and call(48, 7) == N.BF_EUNSUPPORTED and call(256, 7) == N.BF_EUNSUPPORTED
    assert call(16, 7) == N.BF_EUNSUPPORTED and call(64, 7) == N.BF_OK
    torch.cuda.synchronize()


# ---- inference --------------------------------------------------------------------------------------------------------------------

def _check_inference(cfg, shape, options=(), seed=CT.INFER_SEEDS["params"], image_seed=CT.INFER_SEEDS["image"]):
    spec = CT.ConvnextSpec(cfg)
    params, state = CT.init_params(spec, seed=seed)
    m = bf.model_builder(cfg, device="cuda").hydra
    m.set_weights(params, state)
    for key, value in options:
        m.set_option(key, value)
    _, noisy = O.synthetic_batch(*shape, seed=image_seed)
    x = noisy.astype(np.float32)
    got, ref = np.asarray(m(x), np.float64), CT.infer(spec, params, state, x)
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert np.abs(got - ref).mean() / 255.0 <= 1e-4 and np.abs(got - ref).max() <= 0.05, (np.abs(got - ref).mean() / 255.0,
                                                                                         np.abs(got - ref).max())
    u8, want = bf.DenoiserModule(m)(noisy), CT.denoiser_module_call(spec, params, state, noisy)
    d = np.abs(u8.astype(np.int32) - want.astype(np.int32))
    assert u8.shape == noisy.shape[:3] + (3,) and u8.dtype == np.uint8 and d.max() <= 1 and (d > 0).mean() < 0.01, (d.max(), (d > 0).mean())
    return m


@pytest.mark.parametrize("bb,shape", CT.INFER)
def test_inference_matches_the_oracle(bb, shape):
    _check_inference(CT.config(**bb), shape)


@pytest.mark.parametrize("bb,shape,options", [
    (CT.INFER[0][0], CT.INFER[0][1], (("arith", 1),)),                                    # k = 7: the split-f16 MLP behind dw + LN
    (CT.INFER[2][0], CT.INFER[2][1], (("arith", 1),)),                                    # conv2 relu: no MLP kernel, the fp32 operators
    (dict(block_kernels=[5, 1, 1]), (2, 32, 48), (("arith", 1), ("fuse_block", 1))),      # the whole block in one kernel
    (dict(block_kernels=[5, 1, 1]), (2, 32, 48), (("arith", 1), ("fuse_block", 0))),
    (dict(block_kernels=[3, 1, 1], add_learnable_multiplier=True, add_channelwise_scaling=True), (1, 40, 24), (("arith", 1), ("fuse_block", 1))),
    (dict(block_kernels=[3, 1, 1], add_learnable_multiplier=True, add_channelwise_scaling=True), (1, 40, 24), (("arith", 1), ("fuse_block", 0))),
    (dict(filters=64, block_filters=[64, 256, 64]), (1, 40, 24), (("arith", 1),)),
    # closing multipliers behind a GELU conv2: their own pass; a 1 x 1 "depthwise" with an activation in front of the LayerNorm
    (dict(block_kernels=[1, 1, 1], block_activation=["leaky_relu", "relu", "linear"], base_activation="gelu", add_learnable_multiplier=True,
          add_channelwise_scaling=True, add_gates=True), (1, 24, 40), ()),
])
def test_inference_on_the_other_forward_paths(bb, shape, options):
    _check_inference(CT.config(**bb), shape, options)


def _random_convnext_config(rng):
    C = int(rng.choice([32, 64]))
    bb = dict(filters=C, no_layers=int(rng.integers(0, 4)), kernel_size=int(rng.choice([1, 3, 5, 7])),
              block_kernels=[int(rng.choice([1, 3, 5, 7])), 1, 1], block_filters=[C, int(rng.choice([32, 64, 128, 256])), C])
    acts = ["linear", "relu", "gelu", "leaky_relu", "leaky_relu_01"]
    bb["block_activation"] = [str(rng.choice(acts)) for _ in range(3)]
    bb["base_activation"] = str(rng.choice(acts))
    for key in ("add_gates", "add_final_bn", "add_concat_input", "add_channelwise_scaling", "add_learnable_multiplier", "use_bn"):
        bb[key] = bool(rng.integers(0, 2))
    bb["add_initial_bn"] = bool(rng.integers(0, 4))                                       # True three times in four: the default
    if rng.integers(0, 2):
        bb["dropout_rate"] = 0.2
    return bb


@pytest.mark.parametrize("draw", range(int(os.environ.get("BF_SWEEP_N", 12))))
def test_random_convnext_configs(draw):
    rng = np.random.default_rng(7000 + draw)
    bb = _random_convnext_config(rng)
    shape = (int(rng.integers(1, 3)), int(rng.integers(8, 49)), int(rng.integers(8, 49)))
    options = (("arith", int(rng.integers(0, 2))), ("fuse_block", int(rng.integers(0, 2))))
    _check_inference(CT.config(**bb), shape, options, seed=draw, image_seed=draw + 1)


# ---- training ---------------------------------------------------------------------------------------------------------------------

LOSS = {"hinge": 0.0, "cutoff": 255.0, "mae_multiplier": 1.0, "mse_multiplier": 0.5, "regularization": 0.01}


def _train_parity(bb, shape=(2, 32, 32), seed=5):
    cfg = CT.config(**bb)
    spec = CT.ConvnextSpec(cfg)
    params, state = CT.init_params(spec, seed=seed)
    m = bf.model_builder(cfg, device="cuda").hydra
    m.set_weights(params, state)
    clean, noisy = O.synthetic_batch(*shape, seed=seed)
    gt, x = clean.astype(np.float32), noisy.astype(np.float32)
    fns = bf.build_train_functions(m, bf.loss_function_builder(LOSS))
    r = np.random.default_rng(seed)
    ds = None
    if spec.dropout_rate > 0:
        ds = {key: (r.uniform(size=shape[0]) >= spec.dropout_rate).astype(np.float32) / np.float32(1 - spec.dropout_rate)
              for key in range(m.no_layers)}
        ds[0][:] = 0.0                                                     # one block off for sure, the rest as drawn
        ds[m.no_layers - 1][:] = 1.0 / np.float32(1 - spec.dropout_rate)
        fns.train_step_single_gpu.drop_scale = {k: dev_raw(v) for k, v in ds.items()}
    total, model_loss, [dl], pred, grads = fns.train_step_single_gpu(torch.from_numpy(gt), torch.from_numpy(x))
    r_total, r_reg, r_dl, r_pred, r_grads, r_state = CT.train_step(spec, O.LossSpec.from_config(LOSS), params, state,
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
    assert st.size == r_state.size and (np.abs(st - r_state).max() <= 1e-5 * max(1.0, np.abs(r_state).max()) if st.size else True)
    return m, fns, (gt, x)


@pytest.mark.parametrize("bb", [CT.INFER[0][0], CT.INFER[1][0], CT.INFER[2][0]])
def test_training_step_matches_autograd(bb):
    _train_parity(bb)


ADAM = {"type": "Adam", "schedule": {"type": "exponential_decay", "config": {"decay_rate": 0.9, "decay_steps": 100, "learning_rate": 1e-3}}}


def test_one_adam_step_lowers_the_loss():
    m, fns, (gt, x) = _train_parity(dict())
    before = m.get_weights()[0].copy()
    opt, _ = bf.optimizer_builder(ADAM)
    total, _, _, _, grads = fns.train_step_single_gpu(torch.from_numpy(gt), torch.from_numpy(x))
    fns.apply_grads(opt, grads, None)
    torch.cuda.synchronize()
    after = m.get_weights()[0]
    assert np.isfinite(after).all() and 0 < np.abs(after - before).max() <= 1e-3 * 1.01     # Adam's first step: |update| <= lr
    total2, _, _, _, _ = fns.train_step_single_gpu(torch.from_numpy(gt), torch.from_numpy(x))
    torch.cuda.synchronize()
    assert total2.item() < total.item(), (total.item(), total2.item())
    _, noisy = O.synthetic_batch(1, 32, 32, seed=1)
    assert bf.DenoiserModule(m)(noisy).dtype == np.uint8                  # the folded weights follow the step


def test_checkpoint_round_trip_resumes_bit_for_bit(tmp_path):
    from blind_image_denoising_amd.checkpoint import Checkpoint, CheckpointManager
    bb = dict(add_gates=True, add_learnable_multiplier=True, add_final_bn=True)
    cfg = CT.config(**bb)
    params, state = CT.init_params(CT.ConvnextSpec(cfg), seed=8)
    clean, noisy = O.synthetic_batch(2, 32, 32, seed=8)
    gt, x = torch.from_numpy(clean.astype(np.float32)), torch.from_numpy(noisy.astype(np.float32))

    def fresh():
        m = bf.model_builder(cfg, device="cuda").hydra
        m.set_weights(params, state)
        return m, bf.build_train_functions(m, bf.loss_function_builder(LOSS)), bf.optimizer_builder(ADAM)[0]

    def step(fns, opt):
        grads = fns.train_step_single_gpu(gt, x)[4]
        fns.apply_grads(opt, grads, None)

    m1, f1, o1 = fresh()
    step(f1, o1)
    CheckpointManager(Checkpoint(m1, o1, step=1), str(tmp_path)).save()
    step(f1, o1)
    m2, f2, o2 = fresh()
    ck = Checkpoint(m2, o2)
    assert CheckpointManager(ck, str(tmp_path)).restore_latest() and ck.step == 1
    step(f2, o2)
    torch.cuda.synchronize()
    for a, b in zip(m1.get_weights(), m2.get_weights()):
        assert np.array_equal(a, b)
    assert torch.equal(o1.m, o2.m) and torch.equal(o1.v, o2.v) and o1.iterations == o2.iterations


def test_saved_run_loads_into_the_wrappers(tmp_path):
    cfg = CT.config(add_concat_input=True)
    spec = CT.ConvnextSpec(cfg)
    params, state = CT.init_params(spec, seed=4)
    m = bf.model_builder(cfg, device="cuda").hydra
    m.set_weights(params, state)
    _, noisy = O.synthetic_batch(1, 48, 40, seed=6)
    a = bf.DenoiserModule(m)(noisy)
    bf.save_model(m, str(tmp_path / "convnext"))
    module = bf.load_model(str(tmp_path / "convnext"))
    assert isinstance(module, bf.DenoiserModule) and type(module.model_hydra).__name__ == "ConvnextHydra"
    assert np.array_equal(module(noisy), a)
    d = np.abs(a.astype(np.int32) - CT.denoiser_module_call(spec, params, state, noisy).astype(np.int32))
    assert d.max() <= 1 and (d > 0).mean() < 0.01
    # tiled: 32 x 32 tiles over the 48 x 40 frame (several tiles); one tile that holds the frame is the plain call
    tiled = bf.TiledDenoiserModule(module, tile=32, overlap=16, margin=4)
    out = tiled(noisy)
    assert out.shape == a.shape and out.dtype == np.uint8 and tiled.last_plan.tiles > 1
    assert np.array_equal(bf.TiledDenoiserModule(module, tile=64, margin=4)(noisy), a)
    # self-ensemble: the identity alone is the plain call; the D4 mean runs the model on the rotated (40 x 48) frames as well
    assert np.array_equal(bf.SelfEnsembleDenoiserModule(module, transforms=[0])(noisy), a)
    ens = bf.SelfEnsembleDenoiserModule(module)(noisy)
    assert ens.shape == a.shape and ens.dtype == np.uint8
