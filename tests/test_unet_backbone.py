"""CPU tests of the plain U-Net backbone (`"type": "unet"`, blind_image_denoising_amd/unet_backbone.py): the builder returns a
UnetHydra for the configurations the engine builds, its parameter / state inventories equal the test oracle's in Keras creation
order, the options the reference ignores leave the graph alone, and what is not built is refused with the stated error."""
import json

import numpy as np
import pytest

import blind_image_denoising_amd as bf
import unet_backbone_torch as UB

BUILT = [
    dict(),
    dict(no_layers=0),
    dict(no_levels=1),
    dict(no_levels=1, no_layers=2, block_kernels=[3], block_filters=[32]),
    dict(no_levels=3, block_kernels=[1, 3, 1], block_filters=[64, 128, 64], filters=64),
    dict(no_levels=3, no_layers=2, block_kernels=[5, 3], block_filters=[64, 64], filters=64, kernel_size=5),
    dict(add_gates=True, dropout_rate=0.2, add_learnable_multiplier=True, add_concat_input=True),
    dict(add_initial_bn=True, add_final_bn=True, add_channelwise_scaling=True, add_clip=True),
    dict(use_bn=False, activation="leaky_relu_01", base_activation="relu", add_learnable_multiplier=True, add_clip=True),
    dict(no_levels=4, no_layers=1, block_kernels=[3, 1, 3], block_filters=[32, 64, 32], add_gates=True),
]


def _hydra(**bb):
    return bf.model_builder(UB.config(**bb), device="cpu", seed=0).hydra


@pytest.mark.parametrize("bb", BUILT)
def test_builder_returns_unet_with_the_oracle_inventory(bb):
    from blind_image_denoising_amd.unet_backbone import UnetHydra
    m = _hydra(**bb)
    spec = UB.UnetSpec(UB.config(**bb))
    assert isinstance(m, UnetHydra)
    assert [(v[0], tuple(v[1]), v[2]) for v in m.trainable_variables] == [(n, tuple(s), k) for n, s, k in spec.tensors()]
    assert [(v[0], tuple(v[1])) for v in m.non_trainable_variables] == [(n, tuple(s)) for n, s in spec.state_tensors()]
    assert m.count_params() == sum(int(np.prod(s)) for _, s, _ in spec.tensors())
    p, s = m.get_weights()
    assert p.size == m.n_params and s.size == m.n_state
    # creation values: BN gammas / moving variances one, moving means and multipliers zero
    for name, shape, kind, off in m.trainable_variables:
        v = p[off:off + int(np.prod(shape))]
        if kind == "bn_gamma":
            assert (v == 1).all(), name
        elif kind in ("channelwise", "multiplier"):
            assert (v == 0).all(), name
    params, state = UB.init_params(spec, seed=3)
    m.set_weights(params, state)
    assert np.array_equal(m.get_weights()[0], params) and np.array_equal(m.get_weights()[1], state)


def test_ignored_keys_leave_the_inventory_alone():
    base = _hydra(add_gates=True)
    m = _hydra(add_gates=True, add_selector=True, add_sparsity=True, add_mean_sigma_normalization=True, block_depthwise=[-1, 4],
               block_groups=[1, 2], block_activation=["gelu", "linear"], block_regularizer=["l2", "l2"])
    assert [v[:3] for v in m.trainable_variables] == [v[:3] for v in base.trainable_variables]
    assert [v[:2] for v in m.non_trainable_variables] == [v[:2] for v in base.non_trainable_variables]
    assert m.block_activation == base.block_activation


def test_parameter_count_written_out_by_hand():
    # 2 levels, 1 block of [3x3 32, 3x3 32] + BN, 32 filters, 3x3 base, RGB in and out:
    #   base 3*3*3*32 = 864; a block: 2 * 3*3*32*32 + 32 (bn1 gamma) = 18464; a 32 -> 32 entry 3*3*32*32 = 9216;
    #   enc0 block 18464, enc1 entry 9216 + block 18464, dec1 entry 9216 + block 18464, dec0 entry 3*3*64*32 = 18432 + block 18464;
    #   head 32*32 + 32*3 = 1120
    #   864 + 18464 + 9216 + 18464 + 9216 + 18464 + 18432 + 18464 + 1120 = 112704;  state: 4 BNs * 2 * 32 = 256
    m = _hydra()
    assert m.count_params() == 112704 and m.n_state == 256
    # 3 levels, no blocks, [1x1 64], 64 filters, 5x5 base, concat input + channelwise + multiplier:
    #   base 5*5*3*64 = 4800; entries enc1, enc2, dec2: 3 * 64*64 = 12288; dec1, dec0: 2 * 128*64 = 16384;
    #   channelwise 64 + 3 = 67; multiplier 1; head 67*32 + 32*3 = 2240
    #   4800 + 12288 + 16384 + 67 + 1 + 2240 = 35780;  no state
    m = _hydra(no_levels=3, no_layers=0, kernel_size=5, filters=64, block_kernels=[1], block_filters=[64], add_concat_input=True,
               add_channelwise_scaling=True, add_learnable_multiplier=True)
    assert m.count_params() == 35780 and m.n_state == 0


def test_entry_convolutions_take_the_first_block_convolution_parameters():
    m = _hydra(block_kernels=[5, 3], activation="relu", base_activation="linear")
    assert m.entry_activation == "relu"
    shapes = {v[0]: tuple(v[1]) for v in m.trainable_variables}
    assert shapes["enc1/entry/kernel"] == (5, 5, 32, 32) and shapes["dec0/entry/kernel"] == (5, 5, 64, 32)
    m = _hydra(block_kernels=[3], block_filters=[32], base_activation="relu", activation="linear")
    assert m.entry_activation == "relu"                     # one block convolution: convs_params[0] is the last one


@pytest.mark.parametrize("bb,key", [
    (dict(add_sparse_features=True), "add_sparse_features"),
    (dict(use_bias=True), "use_bias"),
    (dict(filters=16, block_filters=[16, 16]), "filters=16"),
    (dict(filters=48, block_filters=[48, 48]), "filters=48"),
    (dict(filters=128, block_filters=[128, 128]), "filters=128"),
    (dict(no_layers=0, block_filters=[64], block_kernels=[3]), "upsampled 64, skip 32"),
    (dict(block_kernels=[7, 3]), "k=7"),
    (dict(no_levels=1, no_layers=1, block_kernels=[1, 1], block_filters=[256, 32]), "32->256"),
])
def test_not_built_is_not_implemented(bb, key):
    with pytest.raises(NotImplementedError, match=key):
        _hydra(**bb)


@pytest.mark.parametrize("key", ["use_bias", "use_bn", "use_ln"])
def test_denoiser_head_options_not_implemented(key):
    cfg = UB.config()
    cfg["denoiser"][key] = True
    with pytest.raises(NotImplementedError, match=key):
        bf.model_builder(cfg, device="cpu")


@pytest.mark.parametrize("bb", [
    dict(block_filters=[32, 64]),                                          # the residual Add: last block conv != block input
    dict(block_filters=[64, 32]),                                          # level 1 blocks take 64 channels and give back 32
    dict(no_levels=1, block_filters=[64, 32]),                             # the deepest decoder's blocks behind a 32 -> 64 entry
    dict(no_levels=0),
    dict(no_layers=-1),
    dict(block_kernels=[3, 3, 3, 3], block_filters=[32] * 4),
    dict(block_filters=[32]),
    dict(block_kernels=[3], block_filters=[32], add_gates=True),
    dict(dropout_rate=1.5),
])
def test_what_keras_rejects_is_a_value_error(bb):
    with pytest.raises(ValueError):
        _hydra(**bb)


def test_image_size_must_divide_by_the_pooling():
    m = _hydra(no_levels=3)
    with pytest.raises(ValueError, match="multiples of 4"):
        m(np.zeros((1, 36, 30, 3), np.float32))
    with pytest.raises(RuntimeError, match="GPU"):                         # a size that fits: no CPU execution path
        m(np.zeros((1, 36, 32, 3), np.float32))


def test_options_and_describe_resnet():
    m = _hydra()
    assert m.fuse_upcat == 1
    m.set_option("fuse_upcat", 0)
    assert m.fuse_upcat == 0
    with pytest.raises(ValueError):
        m.set_option("arith", 1)
    from blind_image_denoising_amd.model import describe_resnet
    cfg = UB.config()
    with pytest.raises(ValueError, match="unet_backbone"):
        describe_resnet(cfg)
    cfg["backbone"]["type"] = "convnext"
    with pytest.raises(NotImplementedError, match="convnext"):
        describe_resnet(cfg)
    with pytest.raises(NotImplementedError):
        bf.model_builder(cfg, device="cpu")


def test_save_and_load_on_the_host(tmp_path):
    m = _hydra(add_gates=True, add_final_bn=True)
    params, state = UB.init_params(UB.UnetSpec(UB.config(add_gates=True, add_final_bn=True)), seed=5)
    m.set_weights(params, state)
    bf.save_model(m, str(tmp_path / "u"))
    cfg = json.load(open(tmp_path / "u" / "pipeline.json"))
    assert cfg["model"]["backbone"]["type"] == "unet"
    from blind_image_denoising_amd.model import load_hydra
    m2 = load_hydra(str(tmp_path / "u"), device="cpu")
    assert np.array_equal(m2.get_weights()[0], params) and np.array_equal(m2.get_weights()[1], state)
