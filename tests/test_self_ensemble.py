"""CPU tests of blind_image_denoising_amd.self_ensemble: argument handling, load_model(self_ensemble=...), and the NumPy statement
of the transform numbering that the GPU tests (tests/test_gpu_self_ensemble.py) use as their reference."""
import numpy as np
import pytest

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import _native as N
from blind_image_denoising_amd import self_ensemble as SE
from oracle import bfcnn_oracle as O
from oracle import unet_oracle as U


# ---- the reference: T_k and its inverse on [B,H,W,C] arrays ---------------------------------------------------------------------

def t_forward(x: np.ndarray, k: int) -> np.ndarray:
    """T_k(x) = flipW^(k >> 2)(rot90^(k & 3)(x))"""
    y = np.rot90(x, k & 3, axes=(1, 2))
    return np.ascontiguousarray(y[:, :, ::-1] if k >> 2 else y)


def t_inverse(y: np.ndarray, k: int) -> np.ndarray:
    """T_k^-1(y) = rot90^(-(k & 3))(flipW^(k >> 2)(y))"""
    x = y[:, :, ::-1] if k >> 2 else y
    return np.ascontiguousarray(np.rot90(x, -(k & 3), axes=(1, 2)))


def stack_reference(x: np.ndarray, ks, joint: bool = False):
    """(even batch, odd batch) of the members, member-major in ascending k; joint: (every member in one batch, None)"""
    ks = sorted(ks)
    cat = lambda sel: np.concatenate([t_forward(x, k) for k in sel]) if sel else None
    if joint:
        return cat(ks), None
    return cat([k for k in ks if k % 2 == 0]), cat([k for k in ks if k % 2 == 1])


def merge_reference(even, odd, ks, B: int, cast_to_uint8: bool):
    """sequential float32 sum of the inverse-transformed members in ascending k, / float32(n), [clip, rint, uint8]"""
    ks = sorted(ks)
    joint = odd is None
    slot = {}
    for k in ks:
        src = even if joint or k % 2 == 0 else odd
        j = ks.index(k) if joint else [q for q in ks if q % 2 == k % 2].index(k)
        slot[k] = src[j * B:(j + 1) * B]
    s = None
    for k in ks:
        v = t_inverse(slot[k], k).astype(np.float32)
        s = v if s is None else (s + v).astype(np.float32)
    m = (s / np.float32(len(ks))).astype(np.float32)
    return np.rint(np.clip(m, 0, 255)).astype(np.uint8) if cast_to_uint8 else m


def test_numbering_is_the_whole_group():
    x = np.arange(2 * 3, dtype=np.int32).reshape(1, 2, 3, 1)
    members = [t_forward(x, k) for k in range(8)]
    for k, y in enumerate(members):
        assert y.shape == ((1, 3, 2, 1) if k & 1 else (1, 2, 3, 1))
        assert np.array_equal(t_inverse(y, k), x), k
    for a in range(8):
        for b in range(a + 1, 8):
            assert members[a].shape != members[b].shape or not np.array_equal(members[a], members[b]), (a, b)
    big = np.random.default_rng(0).integers(0, 256, (2, 5, 7, 3), dtype=np.uint8)
    for k in range(8):
        assert np.array_equal(t_inverse(t_forward(big, k), k), big)
    # the position table of csrc/self_ensemble.hip: source pixel (y, x) of an [H, W] image lands at (row, column) of member k
    FX, FY = (0, 1, 1, 0, 1, 1, 0, 0), (0, 0, 1, 1, 0, 1, 1, 0)
    H, W = 5, 7
    for k in range(8):
        m = t_forward(big, k)
        for y, x_ in ((0, 0), (1, 4), (4, 6), (3, 2)):
            yy, xx = (H - 1 - y if FY[k] else y), (W - 1 - x_ if FX[k] else x_)
            assert np.array_equal(m[:, xx, yy] if k & 1 else m[:, yy, xx], big[:, y, x_]), (k, y, x_)


def test_merge_reference_undoes_the_stack():
    x = np.random.default_rng(1).integers(0, 256, (2, 4, 6, 3), dtype=np.uint8)
    for ks in (range(8), [1], [0, 3, 6]):
        even, odd = stack_reference(x, ks)
        f = lambda a: None if a is None else a.astype(np.float32)
        assert np.array_equal(merge_reference(f(even), f(odd), ks, 2, True), x)
    sq = x[:, :, :4]
    allm, none = stack_reference(sq, [0, 3, 5], joint=True)
    assert none is None and allm.shape == (6, 4, 4, 3) and np.array_equal(allm[2:4], t_forward(sq, 3))
    assert np.array_equal(merge_reference(allm.astype(np.float32), None, [0, 3, 5], 2, True), sq)


# ---- the module --------------------------------------------------------------------------------------------------------------------

def _cpu_module():
    return bf.DenoiserModule(bf.model_builder(O.canonical_config(no_layers=1)["model"], device="cpu").hydra)


def test_transforms_parsing():
    module = _cpu_module()
    assert bf.SelfEnsembleDenoiserModule(module).transforms == (0, 1, 2, 3, 4, 5, 6, 7)
    assert bf.SelfEnsembleDenoiserModule(module, "d4").transforms == (0, 1, 2, 3, 4, 5, 6, 7)
    assert bf.SelfEnsembleDenoiserModule(module, "flips").transforms == (0, 2, 4, 6)
    assert bf.SelfEnsembleDenoiserModule(module, [5, 1]).transforms == (1, 5)
    assert bf.SelfEnsembleDenoiserModule(module, (np.int64(7),)).transforms == (7,)
    for bad in ([], [8], [1, 1], "x", [-1], [1.5], [True], None, 3):
        with pytest.raises(ValueError):
            bf.SelfEnsembleDenoiserModule(module, bad)
    for not_a_module in (None, module.model_hydra, lambda x: x, bf.SelfEnsembleDenoiserModule(module)):
        with pytest.raises(ValueError):
            bf.SelfEnsembleDenoiserModule(not_a_module)
    with pytest.raises(ValueError):                                  # GraphedDenoiserModule around the ensemble is out of scope
        bf.GraphedDenoiserModule(bf.SelfEnsembleDenoiserModule(module))


def test_module_delegates_and_checks_like_the_wrapped_module():
    module = _cpu_module()
    ens = bf.SelfEnsembleDenoiserModule(module, "flips")
    assert ens.model_hydra is module.model_hydra and ens.name == module.name and ens.check_status() is True
    with pytest.raises(ValueError):
        ens(np.zeros((1, 8, 8, 3), np.float32))
    with pytest.raises(ValueError):
        ens(np.zeros((8, 8, 3), np.uint8))
    with pytest.raises(ValueError):
        ens(np.zeros((1, 8, 8, 1), np.uint8))
    with pytest.raises(ValueError):
        ens("image")
    empty = ens(np.zeros((0, 8, 8, 3), np.uint8))
    assert isinstance(empty, np.ndarray) and empty.shape == (0, 8, 8, 3) and empty.dtype == np.uint8
    with pytest.raises(RuntimeError, match="no CPU execution path"):
        ens(np.zeros((1, 8, 8, 3), np.uint8))


def test_load_model_self_ensemble_keyword(tmp_path):
    cfg = U.canonical_config(depth=2, width=1)
    bf.save_model(bf.model_builder(cfg["model"], device="cpu", seed=3).hydra, str(tmp_path / "m"))
    ens = bf.load_model(str(tmp_path / "m"), device="cpu", self_ensemble="flips")
    assert type(ens) is bf.SelfEnsembleDenoiserModule and ens.transforms == (0, 2, 4, 6)
    with pytest.raises(RuntimeError, match="GPU"):
        ens(np.zeros((1, 16, 16, 3), np.uint8))
    assert bf.load_model(str(tmp_path / "m"), device="cpu", self_ensemble=[4, 1]).transforms == (1, 4)
    assert type(bf.load_model(str(tmp_path / "m"), device="cpu")) is bf.DenoiserModule
    assert type(bf.load_model(str(tmp_path / "m"), device="cpu", self_ensemble=None)) is bf.DenoiserModule
    with pytest.raises(ValueError):
        bf.load_model(str(tmp_path / "m"), device="cpu", self_ensemble="x")


def test_wrappers_take_device_tensors_only():
    import torch
    with pytest.raises(RuntimeError, match="GPU"):
        SE.dihedral_stack_u8(torch.zeros((1, 4, 4, 3), dtype=torch.uint8), "d4")
    with pytest.raises(ValueError):
        SE.dihedral_stack_u8(torch.zeros((1, 4, 4, 3), dtype=torch.float32), "d4")
    with pytest.raises(ValueError):
        SE.dihedral_stack_u8(np.zeros((1, 4, 4, 3), np.uint8), "d4")
    with pytest.raises(RuntimeError, match="GPU"):
        SE.dihedral_merge(torch.zeros((1, 4, 4, 3)), None, [0], 1, 4, 4)
    with pytest.raises(ValueError):                                  # odd members without an odd batch: H == W only
        SE.dihedral_merge(torch.zeros((2, 4, 6, 3)), None, [0, 1], 1, 4, 6)


def test_native_entries_refuse_bad_arguments_before_launching():
    L = N.lib()
    for name in ("bf_op_dihedral_stack_u8", "bf_op_dihedral_merge"):
        assert name in N.SIGNATURES and hasattr(L, name)
    a, b, c = 4096, 8192, 12288                                      # never dereferenced: every call below is refused
    assert L.bf_op_dihedral_stack_u8(None, b, c, 1, 4, 4, 3, 255, None) == N.BF_EINVAL
    assert L.bf_op_dihedral_stack_u8(a, None, c, 1, 4, 4, 3, 255, None) == N.BF_EINVAL
    assert L.bf_op_dihedral_stack_u8(a, b, None, 1, 4, 6, 3, 255, None) == N.BF_EINVAL      # joint layout needs H == W
    assert L.bf_op_dihedral_stack_u8(a, a, c, 1, 4, 4, 3, 255, None) == N.BF_EINVAL         # in place
    assert L.bf_op_dihedral_stack_u8(a, b, c, 1, 4, 4, 3, 0, None) == N.BF_EINVAL
    assert L.bf_op_dihedral_stack_u8(a, b, c, 1, 4, 4, 3, 256, None) == N.BF_EINVAL
    assert L.bf_op_dihedral_stack_u8(a, b, c, 0, 4, 4, 3, 255, None) == N.BF_EINVAL
    assert L.bf_op_dihedral_stack_u8(a, b, c, 1, 4, 4, 2, 255, None) == N.BF_EUNSUPPORTED
    assert L.bf_op_dihedral_stack_u8(a, b, c, 1, 4, 4, 4, 255, None) == N.BF_EUNSUPPORTED
    assert L.bf_op_dihedral_merge(a, b, None, 1, 4, 4, 3, 255, 1, None) == N.BF_EINVAL
    assert L.bf_op_dihedral_merge(None, b, c, 1, 4, 4, 3, 255, 1, None) == N.BF_EINVAL
    assert L.bf_op_dihedral_merge(a, None, c, 1, 4, 6, 3, 2, 1, None) == N.BF_EINVAL
    assert L.bf_op_dihedral_merge(a, b, a, 1, 4, 4, 3, 255, 0, None) == N.BF_EINVAL
    assert L.bf_op_dihedral_merge(a, b, c, 1, 4, 4, 16, 255, 0, None) == N.BF_EUNSUPPORTED
