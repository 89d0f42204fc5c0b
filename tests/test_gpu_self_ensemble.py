"""GPU tests of the self-ensemble: bf_op_dihedral_stack_u8 / bf_op_dihedral_merge (csrc/self_ensemble.hip) and
SelfEnsembleDenoiserModule, all exact.

Yardstick: the NumPy statement of T_k / T_k^-1 kept in tests/test_self_ensemble.py (np.rot90 and a reversed slice), sequential
np.float32 adds in ascending k, a division by np.float32(n), np.clip and np.rint.  Nothing here has a tolerance: the kernels move
bytes, add in a fixed order, divide with correct rounding and round half to even, each of which NumPy does bit for bit the same.
The tile of both kernels is 32 x 32 pixels: the shapes sit below a tile, one past a tile edge in each direction (33, 65, 130 = 4
tiles + 2), on both channel counts and on a one-row image."""
import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import self_ensemble as SE
from oracle import bfcnn_oracle as O
from oracle import unet_oracle as U
from test_self_ensemble import t_forward, stack_reference, merge_reference
from guarded import dev as _dev, guard_bands

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guard_bands")]

SHAPES = [(1, 1, 1, 3), (2, 5, 7, 3), (1, 33, 65, 3), (1, 17, 130, 1), (3, 64, 64, 3), (1, 1, 70, 3)]
MEMBERS = [list(range(8)), [1], [0, 3, 6]]
_ids = {"ids": lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "k" + "".join(map(str, v))}


def _host(t):
    return None if t is None else t.cpu().numpy()


def _same(got, ref):
    if ref is None:
        return got is None
    return got is not None and got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got, ref)


# ---- the two kernels ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("members", MEMBERS, **_ids)
@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_stack_matches_numpy(shape, members):
    x = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    even, odd = SE.dihedral_stack_u8(_dev(x), members)
    r_even, r_odd = stack_reference(x, members)
    assert _same(_host(even), r_even) and _same(_host(odd), r_odd)
    if shape[1] == shape[2]:                                         # the joint layout: every member in one batch, ascending k
        joint, none = SE.dihedral_stack_u8(_dev(x), members, joint=True)
        assert none is None and _same(_host(joint), stack_reference(x, members, joint=True)[0])
    else:
        with pytest.raises(ValueError):
            SE.dihedral_stack_u8(_dev(x), members, joint=True)


def test_stack_layout_is_member_major():
    x = np.random.default_rng(5).integers(0, 256, (2, 5, 7, 3), dtype=np.uint8)
    even, odd = (_host(t) for t in SE.dihedral_stack_u8(_dev(x), [6, 0, 3, 1, 4]))          # given unsorted: stored sorted
    assert even.shape == (6, 5, 7, 3) and odd.shape == (4, 7, 5, 3)
    for j, k in enumerate((0, 4, 6)):
        assert np.array_equal(even[2 * j:2 * j + 2], t_forward(x, k)), k                   # member j = images j*B .. (j+1)*B-1
        assert np.array_equal(even[2 * j + 1], t_forward(x[1:2], k)[0]), k                 # ... image 1 of it = T_k of image 1
    for j, k in enumerate((1, 3)):
        assert np.array_equal(odd[2 * j:2 * j + 2], t_forward(x, k)), k
    sq = x[:, :, :5]
    joint, _ = SE.dihedral_stack_u8(_dev(sq), [3, 0, 6], joint=True)
    for j, k in enumerate((0, 3, 6)):
        assert np.array_equal(_host(joint)[2 * j:2 * j + 2], t_forward(sq, k)), k


def test_stack_refuses_other_channel_counts():
    for c in (2, 4):
        with pytest.raises(NotImplementedError):
            SE.dihedral_stack_u8(torch.zeros((1, 4, 4, c), dtype=torch.uint8, device="cuda"), "d4")
        with pytest.raises(NotImplementedError):
            SE.dihedral_merge(torch.zeros((1, 4, 4, c), device="cuda"), None, [0], 1, 4, 4)


def _layout(per_member: dict, joint: bool = False):
    """{k: member array} -> (even batch, odd batch) member-major in ascending k; joint: (one batch of all, None)"""
    ks = sorted(per_member)
    cat = lambda sel: np.concatenate([per_member[k] for k in sel]) if sel else None
    return (cat(ks), None) if joint else (cat([k for k in ks if k % 2 == 0]), cat([k for k in ks if k % 2 == 1]))


def _half_step_members(shape, members, rng):
    """float32 members whose values are random multiples of 0.5 in [-4, 260]: every sum is exact, many means land on .5 ties and
    some fall outside [0, 255].  The members of one pixel scatter by at most 2 around a common value (a tenth of those below 0, a
    tenth above 255): independent draws would put the mean of eight members near 128 everywhere and the clip would decide nothing."""
    base = rng.integers(0, 511, shape) * 0.5
    where = rng.random(shape)
    base = np.where(where < 0.1, rng.integers(-8, 0, shape) * 0.5, np.where(where > 0.9, rng.integers(511, 521, shape) * 0.5, base))
    return {k: t_forward(np.clip(base + rng.integers(-4, 5, shape) * 0.5, -4.0, 260.0).astype(np.float32), k) for k in members}


def _check_ties_and_clips(mean):
    """the float means of a case must make half-to-even and the clip decide results"""
    frac = mean - np.floor(mean)
    assert ((frac == 0.5) & (mean > 0) & (mean < 255)).any() and (mean < 0).any() and (mean > 255).any()


@pytest.mark.parametrize("members", MEMBERS, **_ids)
@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_merge_matches_numpy(shape, members):
    B, H, W, C = shape
    per_member = _half_step_members(shape, members, np.random.default_rng(100 + sum(shape) + len(members)))
    for joint in ((False, True) if H == W else (False,)):
        even, odd = _layout(per_member, joint)
        if B * H * W * C >= 100:
            _check_ties_and_clips(merge_reference(even, odd, members, B, False))
        for cast in (True, False):
            got = _host(SE.dihedral_merge(_dev(even), _dev(odd), members, B, H, W, cast_to_uint8=cast))
            assert _same(got, merge_reference(even, odd, members, B, cast)), (joint, cast)


def test_merge_ties_and_clips_decide():
    """one member: the mean IS the input, so the ties and the out-of-range values are set by hand"""
    v = np.array([0.5, 1.5, 2.5, 253.5, 254.5, -0.5, -3.0, 255.5, 260.0, 254.49998, 0.49999997, 127.5, 128.5], np.float32)
    x = np.resize(v, (1, 7, 13, 3)).astype(np.float32)
    for k in (0, 5):
        src = t_forward(x, k)
        got = _host(SE.dihedral_merge(_dev(src) if k % 2 == 0 else None, _dev(src) if k % 2 else None, [k], 1, 7, 13))
        assert np.array_equal(got, np.rint(np.clip(x, 0, 255)).astype(np.uint8))
        assert got[0, 0, 0, 0] == 0 and got[0, 0, 0, 1] == 2 and got[0, 0, 0, 2] == 2 and got[0, 0, 1, 0] == 254


def test_merge_arbitrary_floats():
    rng = np.random.default_rng(9)
    for shape, ks, joint in (((2, 33, 65, 3), list(range(8)), False), ((1, 40, 40, 1), [1, 2, 7], True)):
        B, H, W, C = shape
        even, odd = _layout({k: rng.uniform(-40.0, 300.0, t_forward(np.empty(shape, np.uint8), k).shape).astype(np.float32) for k in ks},
                            joint)
        for cast in (False, True):
            got = _host(SE.dihedral_merge(_dev(even), _dev(odd), ks, B, H, W, cast_to_uint8=cast))
            assert _same(got, merge_reference(even, odd, ks, B, cast)), (shape, cast)


def test_merge_refuses_wrong_shapes():
    f = lambda *s: torch.zeros(s, device="cuda")
    with pytest.raises(ValueError):
        SE.dihedral_merge(f(2, 4, 6, 3), f(1, 6, 4, 3), [0, 1], 1, 4, 6)         # even batch one member too long
    with pytest.raises(ValueError):
        SE.dihedral_merge(f(1, 4, 6, 3), f(1, 4, 6, 3), [0, 1], 1, 4, 6)         # odd batch not [W, H]
    with pytest.raises(ValueError):
        SE.dihedral_merge(f(1, 4, 6, 3), None, [0, 1], 1, 4, 6)                  # odd member without a batch, H != W
    with pytest.raises(ValueError):
        SE.dihedral_merge(f(1, 4, 6, 3), f(1, 6, 4, 3), [0], 1, 4, 6)            # a batch nobody is in
    with pytest.raises(ValueError):
        SE.dihedral_merge(f(1, 4, 6, 3).to(torch.float64), None, [0], 1, 4, 6)


# ---- the module --------------------------------------------------------------------------------------------------------------

def _resnet():
    cfg = O.canonical_config(no_layers=6)
    spec = O.ResnetSpec.from_config(cfg["model"])
    params, state = O.init_params(spec, seed=42)
    m = bf.model_builder(cfg["model"], device="cuda").hydra
    m.set_weights(params, state)
    return m


def _unet():
    cfg = U.canonical_config(depth=2, width=1)
    m = bf.model_builder(cfg["model"], device="cuda").hydra
    m.set_weights(U.init_params(U.UnetLaplacianSpec.from_config(cfg["model"]), seed=5))
    return m


_MODELS = {}


def _model(name):
    if name not in _MODELS:
        _MODELS[name] = {"resnet": _resnet, "unet": _unet}[name]()
    return _MODELS[name]


def _by_hand(hydra, x: np.ndarray, ks, cast: bool):
    """the ensemble from its parts: NumPy T_k, the plain float module on the batches of the batching contract, NumPy merge"""
    plain = bf.DenoiserModule(hydra, cast_to_uint8=False)
    B, H, W, _ = x.shape
    even, odd = stack_reference(x, ks, joint=H == W)
    calls = [None if b is None else plain(b) for b in (even, odd)]
    assert all(c is None or (c.dtype == np.float32 and c.shape == b.shape) for c, b in zip(calls, (even, odd)))
    return merge_reference(calls[0], calls[1], ks, B, cast), sum(c is not None for c in calls)


@pytest.mark.parametrize("case", [("resnet", (1, 24, 40, 3), 2), ("resnet", (2, 32, 32, 3), 1), ("unet", (1, 32, 48, 3), 2)],
                         ids=lambda c: f"{c[0]}-" + "x".join(map(str, c[1])))
@pytest.mark.parametrize("transforms", ["d4", "flips", [1, 4, 7]], ids=["d4", "flips", "k147"])
def test_end_to_end_is_the_hand_built_ensemble(case, transforms):
    name, shape, hydra_calls = case
    hydra = _model(name)
    x = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    for cast in (True, False):
        ens = bf.SelfEnsembleDenoiserModule(bf.DenoiserModule(hydra), transforms, cast_to_uint8=cast)
        ref, n_calls = _by_hand(hydra, x, list(ens.transforms), cast)
        if transforms == "d4":
            assert n_calls == hydra_calls
        got = ens(x)                                                 # NumPy in, NumPy out
        assert isinstance(got, np.ndarray) and _same(got, ref)
        got_dev = ens(_dev(x))                                       # device tensor in, device tensor out
        assert isinstance(got_dev, torch.Tensor) and got_dev.is_cuda and _same(got_dev.cpu().numpy(), ref)
        assert ens.check_status() is True
        assert ens(x[:0]).shape == (0,) + shape[1:] and ens(x[:0]).dtype == np.uint8


def test_batching_contract_calls(monkeypatch):
    """what the hydra is called on: one [n*B, H, W, C] batch for H == W, else the even batch and then the odd batch"""
    hydra = _model("resnet")
    ens = bf.SelfEnsembleDenoiserModule(bf.DenoiserModule(hydra), "d4")
    seen = []
    real = hydra.infer_u8
    monkeypatch.setattr(hydra, "infer_u8", lambda image, cast=True: (seen.append((image.cpu().numpy(), cast)), real(image, cast))[1])
    x = np.random.default_rng(3).integers(0, 256, (2, 32, 32, 3), dtype=np.uint8)
    ens(_dev(x))
    assert len(seen) == 1 and seen[0][1] is False and np.array_equal(seen[0][0], np.concatenate([t_forward(x, k) for k in range(8)]))
    del seen[:]
    y = x[:1, :24]
    ens(_dev(y))
    assert [s[0].shape for s in seen] == [(4, 24, 32, 3), (4, 32, 24, 3)] and all(s[1] is False for s in seen)
    assert np.array_equal(seen[0][0], np.concatenate([t_forward(y, k) for k in (0, 2, 4, 6)]))
    assert np.array_equal(seen[1][0], np.concatenate([t_forward(y, k) for k in (1, 3, 5, 7)]))


@pytest.mark.parametrize("name", ["resnet", "unet"])
def test_identity_member_is_the_plain_module(name):
    hydra = _model(name)
    for shape in ((2, 32, 32, 3), (1, 24, 40, 3) if name == "resnet" else (1, 32, 48, 3)):
        x = np.random.default_rng(7).integers(0, 256, shape, dtype=np.uint8)
        for cast in (True, False):
            plain = bf.DenoiserModule(hydra, cast_to_uint8=cast)(x)
            got = bf.SelfEnsembleDenoiserModule(bf.DenoiserModule(hydra), [0], cast_to_uint8=cast)(x)
            assert got.dtype == (np.uint8 if cast else np.float32) and np.array_equal(got, plain), (shape, cast)


def test_evaluate_accepts_the_ensemble():
    hydra = _model("resnet")
    clean, _ = O.synthetic_batch(2, 32, 32, seed=1)
    plain = bf.evaluate(bf.DenoiserModule(hydra), [clean], noise_std=(25,), seed=2)
    report = bf.evaluate(bf.SelfEnsembleDenoiserModule(bf.DenoiserModule(hydra)), [clean], noise_std=(25,), seed=2)
    assert len(report) == 1 and set(report[0]) == set(plain[0]) and report[0]["images"] == 2
    assert all(np.isfinite(v) for v in report[0].values())
    assert report[0]["psnr_noisy"] == plain[0]["psnr_noisy"]        # the same noise went in
