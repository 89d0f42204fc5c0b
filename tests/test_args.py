"""CPU tests of what the wrappers around the denoiser share: the argument checks of blind_image_denoising_amd/_args.py, one rule
per row; the float form every wrapper class answers for itself (module_denoiser.float_form); and the one wording of "this is on
the host" that every feature module raises.  Nothing here touches a device."""
import ast
import pathlib
import subprocess
import sys

import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import _args as A
from blind_image_denoising_amd.module_denoiser import float_form
from oracle import bfcnn_oracle as O

ROOT = pathlib.Path(__file__).resolve().parent.parent
U8, F32 = (torch.uint8,), (torch.float32,)


def _u8(*shape):
    return torch.zeros(shape, dtype=torch.uint8)


# ---- the table: every rule of _args once -------------------------------------------------------------------------------------

@pytest.mark.parametrize("call", [
    lambda: A.image_batch(np.zeros((1, 8, 8, 3), np.uint8), "x", U8),                         # wrong type
    lambda: A.image_batch("image", "x", U8),
    lambda: A.image_batch(torch.zeros((1, 8, 8, 3)), "x", U8),                                # wrong dtype
    lambda: A.image_batch(_u8(1, 8, 8, 3), "x", F32),
    lambda: A.image_batch(_u8(8, 8, 3), "x", U8),                                             # rank 3
    lambda: A.image_batch(_u8(1, 8, 8, 0), "x", U8),                                          # 0 and 5 channels
    lambda: A.image_batch(_u8(1, 8, 8, 5), "x", U8),
    lambda: A.image_batch(_u8(1, 8, 8, 3), "x", U8, channels=(1, 1)),
    lambda: A.image_batch(_u8(1, 2, 8, 3), "x", U8, min_hw=3),                                # H, then W, below min_hw
    lambda: A.image_batch(_u8(1, 8, 2, 3), "x", U8, min_hw=3),
    lambda: A.image_batch(_u8(1, 0, 8, 3), "x", U8),
    lambda: A.image_batch(_u8(1, 7, 8, 3), "x", U8, even=True),                               # odd with even=True
    lambda: A.image_batch(_u8(1, 8, 9, 3), "x", U8, even=True),
    lambda: A.image_batch(_u8(0, 8, 8, 3), "x", U8),                                          # B = 0 without allow_empty
    lambda: A.host_or_device(np.zeros((1, 8, 8, 3), np.float32), "x", U8),
    lambda: A.host_or_device(np.zeros((1, 8, 8, 3), np.uint16), "x", U8),
    lambda: A.host_or_device([[1, 2, 3]], "x", U8),
    lambda: A.host_or_device(np.zeros((0, 8, 8, 3), np.uint8), "x", U8),
    lambda: A.uint8_batches([], "x"),
    lambda: A.uint8_batches([np.zeros((1, 8, 8, 3), np.uint8), np.zeros((1, 2, 8, 3), np.uint8)], "x", min_hw=3),
    lambda: A.int_in(True, "x", 0, 4), lambda: A.int_in(1.0, "x", 0, 4), lambda: A.int_in(-1, "x", 0, 4),
    lambda: A.int_in(5, "x", 0, 4), lambda: A.int_in(0, "x", 1), lambda: A.int_in(None, "x", 1),
    lambda: A.seed64(True), lambda: A.seed64(-1), lambda: A.seed64(2 ** 64), lambda: A.seed64(1.5),
    lambda: A.non_negative_float(True, "x"), lambda: A.non_negative_float(float("nan"), "x"),
    lambda: A.non_negative_float(float("inf"), "x"), lambda: A.non_negative_float(-0.5, "x"),
    lambda: A.non_negative_float(2.5, "x", top=2.0), lambda: A.non_negative_float("2", "x"), lambda: A.non_negative_float(None, "x"),
    lambda: A.one_of("median", "x", ("mad", "immerkaer")), lambda: A.one_of(None, "x", ("mad",)), lambda: A.one_of(1, "x", ("mad",)),
    lambda: A.per_image_channel([1.0, 2.0], 2, 3, "x"),                                       # neither [C] nor [B,C]
    lambda: A.per_image_channel(np.zeros((3, 2)), 2, 3, "x"),
    lambda: A.per_image_channel(np.zeros((1, 2, 3)), 2, 3, "x"),
    lambda: A.per_image_channel(-1.0, 2, 3, "x"), lambda: A.per_image_channel(float("nan"), 2, 3, "x"),
    lambda: A.per_image_channel([1.0, float("inf"), 1.0], 2, 3, "x"), lambda: A.per_image_channel("a", 2, 3, "x"),
    lambda: A.broadcasts_to((2,), 2, 3, "x"),
    lambda: A.module_result(np.zeros((1, 8, 8, 3), np.float32), torch.float32, (1, 8, 8, 3)),
    lambda: A.module_result(_u8(1, 8, 8, 3), torch.float32, (1, 8, 8, 3)),
    lambda: A.module_result(torch.zeros((1, 8, 8, 3)), torch.float32, (2, 8, 8, 3)),
    lambda: A.module_result(None, torch.uint8, (1, 8, 8, 3)),
], ids=lambda c: None)
def test_every_rule_refuses_with_a_value_error_that_names_the_argument(call):
    with pytest.raises(ValueError, match=r"^(x|seed|no x|the module) "):
        call()


def test_what_the_rules_accept_and_return():
    t = _u8(2, 8, 6, 3)
    assert A.image_batch(t, "x", U8, min_hw=6, even=True) is t and A.image_batch(t.float(), "x", (torch.uint8, torch.float32)).dtype == torch.float32
    assert A.image_batch(_u8(0, 8, 8, 4), "x", U8, allow_empty=True).shape[0] == 0          # B = 0 with allow_empty
    assert A.image_batch(_u8(1, 0, 8, 1), "x", U8, min_hw=0).shape[1] == 0
    assert A.image_batch(_u8(1, 8, 8, 16), "x", U8, channels=(16, 16)).shape[3] == 16
    array = np.arange(2 * 4 * 4 * 3, dtype=np.uint8).reshape(2, 4, 4, 3)
    wrapped, was_numpy = A.host_or_device(array[:, ::2], "x", U8)                            # not contiguous: wrapped, not uploaded
    assert was_numpy and not wrapped.is_cuda and wrapped.is_contiguous() and np.array_equal(wrapped.numpy(), array[:, ::2])
    same, was_numpy = A.host_or_device(t, "x", U8)
    assert same is t and not was_numpy
    assert [tuple(b.shape) for b in A.uint8_batches([array, t], "x")] == [(2, 4, 4, 3), (2, 8, 6, 3)]
    assert A.int_in(np.int64(4), "x", 0, 4) == 4 and type(A.int_in(np.int64(4), "x", 0, 4)) is int and A.int_in(10 ** 6, "x", 1) == 10 ** 6
    assert A.seed64(0) == 0 and A.seed64(2 ** 64 - 1) == 2 ** 64 - 1
    assert A.non_negative_float(2, "x") == 2.0 and type(A.non_negative_float(np.float32(0.5), "x", top=0.5)) is float
    assert A.one_of("mad", "x", ("mad", "immerkaer")) == "mad"
    for value, want in ((1.5, np.full((2, 3), 1.5)), ([1.0, 2.0, 3.0], np.tile([1.0, 2.0, 3.0], (2, 1))),
                        (np.arange(6.0).reshape(2, 3), np.arange(6.0).reshape(2, 3))):      # a float, [C], [B,C]
        got = A.per_image_channel(value, 2, 3, "x")
        assert got.dtype == torch.float64 and got.is_contiguous() and np.array_equal(got.numpy(), want)
    assert tuple(A.per_image_channel(float("nan"), 0, 3, "x").shape) == (0, 3)              # nothing to look at in no images
    for shape in ((), (3,), (2, 3)):
        A.broadcasts_to(shape, 2, 3, "x")
    f = torch.zeros((1, 8, 8, 3))
    assert A.module_result(f, torch.float32, f.shape) is f
    with pytest.raises(ValueError, match="rounded"):
        A.module_result(t, torch.float32, t.shape, hint=": rounded")


def test_the_upload_rule():
    host = _u8(1, 8, 8, 3)
    with pytest.raises(RuntimeError) as e:
        A.to_device(host, False, None, "noisy", "the feature")                               # a host tensor is never uploaded
    assert str(e.value) == "noisy must live on the GPU: the feature has no CPU execution path"
    assert A.device_of(None).type == "cuda" if torch.cuda.is_available() else True
    if not torch.cuda.is_available():                                                        # NumPy needs a device to go to
        for call in (lambda: A.to_device(host, True, None, "noisy", "the feature"), lambda: A.device_of(object(), "the feature")):
            with pytest.raises(RuntimeError) as e:
                call()
            assert "GPU" in str(e.value) and "no CPU execution path" in str(e.value)


# ---- one wording per feature module ------------------------------------------------------------------------------------------

_HOST_U8, _HOST_F32 = _u8(1, 16, 16, 3), torch.zeros((1, 16, 16, 3))


@pytest.mark.parametrize("call", [
    lambda: bf.image_metrics(_HOST_U8, _HOST_U8),
    lambda: bf.self_ensemble.dihedral_stack_u8(_HOST_U8, "d4"),
    lambda: bf.self_ensemble.dihedral_merge(_HOST_F32, None, [0], 1, 16, 16),
    lambda: bf.noise_statistics(_HOST_U8),
    lambda: bf.noise_level_statistics(_HOST_U8),
    lambda: bf.camera_noise(_HOST_U8, 0.1, 1.0),
    lambda: bf.risk_probe_stack_u8(_HOST_U8),
    lambda: bf.risk_sums(_HOST_U8, torch.zeros((2, 16, 16, 3)), 1, 1, 0),
    lambda: bf.estimate_risk(lambda u: u.float(), _HOST_U8, sigma=1.0),
    lambda: bf.estimate_risk_affine(lambda u: u.float(), _HOST_U8, (0.1, 1.0)),
    lambda: bf.neighbor_pairs(_HOST_U8),
    lambda: bf.stabilise_u8(_HOST_U8, (0.5, 4.0)),
    lambda: bf.unstabilise(_HOST_F32, (0.5, 4.0)),
    lambda: bf.StabilisedDenoiserModule(lambda u: u.float(), (0.5, 4.0))(_HOST_U8),
], ids=["metrics", "self_ensemble.stack", "self_ensemble.merge", "noise_estimate", "noise_level", "noise_level.camera_noise",
        "risk.probe", "risk.sums", "risk.estimate", "risk.affine", "neighbor", "vst.forward", "vst.inverse", "vst.module"])
def test_a_host_tensor_gets_the_same_error_from_every_feature(call):
    with pytest.raises(RuntimeError) as e:
        call()
    assert "GPU" in str(e.value) and "no CPU execution path" in str(e.value)


# ---- the float form ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def module():
    return bf.DenoiserModule(bf.model_builder(O.canonical_config(no_layers=1)["model"], device="cpu").hydra)


def test_float_form_of_a_denoiser_module_and_of_its_graphed_form(module):
    for m in (module, bf.GraphedDenoiserModule(module)):
        f = float_form(m)
        assert type(f) is bf.DenoiserModule and f is not m and f is not module and f._cast_to_uint8 is False
        assert f.model_hydra is module.model_hydra and f._deferred is module._deferred
        assert f is not float_form(m)                                                        # a new one per call


def test_float_form_of_the_ensemble(module):
    ens = bf.SelfEnsembleDenoiserModule(module, [5, 1])
    f = float_form(ens)
    assert type(f) is bf.SelfEnsembleDenoiserModule and f is not ens and f._cast_to_uint8 is False and f.transforms == (1, 5)
    assert f.model_hydra is module.model_hydra and f._module is module
    for e in (ens, f):                                                                       # what runs inside either one
        assert type(e._inner) is bf.DenoiserModule and e._inner._cast_to_uint8 is False and e._inner._deferred is module._deferred


def test_float_form_of_the_stabilised_module(module):
    ens = bf.SelfEnsembleDenoiserModule(module, "flips")
    for inner in (module, ens, bf.GraphedDenoiserModule(module)):
        st = bf.StabilisedDenoiserModule(inner, ([0.1, 0.2, 0.3], 4.0), inverse="algebraic", min_cells=32)
        f = float_form(st)
        assert type(f) is bf.StabilisedDenoiserModule and f is not st and f._cast_to_uint8 is False and st._cast_to_uint8 is True
        assert f.inverse == "algebraic" and f.min_cells == 32 and f.model_hydra is module.model_hydra and f._module is inner
        assert f.noise_level[0].tolist() == [0.1, 0.2, 0.3] and float(f.noise_level[1]) == 4.0
        bottom = f._float._inner if inner is ens else f._float
        assert type(f._float) is (bf.SelfEnsembleDenoiserModule if inner is ens else bf.DenoiserModule)
        assert bottom._cast_to_uint8 is False and bottom._deferred is module._deferred
    assert float_form(bf.StabilisedDenoiserModule(module)).noise_level is None


def test_float_form_of_anything_else():
    fn = lambda u: u.float()
    assert float_form(fn) is fn
    for bad in (None, 3, "unet", object()):
        with pytest.raises(ValueError, match="module"):
            float_form(bad)
    with pytest.raises(ValueError, match="model"):
        float_form(3, "model")


# ---- the protocol of DenoiserWrapper, held by every wrapper class --------------------------------------------------------------

_DENOISE = lambda u8: u8.float()
_WRAPPER_CASES = {                                                # class, settings away from the defaults, what it is built on
    "self_ensemble": (bf.SelfEnsembleDenoiserModule, {"transforms": (1, 5)}, "module"),    # takes a DenoiserModule alone
    "tiled": (bf.TiledDenoiserModule, {"tile": 32, "overlap": 12, "margin": 3, "tile_batch": 4}, _DENOISE),
    "pixel_shuffle": (bf.PixelShuffleDenoiserModule,
                      {"stride": "auto", "max_stride": 3, "threshold": 0.7, "refine": 4, "replace": 0.2, "seed": 9}, _DENOISE),
    "stabilised": (bf.StabilisedDenoiserModule, {"noise_level": ([0.1, 0.2, 0.3], 4.0), "inverse": "algebraic", "min_cells": 32}, _DENOISE),
    "burst": (bf.BurstDenoiserModule, {"reference": 1, "levels": 2, "search": 3, "sigma": 12.5, "k": (1.0, 2.5)}, _DENOISE),
    "video": (bf.VideoDenoiserModule, {"n_max": 5, "levels": 2, "search": 3, "sigma": 12.5, "k": (1.0, 2.5)}, _DENOISE),
    "nlm": (bf.NlmDenoiserModule, {"sigma": 7.0, "patch": 2, "search": 5, "strength": 0.4}, None),      # wraps nothing
}


def _same_setting(a, b) -> bool:
    if isinstance(a, (tuple, list)):
        return type(a) is type(b) and len(a) == len(b) and all(_same_setting(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and bool(np.all(np.asarray(a) == np.asarray(b)))


@pytest.mark.parametrize("case", sorted(_WRAPPER_CASES))
def test_every_wrapper_holds_the_base_protocol(case, module, monkeypatch):
    cls, settings, wrapped = _WRAPPER_CASES[case]
    wrapped = module if wrapped == "module" else wrapped
    w = cls(**settings) if cls is bf.NlmDenoiserModule else cls(wrapped, **settings)
    assert isinstance(w, bf.DenoiserWrapper) and tuple(cls.SETTINGS) == tuple(settings) and w._cast_to_uint8 is True
    assert w._module is wrapped and w._base is (module if wrapped is module else None)
    f = w.float_form()
    assert type(f) is cls and f is not w and f._cast_to_uint8 is False and f._module is w._module and f._base is w._base
    assert hasattr(f, "_record") == hasattr(w, "_record") and getattr(f, "_record", None) is getattr(w, "_record", None)
    assert case in ("self_ensemble", "stabilised") or isinstance(w._record, dict)             # the two that keep no record
    for name in cls.SETTINGS:
        assert _same_setting(getattr(f, name), getattr(w, name)) and getattr(w, name) is getattr(w, "_" + name)
        with pytest.raises(AttributeError):
            setattr(w, name, getattr(w, name))
    for name, value in settings.items():
        if case != "stabilised" or name != "noise_level":
            assert getattr(w, name) == value
    if case == "stabilised":
        assert w.noise_level[0].tolist() == [0.1, 0.2, 0.3] and float(w.noise_level[1]) == 4.0
    assert w.check_status() is True and f.check_status(wait=False) is True
    assert w.model_hydra is (module.model_hydra if wrapped is module else None)
    # a well-formed host tensor: there is nowhere to run it.  (Over a model that lives on the host the model says so itself)
    shape = (1, 2, 16, 16, 3) if case == "burst" else (1, 16, 16, 3)
    with pytest.raises(RuntimeError, match="no CPU execution path") as e:
        w(torch.zeros(shape, dtype=torch.uint8))
    assert wrapped is module or "must live on the GPU" in str(e.value)
    # an empty batch comes back before anything is placed or launched
    def touched(*args, **kwargs):
        raise AssertionError("an empty batch reached the GPU")
    monkeypatch.setattr(bf._native, "call", touched)
    monkeypatch.setattr(A, "to_device", touched)
    monkeypatch.setattr(type(module.model_hydra), "_require_gpu", touched)
    for given in (np.zeros((0,) + shape[1:], np.uint8), torch.zeros((0,) + shape[1:], dtype=torch.uint8)):
        for m in (w, f):
            out = m(given)
            assert type(out) is type(given) and tuple(out.shape) == (0, 16, 16, 3) and "uint8" in str(out.dtype)


# ---- load_model's options: each is parsed before anything is loaded ----------------------------------------------------------

@pytest.mark.parametrize("option, parse, unknown_key, wrong_type, bad_value, good", [
    ("self_ensemble", bf.self_ensemble.parse_setting, None, 3, [8], "flips"),               # not a dict option: no keys
    ("tiled", bf.tiling.parse_setting, {"tiles": 64}, "yes", {"tile": 0}, {"tile": 64}),
    ("pixel_shuffle", bf.pixel_shuffle.parse_setting, {"strides": 2}, 2.5, {"stride": 12}, 2),
    ("stabilise", bf.vst.parse_setting, None, "yes", (-1.0, 0.0), (0.5, 4.0)),               # not a dict option: no keys
    ("burst", bf.burst.parse_setting, {"n_max": 2}, "yes", {"levels": 9}, {"levels": 2}),
    ("video", bf.video_settings, {"reference": 0}, 3, {"n_max": 65}, {"n_max": 4}),
    ("nlm", bf.nlm_settings, {"radius": 2}, True, {"patch": 4}, {"patch": 2}),
])
def test_every_load_model_option_is_parsed_before_anything_is_loaded(option, parse, unknown_key, wrong_type, bad_value, good):
    path = "nlm" if option == "nlm" else "no such model"         # reaching the loader says "does not exist"
    for bad in (unknown_key, wrong_type, bad_value):
        if bad is None:
            continue
        with pytest.raises(ValueError) as e:
            parse(bad)
        assert "does not exist" not in str(e.value)
        with pytest.raises(ValueError) as e:
            bf.load_model(path, **{option: bad})
        assert "does not exist" not in str(e.value)
    if unknown_key is not None:
        with pytest.raises(ValueError, match=f"{option} may set"):
            parse(unknown_key)
    if option == "nlm":                                           # no wrapper but the model itself: None is its defaults
        assert parse(None) == {} and parse(good) == good
        return
    assert parse(None) is None and parse(good) is not None
    if option == "self_ensemble":                                 # the one option that is no switch: False names no transforms
        with pytest.raises(ValueError, match="transforms"):
            parse(False)
    else:
        assert parse(False) is None
    with pytest.raises(ValueError, match="does not exist"):       # a good value, and values that ask for no wrapper, reach the loader
        bf.load_model(path, **{option: good})
    with pytest.raises(ValueError, match="does not exist"):
        bf.load_model(path, **{option: None})


# ---- the import graph --------------------------------------------------------------------------------------------------------

def test_vst_imports_on_its_own_and_no_feature_module_imports_inside_a_function_to_dodge_a_cycle():
    done = subprocess.run([sys.executable, "-c", "import blind_image_denoising_amd.vst"], cwd=str(ROOT), capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    package = ROOT / "blind_image_denoising_amd"
    for name in ("vst", "risk", "self_ensemble", "neighbor", "noise_level", "noise_estimate"):
        tree = ast.parse((package / f"{name}.py").read_text())
        nested = [n for f in ast.walk(tree) if isinstance(f, (ast.FunctionDef, ast.AsyncFunctionDef)) for n in ast.walk(f)
                  if isinstance(n, (ast.Import, ast.ImportFrom))]
        assert not nested, (name, [ast.dump(n) for n in nested])
        helpers = [(n.module, a.name) for n in ast.walk(tree) if isinstance(n, ast.ImportFrom) and n.level == 1
                   for a in n.names if a.name.startswith("_") and n.module is not None]
        assert not helpers, (name, helpers)                      # underscore helpers come from _args / _native only (`from . import`)
