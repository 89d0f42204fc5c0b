"""GPU tests of csrc/video.hip and VideoDenoiserModule.

Yardstick: tests/video_reference.py (with burst_reference for the alignment).  The kernel adds, compares and divides integers, and
its float32 output is an integer below 2^16 over 256: every comparison here is exact."""
import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import _native as N
from oracle import bfcnn_oracle as O
import burst_reference as R
import video_reference as V
from guarded import dev as _dev, guard_bands

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guard_bands")]

# (H, W, C) at B = 2.  5 x 7 is below a tile, 16 x 16 is one tile, 37 x 45 has cut edge tiles and, by its channels, rows of the
# state that start on no dword (C = 1, 3), on a dword for the halfwords alone (C = 2) and for the bytes too (C = 4); 64 x 96 has
# six tiles in a row (24 tiles in all: three to an XCD's share of the grid)
SHAPES = [(5, 7, 1), (5, 7, 3), (16, 16, 3), (37, 45, 1), (37, 45, 2), (37, 45, 3), (37, 45, 4), (64, 96, 3)]
_ids = {"ids": lambda c: "-".join(map(str, c))}


def _same(got, ref):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got, ref)


def _dev_state(acc, cnt):
    return bf.VideoState(_dev(acc), _dev(cnt), _dev(V.state8(acc)))


def _random_case(B, H, W, C, n_max, seed, reach=40):
    """frames of different content per image, a state with acc anywhere in 0..65280 and cnt including 0, 1, 255, 256 and 256 n_max,
    a field that reaches past the frame, and per image thresholds at the 30th and 70th percentile of the reference's D: all three
    weight branches are taken"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (B, H, W, C), dtype=np.uint8)
    acc = rng.integers(0, 65281, (B, H, W, C)).astype(np.uint16)
    acc[:, 0, 0], acc[:, -1, -1] = 0, 65280
    close = rng.random((B, H, W)) < 0.5                            # half of the state near the frame: small D next to large ones
    acc[close] = np.clip(256 * x[close].astype(np.int64) + rng.integers(-2000, 2001, x[close].shape), 0, 65280)
    cnt = rng.choice(np.array([0, 1, 255, 256, 257, 1000, 256 * n_max, 256 * n_max + 5, 65535], np.int64), (B, H, W)).astype(np.uint16)
    gy, gx = -(H // -16), -(W // -16)
    field = rng.integers(-reach, reach + 1, (B, gy, gx, 2)).astype(np.int32)
    field[0, 0, 0] = 0                                             # one tile where the close half matches
    thr = np.empty((B, 2), np.int64)
    for b in range(B):
        D = R.distances(np.stack([x[b], V.state8(acc[b])]), np.stack([np.zeros_like(field[b]), field[b]]), 0)[1]
        thr[b] = np.percentile(D, 30), max(np.percentile(D, 70), np.percentile(D, 30) + 1)
    return x, acc, cnt, field, thr


def _check_update(x, acc, cnt, field, thr, n_max):
    """both output forms of the update against the reference; returns the reference's (acc_out, cnt_out)"""
    state = _dev_state(acc, cnt)
    want_u8, want_acc, want_cnt = V.update(x, acc, cnt, field, thr, n_max, True)
    want_f32 = V.update(x, acc, cnt, field, thr, n_max, False)[0]
    out, new = bf.video_update(_dev(x), state, _dev(field), _dev(thr), n_max)
    assert out.is_cuda and _same(out, want_u8) and out is new.image, "uint8"
    assert _same(new.acc, want_acc) and _same(new.cnt, want_cnt), "state after the uint8 form"
    out, new = bf.video_update(_dev(x), state, _dev(field), _dev(thr), n_max, cast_to_uint8=False)
    assert _same(out, want_f32) and _same(new.image, want_u8) and _same(new.acc, want_acc) and _same(new.cnt, want_cnt), "float32"
    assert _same(state.acc, acc) and _same(state.cnt, cnt), "the step is not in place"
    return want_acc, want_cnt


# ---- the update against the reference ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_update_of_random_states_matches_numpy(shape):
    H, W, C = shape
    x, acc, cnt, field, thr = _random_case(2, H, W, C, 8, seed=sum(shape))
    _, want_cnt = _check_update(x, acc, cnt, field, thr, 8)
    if H >= 37:                                                     # the three weight branches, and a ramp
        assert (want_cnt == 256).any() and (want_cnt == 2048).any() and (want_cnt % 256 != 0).any()
    # an image inside a batch gets the bits of that image alone
    for b in range(2):
        _, alone = bf.video_update(_dev(x[b:b + 1]), _dev_state(acc[b:b + 1], cnt[b:b + 1]), _dev(field[b:b + 1]), _dev(thr[b:b + 1]), 8)
        want = V.update(x[b:b + 1], acc[b:b + 1], cnt[b:b + 1], field[b:b + 1], thr[b:b + 1], 8)
        assert _same(alone.acc, want[1]) and _same(alone.cnt, want[2]) and _same(alone.image, want[0])


@pytest.mark.parametrize("n_max", [1, 2, 64])
def test_update_at_the_ends_of_n_max(n_max):
    x, acc, cnt, field, thr = _random_case(2, 37, 45, 3, n_max, seed=n_max)
    want_acc, want_cnt = _check_update(x, acc, cnt, field, thr, n_max)
    assert want_cnt.max() == 256 * n_max
    if n_max == 1:
        assert np.array_equal(want_acc, 256 * x.astype(np.uint16))
    _check_update(x, acc, cnt, np.zeros_like(field), np.array([[10 ** 12, 10 ** 12 + 1]] * 2, np.int64), n_max)       # every weight 256


def test_update_of_an_empty_state_and_extreme_displacements():
    x, acc, cnt, field, thr = _random_case(2, 37, 45, 3, 8, seed=11)
    field[0, 0, 1], field[0, 2, 2], field[1, 1, 1] = (2 ** 31 - 1, -2 ** 31), (-2 ** 31, 2 ** 31 - 1), (2 ** 31 - 1, 2 ** 31 - 1)
    _check_update(x, acc, cnt, field, thr, 8)                       # clamp saturates
    want_acc, want_cnt = _check_update(x, acc, np.zeros_like(cnt), field, thr, 8)
    assert np.array_equal(want_acc, 256 * x.astype(np.uint16)) and (want_cnt == 256).all()
    out, new = bf.video_update(x, bf.video_state(2, 37, 45, 3), _dev(field), _dev(thr))           # NumPy frames are uploaded
    assert _same(out, x) and _same(new.cnt, want_cnt) and new.acc.is_cuda


def test_update_weight_branches_at_the_thresholds():
    x = np.full((6, 16, 20, 1), 100, np.uint8)
    image = x.copy()
    image[:, 8, 8] = 110                                            # D = 100 in the 5 x 5 windows that hold (8, 8), else 0
    acc, cnt = 256 * image.astype(np.uint16), np.full((6, 16, 20), 768, np.uint16)
    field = np.zeros((6, 1, 2, 2), np.int32)
    # D == lo; D == hi; ramp in 32 bits; ramp of two steps; ramp in 64 bits (hi - lo >= 2^23); all below lo near 2^40
    thr = np.array([[100, 101], [99, 100], [0, 200], [99, 101], [50, 1 << 40], [(1 << 40) - 7, (1 << 40) + 5]], np.int64)
    _, want_cnt = _check_update(x, acc, cnt, field, thr, 8)
    assert want_cnt[:, 8, 8].tolist() == [1024, 256, 640, 640, 1021, 1024] and (want_cnt[:, 0, 0] == 1024).all()
    x3, acc3 = np.repeat(x, 3, axis=-1), np.repeat(acc, 3, axis=-1)                          # three channels: D = 300
    thr3 = np.array([[300, 301], [299, 300], [0, 600], [299, 301], [50, 1 << 40], [0, 1]], np.int64)
    _, want_cnt = _check_update(x3, acc3, cnt, field, thr3, 8)
    assert want_cnt[:, 8, 8].tolist() == [1024, 256, 640, 640, 1021, 256]


def test_entry_point_refuses_overlap_and_bad_settings():
    x, acc, cnt, field, thr = _random_case(2, 16, 20, 3, 8, seed=5)
    d_x, state, d_field, d_thr = _dev(x), _dev_state(acc, cnt), _dev(field), _dev(thr)
    new = bf.VideoState(torch.empty_like(state.acc), torch.empty_like(state.cnt), torch.empty_like(d_x))
    flt = torch.empty((2, 16, 20, 3), dtype=torch.float32, device="cuda")
    entry = N.lib().bf_op_video_update

    def rc(x_=d_x, acc_in=state.acc, cnt_in=state.cnt, field_=d_field, thr_=d_thr, dims=(2, 16, 20, 3), n_max=8, acc_out=new.acc,
           cnt_out=new.cnt, image=new.image, out=None):
        return entry(N.ptr(x_), N.ptr(acc_in), N.ptr(cnt_in), N.ptr(field_), N.ptr(thr_), *dims, n_max, N.ptr(acc_out), N.ptr(cnt_out),
                     N.ptr(image), N.ptr(out), N.stream_ptr(d_x))

    assert rc() == N.BF_OK and rc(out=flt) == N.BF_OK
    assert rc(acc_out=state.acc) == N.BF_EINVAL and rc(cnt_out=state.cnt) == N.BF_EINVAL          # the step is not in place
    assert rc(acc_out=state.acc.view(-1)[6:]) == N.BF_EINVAL and rc(image=d_x) == N.BF_EINVAL
    assert rc(image=new.acc.view(torch.uint8)) == N.BF_EINVAL                                      # two outputs over each other
    for bad in ({"n_max": 0}, {"n_max": 65}, {"dims": (0, 16, 20, 3)}, {"dims": (2, 0, 20, 3)}, {"dims": (2, 16, 20, 5)},
                {"dims": (2, 16, 20, 0)}, {"x_": None}, {"acc_in": None}, {"cnt_in": None}, {"field_": None}, {"thr_": None},
                {"acc_out": None}, {"cnt_out": None}, {"image": None}):
        assert rc(**bad) == N.BF_EINVAL, bad
    torch.cuda.synchronize()


# ---- the module against the sequence driver ----------------------------------------------------------------------------------

def _texture(H, W, C, seed):
    """smooth blobs under 4 x 4 blocks: structure at every level of the pyramid"""
    rng = np.random.default_rng(seed)
    blocks = np.kron(rng.integers(0, 120, (-(H // -4), -(W // -4), C)), np.ones((4, 4, 1), np.int64))[:H, :W]
    yy, xx = np.mgrid[0:H, 0:W]
    blobs = 60 + 60 * np.sin(yy / 7.0 + seed)[..., None] * np.cos(xx / 5.0)[..., None]
    return np.clip(blocks + blobs, 0, 255).astype(np.uint8)


def _sequence(H, W, C, T, seed, shift=6, sigma=6.0, B=2):
    """B streams of different content: crops of a texture that wander within +-`shift` under noise of `sigma`"""
    rng = np.random.default_rng(seed)
    frames = np.empty((B, T, H, W, C), np.uint8)
    for b in range(B):
        big = _texture(H + 2 * shift, W + 2 * shift, C, seed + 17 * b)
        for t in range(T):
            dy, dx = rng.integers(0, 2 * shift + 1, 2)
            crop = big[dy:dy + H, dx:dx + W].astype(np.float64)
            frames[b, t] = np.clip(np.rint(crop + rng.normal(0.0, sigma, crop.shape)), 0, 255)
    return frames


def test_a_sequence_is_the_reference_driver_frame_by_frame():
    frames = _sequence(37, 45, 3, 6, seed=40)
    sigma = [5.0, 8.0]
    outs, cnts, fields = V.run_sequence(frames, n_max=4, levels=2, search=3, sigma=sigma, k=(1.0, 2.5))
    assert (cnts[:, -1] == 1024).any() and (cnts[:, -1] == 256).any() and fields[:, 1:].any()
    module = bf.VideoDenoiserModule(None, n_max=4, levels=2, search=3, sigma=sigma, k=(1.0, 2.5))
    for t in range(6):
        got = module(_dev(frames[:, t]))                            # device tensor in, device tensor out
        assert got.is_cuda and _same(got, outs[:, t]), t
        assert _same(module.last_counts, cnts[:, t]) and _same(module.last_field, fields[:, t]), t
    module.reset()
    for t in range(6):                                              # NumPy in, NumPy out; the float form shares the state
        call = module if t % 2 == 0 else module.float_form()
        got = call(frames[:, t])
        assert isinstance(got, np.ndarray)
        # the float form is acc / 256: floor(. + 0.5), exact in float32, is the uint8 form
        assert _same(got if t % 2 == 0 else np.floor(got + np.float32(0.5)).astype(np.uint8), outs[:, t]) and got.dtype == (np.uint8, np.float32)[t % 2], t
        assert _same(module.last_counts, cnts[:, t]), t
    assert _same(module.denoise_sequence(frames), outs) and _same(module.last_counts, cnts[:, -1])
    got = module.denoise_sequence(_dev(frames))
    assert got.is_cuda and _same(got, outs)
    assert module.denoise_sequence(frames[:0]).shape == (0, 6, 37, 45, 3)


def test_float_form_is_the_state_before_rounding():
    frames = _sequence(37, 45, 3, 3, seed=41)
    flt = bf.VideoDenoiserModule(None, sigma=6.0, cast_to_uint8=False)
    acc, cnt = V.empty_state(2, 37, 45, 3)
    for t in range(3):
        field = V.align(frames[:, t], V.state8(acc))
        want, acc, cnt = V.update(frames[:, t], acc, cnt, field, R.thresholds([6.0, 6.0], 3), 8, cast_to_uint8=False)
        assert _same(flt(_dev(frames[:, t])), want), t


def test_a_sequence_with_sigma_estimated_on_the_device():
    frames = _sequence(64, 96, 3, 6, seed=42, sigma=10.0)
    thr = np.stack([bf.burst_thresholds(bf.estimate_noise(_dev(frames[:, t]), "mad"), 3).cpu().numpy() for t in range(6)])
    outs, cnts, fields = V.run_sequence(frames, thresholds=thr)
    module = bf.VideoDenoiserModule(None)
    for t in range(6):
        assert _same(module(_dev(frames[:, t])), outs[:, t]), t
        assert _same(module.last_counts, cnts[:, t]) and _same(module.last_field, fields[:, t]), t
    assert (cnts[:, -1] == 6 * 256).any()


def test_reset_and_the_shape_change_error():
    frames = _sequence(37, 45, 3, 3, seed=43)
    outs, cnts, _ = V.run_sequence(frames, sigma=6.0)
    module = bf.VideoDenoiserModule(None, sigma=6.0)
    assert module.state is None and _same(module(frames[:, 0]), frames[:, 0]) and (module.last_counts.cpu().numpy() == 256).all()
    assert _same(module(frames[:, 1]), outs[:, 1])
    for bad in (frames[:1, 2], frames[:, 2, :, :40], frames[:, 2, :, :, :1]):
        with pytest.raises(ValueError, match=r"reset\(\)"):
            module(bad)
        with pytest.raises(ValueError, match=r"reset\(\)"):
            module(_dev(bad))
    assert _same(module(frames[:, 2]), outs[:, 2]) and _same(module.last_counts, cnts[:, 2])       # the refused frames left the state alone
    module.reset()
    assert module.state is None and module.last_counts is None and module.last_field is None
    small = np.ascontiguousarray(frames[:1, 2, :20])
    assert _same(module(small), small) and tuple(module.state.acc.shape) == (1, 20, 45, 3)


# ---- the module around a callable and a real model ---------------------------------------------------------------------------

def _callable_denoiser(u8):
    return u8.float() * 0.5 + 3.25


def test_module_around_a_callable_is_the_reference_pipeline():
    frames = _sequence(37, 45, 3, 3, seed=44)
    outs, _, _ = V.run_sequence(frames, sigma=6.0)
    module = bf.VideoDenoiserModule(_callable_denoiser, sigma=6.0)
    for t in range(3):
        want = outs[:, t].astype(np.float32) * np.float32(0.5) + np.float32(3.25)
        got = module(frames[:, t]) if t < 2 else module.float_form()(_dev(frames[:, t]))
        assert _same(got, np.rint(np.clip(want, 0.0, 255.0)).astype(np.uint8) if t < 2 else want), t
    assert module.check_status() is True


_MODEL = []


def _resnet():
    if not _MODEL:
        cfg = bf.CONFIGS_DICT["resnet_color_1x6_bn_16x3x3_256x256_l1_relu"]          # the shipped 1x6 configuration
        spec = O.ResnetSpec.from_config(cfg["model"])
        params, state = O.init_params(spec, seed=42)
        m = bf.model_builder(cfg["model"], device="cuda").hydra
        m.set_weights(params, state)
        _MODEL.append(m)
    return _MODEL[0]


def test_first_frame_and_n_max_one_are_the_wrapped_module():
    module = bf.DenoiserModule(_resnet())
    frames = _dev(_sequence(32, 48, 3, 3, seed=45))
    video = bf.VideoDenoiserModule(module, sigma=6.0)
    assert torch.equal(video(frames[:, 0].contiguous()), module(frames[:, 0].contiguous())) and video.check_status() is True
    assert not torch.equal(video(frames[:, 1].contiguous()), module(frames[:, 1].contiguous()))     # the second frame is filtered
    video.reset()
    assert np.array_equal(video(frames[:, 1].cpu().numpy()), module(frames[:, 1].cpu().numpy()))
    video.reset()
    assert torch.equal(video.float_form()(frames[:, 2].contiguous()), module.float_form()(frames[:, 2].contiguous()))
    passing = bf.VideoDenoiserModule(module, n_max=1, sigma=6.0)
    for t in range(3):
        assert torch.equal(passing(frames[:, t].contiguous()), module(frames[:, t].contiguous())), t
    assert passing(frames[:0, 0]).shape == (0, 32, 48, 3) and passing.check_status() is True


def test_real_model_is_the_hand_built_pipeline_and_stacks_over_tiles():
    module = bf.DenoiserModule(_resnet())
    frames = _dev(_sequence(32, 48, 3, 3, seed=46))
    alone = bf.VideoDenoiserModule(None, sigma=6.0)
    filtered = [alone(frames[:, t].contiguous()) for t in range(3)]
    video = bf.VideoDenoiserModule(module, sigma=6.0)
    tiled = bf.TiledDenoiserModule(module, tile=16, overlap=8, margin=2, tile_batch=8)
    stacked = bf.VideoDenoiserModule(tiled, sigma=6.0)
    for t in range(3):
        assert torch.equal(video(frames[:, t].contiguous()), module(filtered[t])), t
        assert torch.equal(stacked(frames[:, t].contiguous()), tiled(filtered[t])), t
    assert tiled.last_plan.tiles > 1 and video.check_status() is True and stacked.check_status() is True
    assert _same(video.last_counts, alone.last_counts.cpu().numpy()) and torch.equal(stacked.last_field, alone.last_field)
    want = torch.stack([module(f) for f in filtered], dim=1)
    assert torch.equal(video.denoise_sequence(frames), want)
    assert np.array_equal(video.denoise_sequence(frames.cpu().numpy()), want.cpu().numpy())


def test_a_call_replays_from_a_graph():
    module = bf.DenoiserModule(_resnet())
    frames = _dev(_sequence(32, 48, 3, 3, seed=47))
    first, a, b = (frames[:, t].contiguous() for t in range(3))

    def fresh():
        video = bf.VideoDenoiserModule(module, sigma=6.0)
        video(first)
        return video

    want_a, want_b = fresh()(a), fresh()(b)                        # direct calls (also the warm-up: packing, workspace, attributes)
    video = fresh()                                                 # the state a replay starts from: the step is not in place
    static_in = a.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = video(static_in)
    # the module's state is now the capture's output; the state the capture READ must outlive it (the module keeps it).  New
    # tensors of the sizes of acc, cnt and image would land on its memory if the allocator had got it back
    churn = [torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda") for n in (18432, 6144, 9216) for _ in range(6)]
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out, want_a)
    static_in.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out, want_b) and not torch.equal(want_a, want_b)


def test_load_model_wraps_video_outermost(tmp_path):
    bf.save_model(_resnet(), str(tmp_path / "m"))
    frames = _sequence(32, 48, 3, 2, seed=48)
    loaded = bf.load_model(str(tmp_path / "m"), device="cuda", video={"sigma": 6.0, "n_max": 4})
    assert type(loaded) is bf.VideoDenoiserModule and type(loaded._module) is bf.DenoiserModule and loaded.n_max == 4
    mine = bf.VideoDenoiserModule(bf.DenoiserModule(_resnet()), sigma=6.0, n_max=4)
    for t in range(2):
        assert np.array_equal(loaded(frames[:, t]), mine(frames[:, t])) and loaded.check_status()
    assert type(bf.load_model(str(tmp_path / "m"), device="cuda", video=False)) is bf.DenoiserModule
    full = bf.load_model(str(tmp_path / "m"), device="cuda", tiled={"tile": 16, "overlap": 8, "margin": 2}, stabilise=True, video=True)
    assert type(full) is bf.VideoDenoiserModule and type(full._module) is bf.StabilisedDenoiserModule
    assert type(full._module._module) is bf.TiledDenoiserModule
    out = full.denoise_sequence(frames)
    assert out.shape == (2, 2, 32, 48, 3) and out.dtype == np.uint8 and full.check_status() and full.last_counts.shape == (2, 32, 48)
