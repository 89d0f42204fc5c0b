"""The recursive temporal filter without a GPU: the consequences of the definition (tests/video_reference.py), the quality
experiment of DESIGN.md 7.20 on the reference, and every host-side error."""
import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import video as VI
import burst_reference as R
import video_reference as V


def _frame(shape, seed=0):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _random_state(B, H, W, C, n_max, seed):
    rng = np.random.default_rng(seed)
    acc = rng.integers(0, 65281, (B, H, W, C)).astype(np.uint16)
    cnt = rng.choice(np.array([0, 1, 255, 256, 700, 256 * n_max], np.int64), (B, H, W)).astype(np.uint16)
    return acc, cnt


# ---- the consequences of the definition --------------------------------------------------------------------------------------

def test_an_empty_state_passes_the_first_frame_whatever_field_and_acc_hold():
    x = _frame((2, 21, 35, 3))
    acc, _ = _random_state(2, 21, 35, 3, 8, 1)
    field = np.random.default_rng(2).integers(-40, 41, (2, 2, 3, 2)).astype(np.int32)
    for thr in (R.thresholds([0.0, 20.0], 3), np.array([[10 ** 12, 10 ** 12 + 1]] * 2, np.int64)):
        out, acc_out, cnt_out = V.update(x, acc, np.zeros((2, 21, 35), np.uint16), field, thr, 8)
        assert np.array_equal(acc_out, 256 * x.astype(np.uint16)) and (cnt_out == 256).all() and np.array_equal(out, x)
        flt, _, _ = V.update(x, acc, np.zeros((2, 21, 35), np.uint16), field, thr, 8, cast_to_uint8=False)
        assert flt.dtype == np.float32 and np.array_equal(flt, x.astype(np.float32))


def test_n_max_one_passes_every_frame_through():
    x = _frame((2, 21, 35, 3), 3)
    acc, cnt = _random_state(2, 21, 35, 3, 1, 4)
    out, acc_out, cnt_out = V.update(x, acc, cnt, np.zeros((2, 2, 3, 2), np.int32), np.array([[10 ** 12, 10 ** 12 + 1]] * 2, np.int64), 1)
    assert np.array_equal(out, x) and np.array_equal(acc_out, 256 * x.astype(np.uint16)) and (cnt_out == 256).all()
    frames = _frame((1, 4, 16, 16, 1), 5)
    outs, cnts, _ = V.run_sequence(frames, n_max=1, sigma=50.0)
    assert np.array_equal(outs, frames) and (cnts == 256).all()


def test_identical_frames_keep_the_frame_and_count_up_to_n_max():
    frame = _frame((1, 1, 21, 35, 3), 6)
    for n_max, sigma in ((3, 0.0), (5, 10.0)):
        frames = np.repeat(frame, n_max + 3, axis=1)
        acc, cnt = V.empty_state(1, 21, 35, 3)
        for t in range(n_max + 3):
            field = V.align(frames[:, t], V.state8(acc), 2, 2)
            assert t == 0 or not field.any()
            out, acc, cnt = V.update(frames[:, t], acc, cnt, field, R.thresholds([sigma], 3), n_max)
            assert np.array_equal(acc, 256 * frame[:, 0].astype(np.uint16)) and np.array_equal(out, frame[:, 0])
            assert (cnt == 256 * min(t + 1, n_max)).all()


def test_in_the_steady_state_a_new_frame_has_weight_one_over_n_max():
    everything = np.array([[10 ** 12, 10 ** 12 + 1]], np.int64)    # w = 256 everywhere
    field = np.zeros((1, 1, 1, 2), np.int32)
    for n_max in (2, 4, 8, 64):
        acc = np.full((1, 16, 16, 1), 256 * 64, np.uint16)
        cnt = np.full((1, 16, 16), 256 * n_max, np.uint16)
        x = np.full((1, 16, 16, 1), 128, np.uint8)
        _, acc_out, cnt_out = V.update(x, acc, cnt, field, everything, n_max)
        assert (cnt_out == 256 * n_max).all() and (acc_out == 256 * (64 * (n_max - 1) + 128) // n_max).all()      # exact: 64 | 256 * 64
    # and a mismatch restarts the pixel: w = 0 wherever the 5 x 5 window sees the change
    _, acc_out, cnt_out = V.update(x, acc, cnt, field, np.array([[0, 1]], np.int64), 8)
    assert (cnt_out == 256).all() and (acc_out == 256 * 128).all()


def test_weights_take_all_three_branches_at_the_thresholds():
    x = np.full((1, 16, 16, 1), 100, np.uint8)
    acc = np.full((1, 16, 16, 1), 256 * 100, np.uint16)
    acc[0, 8, 8, 0] = 256 * 110                                    # D = 100 in the 5 x 5 windows that hold (8, 8), else 0
    cnt = np.full((1, 16, 16), 256 * 3, np.uint16)
    field = np.zeros((1, 1, 1, 2), np.int32)
    for (lo, hi), w in (((100, 101), 256), ((99, 100), 0), ((0, 100), 0), ((0, 200), 128), ((99, 101), 128), ((50, 1 << 40), 255)):
        _, acc_out, cnt_out = V.update(x, acc, cnt, field, np.array([[lo, hi]], np.int64), 8)
        m = (w * 768) >> 8
        assert cnt_out[0, 8, 8] == 256 + m and cnt_out[0, 0, 0] == 1024, (lo, hi)
        assert acc_out[0, 8, 8, 0] == (65536 * 100 + m * 256 * 110 + ((256 + m) >> 1)) // (256 + m)
        assert acc_out[0, 0, 0, 0] == 25600


def test_the_state_moves_with_the_field():
    # the state holds a frame moved by (3, -2): with that field every interior pixel finds its history, with the zero field none
    big = np.kron(_frame((12, 12, 1), 7), np.ones((8, 8, 1), np.uint8))
    x, old = big[16:80, 16:80][None], big[16 + 3:80 + 3, 16 - 2:80 - 2][None]              # x(p) = old(p + (-3, 2))
    acc, cnt = 256 * old.astype(np.uint16), np.full((1, 64, 64), 512, np.uint16)
    field = V.align(x, old, 3, 4)
    assert (field[0, 1:3, 1:3] == (-3, 2)).all()
    thr = R.thresholds([0.0], 1)
    _, acc_out, cnt_out = V.update(x, acc, cnt, field, thr, 8)
    assert (cnt_out[0, 16:48, 16:48] == 768).all() and np.array_equal(acc_out[0, 16:48, 16:48], 256 * x[0, 16:48, 16:48].astype(np.uint16))
    _, _, cnt_zero = V.update(x, acc, cnt, np.zeros_like(field), thr, 8)
    assert (cnt_zero[0, 16:48, 16:48] == 256).mean() > 0.5


# ---- the quality experiment on the reference (lena 128 x 128, sigma 20, n_max 8, levels 3, search 4) ---------

@pytest.fixture(scope="module")
def lena():
    return R.load_lena()


def test_quality_aligned_against_unaligned_pan(lena):
    clean, noisy = V.pan_scene(lena, 10)
    aligned = V.run_sequence(noisy[None], 8, 3, 4, sigma=V.SIGMA)[0][0]
    unaligned = V.run_sequence(noisy[None], 8, 3, 4, sigma=V.SIGMA, aligned=False)[0][0]
    a, b, single = R.psnr(aligned[9], clean[9]), R.psnr(unaligned[9], clean[9]), R.psnr(noisy[9], clean[9])
    print(f"pan of (2, 3) per frame, frame 10: noisy {single:.2f} dB, unaligned {b:.2f} dB, aligned {a:.2f} dB; "
          f"aligned after 2 / 4 / 8 frames {[round(R.psnr(aligned[t], clean[t]), 2) for t in (1, 3, 7)]}")
    assert a >= b + 2.5                                             # measured 29.79 against 24.80: +4.99
    static_clean, static_noisy = V.pan_scene(lena, 12, step=(0, 0))
    static = V.run_sequence(static_noisy[None], 8, 3, 4, sigma=V.SIGMA)[0][0]
    print(f"static scene after 12 frames: {R.psnr(static[11], static_clean[11]):.2f} dB")          # measured 32.20


def test_quality_robust_against_plain_on_the_moving_square(lena):
    clean, noisy = V.square_scene(lena, 10)
    robust = V.run_sequence(noisy[None], 8, 3, 4, sigma=V.SIGMA)[0][0]
    plain = V.run_sequence(noisy[None], 8, 3, 4, thresholds=np.stack([V.PLAIN] * 10))[0][0]
    a, b = V.track_psnr(robust, clean), V.track_psnr(plain, clean)
    print(f"on the square's track: robust weights {a:.2f} dB, plain recursive mean {b:.2f} dB")
    assert a >= b + 3.6                                             # measured 25.32 against 18.11: +7.21


def test_quality_first_frame_after_a_scene_cut(lena):
    clean, noisy = V.cut_scene(lena, 8)
    outs, cnts, _ = V.run_sequence(noisy[None], 8, 3, 4, sigma=V.SIGMA)
    a, b = R.psnr(outs[0, 8], clean[8]), R.psnr(noisy[8], clean[8])
    print(f"first frame after the cut: filtered {a:.2f} dB, noisy {b:.2f} dB, {cnts[0, 8].mean() / 256.0:.2f} frames per pixel")
    # the state was all but full (a static pixel's D has a tail beyond lo = 1.5 E); the cut dropped about half of it
    assert cnts[0, 7].mean() > 0.9 * 2048 and cnts[0, 8].mean() < 0.6 * 2048
    assert a >= b + 0.19                                            # measured 22.71 against 22.32: +0.39 (other crops: DESIGN.md 7.20)


# ---- argument checks: everything raises before a GPU is needed ---------------------------------------------------------------

def _cpu_state(B, H, W, C):
    return bf.video_state(B, H, W, C, device="cpu")


def test_state_constructor():
    state = _cpu_state(2, 20, 36, 3)
    assert isinstance(state, bf.VideoState) and state.acc.dtype == torch.uint16 and tuple(state.acc.shape) == (2, 20, 36, 3)
    assert state.cnt.dtype == torch.uint16 and tuple(state.cnt.shape) == (2, 20, 36) and state.image.dtype == torch.uint8
    assert not state.acc.numpy().any() and not state.cnt.numpy().any() and not state.image.any()
    for bad in ((-1, 8, 8, 3), (1, 0, 8, 3), (1, 8, 8, 5), (1, 8, 8, 0), (1, 8.0, 8, 3)):
        with pytest.raises(ValueError):
            bf.video_state(*bad, device="cpu")


def test_update_argument_errors():
    good = np.zeros((2, 20, 36, 3), np.uint8)
    state = _cpu_state(2, 20, 36, 3)
    field, thr = torch.zeros((2, 2, 3, 2), dtype=torch.int32), torch.tensor([[0, 1], [5, 9]])
    for bad in (good[0], good[None], good.astype(np.float32), torch.zeros((2, 20, 36, 3)), np.zeros((2, 20, 36, 5), np.uint8), "x"):
        with pytest.raises(ValueError, match="x"):
            bf.video_update(bad, state, field, thr)
    for bad in (field[:1], field.long(), field[..., :1], field.numpy(), torch.zeros((2, 1, 2, 3, 2), dtype=torch.int32)):
        with pytest.raises(ValueError, match="field"):
            bf.video_update(good, state, bad, thr)
    for bad in (thr[:1], thr.int(), thr.reshape(4), [[0, 1], [5, 9]]):
        with pytest.raises(ValueError, match="thresholds"):
            bf.video_update(good, state, field, bad)
    for bad in (0, 65, 8.0, True):
        with pytest.raises(ValueError, match="n_max"):
            bf.video_update(good, state, field, thr, n_max=bad)
    other = _cpu_state(2, 20, 20, 3)
    for bad in (None, (state.acc, state.cnt), other, bf.VideoState(state.acc, state.cnt.to(torch.int32), state.image),
                bf.VideoState(state.acc.view(torch.int16), state.cnt, state.image), _cpu_state(1, 20, 36, 3)):
        with pytest.raises(ValueError, match="state"):
            bf.video_update(good, bad, field, thr)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        bf.video_update(torch.from_numpy(good), state, field, thr)
    out, same = bf.video_update(good[:0], _cpu_state(0, 20, 36, 3), field[:0], thr[:0], cast_to_uint8=False)      # launches nothing
    assert tuple(out.shape) == (0, 20, 36, 3) and out.dtype == torch.float32 and tuple(same.cnt.shape) == (0, 20, 36)


def test_module_argument_errors():
    denoise = lambda u8: u8.float()
    for bad in ({"n_max": 0}, {"n_max": 65}, {"n_max": 8.0}, {"levels": 0}, {"levels": 5}, {"search": 0}, {"search": 8},
                {"sigma": -1.0}, {"sigma": float("nan")}, {"sigma": "20"}, {"sigma": [[1.0]]}, {"k": (3.0, 1.5)}, {"k": (1.0, 1.0)},
                {"k": 2.0}, {"k": (1.0, 2.0, 3.0)}):
        with pytest.raises(ValueError, match=next(iter(bad)) if "k" not in bad else "k"):
            bf.VideoDenoiserModule(denoise, **bad)
    with pytest.raises(ValueError):
        bf.VideoDenoiserModule(42)
    module = bf.VideoDenoiserModule(denoise, n_max=5, levels=2, search=3, sigma=12.5, k=(1.0, 2.5))
    assert (module.n_max, module.levels, module.search, module.sigma, module.k) == (5, 2, 3, 12.5, (1.0, 2.5))
    assert module.last_counts is None and module.last_field is None and module.state is None
    assert module.check_status() is True and module.model_hydra is None
    for inner in (module, bf.BurstDenoiserModule(denoise)):
        with pytest.raises(ValueError, match="already merges frames"):
            bf.VideoDenoiserModule(inner)
    flt = module.float_form()
    assert isinstance(flt, bf.VideoDenoiserModule) and flt._cast_to_uint8 is False and flt._record is module._record
    assert (flt.n_max, flt.levels, flt.search, flt.sigma, flt.k) == (5, 2, 3, 12.5, (1.0, 2.5))
    defaults = bf.VideoDenoiserModule(None)
    assert (defaults.n_max, defaults.levels, defaults.search, defaults.sigma, defaults.k) == (8, 3, 4, None, (1.5, 3.0))
    for bad in (np.zeros((8, 8, 3), np.uint8), np.zeros((1, 8, 8, 3), np.float32), np.zeros((1, 8, 8, 5), np.uint8), "x"):
        with pytest.raises(ValueError, match="frame"):
            defaults(bad)
    for bad in (np.zeros((1, 8, 8, 3), np.uint8), np.zeros((1, 0, 8, 8, 3), np.uint8), np.zeros((1, 2, 8, 8, 3), np.float32)):
        with pytest.raises(ValueError, match="frames"):
            defaults.denoise_sequence(bad)
    with pytest.raises(ValueError, match="sigma"):
        bf.VideoDenoiserModule(None, sigma=[1.0, 2.0])(np.zeros((3, 8, 8, 3), np.uint8))
    empty = defaults(np.zeros((0, 8, 8, 3), np.uint8))
    assert isinstance(empty, np.ndarray) and empty.shape == (0, 8, 8, 3) and empty.dtype == np.uint8
    empty = defaults.denoise_sequence(np.zeros((0, 4, 8, 8, 3), np.uint8))
    assert isinstance(empty, np.ndarray) and empty.shape == (0, 4, 8, 8, 3) and empty.dtype == np.uint8
    tiled = bf.TiledDenoiserModule(denoise, tile=64, margin=3)
    assert bf.VideoDenoiserModule(bf.PixelShuffleDenoiserModule(tiled))._module._module is tiled       # the other wrappers go inside


def test_a_change_of_shape_raises_until_reset():
    module = bf.VideoDenoiserModule(None, sigma=5.0)
    module._record["state"] = _cpu_state(2, 8, 8, 3)              # as after a call on [2,8,8,3] frames
    for bad in (np.zeros((2, 8, 9, 3), np.uint8), np.zeros((1, 8, 8, 3), np.uint8), np.zeros((2, 8, 8, 1), np.uint8)):
        with pytest.raises(ValueError, match=r"reset\(\)"):
            module(bad)
        with pytest.raises(ValueError, match=r"reset\(\)"):
            module.float_form()(bad)
    assert module.last_counts is module.state.cnt
    module.reset()
    assert module.state is None and module.last_counts is None and module.last_field is None and module.float_form().state is None
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        module(torch.zeros((2, 8, 9, 3), dtype=torch.uint8))       # the shape passes now; a host tensor has no execution path


def test_load_model_checks_the_keyword_before_anything_is_loaded():
    for bad in ("yes", 3, [1], {"levels": 9}, {"search": 0}, {"n_max": 0}, {"n_max": 65}, {"k": (2.0, 1.0)}, {"sigma": -3.0},
                {"reference": 0}, {"cast_to_uint8": False}):
        with pytest.raises(ValueError, match="video"):
            bf.load_model("no such model", video=bad)               # the keyword is refused first
    with pytest.raises(ValueError, match="burst and video"):
        bf.load_model("no such model", video=True, burst=True)
    with pytest.raises(ValueError, match="burst and video"):
        bf.load_model("no such model", video={"n_max": 4}, burst={"levels": 2})
    with pytest.raises(ValueError, match="burst"):
        bf.load_model("no such model", video=True, burst={"levels": 9})
    with pytest.raises(ValueError, match="does not exist"):
        bf.load_model("no such model", video={"levels": 2, "sigma": 10.0, "n_max": 16})
    with pytest.raises(ValueError, match="does not exist"):
        bf.load_model("no such model", video=True, burst=False)
    assert VI.parse_setting(None) is None and VI.parse_setting(False) is None and VI.parse_setting(True) == {}
    assert VI.parse_setting({"n_max": 2, "k": (1.0, 2.0)}) == {"n_max": 2, "k": (1.0, 2.0)}
