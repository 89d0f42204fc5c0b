"""tests/backward_reference.py against itself: every backward in it against central finite differences (step 1e-6) of its own
forward in float64, to 1e-6 of the largest gradient entry, on inputs kept at least 1e-3 away from every kink; the explicit tie
and clip rules on hand-written examples.  This is what keeps tests/test_gpu_backward_ops.py honest; it needs no GPU."""
import numpy as np
import pytest
import torch

import backward_reference as R

STEP, BAR, CLEAR = 1e-6, 1e-6, 1e-3


def _agree(got, fn, inputs, cot, which, what):
    num = R.numeric_vjp(fn, inputs, cot, which, STEP)
    got = np.asarray(got, np.float64)
    assert got.shape == num.shape, (what, got.shape, num.shape)
    err, scale = np.abs(got - num).max(), np.abs(num).max()
    assert scale > 0, what
    print(f"{what}: error {err:.3e}, bar {BAR * scale:.3e}")
    assert err <= BAR * scale, f"{what}: {err:.3e} vs {scale:.3e}"


def _away(rng, shape, kinks=(0.0,), scale=1.0):
    """normal values moved out of [kink - 2e-3, kink + 2e-3]"""
    x = rng.standard_normal(shape) * scale
    for k in kinks:
        near = np.abs(x - k) < 2 * CLEAR
        x[near] = k + np.where(x[near] >= k, 2 * CLEAR, -2 * CLEAR)
    for k in kinks:
        assert np.abs(x - k).min() >= CLEAR
    return x


@pytest.mark.parametrize("code,from_output", [(0, False), (1, False), (1, True), (2, False), (2, True), (3, False), (4, False), (4, True)])
def test_act_bwd(code, from_output):
    rng = np.random.default_rng(code)
    x, dy = _away(rng, 40), rng.standard_normal(40)
    ref = R.act(R.t64(x), code, 0.3).numpy() if from_output else x
    _agree(R.act_bwd(ref, dy, code, 0.3, from_output), lambda v: R.act(v, code, 0.3), [x], dy, 0, f"act {code}")


def test_act_bwd_at_zero_and_gelu_from_output():
    assert R.act_bwd([0.0, -0.0, 1.0], [2.0, 2.0, 2.0], 1).tolist() == [0.0, 0.0, 2.0]
    assert R.act_bwd([0.0, 1.0], [2.0, 2.0], 2, 0.25).tolist() == [0.5, 2.0]
    with pytest.raises(NotImplementedError):
        R.act_bwd([1.0], [1.0], 3, 0.0, True)


def test_multiplier_bwd():
    rng = np.random.default_rng(1)
    w = _away(rng, 30, kinks=(-1.0,), scale=1.5)
    assert (w < -1).any() and (w > -1).any()
    dm = rng.standard_normal(30)
    _agree(R.multiplier_bwd(w, dm), R.multiplier, [w], dm, 0, "multiplier")
    assert R.multiplier_bwd([-1.0, -2.0], [1.0, 1.0]).tolist() == [0.0, 0.0]


@pytest.mark.parametrize("with_m,with_s", [(True, True), (True, False), (False, True)])
def test_scale_add_bwd(with_m, with_s):
    rng = np.random.default_rng(2)
    t, dy = rng.standard_normal((3, 5, 4)), rng.standard_normal((3, 5, 4))
    m, s = (rng.standard_normal(4) if with_m else None), (rng.standard_normal(3) if with_s else None)
    dt, dm = R.scale_add_bwd(t, m, s, dy)
    mm = np.ones(4) if m is None else m
    fn = lambda a, b: R.scale_add(None, a, b, None if s is None else R.t64(s))
    _agree(dt, fn, [t, mm], dy, 0, "dt")
    _agree(dm, fn, [t, mm], dy, 1, "dm")


@pytest.mark.parametrize("soft", [0, 1])
def test_selector_mix_bwd(soft):
    rng = np.random.default_rng(3)
    u = _away(rng, 60, kinks=(0.0, 5.0), scale=4.0) + 0.0
    u[:4] = [-1.0, 1.0, 4.0, 6.0]                              # both sides of both clip ends
    assert R.kink_distance_selector(u) >= CLEAR
    x1, x2, dy = rng.standard_normal(60), rng.standard_normal(60), rng.standard_normal(60)
    got = R.selector_mix_bwd(x1, x2, u, dy, soft)
    for i, name in enumerate(("dx1", "dx2", "du")):
        _agree(got[i], lambda a, b, c: R.selector_mix(a, b, c, soft), [x1, x2, u], dy, i, name)


def test_selector_clip_passes_the_gradient_on_its_closed_interval():
    """u = 0 and u = 5 are the ends (0.2 (2.5 - u) + 0.5 = 1 and 0): the gradient passes there, not beyond"""
    u = np.array([0.0, 5.0, -1.0, 6.0, 2.5])
    _, _, du = R.selector_mix_bwd(np.full(5, 3.0), np.full(5, 1.0), u, np.ones(5), 0)
    assert np.allclose(du, [-0.4, -0.4, 0.0, 0.0, -0.4], rtol=0, atol=1e-15)


@pytest.mark.parametrize("b,high", [(1, 0), (2, 1), (4, 0), (16, 1)])
def test_pass_filter_bwd(b, high):
    rng = np.random.default_rng(b)
    x, dy = rng.standard_normal(30) * 0.5, rng.standard_normal(30)
    _agree(R.pass_filter_bwd(x, dy, 4.0, b, high), lambda v: R.pass_filter(v, 4.0, b, high), [x], dy, 0, "pass filter")


def test_center_scale_and_center_sq_bwd():
    rng = np.random.default_rng(4)
    x, m, v, dy = rng.standard_normal(30), rng.standard_normal(30), rng.random(30) + 0.1, rng.standard_normal(30)
    dd, dv = R.center_scale_bwd(x, m, v, dy, 1e-3)
    fn = lambda a, b, c: R.center_scale(a, b, c, 1e-3)
    _agree(dd, fn, [x, m, v], dy, 0, "dd")
    _agree(dv, fn, [x, m, v], dy, 2, "dv")
    # center_sq_bwd: the gradient at x of <dd, x - m> + <t, (x - m)^2>
    t = rng.standard_normal(30)
    num = R.numeric_vjp(lambda a: (a - R.t64(m), R.center_sq(a, R.t64(m))), [x], [dy, t], 0, STEP)
    got = R.center_sq_bwd(x, m, t, dy)
    assert np.abs(got - num).max() <= BAR * np.abs(num).max()


def test_local_normalization_recipe():
    """the chain of the GPU test (center_scale_bwd -> pool^T -> center_sq_bwd -> minus pool^T) against autograd and
    finite differences of the whole forward"""
    rng = np.random.default_rng(5)
    x, dy, pool, eps = rng.standard_normal((1, 5, 4, 2)), rng.standard_normal((1, 5, 4, 2)), (3, 3), 1e-3
    xt = R.t64(x)
    m = R.avgpool_same(xt, pool, (1, 1))
    v = R.avgpool_same(R.center_sq(xt, m), pool, (1, 1))
    dd, dv = R.center_scale_bwd(x, m.numpy(), v.numpy(), dy, eps)
    tot = R.center_sq_bwd(x, m.numpy(), R.avgpool_same_bwd(dv, x.shape, pool, (1, 1)), dd)
    dx = tot - R.avgpool_same_bwd(tot, x.shape, pool, (1, 1))
    _agree(dx, lambda a: R.local_normalization(a, pool, eps), [x], dy, 0, "local normalisation")


def test_sigmoid_gate_bwd():
    rng = np.random.default_rng(6)
    enc, o, dy = rng.standard_normal(30), rng.standard_normal(30) * 0.5, rng.standard_normal(30)
    denc, do = R.sigmoid_gate_bwd(enc, o, dy)
    fn = lambda a, b: R.sigmoid_gate(a, b, None)
    _agree(denc, fn, [enc, o], dy, 0, "denc")
    _agree(do, fn, [enc, o], dy, 1, "do")


@pytest.mark.parametrize("nw", [1, 6])
def test_relu_shift_bwd(nw):
    rng = np.random.default_rng(7)
    w0, dm = _away(rng, nw, kinks=(-0.25,)), rng.standard_normal(6)
    if nw == 1:
        w0[0] = 0.4
    _agree(R.relu_shift_bwd(w0, 0.25, dm), lambda a: R.relu_shift(a, 0.25, 6), [w0], dm, 0, "relu shift")
    assert R.relu_shift_bwd([-0.25], 0.25, dm).tolist() == [0.0]


@pytest.mark.parametrize("shape,k,gauss,stride", [((1, 2, 3, 2), 7, False, 2), ((1, 5, 4, 2), 2, False, 1), ((1, 5, 4, 2), 3, True, 2),
                                                  ((1, 4, 5, 1), 4, True, 1)])
def test_smooth_split_bwd(shape, k, gauss, stride):
    rng = np.random.default_rng(k)
    g = R.gaussian_window(k) if gauss else None
    B, H, W, C = shape
    dlap = rng.standard_normal(shape)
    dd = rng.standard_normal(shape if stride == 1 else (B, (H + 1) // 2, (W + 1) // 2, C))
    _agree(R.smooth_split_bwd(dlap, dd, k, g, stride), lambda v: R.smooth_split(v, k, g, stride), [rng.standard_normal(shape)],
           [dlap, dd], 0, "smooth split")


def test_resamplers_and_pooling_bwd():
    rng = np.random.default_rng(8)
    for bilinear in (0, 1):
        dy = rng.standard_normal((1, 6, 4, 2))
        _agree(R.upsample2x_bwd(dy, bilinear), lambda v: R.upsample2x(v, bilinear), [rng.standard_normal((1, 3, 2, 2))], dy, 0, "upsample")
    for (H, W), (oh, ow) in (((3, 4), (5, 3)), ((1, 1), (2, 3)), ((4, 3), (1, 1))):
        dy = rng.standard_normal((1, oh, ow, 2))
        _agree(R.resize_bilinear_bwd(dy, H, W), lambda v: R.resize_bilinear(v, oh, ow), [rng.standard_normal((1, H, W, 2))], dy, 0, "resize")
    for pool, stride, (H, W) in (((3, 3), (3, 3), (5, 4)), ((5, 5), (2, 2), (4, 3)), ((8, 8), (4, 4), (3, 2))):
        OH, OW = -(-H // stride[0]), -(-W // stride[1])
        dp = rng.standard_normal((1, OH, OW, 2))
        _agree(R.avgpool_same_bwd(dp, (1, H, W, 2), pool, stride), lambda v: R.avgpool_same(v, pool, stride),
               [rng.standard_normal((1, H, W, 2))], dp, 0, "avgpool")


def test_maxpool2_bwd_without_ties():
    rng = np.random.default_rng(9)
    x = rng.permutation(30).reshape(1, 5, 3, 2).astype(np.float64)          # distinct values, at least 1 apart; odd H and W
    dy = rng.standard_normal((1, 3, 2, 2))
    _agree(R.maxpool2_bwd(x, dy), lambda v: torch.from_numpy(R.maxpool2(v.numpy())), [x], dy, 0, "maxpool")


def test_maxpool2_bwd_tie_rule():
    """2 x 2 examples: the first maximum in the order (0,0), (0,1), (1,0), (1,1) takes the gradient"""
    one = np.ones((1, 1, 1, 1))
    case = lambda rows: R.maxpool2_bwd(np.array(rows, np.float64).reshape(1, 2, 2, 1), 7.0 * one).reshape(2, 2).tolist()
    assert case([[1, 1], [1, 1]]) == [[7, 0], [0, 0]]
    assert case([[0, 2], [2, 2]]) == [[0, 7], [0, 0]]
    assert case([[0, 1], [2, 2]]) == [[0, 0], [7, 0]]
    assert case([[0, 1], [2, 3]]) == [[0, 0], [0, 7]]
    assert case([[-np.inf, -np.inf], [-np.inf, -np.inf]]) == [[7, 0], [0, 0]]
    assert case([[-np.inf, 0], [0, -np.inf]]) == [[0, 7], [0, 0]]
    # a 3 x 3 map: partial windows at the odd edge, each input in exactly one window
    x = np.array([[5, 5, 1], [5, 5, 1], [2, 2, 2]], np.float64).reshape(1, 3, 3, 1)
    dy = np.array([[1, 2], [3, 4]], np.float64).reshape(1, 2, 2, 1)
    assert R.maxpool2_bwd(x, dy).reshape(3, 3).tolist() == [[1, 0, 2], [0, 0, 0], [3, 0, 4]]
    assert R.maxpool2(x).reshape(2, 2).tolist() == [[5, 1], [2, 2]]


@pytest.mark.parametrize("k,normalise", [(1, False), (3, True), (7, True)])
def test_conv2d_wgrad(k, normalise):
    rng = np.random.default_rng(k)
    x = rng.uniform(-40, 300, (1, 2, 3, 2)) if normalise else rng.standard_normal((1, 2, 3, 2))
    vr = (0.0, 255.0) if normalise else None
    dy = rng.standard_normal((1, 2, 3, 3))
    _agree(R.conv2d_wgrad(x, dy, k, 2, 3, vr), lambda w: R.conv2d(R.t64(x), w, vr), [rng.standard_normal((k, k, 2, 3))], dy, 0, "wgrad")


def test_dense2_bwd():
    rng = np.random.default_rng(10)
    p, w0, w1 = rng.standard_normal((4, 5)), rng.standard_normal((5, 3)), rng.standard_normal((3, 2))
    assert R.kink_distance_dense2(p, w0, w1, 0.3) >= CLEAR
    du = rng.standard_normal((4, 2))
    got = R.dense2_bwd(p, w0, w1, du, 0.3)
    for i, name in enumerate(("dp", "dw0", "dw1")):
        _agree(got[i], lambda a, b, c: R.dense2_selector(a, b, c, 0.3), [p, w0, w1], du, i, name)


@pytest.mark.parametrize("denormalize", [0, 1])
def test_head_out_bwd(denormalize):
    rng = np.random.default_rng(11)
    h, w1 = R.head_inputs(rng, 12, 8, 3, 1.5)
    assert R.kink_distance_head(h, w1) >= CLEAR
    p = R.head_p(R.t64(h), R.t64(w1)).numpy()
    assert (p > 0.5).any() and (p < -0.5).any() and (np.abs(p) < 0.5).any()
    dpred = rng.standard_normal((12, 3))
    dh, dw1 = R.head_out_bwd(h, w1, dpred, denormalize)
    fn = lambda a, b: R.head_out(a, b, denormalize)
    _agree(dh, fn, [h, w1], dpred, 0, "dh")
    _agree(dw1, fn, [h, w1], dpred, 1, "dw1")


def test_head_clip_passes_the_gradient_on_its_closed_interval():
    """three elements inside, above and below the clip: only the first hands its gradient on.  p = 0.51 tanh(2 h1) = 0.5 has
    no exact h1, so the ends themselves are tried on the bracket head_out_bwd uses"""
    h1 = np.array([[0.1], [3.0], [-3.0]])
    dh, dw1 = R.head_out_bwd(h1, np.ones((1, 1)), np.ones((3, 1)), 1)
    th = np.tanh(2.0 * h1)
    assert dh[1, 0] == 0.0 and dh[2, 0] == 0.0 and np.isclose(dh[0, 0], 255.0 * 1.02 * (1 - th[0, 0] ** 2), rtol=1e-15)
    assert np.isclose(dw1[0, 0], h1[0, 0] * dh[0, 0], rtol=1e-15)
    assert R.clip_passes([-0.5, 0.5, 0.0]).tolist() == [True, True, True]
    assert R.clip_passes([np.nextafter(-0.5, -1.0), np.nextafter(0.5, 1.0)]).tolist() == [False, False]
    # without denormalisation nothing is clipped
    assert np.all(R.head_out_bwd(h1, np.ones((1, 1)), np.ones((3, 1)), 0)[0] != 0.0)


@pytest.mark.parametrize("B,C,mults,hinge,emax", [(1, 1, (1.0, 0.0, 0.0), 0.0, 9.0), (2, 3, (0.0, 0.5, 0.0), 0.0, 9.0),
                                                  (1, 1, (0.0, 0.0, 1.0), 0.0, 20.0), (2, 1, (1.0, 0.5, 1.0), 3.5, 9.0)])
def test_denoiser_loss_grad(B, C, mults, hinge, emax):
    """SSIM alone: a dark image (grey levels 25..70, errors up to 20) on one 7 x 7 window.  Its gradient is small and its
    formula subtracts squares of the means, so on bright images the rounding of a float64 difference quotient (1e-16 of those
    squares over a step of 1e-6) comes within 1e6 of the gradient"""
    rng = np.random.default_rng(B + C)
    gt = rng.integers(*((25, 70) if emax > 9.0 else (70, 180)), (B, 7, 7, C)).astype(np.float64)
    e = rng.uniform(0.5, emax, gt.shape) * rng.choice([-1.0, 1.0], gt.shape)
    e[np.abs(np.abs(e) - hinge) < 0.01] += 0.05
    pred = gt - e
    ls = R.loss_spec(hinge, 255.0, *mults)
    assert R.kink_distance_loss(ls, gt, pred) >= CLEAR
    _, g = R.denoiser_loss_grad(ls, gt, pred, 0.5)
    _agree(g, lambda p: R.denoiser_loss(ls, R.t64(gt), p)["total_loss"] * 0.5, [pred], np.ones(()), 0, "loss")


def test_jvp_is_the_directional_derivative():
    """R.jvp supplies the J v of the GPU test's adjoint identities where no entry point computes it"""
    rng = np.random.default_rng(12)
    p, w0, w1 = R.dense2_inputs(rng, 4, 5, 2, 3, 0.3)
    fn = lambda a, b, c: R.dense2_selector(a, b, c, 0.3)
    v = [rng.standard_normal(a.shape) for a in (p, w0, w1)]
    at = lambda e: fn(*[R.t64(a.astype(np.float64) + e * t) for a, t in zip((p, w0, w1), v)]).numpy()
    num = (at(STEP) - at(-STEP)) / (2 * STEP)
    got = R.jvp(fn, [p, w0, w1], v)[0]
    assert np.abs(got - num).max() <= BAR * np.abs(num).max()
    h, w = R.head_inputs(rng, 5, 8, 2, 1.5)
    fn = lambda a, b: R.head_out(a, b, 1)
    v = [rng.standard_normal(a.shape) for a in (h, w)]
    at = lambda e: fn(*[R.t64(a.astype(np.float64) + e * t) for a, t in zip((h, w), v)]).numpy()
    num = (at(STEP) - at(-STEP)) / (2 * STEP)
    assert np.abs(R.jvp(fn, [h, w], v)[0] - num).max() <= BAR * np.abs(num).max()
