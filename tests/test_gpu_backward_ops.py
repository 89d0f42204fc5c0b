"""Every small training operator of csrc/train_prims.hip and csrc/train_generic.hip called on its own through N.lib(), at the
shapes where such kernels go wrong (one element, a tail, a second trip of the grid-stride loop, more channels than threads, an
image smaller than the window, ties), against the float64 restatement of tests/backward_reference.py (itself checked against
finite differences by tests/test_backward_reference.py).

Each case makes two checks.  (a) output and gradient against the reference: 2e-5 of the reference's largest entry for forwards
and element-wise results, 5e-5 for gradients that sum over pixels (the bars of tests/test_gpu_train_steps.py).  (b) an adjoint
identity <A x, y> = <x, A^T y>, both sides summed in float64 from the float32 results, to 1e-5 of the sum of the absolute terms
of the inner product (at most 49 taps, each rounded at 6e-8, with a threefold margin; the larger of the two sides' sums is
taken, which the sum over the single taps still bounds).  A x comes from the forward entry point where there is one, for an
element-wise backward (a diagonal Jacobian) from the backward itself on a second vector, and otherwise from the float64
forward-mode derivative of the reference.  Layout helpers are compared bit for bit.

No element is left out of a comparison: inputs are built so that nothing lies within 1e-3 of a kink in the float64 reference,
and each test asserts that.  Exactly at a kink only what is exactly representable is tested: integer ties in the max-pool and
zero for ReLU."""
import ctypes as C

import numpy as np
import pytest
import torch

from blind_image_denoising_amd import _native as N

import backward_reference as R

pytestmark = pytest.mark.gpu

FWD, GRAD, ADJ, CLEAR = 2e-5, 5e-5, 1e-5, 1e-3
SENTINEL = 1.0e30
# one element, a tail below and above one workgroup, and one above what a single pass of tp_grid / tg_grid covers (4096 x 256)
NS = (1, 255, 257, 4096 * 256 + 3)
MAPS = ((1, 1), (1, 5), (2, 3), (7, 9), (12, 10))


def _d(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _e(*shape):
    """an output buffer, filled with the sentinel: an element that the kernel leaves out shows"""
    return torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda")


def _f32(rng, shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _h(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().astype(np.float64)


def _scratch(floats):
    """a scratch buffer filled with a large sentinel: a partial sum that is never written cannot pass by luck"""
    return torch.full((max(int(floats), 1),), SENTINEL, dtype=torch.float32, device="cuda")


def _ok(rc, what):
    N.check(rc, None, what)


def _close(got, ref, rel, what):
    got = _h(got) if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref = np.asarray(ref.detach() if torch.is_tensor(ref) else ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, scale = np.abs(got - ref).max(), max(1e-6, np.abs(ref).max())
    print(f"{what}: error {err:.3e}, bar {rel * scale:.3e}")
    assert err <= rel * scale, f"{what}: {err:.3e} vs {scale:.3e}"


def _adjoint(left, right, what):
    """left, right: lists of (a, b) pairs; sum <a, b> over the left pairs equals the sum over the right pairs"""
    def side(pairs):
        terms = [(_h(a) if torch.is_tensor(a) else np.asarray(a, np.float64)).reshape(-1) *
                 (_h(b) if torch.is_tensor(b) else np.asarray(b, np.float64)).reshape(-1) for a, b in pairs]
        return sum(t.sum() for t in terms), sum(np.abs(t).sum() for t in terms)
    (l, la), (r, ra) = side(left), side(right)
    bar = ADJ * max(la, ra, 1e-30)
    print(f"{what}: <A x, y> {l:.9e}, <x, A^T y> {r:.9e}, bar {bar:.3e}")
    assert abs(l - r) <= bar, f"{what}: {l!r} vs {r!r} (bar {bar:.3e})"


def _away(rng, n, kinks, scale=1.0):
    """float32 normal values moved out of [kink - 2e-3, kink + 2e-3]; the clearance is asserted by the caller"""
    x = _f32(rng, n, scale)
    for k in kinks:
        near = np.abs(x.astype(np.float64) - k) < 2 * CLEAR
        x[near] = np.float32(k) + np.where(x[near] >= k, np.float32(2 * CLEAR), np.float32(-2 * CLEAR))
    return x


# ---- element-wise operators ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("code,from_output", [(1, 1), (1, 0), (2, 1), (2, 0), (4, 1), (4, 0), (3, 0)])
def test_act_bwd(code, from_output, n):
    rng, L = np.random.default_rng(code * 7 + n % 13), N.lib()
    x = _away(rng, n, (0.0,))
    assert np.abs(x.astype(np.float64)).min() >= CLEAR
    ref = R.act(R.t64(x), code, 0.3).numpy().astype(np.float32) if from_output else x
    dy, v = _f32(rng, n), _f32(rng, n)
    refd, dyd, vd, dx, jv = _d(ref), _d(dy), _d(v), _e(n), _e(n)
    _ok(L.bf_op_act_bwd(N.ptr(refd), N.ptr(dyd), N.ptr(dx), n, code, 0.3, from_output, N.stream_ptr(dx)), "act_bwd")
    _ok(L.bf_op_act_bwd(N.ptr(refd), N.ptr(vd), N.ptr(jv), n, code, 0.3, from_output, N.stream_ptr(dx)), "act_bwd")
    _close(dx, R.act_bwd(ref, dy, code, 0.3, bool(from_output)), FWD, "dx")
    _adjoint([(jv, dy)], [(v, dx)], "diagonal Jacobian")


def test_act_bwd_linear_gelu_from_output_and_relu_at_zero():
    """code 0 hands dy through; GELU cannot be differentiated from its output: BF_EUNSUPPORTED; relu'(0) = 0, leaky'(0) = alpha"""
    L = N.lib()
    dy = _f32(np.random.default_rng(0), 257)
    refd, dyd, dx = _d(dy[::-1]), _d(dy), _e(257)
    _ok(L.bf_op_act_bwd(N.ptr(refd), N.ptr(dyd), N.ptr(dx), 257, 0, 0.3, 0, N.stream_ptr(dx)), "act_bwd")
    assert np.array_equal(_h(dx), dy.astype(np.float64))
    assert L.bf_op_act_bwd(N.ptr(refd), N.ptr(dyd), N.ptr(dx), 257, 3, 0.3, 1, N.stream_ptr(dx)) == N.BF_EUNSUPPORTED
    assert L.bf_op_act_bwd(N.ptr(refd), N.ptr(dyd), N.ptr(dx), 257, 5, 0.3, 0, N.stream_ptr(dx)) == N.BF_EUNSUPPORTED
    zero, two, out = _d([0.0, -0.0, 1.0, -1.0]), _d([2.0, 2.0, 2.0, 2.0]), _e(4)
    for code, from_output in ((1, 0), (1, 1), (2, 0), (2, 1)):
        _ok(L.bf_op_act_bwd(N.ptr(zero), N.ptr(two), N.ptr(out), 4, code, 0.25, from_output, N.stream_ptr(out)), "act_bwd")
        assert np.array_equal(_h(out), R.act_bwd([0.0, -0.0, 1.0, -1.0], [2.0] * 4, code, 0.25, bool(from_output))), (code, from_output)


@pytest.mark.parametrize("n", NS)
def test_multiplier_bwd(n):
    rng, L = np.random.default_rng(n % 11), N.lib()
    w = _away(rng, n, (-1.0,), 1.5)
    w[:2] = [-1.5, 0.5][:min(n, 2)]
    assert np.abs(1.0 + w.astype(np.float64)).min() >= CLEAR
    assert n < 2 or ((w < -1).any() and (w > -1).any())
    dm, v = _f32(rng, n), _f32(rng, n)
    wd, dmd, vd, dw, jv = _d(w), _d(dm), _d(v), _e(n), _e(n)
    _ok(L.bf_op_multiplier_bwd(N.ptr(wd), N.ptr(dmd), N.ptr(dw), n, N.stream_ptr(dw)), "multiplier_bwd")
    _ok(L.bf_op_multiplier_bwd(N.ptr(wd), N.ptr(vd), N.ptr(jv), n, N.stream_ptr(dw)), "multiplier_bwd")
    _close(dw, R.multiplier_bwd(w, dm), FWD, "dw")
    _adjoint([(jv, dm)], [(v, dw)], "diagonal Jacobian")


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("soft", [0, 1])
def test_selector_mix_and_bwd(soft, n):
    rng, L = np.random.default_rng(soft + n % 17), N.lib()
    u = _f32(rng, n, 4.0) + np.float32(2.5)                          # about a quarter beyond each clip end
    u[np.minimum(np.abs(u), np.abs(u - 5.0)) < 2 * CLEAR] += np.float32(4 * CLEAR)
    u[:4] = np.array([-1.0, 1.0, 4.0, 6.0], np.float32)[:min(n, 4)]  # both sides of both clip ends
    assert R.kink_distance_selector(u) >= CLEAR
    x1, x2, dy, v = _f32(rng, n), _f32(rng, n), _f32(rng, n), _f32(rng, n)
    a, b, c, g, vd = _d(x1), _d(x2), _d(u), _d(dy), _d(v)
    out, dx1, dx2, du, j1, j2, ju = (_e(n) for _ in range(7))
    _ok(L.bf_op_selector_mix(N.ptr(a), N.ptr(b), N.ptr(c), N.ptr(out), n, soft, N.stream_ptr(a)), "selector_mix")
    _ok(L.bf_op_selector_mix_bwd(N.ptr(a), N.ptr(b), N.ptr(c), N.ptr(g), N.ptr(dx1), N.ptr(dx2), N.ptr(du), n, soft, N.stream_ptr(a)),
        "selector_mix_bwd")
    _ok(L.bf_op_selector_mix_bwd(N.ptr(a), N.ptr(b), N.ptr(c), N.ptr(vd), N.ptr(j1), N.ptr(j2), N.ptr(ju), n, soft, N.stream_ptr(a)),
        "selector_mix_bwd")
    _close(out, R.selector_mix(R.t64(x1), R.t64(x2), R.t64(u), soft), FWD, "out")
    for got, ref, name in zip((dx1, dx2, du), R.selector_mix_bwd(x1, x2, u, dy, soft), ("dx1", "dx2", "du")):
        _close(got, ref, FWD, name)
    # out is linear in (x1, x2): <mix(v, v'), dy> = <v, dx1> + <v', dx2> with the forward itself as A
    v2 = _f32(rng, n)
    v2d, lin = _d(v2), _e(n)
    _ok(L.bf_op_selector_mix(N.ptr(vd), N.ptr(v2d), N.ptr(c), N.ptr(lin), n, soft, N.stream_ptr(a)), "selector_mix")
    _adjoint([(lin, dy)], [(v, dx1), (v2, dx2)], "mix in x1, x2")
    _adjoint([(ju, dy)], [(v, du)], "diagonal Jacobian in u")


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("b,high", [(1, 0), (1, 1), (2, 0), (2, 1), (16, 0), (16, 1)])
def test_pass_filter_and_bwd(b, high, n):
    """a = 4 and x of standard deviation 0.5, so that tanh(a x) runs from 0 into saturation.  There 1 - tanh^b cancels in float32:
    its rounding, 6e-8, is 1e-4 of a result of 6e-4, which is nothing against the largest of many entries but would be all of a
    single element's bar; the one-element case is therefore placed at x = 0.3 (tanh 0.83)"""
    rng, L = np.random.default_rng(b + high + n % 19), N.lib()
    x, dy, v = _f32(rng, n, 0.5), _f32(rng, n), _f32(rng, n)
    if n == 1:
        x[0] = np.float32(0.3)
    xd, dyd, vd, out, dx, jv = _d(x), _d(dy), _d(v), _e(n), _e(n), _e(n)
    _ok(L.bf_op_pass_filter(N.ptr(xd), N.ptr(out), n, 4.0, b, high, N.stream_ptr(xd)), "pass_filter")
    _ok(L.bf_op_pass_filter_bwd(N.ptr(xd), N.ptr(dyd), N.ptr(dx), n, 4.0, b, high, N.stream_ptr(xd)), "pass_filter_bwd")
    _ok(L.bf_op_pass_filter_bwd(N.ptr(xd), N.ptr(vd), N.ptr(jv), n, 4.0, b, high, N.stream_ptr(xd)), "pass_filter_bwd")
    _close(out, R.pass_filter(R.t64(x), 4.0, b, high), FWD, "out")
    _close(dx, R.pass_filter_bwd(x, dy, 4.0, b, high), FWD, "dx")
    _adjoint([(jv, dy)], [(v, dx)], "diagonal Jacobian")


def test_pass_filter_refuses_an_exponent_outside_1_to_16():
    L, t = N.lib(), _e(4)
    for b in (0, 17):
        assert L.bf_op_pass_filter(N.ptr(t), N.ptr(t), 4, 4.0, b, 0, N.stream_ptr(t)) == N.BF_EINVAL
        assert L.bf_op_pass_filter_bwd(N.ptr(t), N.ptr(t), N.ptr(t), 4, 4.0, b, 0, N.stream_ptr(t)) == N.BF_EINVAL


@pytest.mark.parametrize("n", NS)
def test_center_scale_and_its_adjoints(n):
    rng, L, eps = np.random.default_rng(n % 23), N.lib(), 1e-3
    x, m, dy, t, v = _f32(rng, n), _f32(rng, n), _f32(rng, n), _f32(rng, n), _f32(rng, n)
    var = (rng.random(n) + 0.1).astype(np.float32)
    xd, md, vard, dyd, td, vd = _d(x), _d(m), _d(var), _d(dy), _d(t), _d(v)
    sq, out, dd, dv, tot, jd, jvv = (_e(n) for _ in range(7))
    _ok(L.bf_op_center_scale(N.ptr(xd), N.ptr(md), None, N.ptr(sq), n, eps, N.stream_ptr(xd)), "center_scale")
    _ok(L.bf_op_center_scale(N.ptr(xd), N.ptr(md), N.ptr(vard), N.ptr(out), n, eps, N.stream_ptr(xd)), "center_scale")
    _ok(L.bf_op_center_scale_bwd(N.ptr(xd), N.ptr(md), N.ptr(vard), N.ptr(dyd), N.ptr(dd), N.ptr(dv), n, eps, N.stream_ptr(xd)), "center_scale_bwd")
    _ok(L.bf_op_center_scale_bwd(N.ptr(xd), N.ptr(md), N.ptr(vard), N.ptr(vd), N.ptr(jd), N.ptr(jvv), n, eps, N.stream_ptr(xd)), "center_scale_bwd")
    _ok(L.bf_op_center_sq_bwd(N.ptr(xd), N.ptr(md), N.ptr(td), N.ptr(dd), N.ptr(tot), n, N.stream_ptr(xd)), "center_sq_bwd")
    _close(sq, R.center_sq(R.t64(x), R.t64(m)), FWD, "(x - m)^2")
    _close(out, R.center_scale(R.t64(x), R.t64(m), R.t64(var), eps), FWD, "(x - m) / sqrt(v + eps)")
    rdd, rdv = R.center_scale_bwd(x, m, var, dy, eps)
    _close(dd, rdd, FWD, "dd")
    _close(dv, rdv, FWD, "dv")
    _close(tot, R.center_sq_bwd(x, m, t, _h(dd)), FWD, "dd + 2 (x - m) t")
    _adjoint([(jd, dy)], [(v, dd)], "diagonal Jacobian in d")
    _adjoint([(jvv, dy)], [(v, dv)], "diagonal Jacobian in v")


@pytest.mark.parametrize("shape,pool", [((2, 7, 9, 4), (3, 3)), ((1, 2, 3, 8), (5, 5)), ((2, 12, 10, 4), (4, 2))])
def test_local_normalisation_chain(shape, pool):
    """avgpool_same -> center_scale(var NULL) -> avgpool_same -> center_scale, and its backward by the recipe of train_generic.hip
    (center_scale_bwd; t = pool^T dv; center_sq_bwd; minus pool^T of that): the whole dx against autograd"""
    rng, L, eps = np.random.default_rng(sum(shape)), N.lib(), 1e-3
    B, H, W, Cc = shape
    x, dy = _f32(rng, shape), _f32(rng, shape)
    n = x.size
    xd, dyd = _d(x), _d(dy)
    mean, sq, var, y, dd, dv, t, tot, back = (_e(*shape) for _ in range(9))
    s = N.stream_ptr(xd)
    pool_args = (B, H, W, Cc, pool[0], pool[1], 1, 1)
    _ok(L.bf_op_avgpool_same(N.ptr(xd), N.ptr(mean), *pool_args, s), "avgpool_same")
    _ok(L.bf_op_center_scale(N.ptr(xd), N.ptr(mean), None, N.ptr(sq), n, eps, s), "center_scale")
    _ok(L.bf_op_avgpool_same(N.ptr(sq), N.ptr(var), *pool_args, s), "avgpool_same")
    _ok(L.bf_op_center_scale(N.ptr(xd), N.ptr(mean), N.ptr(var), N.ptr(y), n, eps, s), "center_scale")
    _ok(L.bf_op_center_scale_bwd(N.ptr(xd), N.ptr(mean), N.ptr(var), N.ptr(dyd), N.ptr(dd), N.ptr(dv), n, eps, s), "center_scale_bwd")
    _ok(L.bf_op_avgpool_same_bwd(N.ptr(dv), N.ptr(t), *pool_args, 0, s), "avgpool_same_bwd")
    _ok(L.bf_op_center_sq_bwd(N.ptr(xd), N.ptr(mean), N.ptr(t), N.ptr(dd), N.ptr(tot), n, s), "center_sq_bwd")
    _ok(L.bf_op_avgpool_same_bwd(N.ptr(tot), N.ptr(back), *pool_args, 0, s), "avgpool_same_bwd")
    dx = _h(tot) - _h(back)
    fn = lambda a: R.local_normalization(a, pool, eps)
    _close(y, fn(R.t64(x)), FWD, "y")
    _close(dx, R.vjp(fn, [x], dy)[0], GRAD, "dx")
    v = _f32(rng, shape)
    _adjoint([(R.jvp(fn, [x], [v])[0], dy)], [(v, dx)], "J v from the reference")


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("with_up", [0, 1])
def test_sigmoid_gate_and_bwd(with_up, n):
    rng, L = np.random.default_rng(with_up + n % 29), N.lib()
    enc, o, up, dy, v = _f32(rng, n), _f32(rng, n, 0.5), _f32(rng, n), _f32(rng, n), _f32(rng, n)
    ed, od, ud, dyd, vd = _d(enc), _d(o), _d(up), _d(dy), _d(v)
    out, denc, do, je, jo, lin = (_e(n) for _ in range(6))
    _ok(L.bf_op_sigmoid_gate(N.ptr(ed), N.ptr(od), N.ptr(ud) if with_up else None, N.ptr(out), n, N.stream_ptr(ed)), "sigmoid_gate")
    _ok(L.bf_op_sigmoid_gate_bwd(N.ptr(ed), N.ptr(od), N.ptr(dyd), N.ptr(denc), N.ptr(do), n, N.stream_ptr(ed)), "sigmoid_gate_bwd")
    _ok(L.bf_op_sigmoid_gate_bwd(N.ptr(ed), N.ptr(od), N.ptr(vd), N.ptr(je), N.ptr(jo), n, N.stream_ptr(ed)), "sigmoid_gate_bwd")
    _close(out, R.sigmoid_gate(R.t64(enc), R.t64(o), R.t64(up) if with_up else None), FWD, "out")
    rdenc, rdo = R.sigmoid_gate_bwd(enc, o, dy)
    _close(denc, rdenc, FWD, "denc")
    _close(do, rdo, FWD, "do")
    # linear in enc: the forward on v (no `up`) is A v
    _ok(L.bf_op_sigmoid_gate(N.ptr(vd), N.ptr(od), None, N.ptr(lin), n, N.stream_ptr(ed)), "sigmoid_gate")
    _adjoint([(lin, dy)], [(v, denc)], "gate in enc")
    _adjoint([(jo, dy)], [(v, do)], "diagonal Jacobian in o")


@pytest.mark.parametrize("B,hw,Cc", [(1, 1, 1), (3, 5, 17), (1, 257, 1), (163, 919, 7)], ids=[str(n) for n in NS])
@pytest.mark.parametrize("with_res,with_m,with_s", [(1, 1, 1), (0, 1, 0), (1, 0, 1), (0, 0, 0)])
def test_scale_add(with_res, with_m, with_s, B, hw, Cc):
    assert B * hw * Cc in NS
    rng, L = np.random.default_rng(B + hw), N.lib()
    res, t, m, s = _f32(rng, (B, hw, Cc)), _f32(rng, (B, hw, Cc)), _f32(rng, Cc), _f32(rng, B)
    rd, td, md, sd, out = _d(res), _d(t), _d(m), _d(s), _e(B, hw, Cc)
    _ok(L.bf_op_scale_add(N.ptr(rd) if with_res else None, N.ptr(td), N.ptr(md) if with_m else None, N.ptr(sd) if with_s else None,
                          N.ptr(out), B, hw, Cc, N.stream_ptr(td)), "scale_add")
    ref = R.scale_add(R.t64(res) if with_res else None, R.t64(t), R.t64(m) if with_m else None, R.t64(s) if with_s else None)
    _close(out, ref, FWD, "out")
    # (b): its adjoint in t is bf_op_scale_add_bwd's dt
    dy = _f32(rng, (B, hw, Cc))
    dyd, dt, lin, scr = _d(dy), _e(B, hw, Cc), _e(B, hw, Cc), _scratch(512 * Cc)
    _ok(L.bf_op_scale_add_bwd(N.ptr(td), N.ptr(md) if with_m else None, N.ptr(sd) if with_s else None, N.ptr(dyd), N.ptr(dt), None,
                              B, hw, Cc, N.ptr(scr), scr.numel(), N.stream_ptr(td)), "scale_add_bwd")
    _ok(L.bf_op_scale_add(None, N.ptr(td), N.ptr(md) if with_m else None, N.ptr(sd) if with_s else None, N.ptr(lin), B, hw, Cc,
                          N.stream_ptr(td)), "scale_add")
    _adjoint([(lin, dy)], [(t, dt)], "scale_add in t")


# ---- per-channel reductions ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cc", [4, 32, 300])
@pytest.mark.parametrize("with_m,with_s,with_dm", [(1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0)])
def test_scale_add_bwd(with_m, with_s, with_dm, Cc):
    """B = 3, hw = 5: a sample boundary inside one workgroup's pixel range, fewer pixels than workgroups.  300 channels: more than
    the 256 threads that stride over them.  A scratch of exactly C floats collapses the grid to one workgroup"""
    rng, L, B, hw = np.random.default_rng(Cc), N.lib(), 3, 5
    t, m, s, dy = _f32(rng, (B, hw, Cc)), _f32(rng, Cc), _f32(rng, B), _f32(rng, (B, hw, Cc))
    td, md, sd, dyd = _d(t), _d(m), _d(s), _d(dy)
    mp, sp = (N.ptr(md) if with_m else None), (N.ptr(sd) if with_s else None)
    rdt, rdm = R.scale_add_bwd(t, m if with_m else None, s if with_s else None, dy)
    for floats in (512 * Cc, Cc):
        scr, dt, dm = _scratch(floats), _e(B, hw, Cc), torch.full((Cc,), SENTINEL, device="cuda")
        _ok(L.bf_op_scale_add_bwd(N.ptr(td), mp, sp, N.ptr(dyd), N.ptr(dt), N.ptr(dm) if with_dm else None, B, hw, Cc, N.ptr(scr), floats,
                                  N.stream_ptr(td)), "scale_add_bwd")
        _close(dt, rdt, FWD, f"dt, scratch {floats}")
        if with_dm:
            _close(dm, rdm, GRAD, f"dm, scratch {floats}")
        else:
            assert np.all(_h(dm) == np.float64(np.float32(SENTINEL)))
        lin = _e(B, hw, Cc)
        _ok(L.bf_op_scale_add(None, N.ptr(td), mp, sp, N.ptr(lin), B, hw, Cc, N.stream_ptr(td)), "scale_add")
        _adjoint([(lin, dy)], [(t, dt)], "scale_add in t")
        if with_dm:                          # out is linear in m as well: <scale_add(t; v, s), dy> = <v, dm>
            v = _f32(rng, Cc)
            vd = _d(v)
            _ok(L.bf_op_scale_add(None, N.ptr(td), N.ptr(vd), sp, N.ptr(lin), B, hw, Cc, N.stream_ptr(td)), "scale_add")
            _adjoint([(lin, dy)], [(v, dm)], "scale_add in m")
    scr, dt, dm = _scratch(Cc), _e(B, hw, Cc), _e(Cc)
    assert L.bf_op_scale_add_bwd(N.ptr(td), mp, sp, N.ptr(dyd), N.ptr(dt), N.ptr(dm), B, hw, Cc, N.ptr(scr), Cc - 1,
                                 N.stream_ptr(td)) == N.BF_EWORKSPACE


@pytest.mark.parametrize("Cc", [4, 32, 300])
@pytest.mark.parametrize("scalar", [0, 1])
def test_relu_shift_linear_shift_and_bwd(scalar, Cc):
    rng, L, w1 = np.random.default_rng(Cc + scalar), N.lib(), 0.25
    nw = 1 if scalar else Cc
    for sign in ((1.0, -1.0) if scalar else (1.0,)):               # the scalar form switched on and off
        w0 = _away(rng, nw, (-w1,))
        if scalar:
            w0[0] = np.float32(0.4 * sign - w1)
        assert np.abs(w0.astype(np.float64) + w1).min() >= CLEAR
        dm = _f32(rng, Cc)
        w0d, dmd, lin, rel, dw0 = _d(w0), _d(dm), _e(Cc), _e(Cc), _e(nw)
        _ok(L.bf_op_linear_shift(N.ptr(w0d), nw, w1, N.ptr(lin), Cc, N.stream_ptr(w0d)), "linear_shift")
        _ok(L.bf_op_relu_shift(N.ptr(w0d), nw, w1, N.ptr(rel), Cc, N.stream_ptr(w0d)), "relu_shift")
        _ok(L.bf_op_relu_shift_bwd(N.ptr(w0d), nw, w1, N.ptr(dmd), N.ptr(dw0), Cc, N.stream_ptr(w0d)), "relu_shift_bwd")
        _close(lin, R.linear_shift(R.t64(w0), w1, Cc), FWD, "w0 + w1")
        _close(rel, R.relu_shift(R.t64(w0), w1, Cc), FWD, "relu(w0 + w1)")
        ref = R.relu_shift_bwd(w0, w1, dm)
        if np.abs(ref).max() == 0.0:
            assert np.all(_h(dw0) == 0.0)
        else:
            _close(dw0, ref, GRAD if scalar else FWD, "dw0")
        v = _f32(rng, nw)
        _adjoint([(R.jvp(lambda a: R.relu_shift(a, w1, Cc), [w0], [v])[0], dm)], [(v, dw0)], "J v from the reference")
    t = _e(Cc)
    assert L.bf_op_relu_shift(N.ptr(t), 2, w1, N.ptr(t), Cc, N.stream_ptr(t)) == N.BF_EINVAL          # nw is 1 or C


@pytest.mark.parametrize("Cc", [4, 32, 300])
def test_channel_mean_broadcast(Cc):
    """the column sums run on 256 / C rows per workgroup: a channel count that does not divide 256 is refused (300 here)"""
    rng, L, B, hw, rows = np.random.default_rng(Cc), N.lib(), 3, 5, 7
    x, y = _f32(rng, (B, hw, Cc)), _f32(rng, (B, rows, Cc))
    xd, out = _d(x), _e(B, rows, Cc)
    floats = max(int(L.bf_op_gate_scratch_floats(B, Cc)), 1)
    scr = _scratch(floats)
    assert scr.data_ptr() % 8 == 0                               # the column sums are doubles
    rc = L.bf_op_channel_mean_broadcast(N.ptr(xd), N.ptr(out), B, hw, Cc, rows, N.ptr(scr), floats, N.stream_ptr(xd))
    if 256 % Cc:
        assert rc == N.BF_EUNSUPPORTED
        return
    _ok(rc, "channel_mean_broadcast")
    _close(out, R.channel_mean_broadcast(R.t64(x), rows), FWD, "mean")
    # A^T y = the sum over the output rows / hw, on every input row
    aty = np.broadcast_to(y.astype(np.float64).sum(axis=1, keepdims=True) / hw, (B, hw, Cc))
    _adjoint([(out, y)], [(x, aty)], "mean and broadcast")
    assert L.bf_op_channel_mean_broadcast(N.ptr(xd), N.ptr(out), B, hw, Cc, rows, N.ptr(scr), floats - 1, N.stream_ptr(xd)) == N.BF_EWORKSPACE


# ---- window operators ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("k,gauss", [(k, 0) for k in range(1, 8)] + [(k, 1) for k in (2, 3, 5, 7)])
def test_smooth_split_bwd_ex(k, gauss, stride):
    """every map of MAPS (2 x 3 under k = 7: smaller than the window), B = 2, C = 4 and 8; the forward bf_op_smooth_split is A"""
    L = N.lib()
    g = R.gaussian_window(k) if gauss else None
    gd = _d(g) if gauss else None
    for (H, W), Cc in zip(MAPS, (4, 8, 4, 8, 4)):
        rng, shape = np.random.default_rng(k * 100 + H), (2, H, W, Cc)
        dshape = shape if stride == 1 else (2, (H + 1) // 2, (W + 1) // 2, Cc)
        x, dlap, dd = _f32(rng, shape), _f32(rng, shape), _f32(rng, dshape)
        xd, dlapd, ddd = _d(x), _d(dlap), _d(dd)
        lap, down, dx = _e(*shape), _e(*dshape), _e(*shape)
        _ok(L.bf_op_smooth_split(N.ptr(xd), N.ptr(lap), N.ptr(down), N.ptr(gd), 2, H, W, Cc, k, stride, N.stream_ptr(xd)), "smooth_split")
        _ok(L.bf_op_smooth_split_bwd_ex(N.ptr(dlapd), N.ptr(ddd), N.ptr(gd), N.ptr(dx), 2, H, W, Cc, k, stride, N.stream_ptr(xd)),
            "smooth_split_bwd_ex")
        rlap, rdown = R.smooth_split(R.t64(x), k, g, stride)
        _close(lap, rlap, FWD, f"lap {H}x{W}")
        _close(down, rdown, FWD, f"down {H}x{W}")
        _close(dx, R.smooth_split_bwd(dlap, dd, k, g, stride), GRAD, f"dx {H}x{W}")
        _adjoint([(lap, dlap), (down, dd)], [(x, dx)], f"split {H}x{W}")
    t = _e(16)
    assert L.bf_op_smooth_split_bwd_ex(N.ptr(t), N.ptr(t), None, N.ptr(t), 1, 2, 2, 4, 8, 2, N.stream_ptr(t)) == N.BF_EUNSUPPORTED
    assert L.bf_op_smooth_split_bwd_ex(N.ptr(t), N.ptr(t), None, N.ptr(t), 1, 2, 2, 4, 3, 3, N.stream_ptr(t)) == N.BF_EINVAL


@pytest.mark.parametrize("bilinear", [0, 1])
def test_upsample2x_bwd(bilinear):
    L = N.lib()
    for (H, W), Cc in zip(MAPS, (4, 8, 4, 8, 4)):
        rng = np.random.default_rng(H * 10 + W)
        x, dy = _f32(rng, (2, H, W, Cc)), _f32(rng, (2, 2 * H, 2 * W, Cc))
        xd, dyd, dx, up = _d(x), _d(dy), _e(2, H, W, Cc), _e(2, 2 * H, 2 * W, Cc)
        _ok(L.bf_op_upsample2x_bwd(N.ptr(dyd), N.ptr(dx), 2, H, W, Cc, bilinear, N.stream_ptr(dyd)), "upsample2x_bwd")
        _close(dx, R.upsample2x_bwd(dy, bilinear), GRAD, f"dx {H}x{W}")
        if bilinear:
            _ok(L.bf_op_upsample_act_add(N.ptr(xd), None, N.ptr(up), 2, H, W, Cc, 0, 0.0, N.stream_ptr(xd)), "upsample_act_add")
            _close(up, R.upsample2x(R.t64(x), 1), FWD, f"up {H}x{W}")
            _adjoint([(up, dy)], [(x, dx)], f"bilinear {H}x{W}")
        else:
            _adjoint([(R.upsample2x(R.t64(x), 0).numpy(), dy)], [(x, dx)], f"nearest {H}x{W}")


@pytest.mark.parametrize("src,dst", [((1, 1), (4, 5)), ((7, 9), (1, 1)), ((2, 3), (7, 9)), ((12, 10), (5, 3)), ((7, 9), (14, 18)),
                                     ((12, 10), (6, 5)), ((1, 5), (1, 5)), ((1, 5), (3, 2))])
def test_resize_bilinear_bwd(src, dst):
    """to and from 1 x 1, up, down, integer and non-integer ratios; the forward bf_op_resize_bilinear is A"""
    rng, L, B, Cc = np.random.default_rng(sum(src) + 7 * sum(dst)), N.lib(), 2, 4
    (H, W), (oh, ow) = src, dst
    x, dy = _f32(rng, (B, H, W, Cc)), _f32(rng, (B, oh, ow, Cc))
    xd, dyd, out, dx, scr = _d(x), _d(dy), _e(B, oh, ow, Cc), _e(B, H, W, Cc), _scratch(B * H * ow * Cc)
    _ok(L.bf_op_resize_bilinear(N.ptr(xd), N.ptr(out), B, H, W, Cc, oh, ow, N.stream_ptr(xd)), "resize_bilinear")
    _ok(L.bf_op_resize_bilinear_bwd(N.ptr(dyd), N.ptr(dx), B, H, W, Cc, oh, ow, N.ptr(scr), N.stream_ptr(xd)), "resize_bilinear_bwd")
    _close(out, R.resize_bilinear(R.t64(x), oh, ow), FWD, "resized")
    _close(dx, R.resize_bilinear_bwd(dy, H, W), GRAD, "dx")
    _adjoint([(out, dy)], [(x, dx)], "resize")


AVGPOOL_CASES = [((2, 32, 48, 8), (32, 32), (8, 8)), ((1, 17, 23, 3), (5, 5), (2, 2)), ((1, 16, 16, 32), (8, 8), (4, 4)),
                 ((2, 9, 9, 4), (3, 3), (3, 3)),                                  # the four of test_avgpool_same_any_pool_and_stride
                 ((2, 2, 3, 4), (7, 7), (1, 1)), ((2, 1, 5, 4), (8, 8), (4, 4)), ((2, 1, 1, 8), (3, 2), (1, 2))]     # pool > image


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("shape,pool,stride", AVGPOOL_CASES)
def test_avgpool_same_bwd(shape, pool, stride, accumulate):
    rng, L = np.random.default_rng(sum(shape) + pool[0]), N.lib()
    B, H, W, Cc = shape
    OH, OW = -(-H // stride[0]), -(-W // stride[1])
    x, dp, before = _f32(rng, shape), _f32(rng, (B, OH, OW, Cc)), _f32(rng, shape)
    xd, dpd, dx, pooled = _d(x), _d(dp), _d(before), _e(B, OH, OW, Cc)
    args = (B, H, W, Cc, pool[0], pool[1], stride[0], stride[1])
    _ok(L.bf_op_avgpool_same(N.ptr(xd), N.ptr(pooled), *args, N.stream_ptr(xd)), "avgpool_same")
    _ok(L.bf_op_avgpool_same_bwd(N.ptr(dpd), N.ptr(dx), *args, accumulate, N.stream_ptr(xd)), "avgpool_same_bwd")
    ref = R.avgpool_same_bwd(dp, shape, pool, stride)
    _close(pooled, R.avgpool_same(R.t64(x), pool, stride), FWD, "pooled")
    _close(dx, ref + before.astype(np.float64) if accumulate else ref, GRAD, "dx")
    # accumulating: dx = before + A^T dp, so <A x, dp> + <x, before> = <x, dx>
    _adjoint([(pooled, dp)] + ([(x, before)] if accumulate else []), [(x, dx)], "pool")


def _maxpool_case(x, Cc, what):
    L = N.lib()
    B, H, W, _ = x.shape
    rng = np.random.default_rng(H * W + Cc)
    dy = _f32(rng, (B, (H + 1) // 2, (W + 1) // 2, Cc))
    xd, dyd, dx = _d(x), _d(dy), torch.full(x.shape, SENTINEL, device="cuda")
    _ok(L.bf_op_maxpool2_bwd(N.ptr(xd), N.ptr(dyd), N.ptr(dx), B, H, W, Cc, N.stream_ptr(xd)), "maxpool2_bwd")
    assert np.array_equal(_h(dx), R.maxpool2_bwd(x, dy)), what         # dy or 0: bit for bit
    if np.isfinite(x).all():
        pooled = _e(*dy.shape)
        _ok(L.bf_op_maxpool2(N.ptr(xd), N.ptr(pooled), B, H, W, Cc, N.stream_ptr(xd)), "maxpool2")
        assert np.array_equal(_h(pooled), R.maxpool2(x)), what
        _adjoint([(pooled, dy)], [(x, dx)], what)


@pytest.mark.parametrize("Cc", [4, 36])
def test_maxpool2_bwd(Cc):
    """odd and even maps; small integers, so that most windows hold a tie; an all-equal map; windows holding -inf"""
    for H, W in MAPS + ((5, 3),):
        rng = np.random.default_rng(H + W)
        ties = rng.integers(0, 3, (2, H, W, Cc)).astype(np.float32)
        _maxpool_case(ties, Cc, f"ties {H}x{W}")
        _maxpool_case(np.full((2, H, W, Cc), 1.5, np.float32), Cc, f"all equal {H}x{W}")
        _maxpool_case(_f32(rng, (2, H, W, Cc)), Cc, f"no ties {H}x{W}")
        holes = ties.copy()
        holes[rng.random(holes.shape) < 0.4] = -np.inf
        holes[0, 0, 0, :] = -np.inf                                   # with the rest of its window in channel 0 ...
        holes[0, :2, :2, 0] = -np.inf                                 # ... a window of nothing but -inf
        _maxpool_case(holes, Cc, f"-inf {H}x{W}")


def test_maxpool2_bwd_refuses_channels_that_are_no_multiple_of_4():
    L, t = N.lib(), _e(2 * 4 * 4 * 6)
    assert L.bf_op_maxpool2_bwd(N.ptr(t), N.ptr(t), N.ptr(t), 2, 4, 4, 6, N.stream_ptr(t)) == N.BF_EINVAL


# ---- weight gradients ----------------------------------------------------------------------------------------------------------

def _conv2d_wgrad_case(x, u8, normalize, k, cout, dy, scratch_floats, what):
    L = N.lib()
    B, H, W, cin = x.shape
    vr = (10.0, 200.0) if (normalize and not u8) else (0.0, 255.0)
    xd, dyd, dw, scr = _d(x, np.uint8 if u8 else np.float32), _d(dy), _e(k, k, cin, cout), _scratch(scratch_floats)
    _ok(L.bf_op_conv2d_wgrad(N.ptr(xd), u8, N.ptr(dyd), N.ptr(dw), B, H, W, cin, cout, k, normalize, vr[0], vr[1], N.ptr(scr), scratch_floats,
                             N.stream_ptr(xd)), "conv2d_wgrad")
    x64 = x.astype(np.float64)
    _close(dw, R.conv2d_wgrad(x64, dy, k, cin, cout, vr if normalize else None), GRAD, what)
    v = _f32(np.random.default_rng(k), (k, k, cin, cout))
    _adjoint([(R.conv2d(R.t64(x64), R.t64(v), vr if normalize else None).numpy(), dy)], [(v, dw)], what)


@pytest.mark.parametrize("mode", ["u8-normalised", "float-normalised", "float-raw"])
@pytest.mark.parametrize("cin", [1, 3, 4])
@pytest.mark.parametrize("k", [1, 3, 5, 7])
def test_conv2d_wgrad(k, cin, mode):
    """2 x 9 x 7 pixels, cout 32; float-normalised: values on both sides of [v_min, v_max] = [10, 200], clipped as the forward clips.
    A scratch of exactly nel floats and a large one (126 pixels are one workgroup either way; see the next test for several)"""
    rng, cout = np.random.default_rng(k * 10 + cin), 32
    u8, normalize = mode == "u8-normalised", mode != "float-raw"
    if u8:
        x = rng.integers(0, 256, (2, 9, 7, cin)).astype(np.uint8)
    elif normalize:
        x = rng.uniform(-60.0, 300.0, (2, 9, 7, cin)).astype(np.float32)
        assert (x < 10.0).any() and (x > 200.0).any()
    else:
        x = _f32(rng, (2, 9, 7, cin))
    dy, nel = _f32(rng, (2, 9, 7, cout)), k * k * cin * cout
    for floats in (nel, 256 * nel):
        _conv2d_wgrad_case(x, int(u8), int(normalize), k, cout, dy, floats, f"dw, scratch {floats}")


@pytest.mark.parametrize("k", [3, 7])
def test_conv2d_wgrad_on_several_workgroups_and_under_the_window(k):
    """2 x 40 x 30 pixels are three workgroups with a large scratch and one with exactly nel floats: both within the bar.  A 2 x 2
    image lies wholly under a 7 x 7 window"""
    rng, cin, cout = np.random.default_rng(k), 3, 32
    nel = k * k * cin * cout
    x, dy = rng.integers(0, 256, (2, 40, 30, cin)).astype(np.uint8), _f32(rng, (2, 40, 30, cout))
    for floats in (nel, 256 * nel):
        _conv2d_wgrad_case(x, 1, 1, k, cout, dy, floats, f"dw 40x30, scratch {floats}")
    x, dy = rng.integers(0, 256, (2, 2, 2, cin)).astype(np.uint8), _f32(rng, (2, 2, 2, cout))
    _conv2d_wgrad_case(x, 1, 1, 7, cout, dy, 7 * 7 * cin * cout, "dw 2x2 under 7x7")


def test_conv2d_wgrad_refusals():
    L, t = N.lib(), _e(1 << 14)
    p, s = N.ptr(t), N.stream_ptr(t)
    nel = 3 * 3 * 3 * 32
    assert L.bf_op_conv2d_wgrad(p, 0, p, p, 2, 9, 7, 3, 32, 3, 0, 0.0, 255.0, p, nel - 1, s) == N.BF_EWORKSPACE
    for k in (2, 4, 6, 9):
        assert L.bf_op_conv2d_wgrad(p, 0, p, p, 1, 4, 4, 1, 4, k, 0, 0.0, 255.0, p, 1 << 14, s) == N.BF_EUNSUPPORTED
    assert L.bf_op_conv2d_wgrad(p, 0, p, p, 1, 4, 4, 1, 4, 3, 1, 255.0, 255.0, p, 1 << 14, s) == N.BF_EUNSUPPORTED     # an empty value range


@pytest.mark.parametrize("n", [1, 50])
@pytest.mark.parametrize("Cs,Cc,C8", [(35, 3, 5), (96, 32, 8), (256, 256, 64)])
def test_dense2_bwd(Cs, Cc, C8, n):
    """the selector form of bf_op_dense2 (no biases, leaky ReLU 0.3, final ReLU): forward, din, dw0, dw1 against autograd"""
    rng, L, alpha = np.random.default_rng(Cs + n), N.lib(), 0.3
    p, w0, w1 = R.dense2_inputs(rng, n, Cs, Cc, C8, alpha)
    assert R.kink_distance_dense2(p, w0, w1, alpha) >= CLEAR
    du = _f32(rng, (n, Cc))
    pd, w0d, w1d, dud = _d(p), _d(w0), _d(w1), _d(du)
    out, din, dw0, dw1 = _e(n, Cc), _e(n, Cs), _e(Cs, C8), _e(C8, Cc)
    floats = int(L.bf_op_dense2_bwd_scratch_floats(n, Cc, C8))
    assert floats == n * (Cc + 2 * C8)
    scr = _scratch(floats)
    _ok(L.bf_op_dense2(N.ptr(pd), N.ptr(w0d), None, N.ptr(w1d), None, N.ptr(out), n, Cs, Cc, C8, 2, alpha, 4, N.stream_ptr(pd)), "dense2")
    _ok(L.bf_op_dense2_bwd(N.ptr(pd), N.ptr(w0d), N.ptr(w1d), N.ptr(dud), N.ptr(din), N.ptr(dw0), N.ptr(dw1), n, Cs, Cc, C8, alpha,
                           N.ptr(scr), floats, N.stream_ptr(pd)), "dense2_bwd")
    fn = lambda a, b, c: R.dense2_selector(a, b, c, alpha)
    _close(out, fn(R.t64(p), R.t64(w0), R.t64(w1)), FWD, "out")
    rdin, rdw0, rdw1 = R.dense2_bwd(p, w0, w1, du, alpha)
    _close(din, rdin, GRAD, "din")
    _close(dw0, rdw0, GRAD, "dw0")
    _close(dw1, rdw1, GRAD, "dw1")
    v = [_f32(rng, a.shape) for a in (p, w0, w1)]
    _adjoint([(R.jvp(fn, [p, w0, w1], v)[0], du)], [(v[0], din), (v[1], dw0), (v[2], dw1)], "J v from the reference")
    assert L.bf_op_dense2_bwd(N.ptr(pd), N.ptr(w0d), N.ptr(w1d), N.ptr(dud), N.ptr(din), N.ptr(dw0), N.ptr(dw1), n, Cs, Cc, C8, alpha,
                              N.ptr(scr), floats - 1, N.stream_ptr(pd)) == N.BF_EWORKSPACE


# ---- head and loss -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("denormalize", [0, 1])
@pytest.mark.parametrize("npix", [1, 7, 4099])
@pytest.mark.parametrize("co", [1, 2, 3, 4])
@pytest.mark.parametrize("hf", [32, 64, 128])
def test_head_out_bwd(hf, co, npix, denormalize):
    """h W1 of standard deviation 1: about a quarter of 0.51 tanh(2 h1) lies beyond +-0.5 (asserted for 4099 pixels).  The scratch
    is filled with 1e30 before each call: a partial sum that no thread writes shows in dw1.  hf x cout = 384 and 512 are more
    entries than the workgroup has threads"""
    rng, L = np.random.default_rng(hf + 10 * co + npix), N.lib()
    h, w1 = R.head_inputs(rng, npix, hf, co, 1.0)
    assert R.kink_distance_head(h, w1) >= CLEAR
    if npix > 7:
        p = R.head_p(R.t64(h), R.t64(w1)).numpy()
        assert (p > 0.5).any() and (p < -0.5).any() and (np.abs(p) < 0.5).any()
    dpred = _f32(rng, (npix, co))
    hd, w1d, dpd = _d(h), _d(w1), _d(dpred)
    rdh, rdw1 = R.head_out_bwd(h, w1, dpred, denormalize)
    vh, vw = _f32(rng, h.shape), _f32(rng, w1.shape)
    jv = R.jvp(lambda a, b: R.head_out(a, b, denormalize), [h, w1], [vh, vw])[0]
    for floats in (hf * co, 512 * hf * co):
        scr, dh, dw1 = _scratch(floats), _e(npix, hf), _e(hf, co)
        _ok(L.bf_op_head_out_bwd(N.ptr(hd), N.ptr(w1d), N.ptr(dpd), N.ptr(dh), N.ptr(dw1), npix, hf, co, denormalize, 0.0, 255.0,
                                 N.ptr(scr), floats, N.stream_ptr(hd)), "head_out_bwd")
        _close(dh, rdh, FWD, f"dh, scratch {floats}")
        _close(dw1, rdw1, GRAD, f"dw1, scratch {floats}")
        _adjoint([(jv, dpred)], [(vh, dh), (vw, dw1)], "J v from the reference")


def test_head_out_bwd_refusals():
    L, t = N.lib(), _e(4096)
    p, s = N.ptr(t), N.stream_ptr(t)
    assert L.bf_op_head_out_bwd(p, p, p, p, p, 4, 128, 4, 1, 0.0, 255.0, p, 128 * 4 - 1, s) == N.BF_EWORKSPACE
    for hf, co in ((16, 3), (256, 3), (96, 3), (32, 5), (32, 0)):
        assert L.bf_op_head_out_bwd(p, p, p, p, p, 4, hf, co, 1, 0.0, 255.0, p, 4096, s) == N.BF_EUNSUPPORTED


def _loss_desc(ls, depth_weight):
    ld = N.LossDesc()
    ld.struct_size = C.sizeof(N.LossDesc)
    ld.hinge, ld.cutoff = ls.hinge, ls.cutoff
    ld.mae_multiplier, ld.mse_multiplier, ld.ssim_multiplier = ls.mae_multiplier, ls.mse_multiplier, ls.ssim_multiplier
    ld.regularization, ld.depth_weight = 0.0, depth_weight
    return ld


@pytest.mark.parametrize("mults,hinge", [((1.0, 0.0, 0.0), 0.0), ((0.0, 0.5, 0.0), 0.0), ((0.0, 0.0, 1.0), 0.0), ((1.0, 0.5, 1.0), 0.0),
                                         ((1.0, 0.5, 1.0), 3.5)], ids=["mae", "mse", "ssim", "all", "all-hinge"])
@pytest.mark.parametrize("B,H,W,Cc", [(1, 7, 7, 1), (2, 7, 7, 3), (2, 9, 8, 1), (1, 8, 11, 3)])
def test_denoiser_loss(B, H, W, Cc, mults, hinge):
    """every slot of losses and dpred against oracle/unet_torch.denoiser_loss under autograd; 7 x 7 is the smallest map the SSIM
    window admits; depth_weight 0.5"""
    rng, L, dw = np.random.default_rng(B * H + W + Cc), N.lib(), 0.5
    gt = rng.integers(40, 216, (B, H, W, Cc)).astype(np.float32)
    e = rng.uniform(0.5, 30.0, gt.shape) * rng.choice([-1.0, 1.0], gt.shape)
    e[np.abs(np.abs(e) - hinge) < 0.01] += 0.05
    pred = (gt - e).astype(np.float32)
    ls = R.loss_spec(hinge, 255.0, *mults)
    assert R.kink_distance_loss(ls, gt, pred) >= CLEAR
    ref, rgrad = R.denoiser_loss_grad(ls, gt, pred, dw)
    ld = _loss_desc(ls, dw)
    floats = int(L.bf_op_denoiser_loss_scratch_floats(B, H, W, Cc))
    pd, gd, dpred, losses, scr = _d(pred), _d(gt), _e(B, H, W, Cc), torch.full((N.BF_LOSS_COUNT,), SENTINEL, device="cuda"), _scratch(floats)
    _ok(L.bf_op_denoiser_loss(N.ptr(pd), N.ptr(gd), B, H, W, Cc, C.byref(ld), N.ptr(dpred), N.ptr(losses), N.ptr(scr), floats,
                              N.stream_ptr(pd)), "denoiser_loss")
    got = _h(losses)
    want = {N.BF_LOSS_TOTAL: ref["total_loss"] * dw, N.BF_LOSS_DENOISER_TOTAL: ref["total_loss"], N.BF_LOSS_MAE: ref["mae_loss"],
            N.BF_LOSS_MSE: ref["mse_loss"], N.BF_LOSS_SSIM: ref["ssim_loss"], N.BF_LOSS_REGULARIZATION: 0.0, N.BF_LOSS_MODEL_TOTAL: 0.0,
            N.BF_LOSS_GRAD_NORM: 0.0}
    assert sorted(want) == list(range(N.BF_LOSS_COUNT))
    for slot, value in want.items():
        print(f"slot {slot}: {got[slot]!r} against {value!r}")
        assert abs(got[slot] - value) <= FWD * abs(value), (slot, got[slot], value)
    _close(dpred, rgrad, GRAD, "dpred")
    v = _f32(rng, pred.shape)
    jv = R.jvp(lambda a: R.denoiser_loss(ls, R.t64(gt), a)["total_loss"] * dw, [pred], [v])[0]
    _adjoint([(jv, 1.0)], [(v, dpred)], "directional derivative from the reference")
    assert L.bf_op_denoiser_loss(N.ptr(pd), N.ptr(gd), B, H, W, Cc, C.byref(ld), N.ptr(dpred), N.ptr(losses), N.ptr(scr), floats - 1,
                                 N.stream_ptr(pd)) == N.BF_EWORKSPACE


def test_denoiser_loss_refuses_a_map_smaller_than_the_ssim_window():
    L = N.lib()
    pred, gt, dpred, losses, scr = torch.zeros(42, device="cuda"), torch.ones(42, device="cuda"), _e(42), _e(N.BF_LOSS_COUNT), _scratch(1 << 14)
    args = lambda ld: (N.ptr(pred), N.ptr(gt), 1, 6, 7, 1, C.byref(ld), N.ptr(dpred), N.ptr(losses), N.ptr(scr), 1 << 14, N.stream_ptr(pred))
    assert L.bf_op_denoiser_loss(*args(_loss_desc(R.loss_spec(0.0, 255.0, 1.0, 0.0, 1.0), 1.0))) == N.BF_EINVAL
    assert L.bf_op_denoiser_loss(*args(_loss_desc(R.loss_spec(0.0, 255.0, 1.0, 0.0, 0.0), 1.0))) == N.BF_OK          # without SSIM: fine
    assert _h(losses)[N.BF_LOSS_MAE] == 1.0


# ---- layout helpers: bit for bit -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("a,b", [(1, 7), (35, 64), (300, 3)])
def test_transpose2d(a, b):
    w = _f32(np.random.default_rng(a), (a, b))
    wd, out = _d(w), _e(b, a)
    _ok(N.lib().bf_op_transpose2d(N.ptr(wd), N.ptr(out), a, b, N.stream_ptr(wd)), "transpose2d")
    assert np.array_equal(out.cpu().numpy(), w.T)


@pytest.mark.parametrize("inner", [1, 96])
@pytest.mark.parametrize("k", [1, 3, 5])
def test_flip_hw(k, inner):
    w = _f32(np.random.default_rng(k + inner), (k, k, inner))
    wd, out = _d(w), _e(k, k, inner)
    _ok(N.lib().bf_op_flip_hw(N.ptr(wd), N.ptr(out), k, inner, N.stream_ptr(wd)), "flip_hw")
    assert np.array_equal(out.cpu().numpy(), w[::-1, ::-1])


@pytest.mark.parametrize("widths", [(35, 3, 32), (3, 32), (1, 300), (7,)])
def test_concat_channels(widths):
    rng, rows = np.random.default_rng(sum(widths)), 37
    parts = [_f32(rng, (rows, c)) for c in widths]
    dev = [_d(p) for p in parts]
    out = torch.full((rows + 1, sum(widths)), SENTINEL, device="cuda")
    ptrs = [N.ptr(t) for t in dev] + [None] * (3 - len(dev))
    cs = list(widths) + [0] * (3 - len(widths))
    _ok(N.lib().bf_op_concat_channels(ptrs[0], ptrs[1], ptrs[2], N.ptr(out), rows, cs[0], cs[1], cs[2], N.stream_ptr(out)), "concat_channels")
    got = out.cpu().numpy()
    assert np.array_equal(got[:rows], np.concatenate(parts, axis=1))
    assert np.all(got[rows] == np.float32(SENTINEL))


@pytest.mark.parametrize("src_channels,offset,channels", [(70, 35, 3), (70, 38, 32), (300, 299, 1), (8, 0, 8)])
def test_slice_channels(src_channels, offset, channels):
    """a slice at an offset into a sentinel-filled destination one row larger than needed: the extra row keeps the sentinel"""
    rows = 37
    src = _f32(np.random.default_rng(offset), (rows, src_channels))
    sd, dst = _d(src), torch.full((rows + 1, channels), SENTINEL, device="cuda")
    L = N.lib()
    _ok(L.bf_op_slice_channels(N.ptr(sd), N.ptr(dst), rows, src_channels, offset, channels, N.stream_ptr(sd)), "slice_channels")
    got = dst.cpu().numpy()
    assert np.array_equal(got[:rows], src[:, offset:offset + channels])
    assert np.all(got[rows] == np.float32(SENTINEL))
    assert L.bf_op_slice_channels(N.ptr(sd), N.ptr(dst), rows, src_channels, src_channels - channels + 1, channels, N.stream_ptr(sd)) == N.BF_EINVAL


@pytest.mark.parametrize("Cc,m", [(3, 2), (32, 4), (300, 1)])
def test_channel_repeat_and_group_sum(Cc, m):
    """small integers: the group sums are exact, so both directions are compared bit for bit"""
    rng, rows, L = np.random.default_rng(Cc + m), 37, N.lib()
    x = rng.integers(-8, 9, (rows, Cc)).astype(np.float32)
    y = rng.integers(-8, 9, (rows, Cc * m)).astype(np.float32)
    xd, yd, xr, ys = _d(x), _d(y), _e(rows, Cc * m), _e(rows, Cc)
    _ok(L.bf_op_channel_repeat(N.ptr(xd), N.ptr(xr), rows, Cc, m, N.stream_ptr(xd)), "channel_repeat")
    _ok(L.bf_op_channel_group_sum(N.ptr(yd), N.ptr(ys), rows, Cc, m, N.stream_ptr(yd)), "channel_group_sum")
    assert np.array_equal(xr.cpu().numpy(), np.repeat(x, m, axis=1))
    assert np.array_equal(ys.cpu().numpy(), y.reshape(rows, Cc, m).sum(axis=2))
    assert float((xr.cpu().numpy().astype(np.float64) * y).sum()) == float((x.astype(np.float64) * ys.cpu().numpy()).sum())
