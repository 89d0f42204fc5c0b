"""GPU tests of the restoration code: the four entries of csrc/restore.hip through their Python operators, and bf.restore.

Yardstick: tests/restore_reference.py in fp64.  Tolerances:
  direction, deterministic step   |got - ref| <= 8 * 2^-24 * M, M = the largest magnitude among the element's operands (the kernels
                                  round once per formula; eight float32 roundings are allowed);
  sum d^2                         1e-12 relative, and bit-equal between two calls and between an image alone and in its batch;
  normals                         2^-18 (1 + |z_ref|): float log, sqrt, sin and cos (observed maximum printed);
  finish                          measured samples bit for bit; block means within s^2 * 2^-23 * 255; ties and clipping as NumPy;
  loop                            step counts equal, trace and float result within 10 F, F = |fp64 loop - float32-storage loop| of the
                                  reference, computed here (the GPU makes the same kind of roundings in another order).
The linear test denoiser is evaluated in float64 on the device and rounded once to float32, as the reference's float32-storage
loop holds D."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import _native as N
from oracle import bfcnn_oracle as O
from oracle import unet_oracle as U
import restore_reference as R
from guarded import dev as _dev, guard_bands

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guard_bands")]

SHAPES = [(1, 1, 1), (3, 5, 3), (16, 16, 4), (37, 45, 3), (70, 83, 3), (96, 128, 3)]
MASKS = ["ones", "zeros", "shared", "per_channel"]
BLOCKS = [(2, 2, 2, 1), (2, 6, 10, 3), (3, 9, 15, 1), (4, 8, 12, 3), (8, 16, 24, 4), (2, 64, 96, 3), (4, 64, 96, 3), (8, 64, 96, 3)]
B = 2
EPS = 2.0 ** -24
_ids = {"ids": lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)}


def _host(t):
    return t.cpu().numpy()


def _mask_case(shape, kind, u8, rng):
    """(reference constraint, bf constraint on the device) for a mask of `kind` over B images of `shape`"""
    H, W, C = shape
    x = rng.integers(0, 256, (B, H, W, C)).astype(np.uint8) if u8 else rng.uniform(0, 255, (B, H, W, C)).astype(np.float32)
    m = {"ones": np.ones((B, H, W, 1), np.uint8), "zeros": np.zeros((B, H, W, C), np.uint8),
         "shared": (rng.random((B, H, W, 1)) < 0.5).astype(np.uint8) * 255,
         "per_channel": (rng.random((B, H, W, C)) < 0.4).astype(np.uint8) * 3}[kind]
    return ("mask", m, x), bf.mask_constraint(_dev(x), _dev(m))


def _block_case(s, H, W, C, u8, rng):
    low = rng.integers(0, 256, (B, H // s, W // s, C)).astype(np.uint8) if u8 else rng.uniform(0, 255, (B, H // s, W // s, C)).astype(np.float32)
    return ("block", s, low), bf.block_constraint(_dev(low), s)


def _iterates(shape4, rng):
    """y and D of magnitude up to about 1000, as sigma_0 = 255 produces"""
    y = np.clip(rng.normal(128, 300, shape4), -1000, 1100).astype(np.float32)
    D = np.clip(y + rng.normal(0, 150, shape4), -1000, 1100).astype(np.float32)
    return y, D


def _magnitude(con, y, D):
    """M per element: the largest magnitude among y, D, a and, for a block constraint, the values of D under the block"""
    M = np.maximum(np.maximum(np.abs(y), np.abs(D)), np.abs(R.anchor(con, y.shape))).astype(np.float64)
    if con[0] == "block":
        s = con[1]
        Bn, H, W, C = y.shape
        top = np.abs(D).astype(np.float64).reshape(Bn, H // s, s, W // s, s, C).max(axis=(2, 4))
        M = np.maximum(M, np.repeat(np.repeat(top, s, axis=1), s, axis=2))
    return M


def _check_direction_and_step(ref_con, con, rng):
    shape4 = R.constraint_shape(ref_con)
    n = int(np.prod(shape4[1:]))
    y, D = _iterates(shape4, rng)
    yd, Dd = _dev(y), _dev(D)
    d, sumsq = bf.restore_direction(yd, Dd, con)
    d_ref, sumsq_ref = R.direction(ref_con, y, D)
    err = np.abs(_host(d).astype(np.float64) - d_ref)
    bound = 8 * EPS * _magnitude(ref_con, y, D)
    print(f"direction {ref_con[0]} {shape4}: max error / bound {np.max(err / bound):.3f}, sumsq relative "
          f"{np.max(np.abs(_host(sumsq) - sumsq_ref) / sumsq_ref):.2e}")
    assert (err <= bound).all()
    assert (np.abs(_host(sumsq) - sumsq_ref) <= 1e-12 * sumsq_ref).all()
    d2, sumsq2 = bf.restore_direction(yd, Dd, con)                                  # two calls: the same bits
    assert torch.equal(d, d2) and torch.equal(sumsq.view(torch.int64), sumsq2.view(torch.int64))
    for b in range(B):                                                              # an image alone: the bits it has in the batch
        one = con._replace(anchor=con.anchor[b:b + 1].clone(), mask=None if con.mask is None else con.mask[b:b + 1].clone(),
                           shape=(1,) + tuple(con.shape[1:]))
        d1, s1 = bf.restore_direction(yd[b:b + 1].clone(), Dd[b:b + 1].clone(), one)
        assert torch.equal(d1[0], d[b]) and torch.equal(s1.view(torch.int64), sumsq[b:b + 1].view(torch.int64))
    # the deterministic step (beta = 1) from the kernel's own d and sumsq
    t, h = 5, R.step_size(5)
    steps = torch.full((B,), t - 1, dtype=torch.int32, device="cuda")
    trace = torch.zeros((t, B), dtype=torch.float64, device="cuda")
    y_new = yd.clone()
    bf.restore_step(y_new, d, sumsq, steps, t, h, beta=1.0, sigma_l=2.55, trace=trace)
    ref_y, ref_steps, ref_sigma = R.step(y, _host(d), _host(sumsq), np.full(B, t - 1), t, h, beta=1.0)
    bound = 8 * EPS * np.maximum(np.abs(y), np.abs(_host(d))).astype(np.float64)
    assert (np.abs(_host(y_new).astype(np.float64) - ref_y) <= bound).all()
    assert np.array_equal(_host(steps), ref_steps)
    assert (np.abs(_host(trace)[t - 1] - ref_sigma) <= 1e-14 * ref_sigma).all() and not _host(trace)[:t - 1].any()
    assert n == d[0].numel()


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_direction_and_step_mask(shape, kind, u8):
    rng = np.random.default_rng(sum(shape) + len(kind) + u8)
    _check_direction_and_step(*_mask_case(shape, kind, u8, rng), rng)


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("case", BLOCKS, **_ids)
def test_direction_and_step_block(case, u8):
    rng = np.random.default_rng(sum(case) + u8)
    _check_direction_and_step(*_block_case(*case, u8, rng), rng)


def test_unaligned_bases_take_the_scalar_path():
    """n % 4 == 0 but the tensors start 4 bytes past a 16-byte boundary: the same bits as the aligned call"""
    rng = np.random.default_rng(3)
    ref_con, con = _mask_case((16, 16, 4), "shared", False, rng)
    y, D = _iterates((B, 16, 16, 4), rng)

    def shifted(a):
        big = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
        view = big[1:].view(a.shape)
        view.copy_(_dev(a))
        assert view.data_ptr() % 16 == 4
        return view
    d, sumsq = bf.restore_direction(_dev(y), _dev(D), con)
    d_s, sumsq_s = bf.restore_direction(shifted(y), shifted(D), con)
    assert torch.equal(d, d_s) and torch.equal(sumsq, sumsq_s)
    steps = torch.zeros(B, dtype=torch.int32, device="cuda")
    y_a, y_s = _dev(y), shifted(y)
    bf.restore_step(y_a, d, sumsq, steps.clone(), 1, 0.3, beta=0.2, seed=5)
    bf.restore_step(y_s, d_s, sumsq, steps.clone(), 1, 0.3, beta=0.2, seed=5)
    assert torch.equal(y_a, y_s)
    assert torch.equal(bf.restore_finish(_dev(D), con, False), bf.restore_finish(shifted(D), con, False))
    assert torch.equal(bf.restore_finish(_dev(D), con, True), bf.restore_finish(shifted(D), con, True))


# ---- noise ---------------------------------------------------------------------------------------------------------------------

def _zero_constraint(shape, batch=B):
    """all measured, measurement 0: y_0 = sigma_0 z_0"""
    H, W, C = shape
    return bf.mask_constraint(torch.zeros((batch, H, W, C), device="cuda"), torch.ones((batch, H, W, 1), dtype=torch.uint8, device="cuda"))


def _step_noise(shape, t, seed, ids, batch=B):
    """y = 0, d = 0, sum d^2 = n, beta = 0, h = 1: gamma = sigma = 1, so the step leaves z_t in y"""
    H, W, C = shape
    y = torch.zeros((batch, H, W, C), device="cuda")
    sumsq = torch.full((batch,), float(H * W * C), dtype=torch.float64, device="cuda")
    steps = torch.full((batch,), t - 1, dtype=torch.int32, device="cuda")
    bf.restore_step(y, torch.zeros_like(y), sumsq, steps, t, 1.0, beta=0.0, sigma_l=0.5, seed=seed, sample_ids=ids)
    return y


@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_normals_match_reference(shape):
    seed, ids = 0x1234567887654321, [7, 2 ** 32 - 1]
    z0 = _host(bf.restore_init(_zero_constraint(shape), sigma_0=1.0, seed=seed, sample_ids=ids)).astype(np.float64)
    z3 = _host(_step_noise(shape, 3, seed, ids)).astype(np.float64)
    worst = 0.0
    for got, t in ((z0, 0), (z3, 3)):
        ref = R.batch_normals(got.shape, seed, ids, t)
        rel = np.abs(got - ref) / (1.0 + np.abs(ref))
        worst = max(worst, rel.max())
        assert (rel <= 2.0 ** -18).all(), (t, rel.max())
    print(f"normals {shape}: max |z - z_ref| / (1 + |z_ref|) = {worst:.3e} (bound {2.0 ** -18:.3e})")


def test_normals_depend_on_seed_step_and_sample_alone():
    shape = (37, 45, 3)
    a = _step_noise(shape, 2, 11, [0, 1])
    assert torch.equal(a, _step_noise(shape, 2, 11, [0, 1])) and torch.equal(a, _step_noise(shape, 2, 11, None))
    assert not torch.equal(a, _step_noise(shape, 2, 12, [0, 1])) and not torch.equal(a, _step_noise(shape, 3, 11, [0, 1]))
    other = _step_noise(shape, 2, 11, [1, 0])
    assert not torch.equal(a, other) and torch.equal(a[0], other[1]) and torch.equal(a[1], other[0])
    assert not torch.equal(a[0], a[1])
    y0 = bf.restore_init(_zero_constraint(shape), sigma_0=1.0, seed=11)
    assert torch.equal(y0, bf.restore_init(_zero_constraint(shape), sigma_0=1.0, seed=11)) and not torch.equal(y0, a)
    alone = bf.restore_init(_zero_constraint(shape, 1), sigma_0=1.0, seed=11, sample_ids=[1])
    assert torch.equal(alone[0], y0[1])                                             # an image alone: the bits it has in the batch


def test_normals_statistics():
    shape = (2, 2 ** 17, 1)
    n = 2 ** 18
    for z in (bf.restore_init(_zero_constraint(shape, 1), sigma_0=1.0, seed=3), _step_noise(shape, 9, 3, None, 1)):
        z = _host(z).astype(np.float64)
        print(f"mean {z.mean():+.5f} (5 s.e. {5 / np.sqrt(n):.5f}), variance {z.var():.5f} (1 +- {5 * np.sqrt(2 / n):.5f})")
        assert abs(z.mean()) <= 5 / np.sqrt(n) and abs(z.var() - 1.0) <= 5 * np.sqrt(2.0 / n)


def test_init_matches_reference():
    rng = np.random.default_rng(8)
    for ref_con, con in (_mask_case((37, 45, 3), "shared", True, rng), _mask_case((16, 16, 4), "per_channel", False, rng),
                         _block_case(3, 9, 15, 1, True, rng), _block_case(4, 8, 12, 3, False, rng)):
        got = _host(bf.restore_init(con, sigma_0=255.0, seed=21)).astype(np.float64)
        ref = R.init(ref_con, 255.0, 21)
        z = R.batch_normals(ref.shape, 21, np.arange(B), 0)
        assert (np.abs(got - ref) <= 255.0 * 2.0 ** -18 * (1 + np.abs(z)) + EPS * np.abs(ref)).all()


# ---- finish --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_finish_mask(shape, kind, u8):
    rng = np.random.default_rng(sum(shape) + 7 * len(kind) + u8)
    ref_con, con = _mask_case(shape, kind, u8, rng)
    Dn = (rng.integers(-8, 521, (B,) + shape) * 0.5).astype(np.float32)             # half steps in [-4, 260]: ties and clipping
    if not u8:                                                                      # a float measurement with ties of its own
        x = (rng.integers(0, 511, (B,) + shape) * 0.5).astype(np.float32)
        ref_con, con = ("mask", ref_con[1], x), bf.mask_constraint(_dev(x), con.mask)
    m = R.measured(ref_con, Dn.shape)
    as_float, as_u8 = _host(bf.restore_finish(_dev(Dn), con, False)), _host(bf.restore_finish(_dev(Dn), con, True))
    expect = np.where(m, ref_con[2].astype(np.float32), Dn)
    assert as_float.dtype == np.float32 and np.array_equal(as_float.view(np.uint32), expect.view(np.uint32))
    assert as_u8.dtype == np.uint8 and np.array_equal(as_u8, np.clip(np.rint(expect), 0, 255).astype(np.uint8))
    if u8:
        assert np.array_equal(as_u8[m], ref_con[2][m])                              # the measurement, bit for bit
    if not m.all() and Dn.size >= 100:
        free = expect[~m]
        assert ((free - np.floor(free) == 0.5) & (free > 0) & (free < 255)).any() and (free < 0).any() and (free > 255).any()


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("case", BLOCKS, **_ids)
def test_finish_block(case, u8):
    rng = np.random.default_rng(sum(case) + 3 * u8)
    ref_con, con = _block_case(*case, u8, rng)
    s = case[0]
    Dn = rng.uniform(-20, 280, R.constraint_shape(ref_con)).astype(np.float32)
    got = _host(bf.restore_finish(_dev(Dn), con, False))
    ref = R.finish(ref_con, Dn)
    top = np.maximum(np.abs(Dn).max(), 255.0)
    assert (np.abs(got.astype(np.float64) - ref) <= 8 * EPS * top).all()
    assert np.abs(R.block_means(got.astype(np.float64), s) - ref_con[2].astype(np.float64)).max() <= s * s * 2.0 ** -23 * 255
    assert np.array_equal(_host(bf.restore_finish(_dev(Dn), con, True)), np.clip(np.rint(got), 0, 255).astype(np.uint8))


def test_finish_never_reads_unmeasured_values():
    x = torch.full((1, 5, 7, 3), float("nan"), device="cuda")
    m = torch.zeros((1, 5, 7, 1), dtype=torch.uint8, device="cuda")
    m[0, 2, 3] = 1
    x[0, 2, 3] = 17.25
    con = bf.mask_constraint(x, m)
    Dn = torch.full((1, 5, 7, 3), 100.0, device="cuda")
    out = bf.restore_finish(Dn, con, False)
    assert torch.isfinite(out).all() and (out[0, 2, 3] == 17.25).all() and (out.sum() == 100.0 * 102 + 3 * 17.25)
    d, sumsq = bf.restore_direction(torch.zeros_like(Dn), Dn, con)
    assert torch.isfinite(d).all() and torch.isfinite(sumsq).all()
    assert torch.isfinite(bf.restore_init(con)).all()


# ---- freezing ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(3, 5, 3), (96, 128, 3)], **_ids)
def test_frozen_image_keeps_y_and_count(shape):
    rng = np.random.default_rng(4)
    n = int(np.prod(shape))
    y, d = (_dev(rng.normal(0, 100, (3,) + shape).astype(np.float32)) for _ in range(2))
    t = 7
    # image 0: sigma_t = sigma_l / 2 -> freezes now; image 1 moves; image 2 froze earlier (its count is behind)
    sumsq = torch.tensor([n * (2.55 / 2) ** 2, n * 50.0 ** 2, n * 50.0 ** 2], dtype=torch.float64, device="cuda")
    steps = torch.tensor([t - 1, t - 1, 3], dtype=torch.int32, device="cuda")
    trace = torch.zeros((t, 3), dtype=torch.float64, device="cuda")
    before = y.clone()
    bf.restore_step(y, d, sumsq, steps, t, 0.25, beta=0.5, sigma_l=2.55, seed=1, trace=trace)
    assert torch.equal(y[0], before[0]) and torch.equal(y[2], before[2]) and not torch.equal(y[1], before[1])
    assert steps.tolist() == [t - 1, t, 3]
    assert np.allclose(_host(trace)[t - 1], [2.55 / 2, 50.0, 50.0], rtol=1e-14)
    bf.restore_step(y, d, sumsq, steps, t + 1, 0.25, beta=0.5, sigma_l=2.55, seed=1)        # and at the next iteration
    assert torch.equal(y[0], before[0]) and torch.equal(y[2], before[2]) and steps.tolist() == [t - 1, t + 1, 3]
    edge = torch.tensor([n * 2.55 ** 2 * (1 - 1e-9)] * 3, dtype=torch.float64, device="cuda")   # just below sigma_l: frozen
    steps = torch.full((3,), t - 1, dtype=torch.int32, device="cuda")
    bf.restore_step(y, d, edge, steps, t, 0.25, beta=1.0, sigma_l=2.55)
    assert steps.tolist() == [t - 1] * 3


# ---- the loop ------------------------------------------------------------------------------------------------------------------

def _blur(x):
    p = F.pad(x, (0, 0, 1, 1), mode="replicate")
    x = (p[:, :, :-2] + 2.0 * p[:, :, 1:-1] + p[:, :, 2:]) / 4.0
    p = F.pad(x, (1, 1, 0, 0), mode="replicate")
    return (p[:, :, :, :-2] + 2.0 * p[:, :, :, 1:-1] + p[:, :, :, 2:]) / 4.0


def linear_denoiser(y: torch.Tensor) -> torch.Tensor:
    """D(y) = 0.2 y + 0.8 G(G(y)), float32 [B,H,W,C] -> float32, evaluated in float64 and rounded once"""
    x = y.double().permute(0, 3, 1, 2)
    return (0.2 * x + 0.8 * _blur(_blur(x))).permute(0, 2, 3, 1).contiguous().float()


def test_linear_denoiser_is_the_reference_one():
    y = np.random.default_rng(0).normal(128, 300, (2, 9, 11, 3)).astype(np.float32)
    assert np.abs(_host(linear_denoiser(_dev(y))).astype(np.float64) - R.linear_denoiser(y.astype(np.float64))).max() <= 2 * EPS * 1500


_CASES, _REF = {}, {}
SEED = 3


def _case(name):
    """(reference constraint, device constraint, clean, baseline)"""
    if name not in _CASES:
        ref_con, clean, base = R.cases()[name]
        con = bf.mask_constraint(_dev(ref_con[2]), _dev(ref_con[1])) if ref_con[0] == "mask" else bf.block_constraint(_dev(ref_con[2]), ref_con[1])
        _CASES[name] = (ref_con, con, clean, base)
    return _CASES[name]


def _reference_run(name, beta, storage=np.float64):
    key = (name, beta, storage)
    if key not in _REF:
        _REF[key] = R.restore(R.linear_denoiser, _case(name)[0], beta=beta, max_iterations=400, seed=SEED, storage=storage)
    return _REF[key]


LOOP_CASES = ["mask", "bayer", "s2", "s4"]


@pytest.mark.parametrize("name", LOOP_CASES)
def test_deterministic_loop_matches_reference(name):
    ref_con, con, clean, base = _case(name)
    ref, ref32 = _reference_run(name, 1.0), _reference_run(name, 1.0, np.float32)
    # precondition, on the reference alone: no sigma_t so close to sigma_l that a rounding could move the freezing
    assert (np.abs(ref["trace"] - R.SIGMA_L) >= 1e-3 * R.SIGMA_L).all()
    assert np.array_equal(ref32["iterations"], ref["iterations"])
    f_image, f_trace = np.abs(ref32["image"] - ref["image"]).max(), np.abs(ref32["trace"] - ref["trace"]).max()
    got = bf.restore(linear_denoiser, con, beta=1.0, max_iterations=400, seed=SEED, cast_to_uint8=False, trace=True, check_every=16)
    steps = _host(got.iterations)
    e_image = np.abs(_host(got.image).astype(np.float64) - ref["image"]).max()
    rows = len(ref["trace"])
    e_trace = np.abs(_host(got.trace)[:rows] - ref["trace"]).max()
    print(f"{name}: iterations {steps.tolist()} (reference {ref['iterations'].tolist()}); image error {e_image:.3e} (F {f_image:.3e}), "
          f"trace error {e_trace:.3e} (F {f_trace:.3e})")
    assert np.array_equal(steps, ref["iterations"])
    assert _host(got.converged).all() and got.trace.shape[0] >= rows
    assert (_host(got.trace)[rows:] == _host(got.trace)[rows - 1]).all()            # frozen: sigma_t repeats
    assert np.allclose(_host(got.sigma), ref["trace"][-1], atol=10 * f_trace)
    assert e_image <= 10 * f_image and e_trace <= 10 * f_trace
    # freezing happens on the device: the result does not depend on how often the host looks
    each = bf.restore(linear_denoiser, con, beta=1.0, max_iterations=400, seed=SEED, cast_to_uint8=False, trace=True, check_every=1)
    assert torch.equal(each.image, got.image) and torch.equal(each.iterations, got.iterations)
    assert each.trace.shape[0] == rows and torch.equal(each.trace, got.trace[:rows])
    # an image alone, with its sample id, is the image of the batch
    for b in range(3):
        one = con._replace(anchor=con.anchor[b:b + 1].clone(), mask=None if con.mask is None else con.mask[b:b + 1].clone(),
                           shape=(1,) + tuple(con.shape[1:]))
        alone = bf.restore(linear_denoiser, one, beta=1.0, max_iterations=400, seed=SEED, cast_to_uint8=False, sample_ids=[b])
        assert torch.equal(alone.image[0], got.image[b]) and int(alone.iterations[0]) == steps[b]
    # quality and the constraint
    x = _host(got.image).astype(np.float64)
    where = R.unmeasured(ref_con, x.shape)
    assert R.psnr(x, clean, where) > R.psnr(base, clean, where)
    u8 = bf.restore(linear_denoiser, con, beta=1.0, max_iterations=400, seed=SEED)
    assert u8.image.dtype == torch.uint8 and np.array_equal(_host(u8.image), np.clip(np.rint(_host(got.image)), 0, 255).astype(np.uint8))
    assert u8.trace is None


def _constraint_holds(ref_con, x):
    if ref_con[0] == "mask":
        m = R.measured(ref_con, x.shape)
        return np.array_equal(x[m], ref_con[2].astype(x.dtype)[m])
    s = ref_con[1]
    return np.abs(R.block_means(x.astype(np.float64), s) - ref_con[2].astype(np.float64)).max() <= s * s * 2.0 ** -23 * 255


@pytest.mark.parametrize("name", LOOP_CASES)
def test_stochastic_loop(name):
    ref_con, con, clean, base = _case(name)
    settings = dict(beta=0.01, max_iterations=1000, seed=SEED, cast_to_uint8=False)
    got = bf.restore(linear_denoiser, con, samples=3, **settings)
    again = bf.restore(linear_denoiser, con, samples=3, **settings)
    assert got.image.shape[0] == 9 and torch.equal(got.image, again.image) and torch.equal(got.iterations, again.iterations)
    assert _host(got.converged).all()
    x = _host(got.image)
    for b in range(3):                                                              # the members of one measurement differ
        assert not np.array_equal(x[3 * b], x[3 * b + 1]) and not np.array_equal(x[3 * b + 1], x[3 * b + 2])
    assert not torch.equal(got.image, bf.restore(linear_denoiser, con, samples=3, **dict(settings, seed=SEED + 1)).image)
    member = np.repeat(np.arange(3), 3)
    rep = lambda a: a[member]
    rep_con = (ref_con[0], rep(ref_con[1]) if ref_con[0] == "mask" else ref_con[1], rep(ref_con[2]))
    assert _constraint_holds(rep_con, x)
    # the gain over the fill / nearest up-sampling: at least half of the reference loop's on the same input
    ref = R.restore(R.linear_denoiser, rep_con, beta=0.01, max_iterations=1000, seed=SEED)
    where = R.unmeasured(rep_con, x.shape)
    floor = R.psnr(rep(base), rep(clean), where)
    gain, ref_gain = R.psnr(x.astype(np.float64), rep(clean), where) - floor, R.psnr(ref["image"], rep(clean), where) - floor
    print(f"{name}: iterations {_host(got.iterations).tolist()} (reference {ref['iterations'].tolist()}); gain {gain:.2f} dB "
          f"(reference {ref_gain:.2f} dB over {floor:.2f} dB)")
    assert ref_gain > 0 and gain >= 0.5 * ref_gain


def test_host_arrays_in_host_arrays_out():
    ref_con, con, _, _ = _case("s2")
    host = bf.super_resolve(linear_denoiser, ref_con[2], 2, beta=1.0, max_iterations=400, seed=SEED, trace=True)
    dev = bf.restore(linear_denoiser, con, beta=1.0, max_iterations=400, seed=SEED, trace=True)
    assert all(isinstance(v, np.ndarray) for v in host) and host.image.dtype == np.uint8
    assert np.array_equal(host.image, _host(dev.image)) and np.array_equal(host.iterations, _host(dev.iterations))
    assert np.array_equal(host.trace, _host(dev.trace)) and host.converged.all()
    ref_con, con, _, _ = _case("bayer")
    host = bf.inpaint(linear_denoiser, ref_con[2], ref_con[1], beta=1.0, max_iterations=400, seed=SEED)
    assert np.array_equal(host.image, _host(bf.restore(linear_denoiser, con, beta=1.0, max_iterations=400, seed=SEED).image))
    with pytest.raises(ValueError, match="float32"):
        bf.restore(lambda y: y.double(), con, max_iterations=2)
    short = bf.restore(linear_denoiser, con, beta=1.0, max_iterations=5, seed=SEED, trace=True)
    assert short.iterations.tolist() == [5, 5, 5] and not short.converged.any() and short.trace.shape == (5, 3)


# ---- a real hydra --------------------------------------------------------------------------------------------------------------

def _resnet():
    cfg = O.canonical_config(no_layers=6)
    params, state = O.init_params(O.ResnetSpec.from_config(cfg["model"]), seed=42)
    m = bf.model_builder(cfg["model"], device="cuda").hydra
    m.set_weights(params, state)
    return m


def _unet():
    cfg = U.canonical_config(depth=2, width=1)
    m = bf.model_builder(cfg["model"], device="cuda").hydra
    m.set_weights(U.init_params(U.UnetLaplacianSpec.from_config(cfg["model"]), seed=5))
    return m


@pytest.mark.parametrize("family", ["resnet", "unet"])
def test_real_hydra(family):
    """random weights: no quality is claimed; the run goes through, stays finite and keeps the constraint"""
    module = bf.DenoiserModule({"resnet": _resnet, "unet": _unet}[family]())
    rng = np.random.default_rng(2)
    x = rng.integers(0, 256, (2, 32, 32, 3)).astype(np.uint8)
    m = (rng.random((2, 32, 32, 1)) < 0.5).astype(np.uint8)
    low = rng.integers(0, 256, (2, 16, 16, 3)).astype(np.uint8)
    for ref_con, con in ((("mask", m, x), bf.mask_constraint(_dev(x), _dev(m))), (("block", 2, low), bf.block_constraint(_dev(low), 2))):
        for beta in (1.0, 0.01):
            got = bf.restore(module, con, beta=beta, max_iterations=8, seed=1, cast_to_uint8=False, trace=True, check_every=3)
            image, steps, converged = _host(got.image), _host(got.iterations), _host(got.converged)
            assert np.isfinite(image).all() and np.isfinite(_host(got.trace)).all() and _constraint_holds(ref_con, image)
            rows = got.trace.shape[0]
            assert rows <= 8 and ((steps < rows) == converged).all() and (steps <= rows).all()
            for b in range(2):
                frozen_at = np.nonzero(_host(got.trace)[:, b] <= 2.55)[0]
                assert steps[b] == (frozen_at[0] if len(frozen_at) else rows)
            graphed = bf.restore(bf.GraphedDenoiserModule(module), con, beta=beta, max_iterations=8, seed=1, cast_to_uint8=False,
                                 trace=True, check_every=3)
            assert torch.equal(graphed.image, got.image) and torch.equal(graphed.trace, got.trace)
            as_u8 = bf.restore(module, con, beta=beta, max_iterations=8, seed=1)
            assert as_u8.image.dtype == torch.uint8
            if ref_con[0] == "mask":
                assert _constraint_holds(ref_con, _host(as_u8.image))


# ---- entry refusals ------------------------------------------------------------------------------------------------------------

def test_entries_refuse_bad_arguments():
    lib = N.lib()
    buf = torch.full((4096,), 7.0, device="cuda")                                   # every pointer argument: nothing may be written
    sums = torch.full((64,), 7.0, dtype=torch.float64, device="cuda")
    byte = torch.full((4096,), 7, dtype=torch.uint8, device="cuda")
    steps = torch.full((8,), 7, dtype=torch.int32, device="cuda")
    p, q, s8, st, null, stream = N.ptr(buf), N.ptr(sums), N.ptr(byte), N.ptr(steps), None, N.stream_ptr(buf)
    good = dict(B=1, H=8, W=8, C=3, kind=0, mask=s8, mc=1, factor=1, anchor=s8, a_u8=1)

    def init(**k):
        a = {**good, "y": p, **k}
        return lib.bf_op_restore_init(a["y"], a["B"], a["H"], a["W"], a["C"], a["kind"], a["mask"], a["mc"], a["factor"], a["anchor"],
                                      a["a_u8"], 255.0, 0, null, stream)

    def direction(**k):
        a = {**good, "y": p, "D": p, "d": N.ptr(buf[2048:]), "scratch": q, "bytes": 64 * 8, "sumsq": N.ptr(sums[32:]), **k}
        return lib.bf_op_restore_direction(a["y"], a["D"], a["B"], a["H"], a["W"], a["C"], a["kind"], a["mask"], a["mc"], a["factor"],
                                           a["anchor"], a["a_u8"], a["d"], a["scratch"], a["bytes"], a["sumsq"], stream)

    def step(**k):
        a = {**good, "y": p, "d": N.ptr(buf[2048:]), "sumsq": q, "h": 0.5, "beta": 0.5, "sigma_l": 2.55, "t": 1, "trace": null, "rows": 0,
             "steps": st, **k}
        return lib.bf_op_restore_step(a["y"], a["d"], a["sumsq"], a["B"], a["H"], a["W"], a["C"], a["h"], a["beta"], a["sigma_l"], a["t"],
                                      0, null, a["trace"], a["rows"], a["steps"], stream)

    def finish(**k):
        a = {**good, "D": p, "out": N.ptr(buf[2048:]), **k}
        return lib.bf_op_restore_finish(a["D"], a["B"], a["H"], a["W"], a["C"], a["kind"], a["mask"], a["mc"], a["factor"], a["anchor"],
                                        a["a_u8"], a["out"], 0, stream)

    shapes = [dict(C=0), dict(C=5), dict(B=0), dict(H=0), dict(W=-1), dict(H=32768, W=32768, C=2), dict(H=65536, W=32768, C=1)]
    constraints = [dict(anchor=null), dict(mask=null), dict(mc=2), dict(kind=2), dict(kind=-1), dict(kind=1, factor=1), dict(kind=1, factor=9),
                   dict(kind=1, factor=3), dict(kind=1, factor=2, H=9), dict(kind=1, factor=4, W=10, H=8)]
    for entry in (init, direction, finish):
        for bad in shapes + constraints:
            assert entry(**bad) == N.BF_EINVAL, (entry.__name__, bad)
    for bad in shapes + [dict(y=null), dict(d=null), dict(sumsq=null), dict(steps=null), dict(h=0.0), dict(h=1.5), dict(beta=-0.1),
                         dict(beta=1.1), dict(sigma_l=0.0), dict(t=0), dict(trace=q, rows=0), dict(d=p)]:
        assert step(**bad) == N.BF_EINVAL, bad
    assert init(y=null) == N.BF_EINVAL and finish(D=null) == N.BF_EINVAL and finish(out=null) == N.BF_EINVAL and finish(out=p) == N.BF_EINVAL
    for bad in (dict(y=null), dict(D=null), dict(d=null), dict(scratch=null), dict(sumsq=null), dict(bytes=0), dict(d=p)):
        assert direction(**bad) == N.BF_EINVAL, bad
    assert lib.bf_op_restore_scratch_bytes(1, 32768, 32768, 2) == N.BF_EINVAL and lib.bf_op_restore_scratch_bytes(2, 96, 128, 3) == 2 * 36 * 8
    assert lib.bf_op_restore_scratch_bytes(1, 1024, 1024, 4) == 256 * 8            # at most 256 workgroups per image
    torch.cuda.synchronize()
    assert (buf == 7.0).all() and (sums == 7.0).all() and (byte == 7).all() and (steps == 7).all()      # nothing was launched
    assert init() == N.BF_OK and direction() == N.BF_OK and finish() == N.BF_OK and step() == N.BF_OK  # and the good call is taken
    torch.cuda.synchronize()
