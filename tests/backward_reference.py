"""Float64 restatement of the small training operators of csrc/train_prims.hip and csrc/train_generic.hip, independent of the
package.  Not a test module: the yardstick of tests/test_backward_reference.py (every backward here against central finite
differences of its own forward) and of tests/test_gpu_backward_ops.py (the HIP entry points against these functions).

Forwards are torch-CPU float64 functions of NHWC tensors, the same formulas as oracle/unet_torch.py and
oracle/resnet_generic_torch.py where those have them.  A backward is `vjp` (torch autograd of the forward) unless a rule has to
be pinned; those are written out in closed form and rely on no library's convention:
  * maxpool2_bwd: the gradient goes to the FIRST maximum of each 2 x 2 "same" window in row-major order (partial windows at
    an odd edge);
  * head_out_bwd and selector_mix_bwd (hard): a clip passes the gradient on its closed interval;
  * act_bwd, multiplier_bwd, relu_shift_bwd: a ReLU passes nothing at exactly zero.
`kink_distance_*` give the distance of an input from the nearest kink of an operator, for the tests to assert on."""
import numpy as np
import torch

from oracle import bfcnn_oracle as O
from oracle import resnet_generic_torch as RT
from oracle import unet_oracle as U
from oracle import unet_torch as T

DT = torch.float64


def t64(a, requires_grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=DT, requires_grad=requires_grad)


def vjp(fn, inputs, cotangents):
    """gradients of sum_k <fn(*inputs)[k], cotangents[k]> with respect to every input: float64 arrays"""
    xs = [t64(a, True) for a in inputs]
    ys = fn(*xs)
    ys = ys if isinstance(ys, (tuple, list)) else [ys]
    cs = cotangents if isinstance(cotangents, (tuple, list)) else [cotangents]
    total = sum((y * t64(c)).sum() for y, c in zip(ys, cs))
    total.backward()
    return [np.zeros(x.shape) if x.grad is None else x.grad.numpy() for x in xs]


def jvp(fn, inputs, tangents):
    """directional derivative of fn(*inputs) along the tangents (forward mode by double backward): float64 arrays, one per
    output -- the J v of the adjoint identity <J v, y> = <v, J^T y> where no entry point computes it"""
    xs = [t64(a, True) for a in inputs]
    ys = fn(*xs)
    ys = list(ys) if isinstance(ys, (tuple, list)) else [ys]
    out = []
    for y in ys:
        dummy = torch.zeros_like(y, requires_grad=True)
        g = torch.autograd.grad(y, xs, dummy, create_graph=True, allow_unused=True)
        s = sum((gi * t64(t)).sum() for gi, t in zip(g, tangents) if gi is not None)
        out.append(torch.autograd.grad(s, dummy, allow_unused=True)[0].numpy())
    return out


def numeric_vjp(fn, inputs, cotangents, which, step=1e-6):
    """central finite differences of sum_k <fn(*inputs)[k], cotangents[k]> with respect to inputs[which]"""
    cs = cotangents if isinstance(cotangents, (tuple, list)) else [cotangents]
    cs = [t64(c) for c in cs]

    def scalar(args):
        ys = fn(*[t64(a) for a in args])
        ys = ys if isinstance(ys, (tuple, list)) else [ys]
        return float(sum((y * c).sum() for y, c in zip(ys, cs)))
    base = [np.array(a, np.float64) for a in inputs]
    g = np.zeros(base[which].shape)
    flat, gf = base[which].reshape(-1), g.reshape(-1)
    for i in range(flat.size):
        keep = flat[i]
        flat[i] = keep + step
        hi = scalar(base)
        flat[i] = keep - step
        lo = scalar(base)
        flat[i] = keep
        gf[i] = (hi - lo) / (2.0 * step)
    return g


# ---- element-wise -------------------------------------------------------------------------------------------------------------

def act(x, code, alpha=0.0):
    """activation codes of bf_op_act_bwd: 0 linear, 1 relu, 2 leaky relu(alpha), 3 exact-erf gelu, 4 tanh"""
    if code == 0:
        return x
    if code == 1:
        return torch.relu(x)
    if code == 2:
        return torch.where(x > 0, x, alpha * x)
    if code == 3:
        return 0.5 * x * (1.0 + torch.erf(x / np.sqrt(2.0)))
    if code == 4:
        return torch.tanh(x)
    raise NotImplementedError(code)


def act_bwd(ref, dy, code, alpha=0.0, ref_is_output=False):
    """dx = dy act'(.), ref the activation's input or (relu, leaky relu, tanh) its output; closed form, relu' (0) = 0"""
    ref, dy = np.asarray(ref, np.float64), np.asarray(dy, np.float64)
    if code == 0:
        return dy.copy()
    if code == 1:
        return dy * (ref > 0)
    if code == 2:
        return dy * np.where(ref > 0, 1.0, alpha)
    if code == 3:
        if ref_is_output:
            raise NotImplementedError("gelu is not invertible from its output")
        cdf = 0.5 * (1.0 + torch.erf(t64(ref) / np.sqrt(2.0)).numpy())
        return dy * (cdf + ref * np.exp(-0.5 * ref * ref) / np.sqrt(2.0 * np.pi))
    if code == 4:
        th = ref if ref_is_output else np.tanh(ref)
        return dy * (1.0 - th * th)
    raise NotImplementedError(code)


def multiplier(w):
    """ChannelLearnableMultiplier: tanh(relu(1 + w))"""
    return torch.tanh(torch.relu(1.0 + w))


def multiplier_bwd(w, dm):
    w, dm = np.asarray(w, np.float64), np.asarray(dm, np.float64)
    m = np.tanh(np.maximum(1.0 + w, 0.0))
    return np.where(1.0 + w > 0, dm * (1.0 - m * m), 0.0)


def scale_add(res, t, m, s):
    """res + t m[c] s[b] on [B,hw,C]; res, m, s may be None"""
    out = t
    if m is not None:
        out = out * m.reshape(1, 1, -1)
    if s is not None:
        out = out * s.reshape(-1, 1, 1)
    return out if res is None else res + out


def scale_add_bwd(t, m, s, dy):
    """(dt, dm) of scale_add; dm as if m were all ones when it is None (what the kernel's reduction yields)"""
    C = np.asarray(t).shape[-1]
    mm = np.ones(C) if m is None else m
    if s is None:
        dt, dm = vjp(lambda a, b: scale_add(None, a, b, None), [t, mm], dy)
    else:
        dt, dm = vjp(lambda a, b: scale_add(None, a, b, t64(s)), [t, mm], dy)
    return dt, dm


def selector_gate(u, soft):
    p = 2.5 - u
    return torch.sigmoid(p) if soft else torch.clamp(0.2 * p + 0.5, 0.0, 1.0)


def selector_mix(x1, x2, u, soft):
    s = selector_gate(u, soft)
    return x1 * s + x2 * (1.0 - s)


def selector_mix_bwd(x1, x2, u, dy, soft):
    """(dx1, dx2, du), closed form; hard: clip(0.2 (2.5 - u) + 0.5, 0, 1) passes the gradient where 0 <= . <= 1"""
    x1, x2, u, dy = (np.asarray(a, np.float64) for a in (x1, x2, u, dy))
    p = 2.5 - u
    if soft:
        s = 1.0 / (1.0 + np.exp(-p))
        dsdu = -s * (1.0 - s)
    else:
        lin = 0.2 * p + 0.5
        s = np.clip(lin, 0.0, 1.0)
        dsdu = np.where(clip_passes(lin, 0.0, 1.0), -0.2, 0.0)
    return dy * s, dy * (1.0 - s), dy * (x1 - x2) * dsdu


def kink_distance_selector(u):
    """distance of u from the two ends of the hard selector's clip (u = 0 and u = 5)"""
    u = np.asarray(u, np.float64)
    return np.minimum(np.abs(u), np.abs(u - 5.0)).min()


def pass_filter(x, a, b, highpass):
    f = torch.tanh(a * x) ** b
    return x * f if highpass else x * (1.0 - f)


def pass_filter_bwd(x, dy, a, b, highpass):
    return vjp(lambda v: pass_filter(v, a, b, highpass), [x], dy)[0]


def center_sq(x, mean):
    return (x - mean) ** 2


def center_scale(x, mean, var, eps):
    return (x - mean) / torch.sqrt(var + eps)


def center_scale_bwd(x, mean, var, dy, eps):
    """(dd, dv): the gradients of y = d (v + eps)^-1/2 with respect to d = x - mean and to v"""
    x, mean, var, dy = (np.asarray(a, np.float64) for a in (x, mean, var, dy))
    r = 1.0 / np.sqrt(var + eps)
    return dy * r, -0.5 * dy * (x - mean) * r ** 3


def center_sq_bwd(x, mean, t, dd):
    """dd + 2 (x - mean) t: the gradient at d = x - mean through both of its uses"""
    x, mean, t, dd = (np.asarray(a, np.float64) for a in (x, mean, t, dd))
    return dd + 2.0 * (x - mean) * t


def avgpool_same(x, pool, stride):
    return RT.avgpool_same(x, pool, stride)


def avgpool_same_bwd(dp, shape, pool, stride):
    return vjp(lambda v: avgpool_same(v, pool, stride), [np.zeros(shape)], dp)[0]


def local_normalization(x, pool, eps):
    """(x - m) / sqrt(pool((x - m)^2) + eps), m = pool(x), pool = AveragePooling2D(pool, strides 1, same)"""
    m = avgpool_same(x, pool, (1, 1))
    return center_scale(x, m, avgpool_same(center_sq(x, m), pool, (1, 1)), eps)


def sigmoid_gate(enc, o, up):
    out = enc * torch.sigmoid(4.0 * o)
    return out if up is None else out + up


def sigmoid_gate_bwd(enc, o, dy):
    """(denc, do), closed form"""
    enc, o, dy = (np.asarray(a, np.float64) for a in (enc, o, dy))
    s = 1.0 / (1.0 + np.exp(-4.0 * o))
    return dy * s, dy * enc * 4.0 * s * (1.0 - s)


# ---- per-channel ----------------------------------------------------------------------------------------------------------------

def linear_shift(w0, w1, C):
    """w0 ([C] or [1]) + w1 as a [C] vector"""
    return (w0 + w1).expand(C) if w0.numel() == 1 else w0 + w1


def relu_shift(w0, w1, C):
    return torch.relu(linear_shift(w0, w1, C))


def relu_shift_bwd(w0, w1, dm):
    """dw0 from dm [C]: dm [w0 + w1 > 0], summed over the channels for the scalar form"""
    w0, dm = np.asarray(w0, np.float64), np.asarray(dm, np.float64)
    if w0.size == 1:
        return np.array([dm.sum() if w0.reshape(-1)[0] + w1 > 0 else 0.0])
    return np.where(w0 + w1 > 0, dm, 0.0)


def channel_mean_broadcast(x, rows_out):
    """x [B,hw,C] -> [B,rows_out,C]: the per-sample channel mean on every row"""
    return x.mean(dim=1, keepdim=True).expand(-1, rows_out, -1)


# ---- windows --------------------------------------------------------------------------------------------------------------------

def gaussian_window(k):
    return U.gaussian_kernel_3((k, k))


def smooth_split(x, k, gauss, down_stride):
    """(lap, down): smooth = k x k average (divisor: taps inside the image) or the fixed Gaussian [k,k] (zero padding), TF same
    padding; lap = x - smooth; down = smooth (stride 1) or smooth[:, ::2, ::2]"""
    if gauss is None:
        smooth = T._avg_pool_same(x, k)
    else:
        smooth = T._depthwise(x, t64(gauss)[:, :, None, None].repeat(1, 1, x.shape[-1], 1))
    return x - smooth, (smooth if down_stride == 1 else smooth[:, ::2, ::2, :])


def smooth_split_bwd(dlap, ddown, k, gauss, down_stride):
    return vjp(lambda v: smooth_split(v, k, gauss, down_stride), [np.zeros(np.asarray(dlap).shape)], [dlap, ddown])[0]


def upsample2x(x, bilinear):
    return T._up2(x) if bilinear else T._up2_nearest(x)


def upsample2x_bwd(dy, bilinear):
    B, H2, W2, C = np.asarray(dy).shape
    return vjp(lambda v: upsample2x(v, bilinear), [np.zeros((B, H2 // 2, W2 // 2, C))], dy)[0]


def resize_bilinear(x, oh, ow):
    return T._resize(x, oh, ow)


def resize_bilinear_bwd(dy, H, W):
    B, oh, ow, C = np.asarray(dy).shape
    return vjp(lambda v: resize_bilinear(v, oh, ow), [np.zeros((B, H, W, C))], dy)[0]


def maxpool2(x):
    """MaxPooling2D(2, 2, same) on a float64 array [B,H,W,C]: padded taps are ignored"""
    return U.max_pool_2x2_same(np.asarray(x, np.float64))


def maxpool2_bwd(x, dy):
    """dx = dy at the first maximum (row-major: (0,0), (0,1), (1,0), (1,1)) of each window, 0 elsewhere; written as loops"""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    B, H, W, C = x.shape
    dx = np.zeros_like(x)
    for b in range(B):
        for oy in range((H + 1) // 2):
            for ox in range((W + 1) // 2):
                taps = [(2 * oy + i, 2 * ox + j) for i in (0, 1) for j in (0, 1) if 2 * oy + i < H and 2 * ox + j < W]
                for c in range(C):
                    best = taps[0]
                    for yx in taps[1:]:
                        if x[b, yx[0], yx[1], c] > x[b, best[0], best[1], c]:
                            best = yx
                    dx[b, best[0], best[1], c] = dy[b, oy, ox, c]
    return dx


# ---- weight gradients -----------------------------------------------------------------------------------------------------------

def normalize(x, v_min, v_max):
    return (torch.clamp(x, v_min, v_max) - v_min) / (v_max - v_min) - 0.5


def conv2d(x, w, value_range=None):
    """k x k convolution (same, stride 1) of the image, normalised first when a value range is given"""
    return T._conv(x if value_range is None else normalize(x, *value_range), w)


def conv2d_wgrad(x, dy, k, cin, cout, value_range=None):
    return vjp(lambda w: conv2d(t64(x), w, value_range), [np.zeros((k, k, cin, cout))], dy)[0]


def dense2_selector(p, w0, w1, alpha0):
    """bf_op_dense2 in its selector form: relu(leaky(p W0) W1), no biases"""
    h = p @ w0
    return torch.relu(torch.where(h > 0, h, alpha0 * h) @ w1)


def dense2_bwd(p, w0, w1, du, alpha0):
    """(dp, dW0, dW1)"""
    return vjp(lambda a, b, c: dense2_selector(a, b, c, alpha0), [p, w0, w1], du)


def dense2_inputs(rng, n, Cs, C, C8, alpha0, clear=2e-3):
    """float32-exact p [n,Cs], W0 [Cs,C8], W1 [C8,C] with no hidden or final pre-activation within `clear` of zero: a row that
    comes too close is drawn again"""
    w0 = (rng.standard_normal((Cs, C8)) / np.sqrt(Cs)).astype(np.float32)
    w1 = (rng.standard_normal((C8, C)) / np.sqrt(C8)).astype(np.float32)
    p = rng.standard_normal((n, Cs)).astype(np.float32)
    for _ in range(200):
        h = p.astype(np.float64) @ w0.astype(np.float64)
        u = np.where(h > 0, h, alpha0 * h) @ w1.astype(np.float64)
        bad = (np.abs(h) < clear).any(axis=1) | (np.abs(u) < clear).any(axis=1)
        if not bad.any():
            return p, w0, w1
        p[bad] = rng.standard_normal((int(bad.sum()), Cs)).astype(np.float32)
    raise AssertionError("no clearance from zero")


def kink_distance_dense2(p, w0, w1, alpha0):
    p, w0, w1 = (np.asarray(a, np.float64) for a in (p, w0, w1))
    h = p @ w0
    u = np.where(h > 0, h, alpha0 * h) @ w1
    return min(np.abs(h).min(), np.abs(u).min())


# ---- head and loss --------------------------------------------------------------------------------------------------------------

def head_p(h, w1):
    """0.51 tanh(2 h W1): the head's output before the clip"""
    return 0.51 * torch.tanh(2.0 * (h @ w1))


def head_out(h, w1, denormalize, v_min=0.0, v_max=255.0):
    """h [npix,hf], w1 [hf,co]: (clip(p, -0.5, 0.5) + 0.5) (v_max - v_min) + v_min, or p itself"""
    p = head_p(h, w1)
    return (torch.clamp(p, -0.5, 0.5) + 0.5) * (v_max - v_min) + v_min if denormalize else p


def clip_passes(p, lo=-0.5, hi=0.5):
    """where clip(p, lo, hi) hands the gradient on: the closed interval, both ends included"""
    p = np.asarray(p, np.float64)
    return (p >= lo) & (p <= hi)


def head_out_bwd(h, w1, dpred, denormalize, v_min=0.0, v_max=255.0):
    """(dh, dw1), closed form: dh1 = dpred [|p| <= 0.5] (v_max - v_min) 1.02 (1 - th^2), the bracket and the range only when
    denormalising; dh = dh1 W1^T; dw1 = h^T dh1"""
    h, w1, dpred = (np.asarray(a, np.float64) for a in (h, w1, dpred))
    th = np.tanh(2.0 * (h @ w1))
    g = dpred.copy()
    if denormalize:
        p = 0.51 * th
        g = g * np.where(clip_passes(p), v_max - v_min, 0.0)
    dh1 = g * 1.02 * (1.0 - th * th)
    return dh1 @ w1.T, h.T @ dh1


def kink_distance_head(h, w1):
    p = 0.51 * np.tanh(2.0 * (np.asarray(h, np.float64) @ np.asarray(w1, np.float64)))
    return np.abs(np.abs(p) - 0.5).min()


def head_inputs(rng, npix, hf, co, spread=1.0, clear=2e-3):
    """float32-exact h [npix,hf] and w1 [hf,co] with h W1 of standard deviation about `spread` (so a good share of p lies
    beyond 0.5 on both sides) and no p within `clear` of the clip ends: a pixel that comes too close has its row of h stretched"""
    h = rng.standard_normal((npix, hf)).astype(np.float32)
    w1 = (rng.standard_normal((hf, co)) * spread / np.sqrt(hf)).astype(np.float32)
    for _ in range(64):
        p = 0.51 * np.tanh(2.0 * (h.astype(np.float64) @ w1.astype(np.float64)))
        bad = (np.abs(np.abs(p) - 0.5) < clear).any(axis=1)
        if not bad.any():
            return h, w1
        h[bad] *= np.float32(1.07)
    raise AssertionError("no clearance from the clip ends")


def loss_spec(hinge=0.0, cutoff=255.0, mae_multiplier=1.0, mse_multiplier=0.0, ssim_multiplier=0.0):
    return O.LossSpec(hinge=hinge, cutoff=cutoff, mae_multiplier=mae_multiplier, mse_multiplier=mse_multiplier,
                      ssim_multiplier=ssim_multiplier, regularization=0.0)


def denoiser_loss(ls, gt, pred):
    """oracle/unet_torch.denoiser_loss: {total_loss, mae_loss, mse_loss, ssim_loss} as float64 scalars"""
    return T.denoiser_loss(ls, gt, pred)


def denoiser_loss_grad(ls, gt, pred, depth_weight):
    """(loss dict as floats, d(total_loss depth_weight) / dpred)"""
    p = t64(pred, True)
    dl = denoiser_loss(ls, t64(gt), p)
    (dl["total_loss"] * depth_weight).backward()
    return {k: float(v.detach()) for k, v in dl.items()}, p.grad.numpy()


def kink_distance_loss(ls, gt, pred):
    """distance of the error from the kinks of the loss: e = 0 and |e| = hinge (the cutoffs lie beyond 8-bit errors)"""
    e = np.abs(np.asarray(gt, np.float64) - np.asarray(pred, np.float64))
    return min(e.min(), np.abs(e - ls.hinge).min()) if ls.hinge > 0 else e.min()
