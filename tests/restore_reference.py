"""NumPy fp64 statement of the restoration loop (blind_image_denoising_amd/restore.py, csrc/restore.hip): Kadkhodaie & Simoncelli
2021, Algorithm 2, with a mask or a block-mean constraint.  Images are [B,H,W,C] on the 0..255 scale; a constraint is the tuple
("mask", m uint8 [B,H,W,1 or C], x [B,H,W,C]) or ("block", s, low [B,H/s,W/s,C]).  `storage` = np.float32 holds y, D and d in
float32 between the steps (each formula still evaluated in fp64 and rounded once), which is how the kernels hold them."""
import numpy as np

from oracle.bfcnn_oracle import _philox4x32_10

PHILOX_STREAM = 6
SIGMA_0, SIGMA_L, H0, BETA = 255.0, 2.55, 0.01, 0.01


# ---- the two projections -------------------------------------------------------------------------------------------------------

def measured(con, shape):
    """bool [B,H,W,C]: the mask, broadcast over the channels (all True for a block constraint)"""
    if con[0] == "mask":
        return np.broadcast_to(con[1] != 0, shape)
    return np.ones(shape, bool)


def project(con, v):
    v = np.asarray(v, np.float64)
    if con[0] == "mask":
        return np.where(measured(con, v.shape), v, 0.0)
    s = con[1]
    B, H, W, C = v.shape
    means = v.reshape(B, H // s, s, W // s, s, C).mean(axis=(2, 4))
    return np.repeat(np.repeat(means, s, axis=1), s, axis=2)


def anchor(con, shape):
    if con[0] == "mask":
        return np.where(measured(con, shape), np.asarray(con[2], np.float64), 0.0)
    s = con[1]
    return np.repeat(np.repeat(np.asarray(con[2], np.float64), s, axis=1), s, axis=2)


def constraint_shape(con):
    if con[0] == "mask":
        return tuple(con[2].shape)
    B, h, w, C = con[2].shape
    return (B, h * con[1], w * con[1], C)


# ---- the normals ---------------------------------------------------------------------------------------------------------------

def normals(shape, seed: int, sample_id: int, t: int) -> np.ndarray:
    """z of ONE image [H,W,C], fp64: elements 4 g .. 4 g + 3 share philox(counter = (g, sample_id, t, 6), key = seed); words (0, 1)
    give the cosine and sine branch of Box-Muller, words (2, 3) the next two"""
    n = int(np.prod(shape))
    g = np.arange((n + 3) // 4, dtype=np.uint64)
    r = _philox4x32_10(g, np.full_like(g, sample_id), np.full_like(g, t), np.full_like(g, PHILOX_STREAM), seed & 0xFFFFFFFF,
                       (seed >> 32) & 0xFFFFFFFF)
    z = np.empty((g.size, 4), np.float64)
    for h in range(2):
        u1 = ((r[2 * h] >> np.uint64(8)).astype(np.float64) + 1.0) / 16777216.0
        u2 = (r[2 * h + 1] >> np.uint64(8)).astype(np.float64) / 16777216.0
        rad = np.sqrt(-2.0 * np.log(u1))
        z[:, 2 * h] = rad * np.cos(2.0 * np.pi * u2)
        z[:, 2 * h + 1] = rad * np.sin(2.0 * np.pi * u2)
    return z.reshape(-1)[:n].reshape(shape)


def batch_normals(shape, seed, sample_ids, t):
    return np.stack([normals(shape[1:], seed, int(sample_ids[b]), t) for b in range(shape[0])])


# ---- init, direction, step, finish ---------------------------------------------------------------------------------------------

def init(con, sigma_0=SIGMA_0, seed=0, sample_ids=None):
    shape = constraint_shape(con)
    ids = np.arange(shape[0]) if sample_ids is None else sample_ids
    return 127.5 * (1.0 - project(con, np.ones(shape))) + anchor(con, shape) + sigma_0 * batch_normals(shape, seed, ids, 0)


def direction(con, y, D):
    """(d, sum d^2 per image)"""
    y, D = np.asarray(y, np.float64), np.asarray(D, np.float64)
    d = D - y + anchor(con, y.shape) - project(con, D)
    return d, (d * d).reshape(d.shape[0], -1).sum(axis=1)


def step_size(t, h0=H0):
    return h0 * t / (1.0 + h0 * (t - 1))


def gamma_squared(h, beta, sigma):
    return ((1.0 - beta * h) ** 2 - (1.0 - h) ** 2) * sigma ** 2


def step(y, d, sumsq, steps, t, h, beta=BETA, sigma_l=SIGMA_L, seed=0, sample_ids=None):
    """(new y, new steps, sigma_t): the images with steps == t - 1 and sigma_t > sigma_l move"""
    y, d = np.asarray(y, np.float64), np.asarray(d, np.float64)
    B = y.shape[0]
    n = y[0].size
    ids = np.arange(B) if sample_ids is None else sample_ids
    sigma = np.sqrt(np.asarray(sumsq, np.float64) / n)
    moves = (np.asarray(steps) == t - 1) & (sigma > sigma_l)
    out, new_steps = y.copy(), np.asarray(steps).copy()
    for b in np.nonzero(moves)[0]:
        gamma = np.sqrt(max(gamma_squared(h, beta, sigma[b]), 0.0))
        out[b] = y[b] + h * d[b] + (gamma * normals(y.shape[1:], seed, int(ids[b]), t) if gamma > 0.0 else 0.0)
        new_steps[b] = t
    return out, new_steps, sigma


def finish(con, D):
    D = np.asarray(D, np.float64)
    x = D - project(con, D) + anchor(con, D.shape)
    if con[0] == "mask":
        x = np.where(measured(con, D.shape), np.asarray(con[2], np.float64), x)
    return x


def to_uint8(x):
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


# ---- the loop ------------------------------------------------------------------------------------------------------------------

def restore(denoiser, con, sigma_0=SIGMA_0, sigma_l=SIGMA_L, h0=H0, beta=BETA, max_iterations=2000, seed=0, sample_ids=None,
            storage=np.float64):
    """dict(image fp64, iterations [B], trace [iterations run, B], y the final iterate); denoiser: fp64 [B,H,W,C] -> the same"""
    hold = lambda a: a.astype(storage).astype(np.float64)
    y = hold(init(con, sigma_0, seed, sample_ids))
    steps = np.zeros(y.shape[0], np.int64)
    trace = []
    for t in range(1, max_iterations + 1):
        D = hold(denoiser(y))
        d, sumsq = direction(con, y, D)
        y, steps, sigma = step(y, hold(d), sumsq, steps, t, step_size(t, h0), beta, sigma_l, seed, sample_ids)
        y = hold(y)
        trace.append(sigma)
        if (steps < t).all():
            break
    return {"image": hold(finish(con, hold(denoiser(y)))), "iterations": steps, "trace": np.array(trace), "y": y}


# ---- the linear test denoiser and the scenes -----------------------------------------------------------------------------------

def binomial_blur(x):
    """G: the 3 x 3 binomial blur (1 2 1)^T (1 2 1) / 16 with replicated edges, on [B,H,W,C]"""
    p = np.pad(x, ((0, 0), (1, 1), (0, 0), (0, 0)), mode="edge")
    x = (p[:, :-2] + 2.0 * p[:, 1:-1] + p[:, 2:]) / 4.0
    p = np.pad(x, ((0, 0), (0, 0), (1, 1), (0, 0)), mode="edge")
    return (p[:, :, :-2] + 2.0 * p[:, :, 1:-1] + p[:, :, 2:]) / 4.0


def linear_denoiser(y):
    """D(y) = 0.2 y + 0.8 G(G(y)): linear and a contraction, so rounding does not grow along the loop"""
    return 0.2 * y + 0.8 * binomial_blur(binomial_blur(y))


def scenes(H=24, W=32, C=3):
    """float64 [3,H,W,C]: a smooth pattern, a flat image at 90, the pattern flipped"""
    i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    wave = 128.0 + 60.0 * np.sin(i / 6.0) * np.cos(j / 5.0) + 30.0 * np.sin((i + j) / 9.0)
    planes = np.stack([wave, np.full_like(wave, 90.0), wave[::-1, ::-1]])
    return np.repeat(planes[..., None], C, axis=3)


def bayer_mask(B, H, W):
    m = np.zeros((B, H, W, 3), np.uint8)
    m[:, 0::2, 0::2, 0] = 1
    m[:, 0::2, 1::2, 1] = 1
    m[:, 1::2, 0::2, 1] = 1
    m[:, 1::2, 1::2, 2] = 1
    return m


def block_means(x, s):
    B, H, W, C = x.shape
    return x.reshape(B, H // s, s, W // s, s, C).mean(axis=(2, 4))


def psnr(a, b, where=None):
    e = (np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2
    mse = e[where].mean() if where is not None else e.mean()
    return 10.0 * np.log10(255.0 ** 2 / mse) if mse > 0 else np.inf


def cases(seed=0):
    """{name: (constraint, clean scenes, baseline image)} for the loop tests: a random half mask, the Bayer mask, s = 2 and s = 4;
    the measurements are the clean scenes rounded to uint8"""
    clean = scenes()
    u8 = to_uint8(clean)
    B, H, W, C = clean.shape
    rng = np.random.default_rng(seed)
    half = (rng.random((B, H, W, 1)) < 0.5).astype(np.uint8)
    out = {}
    for name, m in (("mask", half), ("bayer", bayer_mask(B, H, W))):
        fill = np.where(np.broadcast_to(m != 0, u8.shape), u8, 127.5)
        out[name] = (("mask", m, u8), clean, fill)
    for s in (2, 4):
        low = block_means(u8.astype(np.float64), s).astype(np.float32)
        out[f"s{s}"] = (("block", s, low), clean, np.repeat(np.repeat(low.astype(np.float64), s, axis=1), s, axis=2))
    return out


def unmeasured(con, shape):
    """where quality is scored: the samples the mask leaves out; everything for a block constraint"""
    return ~measured(con, shape) if con[0] == "mask" else np.ones(shape, bool)
