"""NumPy restatement of the signal-dependent noise chain (csrc/noise_level.hip, the camera noise of csrc/augment.hip, the affine
sums of csrc/risk.hip and their host sides), independent of the package.  Not a test module: the yardstick of
tests/test_noise_level.py and tests/test_gpu_noise_level.py."""
import numpy as np

import noise_reference as NR
import risk_reference as RR
from oracle import bfcnn_oracle as O

LEVELS = 16


def cells(plane: np.ndarray):
    """(q, s, excluded) per complete 2x2 cell of ONE uint8 plane [H,W]: int64 q = |x00 - x01 - x10 + x11|, s = the sum of the four
    samples, excluded = a sample is 0 or 255; the last row / column of an odd size is dropped"""
    H, W = plane.shape
    x = plane[:H // 2 * 2, :W // 2 * 2].astype(np.int64)
    x00, x01, x10, x11 = x[0::2, 0::2], x[0::2, 1::2], x[1::2, 0::2], x[1::2, 1::2]
    sat = np.zeros(x00.shape, bool)
    for v in (x00, x01, x10, x11):
        sat |= (v == 0) | (v == 255)
    return np.abs(x00 - x01 - x10 + x11), x00 + x01 + x10 + x11, sat


def noise_level_statistics(images: np.ndarray):
    """(levels [B,C,16,3] float64 = (n, sum of s, sigma_l), excluded [B,C] float64)"""
    assert images.ndim == 4 and images.dtype == np.uint8
    B, H, W, C = images.shape
    levels, excluded = np.zeros((B, C, LEVELS, 3), np.float64), np.zeros((B, C), np.float64)
    for b in range(B):
        for c in range(C):
            q, s, sat = cells(images[b, :, :, c])
            excluded[b, c] = sat.sum()
            level = s >> 6
            for l in range(LEVELS):
                pick = ~sat & (level == l)
                hist = np.bincount(q[pick], minlength=NR.HIST_BINS)
                levels[b, c, l] = (pick.sum(), s[pick].sum(), NR.grouped_median(hist) / 2.0 / NR.MAD_TO_SIGMA)
    return levels, excluded


def fit_plane(levels: np.ndarray, fallback_variance: float, min_cells: int = 64):
    """(gain, offset) of ONE plane from its levels [16,3]: weighted least squares of sigma_l^2 on sum_s / (4 n), weights n, over
    the levels with n >= min_cells, with the fallbacks of noise_level.fit_noise_levels"""
    use = levels[:, 0] >= min_cells
    if not use.any():
        return 0.0, float(fallback_variance)
    w = levels[use, 0]
    m = levels[use, 1] / (4.0 * w)
    v = levels[use, 2] ** 2
    mean_m, mean_v = (w * m).sum() / w.sum(), (w * v).sum() / w.sum()
    sxx = (w * (m - mean_m) ** 2).sum()
    gain = (w * (m - mean_m) * (v - mean_v)).sum() / sxx if use.sum() >= 2 and sxx > 0 else -1.0
    if gain < 0:
        return 0.0, float(mean_v)
    offset = mean_v - gain * mean_m
    if offset < 0:
        return float((w * m * v).sum() / (w * m * m).sum()), 0.0
    return float(gain), float(offset)


def noise_level_function(images: np.ndarray, min_cells: int = 64):
    """(gain [B,C], offset [B,C]) of a uint8 batch"""
    levels, _ = noise_level_statistics(images)
    B, C = levels.shape[:2]
    fallback = NR.noise_statistics(images)[:, :, 2] ** 2
    fit = np.array([[fit_plane(levels[b, c], fallback[b, c], min_cells) for c in range(C)] for b in range(B)], np.float64)
    return fit[:, :, 0], fit[:, :, 1]


def sigma_at(gain, offset, x):
    return np.sqrt(np.maximum(gain * x + offset, 0.0))


def camera_normals(shape, seed: int) -> np.ndarray:
    """the untruncated standard normal z of every element of ONE image [H,W,C], fp64: Box-Muller on words 0 and 1 of
    philox(counter = (lo32 e, hi32 e, 0, 3), key = seed), e the element's flat index"""
    e = np.arange(int(np.prod(shape)), dtype=np.uint64)
    r = O._philox4x32_10(e & np.uint64(0xFFFFFFFF), e >> np.uint64(32), np.zeros_like(e), np.full_like(e, 3), seed & 0xFFFFFFFF,
                         (seed >> 32) & 0xFFFFFFFF)
    u1 = ((r[0] >> np.uint64(8)).astype(np.float64) + 1.0) / 16777216.0
    u2 = (r[1] >> np.uint64(8)).astype(np.float64) / 16777216.0
    return (np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)).reshape(shape)


def camera_noise(clean: np.ndarray, gain, read_sigma, seed: int = 0) -> np.ndarray:
    """clip(rint(x + sqrt(gain_c x + read_sigma_c^2) z), 0, 255) in fp64 on a uint8 batch [B,H,W,C]; the parameters as the float32
    values the kernel receives"""
    C = clean.shape[3]
    g = np.broadcast_to(np.asarray(gain, np.float32), (C,)).astype(np.float64)
    r = np.broadcast_to(np.asarray(read_sigma, np.float32), (C,)).astype(np.float64)
    x = clean.astype(np.float64)
    z = camera_normals(clean.shape[1:], seed)[None]
    return np.clip(np.rint(x + np.sqrt(g * x + r * r) * z), 0, 255).astype(np.uint8)


def risk_sums_affine(y: np.ndarray, f: np.ndarray, probes: int, amplitude: int, seed: int) -> np.ndarray:
    """float64 [B, C, 2 + 2 probes] = (R, Y, D_1..K, Dy_1..K); f = [(1 + probes) B, H, W, C]"""
    B, K = y.shape[0], probes
    base = RR.risk_sums(y, f, probes, amplitude, seed)
    f = f.astype(np.float64).reshape((1 + K, B) + y.shape[1:])
    yd = y.astype(np.float64)
    out = np.zeros((B, y.shape[3], 2 + 2 * K), np.float64)
    out[:, :, 0] = base[:, :, 0]
    out[:, :, 1] = y.astype(np.int64).sum(axis=(1, 2))
    out[:, :, 2:2 + K] = base[:, :, 1:]
    for p in range(1, K + 1):
        s = np.stack([RR.probe_signs(img, p, amplitude, seed) for img in y]).astype(np.float64)
        out[:, :, 1 + K + p] = (yd * s * (f[p] - f[0])).sum(axis=(1, 2))
    return out


def risk_from_affine_sums(sums: np.ndarray, gain, offset, height: int, width: int, amplitude: int) -> dict:
    """the host formula on sums [B, C, 2 + 2 K]; gain, offset broadcast to [B, C]"""
    B, C = sums.shape[:2]
    K = (sums.shape[2] - 2) // 2
    hw = float(height * width)
    g, o = np.broadcast_to(np.asarray(gain, np.float64), (B, C)), np.broadcast_to(np.asarray(offset, np.float64), (B, C))
    R, Y, D, Dy = sums[:, :, 0], sums[:, :, 1], sums[:, :, 2:2 + K], sums[:, :, 2 + K:]
    mse_c = (R - (g * Y + o * hw) + 2.0 * (g * Dy.mean(axis=2) + o * D.mean(axis=2)) / amplitude) / hw
    return {"mse": mse_c.mean(axis=1), "sigma": np.sqrt(g * Y / hw + o), "residual_rms": np.sqrt((R / hw).mean(axis=1)),
            "divergence": (D.mean(axis=2) / amplitude / hw).mean(axis=1)}


def estimate_risk_affine(f, y: np.ndarray, gain, offset, probes: int = 1, amplitude: int = 1, seed: int = 0) -> dict:
    """f: uint8 [N,H,W,C] -> float [N,H,W,C]"""
    sums = risk_sums_affine(y, f(RR.probe_stack(y, probes, amplitude, seed)), probes, amplitude, seed)
    return {"sums": sums, **risk_from_affine_sums(sums, gain, offset, y.shape[1], y.shape[2], amplitude)}


# ---- the cases of the issue ---------------------------------------------------------------------------------------------------

FIT_PARAMETERS = ((0.2, 1.0), (0.5, 2.0), (1.0, 3.0), (0.0, 10.0))      # (a, read sigma)
FIT_SEEDS = range(5)
FIT_AT = (64.0, 128.0, 192.0)


def noisy(clean: np.ndarray, a: float, read_sigma: float, seed: int) -> np.ndarray:
    """clean + sqrt(a clean + read_sigma^2) N(0,1), rounded and clipped, from NumPy's generator"""
    x = clean.astype(np.float64)
    z = np.random.default_rng(seed).standard_normal(x.shape)
    return np.clip(np.rint(x + np.sqrt(a * x + read_sigma ** 2) * z), 0, 255).astype(np.uint8)


def ramp_image() -> np.ndarray:
    """256 x 256 x 1: a horizontal ramp from 24 to 232"""
    row = np.rint(np.linspace(24.0, 232.0, 256))
    return np.broadcast_to(row[None, :, None], (256, 256, 1)).astype(np.uint8)


def fit_case(a: float, read_sigma: float, seed: int) -> np.ndarray:
    return noisy(ramp_image(), a, read_sigma, seed)[None]


def two_level_image(height: int, width: int) -> np.ndarray:
    """[1,H,W,1]: left half 40, right half 200"""
    img = np.full((1, height, width, 1), 200, np.uint8)
    img[:, :, :width // 2] = 40
    return img


def half_field_blur(stack_u8: np.ndarray) -> np.ndarray:
    """3x3 box blur (replicated edges) on the left half of the columns, identity on the right: float32 [N,H,W,C].  The blurred
    value is the integer 3x3 sum / 9 divided in float64 and rounded to float32."""
    x = stack_u8.astype(np.int64)
    pad = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge")
    H, W = x.shape[1:3]
    box = sum(pad[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3))
    out = x.astype(np.float64)
    out[:, :, :W // 2] = box[:, :, :W // 2].astype(np.float64) / 9.0
    return out.astype(np.float32)


SURE_A, SURE_READ = 0.5, 2.0
SURE_OFFSET = SURE_READ ** 2 + 1.0 / 12.0                               # the rounding to grey levels adds 1/12
SURE_SHAPES = ((128, 128, 4), (64, 96, 8))                              # (H, W, probes)
SURE_SEEDS = range(100, 106)


def sure_case(height: int, width: int, seed: int):
    """(clean, noisy) uint8 [1,H,W,1]"""
    clean = two_level_image(height, width)
    return clean, noisy(clean, SURE_A, SURE_READ, seed)
