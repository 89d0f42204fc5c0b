"""NumPy int64 restatement of the three degradation contracts (include/bfcnn_hip.h, csrc/degrade.hip): the JPEG round trip without
entropy coding, the separable integer Gaussian and the clip / quantise / drop pass.  Everything after the first clip is integer
arithmetic, so the kernels equal this bit for bit.  Not a test module: the yardstick of tests/test_degrade.py and
tests/test_gpu_degrade.py."""
import numpy as np

from oracle import bfcnn_oracle as O

# ISO/IEC 10918-1 Annex K.1 / K.2, natural (row = vertical frequency) order
LUMINANCE = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                      14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64).reshape(8, 8)
CHROMINANCE = np.full((8, 8), 99, np.int64)
CHROMINANCE[:4, :4] = [[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]]

_u, _x = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
# T[u][x] = rint(8192 c(u) / 2 cos((2 x + 1) u pi / 16)): first row 2896, second row 4017 3406 2276 799 -799 ...
T = np.rint(8192.0 * np.where(_u == 0, np.sqrt(0.5), 1.0) / 2.0 * np.cos((2 * _x + 1) * _u * np.pi / 16.0)).astype(np.int64)


def codes(x: np.ndarray) -> np.ndarray:
    """the 8-bit codes of a batch: round half to even (a no-op on integer-valued samples), then clip to 0..255; int64"""
    return np.clip(np.rint(np.asarray(x, np.float64)), 0, 255).astype(np.int64)


def _per_image(value, B):
    return np.broadcast_to(np.asarray(value), (B,))


# ---- JPEG ---------------------------------------------------------------------------------------------------------------------

def quant_table(base: np.ndarray, quality: int) -> np.ndarray:
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((base * s + 50) // 100, 1, 255)


def _pad(plane: np.ndarray, m: int) -> np.ndarray:
    H, W = plane.shape
    return np.pad(plane, ((0, -H % m), (0, -W % m)), mode="edge")


def _round_trip(plane: np.ndarray, q: np.ndarray) -> np.ndarray:
    """forward DCT, quantise, dequantise, inverse DCT of every 8x8 block of a padded plane of codes"""
    H, W = plane.shape
    p = plane.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3) - 128                   # [by, bx, y, x]
    a = (np.einsum("ux,byx->byu", T, p.reshape(-1, 8, 8)) + 512) >> 10                    # a[y][u]
    c8 = (np.einsum("vy,byu->bvu", T, a) + 4096) >> 13                                    # 8 x coefficient [v][u]
    k = np.sign(c8) * ((np.abs(c8) + 4 * q) // (8 * q))
    c = k * q
    a = (np.einsum("vy,bvu->byu", T, c) + 512) >> 10
    out = (np.einsum("ux,byu->byx", T, a) + 32768) >> 16
    out = np.clip(out + 128, 0, 255).reshape(H // 8, W // 8, 8, 8).transpose(0, 2, 1, 3)
    return out.reshape(H, W)


def _upsample(c: np.ndarray) -> np.ndarray:
    """the triangle filter on a half-size plane, edges replicated: [h, w] -> [2 h, 2 w]"""
    up = np.pad(c, 1, mode="edge")
    v = np.empty((2 * c.shape[0], c.shape[1] + 2), np.int64)
    v[0::2] = 3 * up[1:-1] + up[:-2]
    v[1::2] = 3 * up[1:-1] + up[2:]
    out = np.empty((2 * c.shape[0], 2 * c.shape[1]), np.int64)
    out[:, 0::2] = (3 * v[:, 1:-1] + v[:, :-2] + 8) >> 4
    out[:, 1::2] = (3 * v[:, 1:-1] + v[:, 2:] + 7) >> 4
    return out


def jpeg_image(img: np.ndarray, quality: int, subsampling: int) -> np.ndarray:
    """one image of codes [H,W,C], C in (1, 3) -> int64 [H,W,C]"""
    H, W, C = img.shape
    assert C in (1, 3) and 0 <= quality <= 100 and subsampling in (444, 420)
    if quality == 0:                                                # an image of the batch that is not encoded
        return img
    ql, qc = quant_table(LUMINANCE, quality), quant_table(CHROMINANCE, quality)
    if C == 1:
        return _round_trip(_pad(img[..., 0], 8), ql)[:H, :W, None]
    m = 16 if subsampling == 420 else 8
    R, G, B = (_pad(img[..., i], m) for i in range(3))
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11058 * R - 21710 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    if subsampling == 420:
        Cb, Cr = ((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2 for p in (Cb, Cr))
    Y, Cb, Cr = _round_trip(Y, ql), _round_trip(Cb, qc), _round_trip(Cr, qc)
    if subsampling == 420:
        Cb, Cr = _upsample(Cb), _upsample(Cr)
    cb, cr = Cb - 128, Cr - 128
    rgb = np.stack([Y + ((91881 * cr + 32768) >> 16), Y + ((-22553 * cb - 46802 * cr + 32768) >> 16),
                    Y + ((116130 * cb + 32768) >> 16)], axis=-1)
    return np.clip(rgb, 0, 255)[:H, :W]


def jpeg(x: np.ndarray, quality, subsampling: int = 420) -> np.ndarray:
    """x uint8 or float32 [B,H,W,C] -> float32 [B,H,W,C]; `quality` a scalar or one per image, 0 = that image keeps its codes"""
    p, q = codes(x), _per_image(quality, x.shape[0])
    return np.stack([jpeg_image(p[b], int(q[b]), subsampling) for b in range(x.shape[0])]).astype(np.float32)


# ---- blur ---------------------------------------------------------------------------------------------------------------------

def gaussian_taps(sigma: float) -> np.ndarray:
    """int64 [2 r + 1]: r = max(1, int(3 sigma + 0.5)), w = floor(65536 g + 0.5) of the normalised fp64 Gaussian, the residual
    65536 - sum w on the centre tap; sigma = 0 is the identity [65536]"""
    if sigma == 0:
        return np.array([65536], np.int64)
    r = max(1, int(3.0 * sigma + 0.5))
    k = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-(k * k) / (2.0 * float(sigma) * float(sigma)))
    g = g / g.sum()
    w = np.floor(65536.0 * g + 0.5).astype(np.int64)
    w[r] += 65536 - w.sum()
    return w


def blur_image(img: np.ndarray, w: np.ndarray) -> np.ndarray:
    """one image of codes [H,W,C] -> int64 [H,W,C]; borders clamp"""
    H, W, _ = img.shape
    r = (len(w) - 1) // 2
    xs = np.clip(np.arange(W)[:, None] + np.arange(-r, r + 1)[None, :], 0, W - 1)          # [W, taps]
    h = np.einsum("hwkc,k->hwc", img[:, xs], w)
    assert h.max() < 2 ** 24
    h8 = (h + 128) >> 8
    ys = np.clip(np.arange(H)[:, None] + np.arange(-r, r + 1)[None, :], 0, H - 1)
    v = np.einsum("hkwc,k->hwc", h8[ys], w)
    assert v.max() < 2 ** 32
    return (v + (1 << 23)) >> 24


def blur(x: np.ndarray, sigma) -> np.ndarray:
    p, s = codes(x), _per_image(sigma, x.shape[0])
    return np.stack([blur_image(p[b], gaussian_taps(float(s[b]))) for b in range(x.shape[0])]).astype(np.float32)


# ---- clip, quantise, drop -------------------------------------------------------------------------------------------------------

def drop_mask(B: int, H: int, W: int, rate, seed: int) -> np.ndarray:
    """uint8 [B,H,W], 1 = dropped: pixel i = y W + x of image b falls when t = floor(rate 2^24) > 0 and word 0 of
    philox(counter = (lo32 i, hi32 i, b, 4), key = seed) >> 8 is below t; image b draws the same in a batch of any size"""
    rate = _per_image(rate, B)
    i = np.arange(H * W, dtype=np.uint64)
    out = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        t = int(np.floor(float(rate[b]) * 2.0 ** 24))
        if t > 0:
            word = O._philox4x32_10(i & np.uint64(0xFFFFFFFF), i >> np.uint64(32), np.full_like(i, b), np.full_like(i, 4),
                                    seed & 0xFFFFFFFF, seed >> 32)[0]
            out[b] = ((word.astype(np.int64) >> 8) < t).reshape(H, W)
    return out


def pointwise(x: np.ndarray, step=1, drop_rate=0.0, seed: int = 0):
    """(float32 [B,H,W,C], uint8 mask [B,H,W])"""
    B, H, W, _ = x.shape
    q = _per_image(step, B).astype(np.int64)[:, None, None, None]
    assert (q >= 1).all()
    out = np.minimum(255, ((codes(x) + q // 2) // q) * q)
    mask = drop_mask(B, H, W, drop_rate, seed)
    out[mask.astype(bool)] = 0
    return out.astype(np.float32), mask
