"""The NumPy statement of blind_image_denoising_amd/pixel_shuffle.py and csrc/pixel_shuffle.hip: the dilated Haar statistic, the
stride rule, pixel-shuffle split and merge by slicing, random replacing through the oracle's Philox, the fp64 mean and the
pipeline of PixelShuffleDenoiserModule.  Written from the definitions, not from the package's code.

    q_s(y,x) = |x(y,x) - x(y,x+s) - x(y+s,x) + x(y+s,x+s)| for y + s < H, x + s < W;  sigma_s = grouped median / 2 / 0.6745
    grouped median: bin 0 covers [0, 1/2), bin k >= 1 covers [k - 1/2, k + 1/2); the bin k with cum(k-1) < n/2 <= cum(k) is
        interpolated linearly; an empty histogram or one with all its mass in bin 0 gives 0
    sigma[b,s] = sqrt((sum over c, ascending, of sigma_s^2) / C);  stride = the smallest s in 1..S-1 with sigma[s] >= threshold
        sigma[s+1], else S;  sigma_white = sigma[min(stride + 1, S)]
    split: member b s^2 + i s + j at (u,v) = pixel (u s + i, v s + j), a coordinate past the frame lowered by s;  merge: its inverse
    replace: pixel p = y W + x of copy t is replaced when word p & 3 of philox4x32_10((lo32 g, hi32 g, t, 5), (lo32 seed, hi32 seed)),
        g = p >> 2, is below min(int(replace 2^32), 2^32 - 1)
    mean: fp64 sum in ascending t, one division, (float) q;  uint8: rint(clip((float) q, 0, 255))"""
import numpy as np

from oracle.bfcnn_oracle import _philox4x32_10

BINS, BINS_PAD = 511, 512
MAD_TO_SIGMA = 0.6745
PHILOX_STREAM = 5


def dilated_haar(images: np.ndarray, s: int) -> np.ndarray:
    """q_s of a uint8 [B,H,W,C] batch: int64 [B, H - s, W - s, C]"""
    x = images.astype(np.int64)
    return np.abs(x[:, :-s, :-s] - x[:, :-s, s:] - x[:, s:, :-s] + x[:, s:, s:])


def grouped_median(hist: np.ndarray) -> float:
    hist = np.asarray(hist, np.int64)
    n = int(hist.sum())
    if n == 0 or int(hist[0]) == n:
        return 0.0
    cum = np.cumsum(hist)
    half = n / 2.0
    k = int(np.argmax(cum >= half))
    before = float(cum[k - 1]) if k > 0 else 0.0
    lo, width = (0.0, 0.5) if k == 0 else (k - 0.5, 1.0)
    return lo + width * (half - before) / float(hist[k])


def correlation_statistics(images: np.ndarray, S: int):
    """(hist int64 [B,C,S,512], sigma float64 [B,C,S])"""
    assert images.dtype == np.uint8 and images.ndim == 4 and 1 <= S <= 8 and min(images.shape[1:3]) >= S + 1
    B, H, W, C = images.shape
    hist = np.zeros((B, C, S, BINS_PAD), np.int64)
    sigma = np.zeros((B, C, S), np.float64)
    for s in range(1, S + 1):
        q = dilated_haar(images, s)
        for b in range(B):
            for c in range(C):
                hist[b, c, s - 1] = np.bincount(q[b, :, :, c].ravel(), minlength=BINS_PAD)
                sigma[b, c, s - 1] = grouped_median(hist[b, c, s - 1, :BINS]) / 2.0 / MAD_TO_SIGMA
    return hist, sigma


def stride_rule(sigma: np.ndarray, threshold: float):
    """(stride [B] int64, sigma_white [B]) of a [B,S] curve"""
    B, S = sigma.shape
    stride = np.full(B, S, np.int64)
    for b in range(B):
        for s in range(1, S):
            if sigma[b, s - 1] >= threshold * sigma[b, s]:
                stride[b] = s
                break
    white = np.array([sigma[b, min(stride[b] + 1, S) - 1] for b in range(B)], np.float64).reshape(B)
    return stride, white


def correlation(images: np.ndarray, S: int = 6, threshold: float = 0.8):
    """(sigma [B,S], stride [B], sigma_white [B])"""
    per_channel = correlation_statistics(images, S)[1]
    total = per_channel[:, 0] * per_channel[:, 0]
    for c in range(1, per_channel.shape[1]):
        total = total + per_channel[:, c] * per_channel[:, c]
    sigma = np.sqrt(total / float(per_channel.shape[1]))
    return (sigma,) + stride_rule(sigma, threshold)


def split(x: np.ndarray, s: int) -> np.ndarray:
    B, H, W, C = x.shape
    assert s == 1 or (H >= 2 * s and W >= 2 * s)
    Hs, Ws = -(H // -s), -(W // -s)
    out = np.empty((B * s * s, Hs, Ws, C), x.dtype)
    for b in range(B):
        for i in range(s):
            for j in range(s):
                rows = np.arange(Hs) * s + i
                cols = np.arange(Ws) * s + j
                rows[rows >= H] -= s
                cols[cols >= W] -= s
                out[b * s * s + i * s + j] = x[b][rows][:, cols]
    return out


def to_uint8(q: np.ndarray) -> np.ndarray:
    return np.rint(np.clip(q.astype(np.float32), 0, 255)).astype(np.uint8)


def merge(members: np.ndarray, B: int, H: int, W: int, s: int, cast: bool) -> np.ndarray:
    C = members.shape[-1]
    assert members.shape == (B * s * s, -(H // -s), -(W // -s), C) and members.dtype == np.float32
    out = np.empty((B, H, W, C), np.float32)
    for b in range(B):
        for i in range(s):
            for j in range(s):
                part = out[b, i::s, j::s]
                part[...] = members[b * s * s + i * s + j, :part.shape[0], :part.shape[1]]
    return to_uint8(out) if cast else out


def replace_threshold(replace: float) -> int:
    return min(int(replace * 2.0 ** 32), 2 ** 32 - 1)


def replace_masks(H: int, W: int, T: int, replace: float, seed: int) -> np.ndarray:
    """bool [T, H, W]: the pixels of copy t that take the noisy value"""
    p = np.arange(H * W, dtype=np.uint64)
    g = p >> np.uint64(2)
    masks = np.empty((T, H * W), bool)
    for t in range(T):
        words = _philox4x32_10(g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), np.full(g.shape, t, np.uint64),
                               np.full(g.shape, PHILOX_STREAM, np.uint64), seed & 0xFFFFFFFF, seed >> 32)
        word = np.stack(words)[(p & np.uint64(3)).astype(np.int64), np.arange(H * W)]
        masks[t] = word < np.uint64(replace_threshold(replace))
    return masks.reshape(T, H, W)


def replace_copies(base: np.ndarray, noisy: np.ndarray, T: int, replace: float, seed: int) -> np.ndarray:
    B, H, W, C = base.shape
    masks = replace_masks(H, W, T, replace, seed)
    out = np.empty((B * T, H, W, C), np.uint8)
    for b in range(B):
        for t in range(T):
            out[b * T + t] = np.where(masks[t][:, :, None], noisy[b], base[b])
    return out


def mean(members: np.ndarray, T: int, cast: bool) -> np.ndarray:
    assert members.dtype == np.float32 and members.shape[0] % T == 0
    stack = members.reshape((members.shape[0] // T, T) + members.shape[1:])
    total = np.zeros(stack[:, 0].shape, np.float64)
    for t in range(T):
        total = total + stack[:, t].astype(np.float64)
    q = (total / float(T)).astype(np.float32)
    return to_uint8(q) if cast else q


def pipeline(denoise, x: np.ndarray, s: int, refine: int = 0, replace: float = 0.16, seed: int = 0, cast: bool = True) -> np.ndarray:
    """PixelShuffleDenoiserModule from its parts; `denoise`: uint8 array -> float32 array of the same shape"""
    B, H, W, _ = x.shape
    out = merge(denoise(split(x, s)), B, H, W, s, cast or refine > 0)
    if refine > 0:
        out = mean(denoise(replace_copies(out, x, refine, replace, seed)), refine, cast)
    return out


def correlated_noise_image(taps, sigma: float, seed: int, H: int = 96, W: int = 96, C: int = 1, flat: float = 128.0) -> np.ndarray:
    """uint8 [1,H,W,C]: white Gaussian noise filtered separably (circularly) by `taps`, rescaled to `sigma`, on a flat image"""
    rng = np.random.default_rng(seed)
    n = rng.standard_normal((H, W, C))
    taps = np.asarray(taps, np.float64)
    for axis in (0, 1):
        n = sum(w * np.roll(n, k, axis=axis) for k, w in enumerate(taps))
    n = n * (sigma / n.std())
    return np.clip(np.rint(flat + n), 0, 255).astype(np.uint8)[None]
