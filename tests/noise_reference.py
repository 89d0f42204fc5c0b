"""NumPy restatement of the no-reference noise statistics (csrc/noise_estimate.hip), independent of the package: int64 for uint8
images, float64 for float32 images.  Per image and channel of a [B,H,W,C] batch

    S             = sum |L| over the (H-2)(W-2) interior pixels, L = x (*) [[1,-2,1],[-2,4,-2],[1,-2,1]]      (Immerkaer 1996)
    sigma_fast    = sqrt(pi/2) / 6 * S / ((H-2)(W-2))
    sigma_mad     = grouped median of q = |x00 - x01 - x10 + x11| over the complete 2x2 cells / 2 / 0.6745      (Donoho's MAD rule; q is
                    twice the modulus of the orthonormal Haar HH coefficient), uint8 only, NaN for float32
    clipped_count = number of samples equal to 0 or 255, uint8 only, NaN for float32
"""
import numpy as np

HIST_BINS = 511                     # q of a uint8 cell is an integer in 0..510
MAD_TO_SIGMA = 0.6745


def immerkaer_sum(images: np.ndarray) -> np.ndarray:
    """S per image and channel, [B,C]: int64 (exact) for uint8, float64 for float32.  The mask is the outer product of [1,-2,1]
    with itself, so L is the vertical second difference of the horizontal second difference."""
    x = images.astype(np.int64 if images.dtype == np.uint8 else np.float64)
    h = x[:, :, :-2] - 2 * x[:, :, 1:-1] + x[:, :, 2:]
    lap = h[:, :-2] - 2 * h[:, 1:-1] + h[:, 2:]
    return np.abs(lap).sum(axis=(1, 2))


def haar_histogram(images: np.ndarray) -> np.ndarray:
    """the 511-bin histogram of q per image and channel, [B,C,511] int64; the last row / column of an odd size is dropped"""
    assert images.dtype == np.uint8
    B, H, W, C = images.shape
    x = images[:, :H // 2 * 2, :W // 2 * 2].astype(np.int64)
    q = np.abs(x[:, 0::2, 0::2] - x[:, 0::2, 1::2] - x[:, 1::2, 0::2] + x[:, 1::2, 1::2])
    hist = np.zeros((B, C, HIST_BINS), np.int64)
    for b in range(B):
        for c in range(C):
            hist[b, c] = np.bincount(q[b, :, :, c].ravel(), minlength=HIST_BINS)
    return hist


def grouped_median(hist: np.ndarray) -> float:
    """median of grouped data: bin k >= 1 covers [k - 1/2, k + 1/2), bin 0 covers [0, 1/2); linear inside the bin that holds the
    n/2-th value.  A histogram with every cell in bin 0 (no cell differs from zero: nothing to interpolate) has median 0."""
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


def noise_statistics(images: np.ndarray) -> np.ndarray:
    """[B,C,4] float64: S, sigma_fast, sigma_mad, clipped_count"""
    assert images.ndim == 4 and images.dtype in (np.uint8, np.float32)
    B, H, W, C = images.shape
    out = np.empty((B, C, 4), np.float64)
    s = immerkaer_sum(images)
    out[:, :, 0] = s
    out[:, :, 1] = np.sqrt(np.pi / 2.0) / 6.0 * s.astype(np.float64) / float((H - 2) * (W - 2))
    if images.dtype == np.uint8:
        hist = haar_histogram(images)
        for b in range(B):
            for c in range(C):
                out[b, c, 2] = grouped_median(hist[b, c]) / 2.0 / MAD_TO_SIGMA
        out[:, :, 3] = ((images == 0) | (images == 255)).sum(axis=(1, 2))
    else:
        out[:, :, 2:] = np.nan
    return out


def combine_channels(sigma: np.ndarray) -> np.ndarray:
    """[B,C] channel sigmas -> [B]: the root mean square"""
    return np.sqrt((sigma * sigma).mean(axis=1))
