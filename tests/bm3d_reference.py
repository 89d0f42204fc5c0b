"""NumPy restatement of BM3D (csrc/bm3d.hip, blind_image_denoising_amd/bm3d.py; Dabov, Foi, Katkovnik, Egiazarian, IEEE TIP 2007),
independent of the package: a loop over the reference blocks, vectorised over the candidates of each, everything int64 up to the
one float64 division.  Not a test module: the yardstick of tests/test_bm3d.py and tests/test_gpu_bm3d.py.

    blocks 8 x 8, groups of at most 16; H2n = [[Hn, Hn], [Hn, -Hn]]; per channel count C a forward matrix A with squared row norms
    n2 and a back matrix Bk, Bk A = s I (CHANNELS below)
    params   int64 [B,4] = (tau1, thr1, tau2, v1)
    a step   (noisy, guide, wiener): reference blocks at 0, step, 2 step, ... <= n - 8 and at n - 8 along each axis; candidates
             within `search` of the reference, wholly inside the frame; D = the squared difference of the guide blocks; a candidate
             counts if D <= tau; key = (D << 10) | index in the window, the reference's own -1; the first K of ascending key, K the
             largest power of two <= min(count, 16)
             t = H8 block H8, HK along the group, A along the channels (tb: the same of the guide's blocks)
             hard:    t kept where t t > (thr1 K) n2[c];  w = max(4096 // max(kept, 1), 1)
             wiener:  S = tb tb, g = (S << 12) // max(S + (v1 K) n2[c], 1), t = (t g + 2048) >> 12;
                      w = min(max(2^36 // max(sum g g, 1), 1), 2^14)
             back: Bk, HK, H8 . H8, times 16 // K;  num[pixel, c] += w value, den[pixel] += w over the K blocks
    finish   d = den 1024 s;  uint8 clip((2 max(num, 0) + d) // (2 d), 0, 255);  float32(float64(num) / float64(d))
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

BLOCK, GROUP = 8, 16
THRESHOLD, MATCH = 2.7, (2500.0, 400.0)


def hadamard(n: int) -> np.ndarray:
    h = np.ones((1, 1), np.int64)
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    return h


# C -> (A, n2, Bk, s)
CHANNELS = {
    1: (np.array([[1]], np.int64), np.array([1], np.int64), np.array([[1]], np.int64), 1),
    2: (hadamard(2), np.array([2, 2], np.int64), hadamard(2), 2),
    3: (np.array([[1, 1, 1], [1, 0, -1], [1, -2, 1]], np.int64), np.array([3, 2, 6], np.int64),
        np.array([[2, 3, 1], [2, 0, -2], [2, -3, 1]], np.int64), 6),
    4: (hadamard(4), np.array([4, 4, 4, 4], np.int64), hadamard(4), 4),
}
H8 = hadamard(8)


def params(sigma, C: int, threshold: float = THRESHOLD, match=MATCH) -> np.ndarray:
    """int64 [B,4] = (tau1, thr1, tau2, v1) for sigma [B]"""
    s = np.atleast_1d(np.asarray(sigma, np.float64))
    tau1 = np.full(s.shape, np.floor((match[0] * 64.0) * C))
    thr1 = np.floor((((threshold * threshold) * s) * s) * 64.0)
    tau2 = np.full(s.shape, np.floor((match[1] * 64.0) * C))
    v1 = np.floor((64.0 * s) * s)
    return np.stack([tau1, thr1, tau2, v1], axis=1).astype(np.int64)


def positions(n: int, step: int):
    p = list(range(0, n - BLOCK + 1, step))
    if p[-1] != n - BLOCK:
        p.append(n - BLOCK)
    return p


def _transform(blocks: np.ndarray, A: np.ndarray) -> np.ndarray:
    """[K,C,8,8] -> the same shape: H8 . H8 per block, HK along k, A along c"""
    t = H8 @ blocks @ H8
    t = np.einsum("jk,kcuv->jcuv", hadamard(blocks.shape[0]), t)
    return np.einsum("dc,kcuv->kduv", A, t)


def step_image(noisy: np.ndarray, guide: np.ndarray, prm, search: int, step: int, wiener: bool):
    """one step on one image [H,W,C]: (num int64 [H,W,C], den int64 [H,W], the histogram of K over the reference blocks int64 [5]
    for K = 1, 2, 4, 8, 16, (coefficients kept, coefficients zeroed) -- of the hard threshold; of the Wiener gains, g > 0 and
    g == 0)"""
    H, W, C = noisy.shape
    assert guide.shape == noisy.shape and 1 <= C <= 4 and H >= BLOCK and W >= BLOCK
    r = search
    A, n2, Bk, _ = CHANNELS[C]
    tau1, thr1, tau2, v1 = (int(v) for v in prm)
    tau = tau2 if wiener else tau1
    x, gd = noisy.astype(np.int64), guide.astype(np.int64)
    win_x = sliding_window_view(x, (BLOCK, BLOCK), axis=(0, 1))      # [H-7, W-7, C, 8, 8]
    win_g = sliding_window_view(gd, (BLOCK, BLOCK), axis=(0, 1))
    num, den = np.zeros((H, W, C), np.int64), np.zeros((H, W), np.int64)
    hist, kept, zeroed = np.zeros(5, np.int64), 0, 0
    for y in positions(H, step):
        ya, yb = max(0, y - r), min(H - BLOCK, y + r)
        for xx in positions(W, step):
            xa, xb = max(0, xx - r), min(W - BLOCK, xx + r)
            cand = win_g[ya:yb + 1, xa:xb + 1]
            D = ((cand - win_g[y, xx]) ** 2).sum(axis=(2, 3, 4))
            cy, cx = np.mgrid[ya:yb + 1, xa:xb + 1]
            key = (D << 10) | ((cy - y + r) * (2 * r + 1) + (cx - xx + r))
            own = (cy == y) & (cx == xx)
            key[own] = -1
            counts = (D <= tau) | own
            order = np.argsort(key[counts], kind="stable")[:GROUP]
            K = 1 << (int(len(order)).bit_length() - 1)
            order = order[:K]
            gy, gx = cy[counts][order], cx[counts][order]
            hist[K.bit_length() - 1] += 1
            t = _transform(win_x[gy, gx], A)
            if wiener:
                tb = _transform(win_g[gy, gx], A)
                S = tb * tb
                g = (S << 12) // np.maximum(S + ((v1 * K) * n2)[None, :, None, None], 1)
                t = (t * g + 2048) >> 12
                w = min(max(2 ** 36 // max(int((g * g).sum()), 1), 1), 2 ** 14)
                kept += int((g > 0).sum())
                zeroed += int((g == 0).sum())
            else:
                keep = t * t > ((thr1 * K) * n2)[None, :, None, None]
                t = np.where(keep, t, 0)
                nnz = int(keep.sum())
                w = max(4096 // max(nnz, 1), 1)
                kept += nnz
                zeroed += keep.size - nnz
            v = np.einsum("dc,kcuv->kduv", Bk, t)
            v = np.einsum("jk,kcuv->jcuv", hadamard(K), v)
            v = (H8 @ v @ H8) * (GROUP // K)
            for k in range(K):
                num[gy[k]:gy[k] + BLOCK, gx[k]:gx[k] + BLOCK] += w * v[k].transpose(1, 2, 0)
                den[gy[k]:gy[k] + BLOCK, gx[k]:gx[k] + BLOCK] += w
    return num, den, hist, (kept, zeroed)


def step_batch(noisy: np.ndarray, guide: np.ndarray, prm, search: int = 12, step: int = 4, wiener: bool = False):
    """a step on a batch [B,H,W,C]: (num [B,H,W,C], den [B,H,W], hist [5], (kept, zeroed)), the last two summed over the batch"""
    assert noisy.ndim == 4 and noisy.dtype == np.uint8 and guide.dtype == np.uint8
    prm = np.asarray(prm, np.int64).reshape(noisy.shape[0], 4)
    parts = [step_image(noisy[b], guide[b], prm[b], search, step, wiener) for b in range(noisy.shape[0])]
    num, den = np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])
    hist = sum(p[2] for p in parts)
    return num, den, hist, (sum(p[3][0] for p in parts), sum(p[3][1] for p in parts))


def finish(num: np.ndarray, den: np.ndarray, cast_to_uint8: bool = True) -> np.ndarray:
    d = (den * 1024 * CHANNELS[num.shape[-1]][3])[..., None]
    if cast_to_uint8:
        return np.clip((2 * np.maximum(num, 0) + d) // (2 * d), 0, 255).astype(np.uint8)
    return (num.astype(np.float64) / d.astype(np.float64)).astype(np.float32)


def bm3d_step(noisy, guide, prm, wiener: bool, search: int = 12, step: int = 4, cast_to_uint8: bool = True):
    """(the filtered batch, uint8 or float32 [B,H,W,C]; weights int64 [B,H,W] = den)"""
    num, den = step_batch(noisy, guide, prm, search, step, wiener)[:2]
    return finish(num, den, cast_to_uint8), den


def bm3d(images, prm, search: int = 12, step: int = 4, wiener: bool = True, cast_to_uint8: bool = True):
    """step one (uint8 out), then step two on (images, basic); with wiener=False step one alone: (out, weights)"""
    if not wiener:
        return bm3d_step(images, images, prm, False, search, step, cast_to_uint8)
    basic = bm3d_step(images, images, prm, False, search, step, True)[0]
    return bm3d_step(images, basic, prm, True, search, step, cast_to_uint8)
