"""NumPy statement of the recursive temporal filter (blind_image_denoising_amd/video.py, include/bfcnn_hip.h), written from the
contract and not from the kernel: the update of one step in int64, and the sequence driver that VideoDenoiserModule(None) is
compared with.  Distances, thresholds and the alignment are those of burst_reference.  Everything is integer arithmetic: the GPU
tests compare with no tolerance.  `pan_scene`, `square_scene` and `cut_scene` are the experiment of DESIGN.md 7.20."""
import numpy as np

import burst_reference as R

TILE = R.TILE


def empty_state(B: int, H: int, W: int, C: int):
    """(acc uint16 [B,H,W,C], cnt uint16 [B,H,W]), both zero"""
    return np.zeros((B, H, W, C), np.uint16), np.zeros((B, H, W), np.uint16)


def state8(acc: np.ndarray) -> np.ndarray:
    """the state's image: uint8 (acc + 128) >> 8"""
    return ((acc.astype(np.int64) + 128) >> 8).astype(np.uint8)


def update_image(x: np.ndarray, acc: np.ndarray, cnt: np.ndarray, field: np.ndarray, lo: int, hi: int, n_max: int):
    """one image: x uint8 [H,W,C], acc uint16 [H,W,C], cnt uint16 [H,W], field [gy,gx,2] -> (acc_out uint16, cnt_out uint16)"""
    H, W, _ = x.shape
    lo, hi = int(lo), int(hi)
    pair = np.stack([x, state8(acc)])
    D = R.distances(pair, np.stack([np.zeros_like(field), field]), 0)[1]
    ramp = ((hi - D) * 256) // (hi - lo)
    w = np.where(D <= lo, 256, np.where(D >= hi, 0, ramp))
    yy, xx = np.mgrid[0:H, 0:W]
    dy, dx = field[yy // TILE, xx // TILE, 0].astype(np.int64), field[yy // TILE, xx // TILE, 1].astype(np.int64)
    sy, sx = np.clip(yy + dy, 0, H - 1), np.clip(xx + dx, 0, W - 1)
    n = np.minimum(cnt.astype(np.int64)[sy, sx], 256 * (n_max - 1))
    m = (w * n) >> 8
    den = 256 + m
    acc_out = (65536 * x.astype(np.int64) + m[..., None] * acc.astype(np.int64)[sy, sx] + (den >> 1)[..., None]) // den[..., None]
    assert acc_out.max() <= 65535 and den.max() <= 65535
    return acc_out.astype(np.uint16), den.astype(np.uint16)


def update(x: np.ndarray, acc: np.ndarray, cnt: np.ndarray, field: np.ndarray, thr: np.ndarray, n_max: int = 8,
           cast_to_uint8: bool = True):
    """x uint8 [B,H,W,C], state (acc, cnt), field [B,gy,gx,2], thr int64 [B,2] -> (out, acc_out, cnt_out); out = uint8 state8 of
    the new state, or float32 acc_out / 256"""
    parts = [update_image(x[b], acc[b], cnt[b], field[b], thr[b, 0], thr[b, 1], n_max) for b in range(x.shape[0])]
    acc_out, cnt_out = np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])
    out = state8(acc_out) if cast_to_uint8 else (acc_out.astype(np.float64) / 256.0).astype(np.float32)
    return out, acc_out, cnt_out


def align(x: np.ndarray, image: np.ndarray, levels: int = 3, search: int = 4) -> np.ndarray:
    """the field of the state's image against the frame: frame 1 of burst_reference.align on the pair, reference 0; [B,gy,gx,2]"""
    return R.align(np.stack([x, image], axis=1), 0, levels, search)[:, 1]


def run_sequence(frames: np.ndarray, n_max: int = 8, levels: int = 3, search: int = 4, sigma=None, k=(1.5, 3.0), thresholds=None,
                 aligned: bool = True):
    """the sequence driver: uint8 [B,T,H,W,C] -> (outs uint8 [B,T,H,W,C], cnts uint16 [B,T,H,W], fields int32 [B,T,gy,gx,2]).
    `sigma`: a float or [B]; or `thresholds` int64 [T,B,2] given per frame (what an estimate made of them).  `aligned=False` keeps
    the zero field (the experiment)."""
    B, T, H, W, C = frames.shape
    acc, cnt = empty_state(B, H, W, C)
    outs, cnts, fields = [], [], []
    for t in range(T):
        x = frames[:, t]
        thr = thresholds[t] if thresholds is not None else R.thresholds(np.broadcast_to(np.asarray(sigma, np.float64), (B,)), C, *k)
        field = align(x, state8(acc), levels, search)
        if not aligned:
            field = np.zeros_like(field)
        out, acc, cnt = update(x, acc, cnt, field, thr, n_max)
        outs.append(out), cnts.append(cnt), fields.append(field)
    return np.stack(outs, axis=1), np.stack(cnts, axis=1), np.stack(fields, axis=1)


# ---- the quality experiment --------------------------------------------------------------------------------------------------

SIZE, SIGMA, ORIGIN = 128, 20.0, (100, 100)
PLAIN = np.array([[10 ** 12, 10 ** 12 + 1]], np.int64)             # every weight 256: the plain recursive mean


def _noisy(clean: np.ndarray, rng) -> np.ndarray:
    return np.clip(np.rint(clean + rng.normal(0.0, SIGMA, clean.shape)), 0, 255).astype(np.uint8)


def pan_scene(image: np.ndarray, T: int, step=(2, 3), seed: int = 0):
    """(clean [T,S,S,C], noisy uint8 [T,S,S,C]): crops of `image` moving by `step` pixels per frame ((0, 0): a static scene)"""
    rng = np.random.default_rng(seed)
    y0, x0 = ORIGIN
    clean = np.stack([image[y0 + t * step[0]:y0 + t * step[0] + SIZE, x0 + t * step[1]:x0 + t * step[1] + SIZE] for t in range(T)])
    return clean, np.stack([_noisy(c, rng) for c in clean])


SQUARE_ROWS, SQUARE_SIDE, SQUARE_X0, SQUARE_STEP = slice(50, 74), 24, 10, 6


def square_scene(image: np.ndarray, T: int = 10, seed: int = 0):
    """a static scene in which a 24 x 24 square, inverted, moves 6 pixels per frame along its rows: (clean, noisy)"""
    rng = np.random.default_rng(seed)
    y0, x0 = ORIGIN
    base = image[y0:y0 + SIZE, x0:x0 + SIZE]
    clean = np.stack([base] * T).copy()
    for t in range(T):
        cols = slice(SQUARE_X0 + SQUARE_STEP * t, SQUARE_X0 + SQUARE_STEP * t + SQUARE_SIDE)
        clean[t, SQUARE_ROWS, cols] = 255 - clean[t, SQUARE_ROWS, cols]
    return clean, np.stack([_noisy(c, rng) for c in clean])


def track_psnr(outs: np.ndarray, clean: np.ndarray) -> float:
    """the PSNR on the square's track: over the frames t >= 1, the pixels the square covers in frame t - 1 or in frame t (where
    it is, and where it has just left)"""
    se, count = 0.0, 0
    for t in range(1, outs.shape[0]):
        cols = slice(SQUARE_X0 + SQUARE_STEP * (t - 1), SQUARE_X0 + SQUARE_STEP * t + SQUARE_SIDE)
        diff = outs[t, SQUARE_ROWS, cols].astype(np.float64) - clean[t, SQUARE_ROWS, cols].astype(np.float64)
        se, count = se + float((diff ** 2).sum()), count + diff.size
    return float(10.0 * np.log10(255.0 ** 2 / (se / count)))


CUT_ORIGINS = ((250, 250), (0, 0))                                 # DESIGN.md 7.20 lists what other pairs of crops give


def cut_scene(image: np.ndarray, before: int = 8, origins=CUT_ORIGINS, seed: int = 0):
    """`before` static frames of one crop, then one frame of another part of the image: (clean, noisy), the cut is the last frame"""
    rng = np.random.default_rng(seed)
    (ay, ax), (by, bx) = origins
    a, b = image[ay:ay + SIZE, ax:ax + SIZE], image[by:by + SIZE, bx:bx + SIZE]
    clean = np.stack([a] * before + [b])
    return clean, np.stack([_noisy(c, rng) for c in clean])
