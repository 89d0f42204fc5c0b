"""NumPy statements of the burst merge (blind_image_denoising_amd/burst.py, include/bfcnn_hip.h), written from the contract and
not from the kernels: the luma pyramid, the block-matching alignment, the thresholds and the robust merge.  Everything up to the
one division of the merge is int64; the division is one fp64 division and one cast, which NumPy does as the GPU does: the GPU
tests compare with `torch.equal` and no tolerance.  `quality_scene` and its helpers are the experiment of DESIGN.md 7.16."""
import pathlib

import numpy as np

TILE = 16


def _ceil_div(a: int, b: int) -> int:
    return -(a // -b)


# ---- luma pyramid ------------------------------------------------------------------------------------------------------------

def luma(frames: np.ndarray) -> np.ndarray:
    """uint8 [...,H,W,C] -> uint8 [...,H,W]: (2 sum_c x_c + C) // (2 C)"""
    C = frames.shape[-1]
    return ((2 * frames.astype(np.int64).sum(axis=-1) + C) // (2 * C)).astype(np.uint8)


def down(level: np.ndarray) -> np.ndarray:
    """uint8 [...,H,W] -> uint8 [...,ceil(H/2),ceil(W/2)]: (the 2 x 2 cell at (2 y, 2 x), coordinates clamped, + 2) >> 2"""
    H, W = level.shape[-2:]
    ya, xa = 2 * np.arange(_ceil_div(H, 2)), 2 * np.arange(_ceil_div(W, 2))
    yb, xb = np.minimum(ya + 1, H - 1), np.minimum(xa + 1, W - 1)
    v = level.astype(np.int64)
    cell = v[..., ya[:, None], xa] + v[..., ya[:, None], xb] + v[..., yb[:, None], xa] + v[..., yb[:, None], xb]
    return ((cell + 2) >> 2).astype(np.uint8)


def pyramid(frames: np.ndarray, levels: int) -> list:
    """the K luma levels of uint8 [...,H,W,C], finest first"""
    out = [luma(frames)]
    for _ in range(1, levels):
        out.append(down(out[-1]))
    return out


# ---- alignment ---------------------------------------------------------------------------------------------------------------

def _tile_sums(values: np.ndarray) -> np.ndarray:
    """int64 [H,W] -> [gy,gx]: the sum over every 16 x 16 tile, edge tiles cut by the frame"""
    H, W = values.shape
    gy, gx = _ceil_div(H, TILE), _ceil_div(W, TILE)
    padded = np.zeros((gy * TILE, gx * TILE), np.int64)
    padded[:H, :W] = values
    return padded.reshape(gy, TILE, gx, TILE).sum(axis=(1, 3))


def align_level(l_ref: np.ndarray, l_alt: np.ndarray, d0: np.ndarray, search: int) -> np.ndarray:
    """one level: luma [H,W] of the reference and the alternate frame, the prediction d0 int64 [gy,gx,2] -> the winners [gy,gx,2]"""
    H, W = l_ref.shape
    ref, alt = l_ref.astype(np.int64), l_alt.astype(np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    ty, tx = yy // TILE, xx // TILE
    best = None
    for u in range(-search, search + 1):
        for v in range(-search, search + 1):
            sy = np.clip(yy + d0[ty, tx, 0] + u, 0, H - 1)
            sx = np.clip(xx + d0[ty, tx, 1] + v, 0, W - 1)
            cost = _tile_sums(np.abs(ref - alt[sy, sx]))
            key = np.stack([cost, np.full_like(cost, u * u + v * v), np.full_like(cost, u), np.full_like(cost, v)], axis=-1)
            if best is None:
                best = key
                continue
            less, equal = np.zeros(cost.shape, bool), np.ones(cost.shape, bool)
            for i in range(4):                                     # lexicographic (cost, u u + v v, u, v)
                less |= equal & (key[..., i] < best[..., i])
                equal &= key[..., i] == best[..., i]
            best = np.where(less[..., None], key, best)
    return d0 + best[..., 2:4]


def align_pair(p_ref: list, p_alt: list, search: int) -> np.ndarray:
    """the level-0 field int64 [gy,gx,2] of one alternate frame from the two pyramids (lists of [H_k,W_k])"""
    d = None
    for k in range(len(p_ref) - 1, -1, -1):
        H, W = p_ref[k].shape
        gy, gx = _ceil_div(H, TILE), _ceil_div(W, TILE)
        if d is None:
            d0 = np.zeros((gy, gx, 2), np.int64)
        else:
            iy, ix = np.minimum(np.arange(gy) >> 1, d.shape[0] - 1), np.minimum(np.arange(gx) >> 1, d.shape[1] - 1)
            d0 = 2 * d[iy[:, None], ix]
        d = align_level(p_ref[k], p_alt[k], d0, search)
    return d


def align(frames: np.ndarray, reference: int = 0, levels: int = 3, search: int = 4) -> np.ndarray:
    """uint8 [B,T,H,W,C] -> int32 [B,T,gy,gx,2] as (dy, dx), zero for t == reference"""
    B, T, H, W, _ = frames.shape
    pyr = pyramid(frames, levels)
    field = np.zeros((B, T, _ceil_div(H, TILE), _ceil_div(W, TILE), 2), np.int32)
    for b in range(B):
        for t in range(T):
            if t != reference:
                field[b, t] = align_pair([p[b, reference] for p in pyr], [p[b, t] for p in pyr], search)
    return field


# ---- thresholds and merge ----------------------------------------------------------------------------------------------------

def thresholds(sigma, C: int, k_lo: float = 1.5, k_hi: float = 3.0) -> np.ndarray:
    """sigma [B] -> int64 [B,2] = (lo, hi): E = ((sigma sigma) 2) (25 C) in fp64, lo = floor(k_lo E), hi = floor(k_hi E) + 1"""
    sigma = np.asarray(sigma, np.float64).reshape(-1)
    E = ((sigma * sigma) * 2.0) * float(25 * C)
    return np.stack([np.floor(k_lo * E).astype(np.int64), np.floor(k_hi * E).astype(np.int64) + 1], axis=-1)


def distances(frames: np.ndarray, field: np.ndarray, reference: int) -> np.ndarray:
    """one image: frames uint8 [T,H,W,C], field [T,gy,gx,2] -> D int64 [T,H,W] (zero for the reference frame)"""
    T, H, W, _ = frames.shape
    x = frames.astype(np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    D = np.zeros((T, H, W), np.int64)
    for t in range(T):
        if t == reference:
            continue
        dy, dx = field[t, yy // TILE, xx // TILE, 0].astype(np.int64), field[t, yy // TILE, xx // TILE, 1].astype(np.int64)
        for a in range(-2, 3):
            for b in range(-2, 3):
                qy, qx = np.clip(yy + a, 0, H - 1), np.clip(xx + b, 0, W - 1)                 # q clamped first
                moved = x[t, np.clip(qy + dy, 0, H - 1), np.clip(qx + dx, 0, W - 1)]
                D[t] += ((moved - x[reference, qy, qx]) ** 2).sum(axis=-1)
    return D


def merge_image(frames: np.ndarray, field: np.ndarray, lo: int, hi: int, reference: int = 0, cast_to_uint8: bool = True):
    """one image: (out [H,W,C] float32 or uint8, counts int32 [H,W,2] = (den, sq))"""
    T, H, W, C = frames.shape
    lo, hi = int(lo), int(hi)
    x = frames.astype(np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    D = distances(frames, field, reference)
    num, den, sq = 256 * x[reference], np.full((H, W), 256, np.int64), np.full((H, W), 256 * 256, np.int64)
    for t in range(T):
        if t == reference:
            continue
        ramp = ((hi - D[t]) * 256) // (hi - lo)
        w = np.where(D[t] <= lo, 256, np.where(D[t] >= hi, 0, ramp))
        dy, dx = field[t, yy // TILE, xx // TILE, 0].astype(np.int64), field[t, yy // TILE, xx // TILE, 1].astype(np.int64)
        num = num + w[..., None] * x[t, np.clip(yy + dy, 0, H - 1), np.clip(xx + dx, 0, W - 1)]
        den, sq = den + w, sq + w * w
    out = (num.astype(np.float64) / den[..., None].astype(np.float64)).astype(np.float32)
    if cast_to_uint8:
        out = np.rint(out).astype(np.uint8)                        # half to even
    return out, np.stack([den, sq], axis=-1).astype(np.int32)


def merge(frames: np.ndarray, field: np.ndarray, thr: np.ndarray, reference: int = 0, cast_to_uint8: bool = True):
    """uint8 [B,T,H,W,C], field [B,T,gy,gx,2], thr int64 [B,2] -> (out [B,H,W,C], counts int32 [B,H,W,2])"""
    parts = [merge_image(frames[b], field[b], thr[b, 0], thr[b, 1], reference, cast_to_uint8) for b in range(frames.shape[0])]
    return np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])


# ---- the quality experiment --------------------------------------------------------------------------------------------------

SHIFTS = ((0, 0), (3, -5), (-11, 7), (19, 14), (-23, -20), (6, 26))
TRACK = (slice(100, 140), slice(100, 190))                         # where the intruder of `with_intruder` passes


def psnr(a: np.ndarray, b: np.ndarray) -> float:
    return float(10.0 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def quality_scene(image: np.ndarray, sigma: float = 20.0, size: int = 256, origin=(100, 100), seed: int = 0):
    """(clean reference crop [size,size,C], noisy burst uint8 [T,size,size,C]): crops of `image` at origin + SHIFTS[t] under white
    noise of `sigma` from default_rng(seed), frame after frame"""
    rng = np.random.default_rng(seed)
    y0, x0 = origin
    clean = [image[y0 + dy:y0 + dy + size, x0 + dx:x0 + dx + size] for dy, dx in SHIFTS]
    frames = [np.clip(np.rint(c + rng.normal(0.0, sigma, c.shape)), 0, 255).astype(np.uint8) for c in clean]
    return clean[0], np.stack(frames)


def with_intruder(frames: np.ndarray) -> np.ndarray:
    """a 40 x 40 square inverted at another place in every alternate frame, moving along TRACK"""
    out = frames.copy()
    for t in range(1, out.shape[0]):
        out[t, 100:140, 100 + 8 * t:140 + 8 * t] = 255 - out[t, 100:140, 100 + 8 * t:140 + 8 * t]
    return out


def load_lena() -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(pathlib.Path(__file__).resolve().parent / "golden" / "lena.jpg").convert("RGB"))
