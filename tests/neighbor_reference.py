"""NumPy restatement of the Neighbor2Neighbor pair contract (include/bfcnn_hip.h, csrc/neighbor.hip): the choice k per cell from the
oracle's Philox4x32-10, the table of ordered adjacent pairs, `input` and `target`.  Not a test module: the yardstick of
tests/test_neighbor.py and tests/test_gpu_neighbor.py."""
import numpy as np

from oracle import bfcnn_oracle as O

# position 0 = (0,0), 1 = (0,1), 2 = (1,0), 3 = (1,1) (row, column) of a 2x2 cell; (p1, p2) = TABLE[k]
TABLE = np.array([(0, 1), (0, 2), (1, 3), (2, 3), (1, 0), (2, 0), (3, 1), (3, 2)], np.int64)


def choices(B: int, H: int, W: int, seed: int) -> np.ndarray:
    """k in 0..7 per cell, int64 [B, H/2, W/2]: cell (i, j) of image b belongs to group g = i ceil(W2 / 4) + (j >> 2) and takes
    r[j & 3] >> 29 of philox(counter = (lo32 g, hi32 g, b, 3), key = (lo32 seed, hi32 seed))"""
    assert H % 2 == 0 and W % 2 == 0 and H >= 2 and W >= 2
    H2, W2 = H // 2, W // 2
    groups_row = (W2 + 3) // 4
    i, j = np.meshgrid(np.arange(H2, dtype=np.uint64), np.arange(W2, dtype=np.uint64), indexing="ij")
    g = i * np.uint64(groups_row) + (j >> np.uint64(2))
    out = np.empty((B, H2, W2), np.int64)
    for b in range(B):
        words = O._philox4x32_10(g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), np.full_like(g, b), np.full_like(g, 3),
                                 seed & 0xFFFFFFFF, seed >> 32)
        word = np.choose((j & np.uint64(3)).astype(np.int64), [w.astype(np.int64) for w in words])
        out[b] = word >> 29
    return out


def positions(k: np.ndarray):
    """(p1, p2) per cell, each in 0..3"""
    return TABLE[k, 0], TABLE[k, 1]


def gather(x: np.ndarray, p: np.ndarray) -> np.ndarray:
    """x [B,H,W,C] at position p [B,H/2,W/2] of every cell: [B,H/2,W/2,C], the dtype of x"""
    B, H, W, C = x.shape
    b, i, j = np.meshgrid(np.arange(B), np.arange(H // 2), np.arange(W // 2), indexing="ij")
    return x[b, 2 * i + (p >> 1), 2 * j + (p & 1)]


def pairs(y: np.ndarray, seed: int, f: np.ndarray = None, weight: float = 0.0):
    """(input, target) for y uint8 or float32 [B,H,W,C]: input = y[p1] as float32 (exact); target = y[p2] as float32 without f,
    else the fp64 value y[p2] + float32(weight) * fl32(f[p1] - f[p2]) -- the kernel's fused multiply-add rounds that once."""
    p1, p2 = positions(choices(y.shape[0], y.shape[1], y.shape[2], seed))
    inp, y2 = gather(y, p1).astype(np.float32), gather(y, p2).astype(np.float32)
    if f is None:
        return inp, y2
    d = (gather(f.astype(np.float32), p1) - gather(f.astype(np.float32), p2)).astype(np.float32)       # rounded to fp32 first
    return inp, y2.astype(np.float64) + np.float64(np.float32(weight)) * d.astype(np.float64)
