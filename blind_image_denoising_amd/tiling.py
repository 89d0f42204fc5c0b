"""Tiled inference: a frame is cut into overlapping tiles of one shape, the denoiser runs on batches of one shape, and the float
results are blended back.  Two kernels of csrc/tiling.hip carry everything that is not the denoiser: `bf_op_tile_split_u8` (tiles
[first, first + count) of the tile order out of the uint8 frame) and `bf_op_tile_blend` (a gather over the float tiles: integer
weights, fp64 sum in ascending tile order, one correctly rounded division, round half to even, cast, one write).

The plan, per axis (length H, nominal tile T, overlap O, margin M; the same in the C ABI, here, in DESIGN 7.13 and in the tests):

    valid     T >= 1 and 0 <= 2 M <= O <= T // 2
    extent    t = min(T, H)
    count     n = 1 if H <= T else ceil((H - O) / (T - O))
    origins   y_i = (i (H - t)) // (n - 1),  y_0 = 0 for n == 1
    weight    a_i(u) = min(lead, trail) for u in [0, t), with R = O - 2 M,
              lead = R + 1 if y_i == 0 else clamp(u - M + 1, 0, R + 1),  trail = R + 1 if y_i + t == H else clamp(t - M - u, 0, R + 1)

A tile's weight at a pixel is a_iy(y - y_iy) a_ix(x - x_ix): the outer M pixels of every interior tile edge weigh nothing (what
the network computed there saw the cut), a ramp of R + 1 steps follows, edges on the image border lose nothing.  Tile order:
(b, iy, ix) row-major, N = B ny nx tiles of [t_h, t_w].  There is no CPU execution path for the kernels; `tile_plan` is pure
Python."""
from typing import NamedTuple, Optional, Tuple

import torch

from . import _args as A
from . import _native as N
from .model import HydraModel
from .module_denoiser import DenoiserWrapper

_FEATURE = "the tiling code"
SETTINGS = ("tile", "overlap", "margin", "tile_batch")
DEFAULT_MARGIN = 8              # of a model without a finite receptive field (attention, pyramids): a guard band, not exactness


class TilePlan(NamedTuple):
    """the tiles of one [H, W] frame: their shape, their number and origins per axis, and the integer weights a_i(u) per axis
    (weights_y[i][u] for tile row i at its local row u; a tile's weight at a pixel is weights_y[iy][u] * weights_x[ix][v])"""
    t_h: int
    t_w: int
    ny: int
    nx: int
    origins_y: Tuple[int, ...]
    origins_x: Tuple[int, ...]
    weights_y: Tuple[Tuple[int, ...], ...]
    weights_x: Tuple[Tuple[int, ...], ...]

    @property
    def tiles(self) -> int:
        """tiles per image"""
        return self.ny * self.nx


def _checked_plan_arguments(tile, overlap, margin) -> Tuple[int, int, int]:
    T, O, M = A.int_in(tile, "tile", 1), A.int_in(overlap, "overlap", 0), A.int_in(margin, "margin", 0)
    if O > T // 2:
        raise ValueError(f"overlap <= tile // 2 does not hold: overlap {O}, tile {T}")
    if 2 * M > O:
        raise ValueError(f"2 * margin <= overlap does not hold: margin {M}, overlap {O}")
    return T, O, M


def _count(length: int, T: int, O: int) -> int:
    return 1 if length <= T else -((length - O) // -(T - O))


def _axis(length: int, T: int, O: int, M: int):
    t, n = min(T, length), _count(length, T, O)
    origins = tuple((i * (length - t)) // (n - 1) if n > 1 else 0 for i in range(n))
    ramp = O - 2 * M + 1
    weights = tuple(tuple(min(ramp if y0 == 0 else min(max(u - M + 1, 0), ramp),
                              ramp if y0 + t == length else min(max(t - M - u, 0), ramp)) for u in range(t)) for y0 in origins)
    return t, n, origins, weights


def tile_plan(H: int, W: int, tile: int, overlap: int, margin: int) -> TilePlan:
    """the plan of an [H, W] frame (module docstring); ValueError naming the rule an invalid plan breaks"""
    H, W = A.int_in(H, "H", 1), A.int_in(W, "W", 1)
    T, O, M = _checked_plan_arguments(tile, overlap, margin)
    t_h, ny, oy, wy = _axis(H, T, O, M)
    t_w, nx, ox, wx = _axis(W, T, O, M)
    return TilePlan(t_h, t_w, ny, nx, oy, ox, wy, wx)


def _tile_counts(H: int, W: int, T: int, O: int) -> Tuple[int, int, int, int]:
    """(t_h, t_w, ny, nx) without the weights"""
    return min(T, H), min(T, W), _count(H, T, O), _count(W, T, O)


def tile_split_u8(image_u8: torch.Tensor, tile: int, overlap: int, first: int = 0, count: Optional[int] = None) -> torch.Tensor:
    """bf_op_tile_split_u8 on a uint8 device tensor [B,H,W,C] (C = 1 or 3): tiles [first, first + count) of the tile order
    (b, iy, ix) as uint8 [count, t_h, t_w, C]; count=None: every tile from `first` on"""
    T, O, _ = _checked_plan_arguments(tile, overlap, 0)
    image_u8 = A.to_device(A.image_batch(image_u8, "image_u8", (torch.uint8,)), False, None, "image_u8", _FEATURE).contiguous()
    B, H, W, C = image_u8.shape
    t_h, t_w, ny, nx = _tile_counts(H, W, T, O)
    total = B * ny * nx
    first = A.int_in(first, "first", 0, total - 1)
    count = total - first if count is None else A.int_in(count, "count", 1, total - first)
    out = torch.empty((count, t_h, t_w, C), dtype=torch.uint8, device=image_u8.device)
    N.call("bf_op_tile_split_u8", N.ptr(image_u8), N.ptr(out), B, H, W, C, T, T, O, first, count, N.stream_ptr(image_u8))
    return out


def tile_blend(tiles_f32: torch.Tensor, B: int, H: int, W: int, tile: int, overlap: int, margin: int,
               cast_to_uint8: bool = True) -> torch.Tensor:
    """bf_op_tile_blend on the float32 device results of all N = B ny nx tiles of the plan, [N, t_h, t_w, C] in tile order: per
    output sample the weighted mean of the tiles with a positive weight there (fp64 sum in ascending tile order, one division);
    [B,H,W,C] float32, or rounded half to even and clipped to uint8"""
    B, H, W = A.int_in(B, "B", 1), A.int_in(H, "H", 1), A.int_in(W, "W", 1)
    T, O, M = _checked_plan_arguments(tile, overlap, margin)
    A.image_batch(tiles_f32, "tiles_f32", (torch.float32,))
    t_h, t_w, ny, nx = _tile_counts(H, W, T, O)
    C = int(tiles_f32.shape[-1])
    if tuple(tiles_f32.shape) != (B * ny * nx, t_h, t_w, C):
        raise ValueError(f"tiles_f32 must be {(B * ny * nx, t_h, t_w, C)} for {B} frames of {H} x {W}, tile {T}, overlap {O}; got "
                         f"{tuple(tiles_f32.shape)}")
    tiles_f32 = A.to_device(tiles_f32, False, None, "tiles_f32", _FEATURE).contiguous()
    out = torch.empty((B, H, W, C), dtype=torch.uint8 if cast_to_uint8 else torch.float32, device=tiles_f32.device)
    N.call("bf_op_tile_blend", N.ptr(tiles_f32), N.ptr(out), int(bool(cast_to_uint8)), B, H, W, C, T, T, O, M,
           N.stream_ptr(tiles_f32))
    return out


def receptive_radius(hydra) -> Optional[int]:
    """How far a pixel's input reaches into the output, in pixels: for the 16-filter resnet engine (HydraModel) the radius of
    the base convolution plus that of every block convolution, read from `hydra.desc`; None for every other model (attention
    and pyramids see the whole frame: no finite margin makes tiling exact)."""
    if not isinstance(hydra, HydraModel):
        return None
    d = hydra.desc
    return (d.kernel_size - 1) // 2 + d.no_layers * d.block_convs * (d.block_kernel - 1) // 2


def default_overlap(tile: int, margin: int) -> int:
    return min(tile // 2, max(32, 2 * margin + 16))


def checked_settings(tile: int = 256, overlap: Optional[int] = None, margin: Optional[int] = None, tile_batch: int = 16):
    """the settings of TiledDenoiserModule, checked: (tile, overlap, margin, tile_batch).  A margin of None is the model's own,
    known once there is a model: it stays None, and so does an overlap that follows from it."""
    tile, tile_batch = A.int_in(tile, "tile", 1), A.int_in(tile_batch, "tile_batch", 1)
    if margin is None:
        if overlap is not None:
            overlap = _checked_plan_arguments(tile, overlap, 0)[1]
        return tile, overlap, None, tile_batch
    margin = A.int_in(margin, "margin", 0)
    if 2 * margin > tile // 2:
        raise ValueError(f"margin {margin} needs 2 * margin <= tile // 2: the smallest tile that works is {4 * margin}, got {tile}")
    overlap = default_overlap(tile, margin) if overlap is None else overlap
    return _checked_plan_arguments(tile, overlap, margin) + (tile_batch,)


def parse_setting(tiled) -> Optional[dict]:
    """load_model's `tiled`: None | False -> None; True -> the defaults; a dict of SETTINGS -> itself.  Everything that does not
    depend on the model is checked here, before anything is loaded."""
    if isinstance(tiled, dict) and set(tiled) - set(SETTINGS):
        raise ValueError(f"tiled may set tile, overlap, margin and tile_batch, got {sorted(tiled)}")
    settings = A.parse_setting(tiled, "tiled", "None, a bool or a dict of TiledDenoiserModule settings", SETTINGS)
    if settings:
        checked_settings(**settings)
    return settings


class TiledDenoiserModule(DenoiserWrapper):
    """A denoiser run tile by tile: uint8 [B,H,W,C] -> uint8 [B,H,W,C] (float32, not rounded, with cast_to_uint8=False).
    `module`, argument checks, input handling, return types, empty batches and f16-range status as every wrapper
    (DenoiserWrapper).

    `margin` defaults to receptive_radius(model) -- with it a tile's weighted pixels never saw the cut, and the 16-filter resnet
    gives what it gives on the whole frame wherever the frame's own padding does not reach -- or to 8 where
    there is none; `overlap` defaults to min(tile // 2, max(32, 2 * margin + 16)).

    Batching contract: with N = B ny nx tiles and K = min(tile_batch, N), the chunks start at tiles 0, K, 2K, ... and the last
    one at N - K (it is shifted back and computes a few tiles again), so that every denoiser call has the shape [K, t_h, t_w, C]
    and every slot of it holds a real tile.  Each chunk is tile_split_u8, the float module, a store into the results
    [N, t_h, t_w, C]; one tile_blend follows.  `last_plan` is the TilePlan of the last call."""
    SETTINGS = SETTINGS

    def __init__(self, module, tile: int = 256, overlap: Optional[int] = None, margin: Optional[int] = None, tile_batch: int = 16,
                 cast_to_uint8: bool = True):
        if isinstance(module, TiledDenoiserModule):
            raise ValueError("module is already tiled")
        self._wrap(module, cast_to_uint8)
        if margin is None:
            radius = receptive_radius(self.model_hydra)
            margin = DEFAULT_MARGIN if radius is None else radius
        self._tile, self._overlap, self._margin, self._tile_batch = checked_settings(tile, overlap, margin, tile_batch)
        self._record = {"plan": None}

    @property
    def last_plan(self) -> Optional[TilePlan]:
        """the TilePlan of the last call of this module or of its float form"""
        return self._record["plan"]

    @staticmethod
    def chunk_starts(tiles: int, tile_batch: int):
        """(K, the first tile of every denoiser call) of the batching contract"""
        K = min(tile_batch, tiles)
        starts = list(range(0, tiles - K + 1, K))
        if starts[-1] != tiles - K:
            starts.append(tiles - K)
        return K, starts

    def __call__(self, image):
        image, was_numpy = self._checked_input(image)
        B, H, W, _ = image.shape
        if B == 0:
            return self._empty_output(image, was_numpy)
        image = self._place(image, was_numpy, "image", _FEATURE)
        plan = self._record["plan"] = tile_plan(H, W, self._tile, self._overlap, self._margin)
        K, starts = self.chunk_starts(B * plan.tiles, self._tile_batch)
        results = None
        for start in starts:
            batch = tile_split_u8(image, self._tile, self._overlap, start, K)
            result = self._run(batch)
            if self._repeat_in_fp32(was_numpy):
                return self(image.cpu().numpy())
            if results is None:
                results = torch.empty((B * plan.tiles,) + tuple(result.shape[1:]), dtype=torch.float32, device=image.device)
            results[start:start + K].copy_(result)
        return self._deliver(tile_blend(results, B, H, W, self._tile, self._overlap, self._margin, self._cast_to_uint8), was_numpy)
