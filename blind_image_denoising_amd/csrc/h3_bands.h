// Band policy of the four row-streaming block kernels: fused_block_h3v_kernel (fused_h3v.hip), fused_block2_h3w_kernel
// (fused_h3w.hip), fwd_block_h3t_kernel (train_fwd_h3t.hip) and bwd_block_h3t_kernel (train_bwd_h3t.hip).
//
// Every [strip of every] image is cut into ceil(H / rows) bands of `rows` rows; one band of one strip = one unit of work of a
// workgroup, and a workgroup walks units blockIdx.x, blockIdx.x + gridDim.x, ...  The host half sizes the bands (bf_band_plan),
// the device half turns a unit's launch-order index into its rows (bf_band_unit; fwd_block_h3t_kernel keeps a copy of its own, see there).
#pragma once
#include "bf_common.h"

// Workgroups a launch of these kernels uses at most: one per CU of the MI355X.  Launch grids AND workspace sizing (the
// bf_*_h3t_grid helpers: rows of partial sums per launch) both derive from this one constant, through bf_band_plan.
constexpr int BF_BAND_WORKGROUPS = 256;

struct BandPlan {
    int nstrips, rows_per_tile, tiles_y, ntiles, grid;
};

// rows per band such that the slowest workgroup (ceil(units / workgroups) units of rows + lead_steps steps each) finishes
// earliest; lead_steps = the steps of a band beyond its rows (pipeline fill / drain + the prologue).
static inline BandPlan bf_band_plan(const int B, const int H, const int nstrips, const int lead_steps)
{
    const long cap = BF_BAND_WORKGROUPS;
    int best = H;
    long best_cost = -1;
    for (int ty = 1; ty <= (H + 7) / 8; ++ty) {
        const int rows = (H + ty - 1) / ty;
        if ((H + rows - 1) / rows != ty) continue;
        const long units = (long)B * ty * nstrips;
        const long cost = ((units + cap - 1) / cap) * (rows + lead_steps);
        if (best_cost < 0 || cost < best_cost) {
            best_cost = cost;
            best = rows;
        }
    }
    BandPlan p;
    p.nstrips = nstrips;
    p.rows_per_tile = best;
    p.tiles_y = (H + best - 1) / best;
    const long units = (long)B * p.tiles_y * nstrips;
    p.ntiles = (int)units;
    p.grid = (int)(units < cap ? units : cap);
    return p;
}

// ---- device: unit decode ------------------------------------------------------------------------------------------------
// The decode reads the plan out of the kernel's own argument struct (their layouts are fixed: bf_common.h); the structs name
// the direction flag differently and the full-row kernel has no strips.
__device__ __forceinline__ int bf_band_reverse(const FusedH3Args& a) { return a.reverse_tiles; }
__device__ __forceinline__ int bf_band_reverse(const FusedH3WArgs& a) { return a.reverse_tiles; }
__device__ __forceinline__ int bf_band_reverse(const BwdBlockH3Args& a) { return a.reverse; }
__device__ __forceinline__ int bf_band_nstrips(const FusedH3Args&) { return 1; }
__device__ __forceinline__ int bf_band_nstrips(const FusedH3WArgs& a) { return a.nstrips; }
__device__ __forceinline__ int bf_band_nstrips(const BwdBlockH3Args& a) { return a.nstrips; }

struct BandUnit {
    int sx, b;                   // strip index, image index
    int nrows;                   // rows of the band
    size_t img;                  // byte offset of the image in a tensor of 64 bytes per pixel (fp32 NHWC C16 / split-planar)
    int ybase, ystep;            // image row of band-relative row k: ybase + ystep * k (a reversed band walks bottom-up)
    __device__ __forceinline__ int y(const int k) const { return ybase + ystep * k; }
};

// unit t of the launch order = (image, band of rows, strip).
// reverse: last unit first and bottom-up.  Consecutive launches alternate, so a launch starts on the rows the previous one
// wrote last -- the ones still in the 256 MB Infinity Cache.  Walking up only mirrors the vertical taps (bf_band_wimage) and
// the row addresses.
// XCD_ORDER: workgroup ids go round the 8 XCDs, so unit t becomes unit (t mod 8) * ntiles / 8 + t / 8 (when 8 divides ntiles):
// an XCD walks a contiguous eighth of the units, and the halo rows two vertically adjacent bands both read (and the 16 halo
// columns two neighbouring strips share) are found in ITS L2.  Without it the neighbours sit on different XCDs and every halo
// is fetched twice from the Infinity Cache / HBM: 626 MB per launch for 537 MB algorithmic in the training forward, 934 MB for
// 671 MB in the backward.
template <bool XCD_ORDER, class Args>
__device__ __forceinline__ BandUnit bf_band_unit(const Args& a, const int t)
{
    BandUnit r;
    const int reverse = bf_band_reverse(a), nstrips = bf_band_nstrips(a);
    const int tp = (XCD_ORDER && (a.ntiles & 7) == 0) ? (t & 7) * (a.ntiles >> 3) + (t >> 3) : t;
    const int tt = reverse ? a.ntiles - 1 - tp : tp;
    const int rest = tt / nstrips;
    r.sx = tt % nstrips;
    r.b = rest / a.tiles_y;
    const int ty = rest - r.b * a.tiles_y;
    const int y0 = ty * a.rows_per_tile;
    r.nrows = min(a.rows_per_tile, a.H - y0);
    r.img = (size_t)r.b * a.H * a.W * 64;
    r.ybase = reverse ? y0 + r.nrows - 1 : y0;
    r.ystep = reverse ? -1 : 1;
    return r;
}

// weight image i = dy * 4 + kind (12 = s2 * identity) as the code's tap row dy: mirrored (dy -> 2 - dy) for a band that walks
// bottom-up
template <class Args>
__device__ __forceinline__ int bf_band_wimage(const Args& a, const int i)
{
    return (bf_band_reverse(a) && i < 12) ? (2 - i / 4) * 4 + i % 4 : i;
}
