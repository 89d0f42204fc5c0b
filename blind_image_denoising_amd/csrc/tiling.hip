// Tiled inference around the denoiser: a frame cut into overlapping tiles of one shape (bf_op_tile_split_u8) and the float
// results of the tiles blended back into the frame (bf_op_tile_blend).  Both take scalars only: the tile origins and weights come
// from the closed forms below inside the kernels, nothing is uploaded, allocated or synchronised.
//
// Plan per axis (length H, nominal tile T, overlap O, margin M; 0 <= 2 M <= O <= T / 2):
//     t = min(T, H),  n = H <= T ? 1 : ceil((H - O) / (T - O)),  y_i = (i (H - t)) / (n - 1)  (y_0 = 0 for n == 1)
// Integer weight of tile i at its local coordinate u, R = O - 2 M:
//     lead = y_i == 0 ? R + 1 : clamp(u - M + 1, 0, R + 1),  trail = y_i + t == H ? R + 1 : clamp(t - M - u, 0, R + 1)
//     a_i(u) = min(lead, trail);  the weight of a tile at a pixel is a_iy(y - y_iy) a_ix(x - x_ix)
// Tile order: (b, iy, ix) row-major, N = B ny nx tiles of [t_h, t_w, C].
//
// Memory pattern as in self_ensemble.hip: a row is indexed by BYTE (split) or by FLOAT (blend), so the lanes of a wave touch
// consecutive addresses of one row in the read and in the write.  The blend is a gather: one thread per output pixel (its C
// floats; the plan arithmetic, a handful of 32-bit divisions, is what a thread spends its time on, and the pixel shares it), one
// workgroup per piece of an output row (the tiles over a row and their weights are the same for the whole workgroup), at most
// 3 x 3 tile reads with positive weight, one write; no atomics, no LDS.  Every element offset
// is int64 (a 50-megapixel frame in float tiles passes 2^31 bytes); the products inside the origin formula stay below 2^31,
// which the launchers check.
#include "bf_common.h"

namespace {

constexpr int TL_THREADS = 256;
constexpr int TL_MAX_CHUNKS = 1024;      // grid.y of the split: the pieces of one tile walk the rest in a loop

struct TileAxis {
    int len, t, n, span;                 // span = len - t
    int margin, ramp;                    // ramp = R + 1
};

__host__ __device__ inline int tl_count(int len, int T, int O)
{
    return len <= T ? 1 : (len - O + (T - O) - 1) / (T - O);
}

__host__ __device__ inline TileAxis tl_axis(int len, int T, int O, int M)
{
    TileAxis a;
    a.len = len;
    a.t = len < T ? len : T;
    a.n = tl_count(len, T, O);
    a.span = len - a.t;
    a.margin = M;
    a.ramp = O - 2 * M + 1;
    return a;
}

__device__ __forceinline__ int tl_origin(const TileAxis& a, int i)
{
    return a.n == 1 ? 0 : (int)((unsigned)i * (unsigned)a.span / (unsigned)(a.n - 1));
}

__device__ __forceinline__ int tl_weight(const TileAxis& a, int origin, int u)
{
    const int lead = origin == 0 ? a.ramp : min(max(u - a.margin + 1, 0), a.ramp);
    const int trail = origin + a.t == a.len ? a.ramp : min(max(a.t - a.margin - u, 0), a.ramp);
    return min(lead, trail);
}

// the tiles [lo, hi] whose extent holds coordinate p: hi = the last tile with origin <= p, found from the inverse of the origin
// formula and then corrected by walking (the walk also makes an off-by-one of the estimate harmless); lo by walking down
__device__ __forceinline__ void tl_covering(const TileAxis& a, int p, int& lo, int& hi)
{
    int i = a.span > 0 ? min((int)((unsigned)p * (unsigned)(a.n - 1) / (unsigned)a.span), a.n - 1) : 0;
    while (i + 1 < a.n && tl_origin(a, i + 1) <= p) ++i;
    while (i > 0 && tl_origin(a, i) > p) --i;
    hi = i;
    while (i > 0 && tl_origin(a, i - 1) + a.t > p) --i;
    lo = i;
}

template <int C>
__global__ __launch_bounds__(TL_THREADS) void tile_split_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                   int W, TileAxis ay, TileAxis ax, int64_t first)
{
    const int64_t g = first + blockIdx.x;                // tile number in the (b, iy, ix) order
    const int per_image = ay.n * ax.n;
    const int64_t b = g / per_image;
    const int in_image = (int)(g - b * per_image);
    const int y0 = tl_origin(ay, in_image / ax.n), x0 = tl_origin(ax, in_image % ax.n);
    const int row_bytes = ax.t * C, tile_bytes = ay.t * row_bytes;
    const uint8_t* __restrict__ s = src + ((b * ay.len + y0) * W + x0) * C;
    uint8_t* __restrict__ d = dst + (int64_t)blockIdx.x * tile_bytes;
    for (int e = blockIdx.y * TL_THREADS + threadIdx.x; e < tile_bytes; e += gridDim.y * TL_THREADS) {
        const int r = e / row_bytes, cb = e - r * row_bytes;
        d[e] = s[(int64_t)r * W * C + cb];
    }
}

template <int C>
__global__ __launch_bounds__(TL_THREADS) void tile_blend_kernel(const float* __restrict__ tiles, void* __restrict__ out, int out_u8,
                                                                TileAxis ay, TileAxis ax)
{
    const int64_t row = blockIdx.x;                      // b * H + y
    const int64_t b = row / ay.len;
    const int y = (int)(row - b * ay.len);
    const int x = blockIdx.y * TL_THREADS + threadIdx.x; // one thread per pixel: the plan arithmetic serves its C samples
    if (x >= ax.len) return;

    int iy_lo, iy_hi, ix_lo, ix_hi;
    tl_covering(ay, y, iy_lo, iy_hi);
    tl_covering(ax, x, ix_lo, ix_hi);

    double num[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) num[ch] = 0.0;
    int64_t den = 0;
    for (int iy = iy_lo; iy <= iy_hi; ++iy) {            // ascending tile order: the order of the sum is part of the contract
        const int oy = tl_origin(ay, iy);
        const int wy = tl_weight(ay, oy, y - oy);
        if (wy == 0) continue;
        const int64_t first_tile = (b * ay.n + iy) * ax.n;
        for (int ix = ix_lo; ix <= ix_hi; ++ix) {
            const int ox = tl_origin(ax, ix);
            const int64_t w = (int64_t)wy * tl_weight(ax, ox, x - ox);
            if (w == 0) continue;
            // pixel (tile (b, iy, ix), row y - oy, column x - ox) of tiles[N, t_h, t_w, C]
            const float* __restrict__ f = tiles + (((first_tile + ix) * ay.t + (y - oy)) * ax.t + (x - ox)) * C;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) num[ch] = fma((double)w, (double)f[ch], num[ch]);
            den += w;
        }
    }
    const int64_t o = (row * ax.len + x) * C;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        const float q = (float)__ddiv_rn(num[ch], (double)den);
        if (out_u8) ((uint8_t*)out)[o + ch] = (uint8_t)rintf(fminf(fmaxf(q, 0.f), 255.f));   // half to even, as the head kernel
        else ((float*)out)[o + ch] = q;
    }
}

// the checks both entry points share; N = the number of tiles of the plan
int tl_check(int B, int H, int W, int C, int tile_h, int tile_w, int overlap, int margin, int64_t& N)
{
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || tile_h <= 0 || tile_w <= 0) return BF_EINVAL;
    if (margin < 0 || overlap < 2 * margin || overlap > tile_h / 2 || overlap > tile_w / 2) return BF_EINVAL;
    if (C != 1 && C != 3) return BF_EUNSUPPORTED;
    const int64_t ny = tl_count(H, tile_h, overlap), nx = tl_count(W, tile_w, overlap);
    // 32-bit arithmetic inside the kernels: i (H - t) and p (n - 1) of the origin formula, the bytes of one tile, one row
    if ((ny - 1) * (int64_t)H > INT32_MAX || (nx - 1) * (int64_t)W > INT32_MAX) return BF_EUNSUPPORTED;
    if ((int64_t)(H < tile_h ? H : tile_h) * (W < tile_w ? W : tile_w) * C > INT32_MAX) return BF_EUNSUPPORTED;
    if ((int64_t)B * H > INT32_MAX || ((int64_t)W + TL_THREADS - 1) / TL_THREADS > 65535) return BF_EUNSUPPORTED;
    N = (int64_t)B * ny * nx;
    return BF_OK;
}

}  // namespace

extern "C" int bf_op_tile_split_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, int C, int tile_h, int tile_w,
                                   int overlap, int64_t first, int64_t count, void* stream)
{
    if (!src || !dst || src == dst) return BF_EINVAL;
    int64_t N = 0;
    const int rc = tl_check(B, H, W, C, tile_h, tile_w, overlap, 0, N);
    if (rc != BF_OK) return rc;
    if (first < 0 || count < 1 || first > N - count) return BF_EINVAL;
    if (count > INT32_MAX) return BF_EUNSUPPORTED;
    const TileAxis ay = tl_axis(H, tile_h, overlap, 0), ax = tl_axis(W, tile_w, overlap, 0);
    const int64_t tile_bytes = (int64_t)ay.t * ax.t * C;
    const int chunks = (int)((tile_bytes + TL_THREADS - 1) / TL_THREADS);
    const dim3 grid((unsigned)count, chunks < TL_MAX_CHUNKS ? chunks : TL_MAX_CHUNKS);
    if (C == 3) hipLaunchKernelGGL(tile_split_u8_kernel<3>, grid, dim3(TL_THREADS), 0, (hipStream_t)stream, src, dst, W, ay, ax, first);
    else hipLaunchKernelGGL(tile_split_u8_kernel<1>, grid, dim3(TL_THREADS), 0, (hipStream_t)stream, src, dst, W, ay, ax, first);
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}

extern "C" int bf_op_tile_blend(const float* tiles, void* out, int out_is_u8, int B, int H, int W, int C, int tile_h, int tile_w,
                                int overlap, int margin, void* stream)
{
    if (!tiles || !out || out == (const void*)tiles) return BF_EINVAL;
    int64_t N = 0;
    const int rc = tl_check(B, H, W, C, tile_h, tile_w, overlap, margin, N);
    if (rc != BF_OK) return rc;
    const TileAxis ay = tl_axis(H, tile_h, overlap, margin), ax = tl_axis(W, tile_w, overlap, margin);
    const dim3 grid((unsigned)(B * H), (unsigned)((W + TL_THREADS - 1) / TL_THREADS));
    if (C == 3) hipLaunchKernelGGL(tile_blend_kernel<3>, grid, dim3(TL_THREADS), 0, (hipStream_t)stream, tiles, out, out_is_u8, ay, ax);
    else hipLaunchKernelGGL(tile_blend_kernel<1>, grid, dim3(TL_THREADS), 0, (hipStream_t)stream, tiles, out, out_is_u8, ay, ax);
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}
