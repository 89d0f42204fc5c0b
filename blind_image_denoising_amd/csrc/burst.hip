// Burst merge: block-matching alignment of the T frames of a burst to one of them (bf_burst_align) and the robust temporal merge
// along the alignment field (bf_op_burst_merge).  The host side is blind_image_denoising_amd/burst.py; the contract is in
// include/bfcnn_hip.h, the choices and the measurements are DESIGN.md 7.16.  Everything is integer arithmetic up to the one
// fp64 division of the merge; scalars only: nothing is uploaded, allocated or synchronised.
//
// Luma pyramid.  Level 0 is a per-pixel map between two flat arrays: a thread owns four consecutive pixels, reads their 4 C
// bytes as C dwords and writes one dword (the byte form at an unaligned base and for the last pixels).  Level k + 1 is one thread
// per output pixel.
//
// Alignment, one launch per level, coarsest first.  A WAVE owns one 16 x 16 tile of one alternate frame (four tiles of a tile
// row per workgroup): the reference tile (pixels past the frame as 0) and the (16 + 2 R)^2 search window around the predicted
// displacement (gathered with the clamp, rows of nine dwords) go to LDS once, then the candidates are dealt over the lanes, each
// to a pair of lanes that take eight rows of the tile each: a tile row is four dwords of the reference (one address for the
// whole wave) against five dwords of the window row, byte-aligned to the candidate's column with v_alignbyte_b32 and, where the
// frame cuts the tile, masked to its width, and four v_sad_u8.  The candidate's packed key cost << 15 | (u^2 + v^2) << 8 |
// (u + R) << 4 | (v + R) orders as (cost, u^2 + v^2, u, v) does (cost <= 65 280 < 2^16); its minimum over the wave is a butterfly
// of six shuffles.  -DBF_BURST_PLAIN_SAD builds the byte-by-byte form of the same sum (the comparison of DESIGN.md 7.16).
//
// Merge.  A workgroup owns one tile, where the displacement of every frame is uniform, and a thread one pixel.  The reference
// patch (20 x 20 x C, coordinates clamped) is staged once; per alternate frame the displaced patch, then the squared
// differences summed over the channels, then the 5 x 5 box sum as a row pass and a column pass through LDS.  num, den and the
// sum of squared weights stay in integer registers; the threshold ramp divides in 32 bits when hi - lo < 2^23 (every threshold
// burst_thresholds makes for sigma < 193 at C = 3 and k = (1.5, 3)) and in 64 bits otherwise.
#include "bf_common.h"

namespace {

constexpr int BU_TILE = 16, BU_MAXC = 4, BU_MAXT = 16, BU_MAXK = 4, BU_MAXR = 7;
constexpr int BU_THREADS = 256, BU_WAVES = BU_THREADS / 64;
constexpr int BU_WIN_ROWS = BU_TILE + 2 * BU_MAXR;               // 30 rows of 30 pixels at R = 7
constexpr int BU_WIN_COLS = 32;                                  // bytes of a window row that are filled (30 are read at R = 7)
constexpr int BU_WIN_PITCH = 36;                                 // bytes from a window row to the next in LDS: nine dwords, so that the lanes'
                                                                 // rows (one per u) start on different banks; at eight, u and u + 4 collide
constexpr int BU_PATCH = BU_TILE + 4;                            // merge: the 5 x 5 windows of a tile reach two pixels past it

__host__ __device__ inline int bu_ceil_div(int a, int b) { return (a + b - 1) / b; }
__device__ __forceinline__ int bu_clamp(int v, int last) { return min(max(v, 0), last); }

// the scratch of bf_burst_align (bfcnn_hip.h): byte offsets of the luma levels and of the fields of the levels above 0
struct BuLayout {
    int h[BU_MAXK], w[BU_MAXK], gy[BU_MAXK], gx[BU_MAXK];
    int64_t luma[BU_MAXK], field[BU_MAXK], bytes;
};

bool bu_shape_ok(int B, int T, int H, int W, int C)
{
    if (B <= 0 || T < 1 || T > BU_MAXT || H <= 0 || W <= 0 || C < 1 || C > BU_MAXC) return false;
    const int64_t frame = (int64_t)H * W;
    // one frame in 32-bit byte arithmetic; every grid below INT32_MAX workgroups: the smallest unit of work is a tile, and a frame
    // has ceil(H / 16) ceil(W / 16) <= H W / 256 + H / 16 + W / 16 + 1 of them
    return frame * C <= INT32_MAX / 4 && (int64_t)B * T <= INT32_MAX / 4 && (frame / 16 + H + W + 1) * B * T <= INT32_MAX / 4;
}

bool bu_layout(int B, int T, int H, int W, int K, BuLayout& L)
{
    if (K < 1 || K > BU_MAXK) return false;
    int64_t off = 0;
    for (int k = 0; k < K; ++k) {
        L.h[k] = k ? bu_ceil_div(L.h[k - 1], 2) : H;
        L.w[k] = k ? bu_ceil_div(L.w[k - 1], 2) : W;
        L.gy[k] = bu_ceil_div(L.h[k], BU_TILE);
        L.gx[k] = bu_ceil_div(L.w[k], BU_TILE);
        L.luma[k] = off;
        off += ((int64_t)B * T * L.h[k] * L.w[k] + 15) / 16 * 16;
    }
    for (int k = 0; k < K; ++k) {
        L.field[k] = off;
        if (k) off += ((int64_t)B * T * L.gy[k] * L.gx[k] * 2 * (int64_t)sizeof(int) + 15) / 16 * 16;
    }
    L.bytes = off;
    return true;
}

// ---- luma pyramid ------------------------------------------------------------------------------------------------------------

// dst[p] = (2 sum_c src[p C + c] + C) / (2 C) over the flat pixel index p of the whole burst
template <int C>
__global__ __launch_bounds__(BU_THREADS) void burst_luma_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int64_t pixels, int vec)
{
    const int64_t p = 4 * ((int64_t)blockIdx.x * BU_THREADS + threadIdx.x);
    if (p >= pixels) return;
    if (vec && p + 4 <= pixels) {                                // 4 C bytes from a dword boundary (p C is a multiple of 4)
        unsigned in[C], out = 0u;
#pragma unroll
        for (int k = 0; k < C; ++k) in[k] = *reinterpret_cast<const unsigned*>(src + p * C + 4 * k);
#pragma unroll
        for (int px = 0; px < 4; ++px) {
            unsigned sum = 0u;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int byte = px * C + c;                     // compile-time after unrolling
                sum += (in[byte >> 2] >> (8 * (byte & 3))) & 0xFFu;
            }
            out |= ((2u * sum + C) / (2u * C)) << (8 * px);
        }
        *reinterpret_cast<unsigned*>(dst + p) = out;
        return;
    }
    for (int i = 0; i < 4 && p + i < pixels; ++i) {
        unsigned sum = 0u;
#pragma unroll
        for (int c = 0; c < C; ++c) sum += src[(p + i) * C + c];
        dst[p + i] = (uint8_t)((2u * sum + C) / (2u * C));
    }
}

// dst[f, y, x] = (the 2 x 2 cell of src[f] at (2 y, 2 x), coordinates clamped, + 2) >> 2; blockIdx.x = f blocks + piece of 256 pixels
__global__ __launch_bounds__(BU_THREADS) void burst_down_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int h, int w, int h2,
                                                                int w2, int blocks)
{
    const int64_t f = blockIdx.x / blocks;
    const int e = (blockIdx.x % blocks) * BU_THREADS + threadIdx.x;
    if (e >= h2 * w2) return;
    const int y = e / w2, x = e - y * w2;
    const int ya = 2 * y, yb = min(2 * y + 1, h - 1), xa = 2 * x, xb = min(2 * x + 1, w - 1);      // 2 y <= h - 1 as y < ceil(h / 2)
    const uint8_t* __restrict__ s = src + f * h * w;
    const unsigned sum = (unsigned)s[ya * w + xa] + s[ya * w + xb] + s[yb * w + xa] + s[yb * w + xb];
    dst[f * h2 * w2 + e] = (uint8_t)((sum + 2u) >> 2);
}

// ---- alignment ---------------------------------------------------------------------------------------------------------------

// sum over the rows r0 <= r < r1 of a tile of |ref[r][0..15] - win[r][cv .. cv + 15]|, both as dwords in LDS; MASKED: the window's
// bytes are cleared where the tile is cut by the frame (the reference holds 0 there)
template <bool MASKED>
__device__ __forceinline__ unsigned bu_rows_sad(const unsigned (*win)[BU_WIN_PITCH / 4], const unsigned (*ref)[BU_TILE / 4], int r0, int r1, int cv,
                                                const unsigned (&mask)[4])
{
    unsigned cost = 0u;
#ifndef BF_BURST_PLAIN_SAD
    const int first = cv >> 2;                                   // dwords first .. first + 4 <= 7 of the window row
    const unsigned shift = (unsigned)(cv & 3);
    for (int r = r0; r < r1; ++r) {
        const unsigned* __restrict__ wr = win[r] + first;
        const unsigned* __restrict__ rr = ref[r];
        const unsigned w0 = wr[0], w1 = wr[1], w2 = wr[2], w3 = wr[3], w4 = wr[4];
        unsigned a[4] = {__builtin_amdgcn_alignbyte(w1, w0, shift), __builtin_amdgcn_alignbyte(w2, w1, shift),
                         __builtin_amdgcn_alignbyte(w3, w2, shift), __builtin_amdgcn_alignbyte(w4, w3, shift)};
#pragma unroll
        for (int q = 0; q < 4; ++q) cost = __builtin_amdgcn_sad_u8(rr[q], MASKED ? a[q] & mask[q] : a[q], cost);
    }
#else
    const uint8_t* rt = reinterpret_cast<const uint8_t*>(ref);
    const uint8_t* wt = reinterpret_cast<const uint8_t*>(win);
    for (int r = r0; r < r1; ++r)
        for (int c = 0; c < BU_TILE; ++c) {
            const int keep = (int)((mask[c >> 2] >> (8 * (c & 3))) & 1u);
            const int d = (int)rt[r * BU_TILE + c] - keep * (int)wt[r * BU_WIN_PITCH + c + cv];
            cost += (unsigned)(d < 0 ? -d : d);
        }
#endif
    return cost;
}

// field[bt, i, j] = the winner of tile (i, j) of frame bt = b T + t at one level (zero for t == ref).  `coarse` (the field of the
// level above, [B T, cgy, cgx, 2]) predicts, NULL at the coarsest level.  blockIdx.x = (bt gy + i) ceil(gx / 4) + group of four j.
__global__ __launch_bounds__(BU_THREADS) void burst_align_kernel(const uint8_t* __restrict__ luma, const int* __restrict__ coarse,
                                                                 int* __restrict__ field, int T, int ref, int h, int w, int gy, int gx,
                                                                 int cgy, int cgx, int R)
{
    __shared__ unsigned ref_tile[BU_WAVES][BU_TILE][BU_TILE / 4];
    __shared__ unsigned window[BU_WAVES][BU_WIN_ROWS][BU_WIN_PITCH / 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int groups = bu_ceil_div(gx, BU_WAVES);
    int g = blockIdx.x;
    const int j = (g % groups) * BU_WAVES + wave;
    g /= groups;
    const int i = g % gy;
    const int64_t bt = g / gy;
    const int t = (int)(bt % T);
    const bool live = j < gx;                                    // the last group of a tile row may hold fewer than four tiles
    int* __restrict__ mine = field + ((bt * gy + i) * gx + j) * 2;
    if (t == ref) {                                              // the whole workgroup
        if (live && lane < 2) mine[lane] = 0;
        return;
    }
    int d0y = 0, d0x = 0;
    if (coarse && live) {
        const int* __restrict__ c = coarse + ((bt * cgy + min(i >> 1, cgy - 1)) * cgx + min(j >> 1, cgx - 1)) * 2;
        d0y = 2 * c[0];
        d0x = 2 * c[1];
    }
    const int y0 = i * BU_TILE, x0 = j * BU_TILE;
    const int th = live ? min(BU_TILE, h - y0) : 0, tw = live ? min(BU_TILE, w - x0) : 0;          // >= 1 for a live tile
    const uint8_t* __restrict__ lr = luma + (bt - t + ref) * h * w;
    const uint8_t* __restrict__ la = luma + bt * h * w;
    // staging: a lane keeps its column and walks the rows, so that a pass is one clamp, one multiply-add, one load and one byte
    uint8_t* rt = reinterpret_cast<uint8_t*>(ref_tile[wave]);
    for (int r = lane >> 4, c = lane & 15; r < BU_TILE; r += 4)
        rt[r * BU_TILE + c] = (r < th && c < tw) ? lr[(y0 + r) * w + x0 + c] : (uint8_t)0;
    uint8_t* wt = reinterpret_cast<uint8_t*>(window[wave]);
    const int rows = BU_TILE + 2 * R;                            // <= BU_WIN_ROWS; a row is filled to 32 bytes, all of them clamped
    const int wx = lane & (BU_WIN_COLS - 1), xx = bu_clamp(x0 + d0x - R + wx, w - 1);
    for (int wy = lane / BU_WIN_COLS; wy < rows; wy += 64 / BU_WIN_COLS)
        wt[wy * BU_WIN_PITCH + wx] = live ? la[bu_clamp(y0 + d0y - R + wy, h - 1) * w + xx] : (uint8_t)0;
    __syncthreads();

    // A work item is a candidate and one half of the tile's rows: lanes 2 k and 2 k + 1 share candidate k and add their halves
    // with one shuffle (81 candidates: three passes of eight rows over 64 lanes instead of two of sixteen).
    const int side = 2 * R + 1, items = 2 * side * side;
    const unsigned side_inv = (65536u + side - 1) / side;        // (c side_inv) >> 16 == c / side for c < side^2 <= 225, side <= 15
    unsigned mask[4];                                            // the bytes of a tile row that lie inside the frame
#pragma unroll
    for (int q = 0; q < 4; ++q) mask[q] = tw >= 4 * q + 4 ? 0xFFFFFFFFu : (tw <= 4 * q ? 0u : (1u << (8 * (tw - 4 * q))) - 1u);
    unsigned best = 0xFFFFFFFFu;
    for (int base = 0; base < items; base += 64) {               // the same passes for every lane: the shuffle below needs both of a pair
        const int item = base + lane;
        const bool valid = live && item < items;                 // items is even: a pair is valid or not as a whole
        const int cand = min(item, items - 1) >> 1;
        const int cu = (int)(((unsigned)cand * side_inv) >> 16), cv = cand - cu * side;      // u + R, v + R
        const int r0 = 8 * (item & 1), r1 = valid ? min(th, r0 + 8) : r0;
        const unsigned (*win)[BU_WIN_PITCH / 4] = window[wave] + cu;                      // row r + cu <= 15 + 2 R
        unsigned cost = tw == BU_TILE ? bu_rows_sad<false>(win, ref_tile[wave], r0, r1, cv, mask)
                                      : bu_rows_sad<true>(win, ref_tile[wave], r0, r1, cv, mask);
        cost += (unsigned)__shfl_xor((int)cost, 1);
        const int u = cu - R, v = cv - R;
        if (valid) best = min(best, (cost << 15) | ((unsigned)(u * u + v * v) << 8) | ((unsigned)cu << 4) | (unsigned)cv);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, off));
    if (live && lane == 0) {
        mine[0] = d0y + (int)((best >> 4) & 15u) - R;
        mine[1] = d0x + (int)(best & 15u) - R;
    }
}

// ---- merge -------------------------------------------------------------------------------------------------------------------

// lo < D < hi: ((hi - D) 256) / (hi - lo), in 32 bits when `narrow` (hi - lo < 2^23: the product is below 2^31)
__device__ __forceinline__ int bu_weight(int D, long long lo, long long hi, bool narrow)
{
    if (D <= lo) return 256;
    if (D >= hi) return 0;
    if (narrow) return (int)(((unsigned)(hi - D) << 8) / (unsigned)(hi - lo));
    return (int)(((hi - D) * 256) / (hi - lo));
}

// blockIdx.x = (b gy + i) gx + j; thread (ty, tx) = pixel (16 i + ty, 16 j + tx)
template <int C>
__global__ __launch_bounds__(BU_THREADS) void burst_merge_kernel(const uint8_t* __restrict__ frames, const int* __restrict__ field,
                                                                 const long long* __restrict__ thresholds, int T, int H, int W, int ref,
                                                                 int gy, int gx, void* __restrict__ out, int out_u8, int* __restrict__ counts)
{
    __shared__ uint8_t ref_patch[BU_PATCH * BU_PATCH * C], alt_patch[BU_PATCH * BU_PATCH * C];
    __shared__ int sq_diff[BU_PATCH][BU_PATCH], row_sum[BU_PATCH][BU_TILE];
    int g = blockIdx.x;
    const int j = g % gx;
    g /= gx;
    const int i = g % gy;
    const int64_t b = g / gy;
    const int y0 = i * BU_TILE, x0 = j * BU_TILE;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int y = y0 + ty, x = x0 + tx;
    const bool inside = y < H && x < W;
    const int64_t frame = (int64_t)H * W * C;
    const uint8_t* __restrict__ fr = frames + (b * T + ref) * frame;
    for (int e = threadIdx.x; e < BU_PATCH * BU_PATCH; e += BU_THREADS) {
        const int qy = bu_clamp(y0 - 2 + e / BU_PATCH, H - 1), qx = bu_clamp(x0 - 2 + e % BU_PATCH, W - 1);
#pragma unroll
        for (int c = 0; c < C; ++c) ref_patch[e * C + c] = fr[((int64_t)qy * W + qx) * C + c];
    }
    const long long lo = thresholds[2 * b], hi = thresholds[2 * b + 1];
    const bool narrow = hi - lo < (1 << 23) && hi > lo;
    const int centre = ((ty + 2) * BU_PATCH + tx + 2) * C;
    __syncthreads();
    int num[C], den = 256, sq = 256 * 256;
#pragma unroll
    for (int c = 0; c < C; ++c) num[c] = 256 * (int)ref_patch[centre + c];
    for (int t = 0; t < T; ++t) {
        if (t == ref) continue;
        const int* __restrict__ d = field + (((b * T + t) * gy + i) * gx + j) * 2;
        // clamp(q + d) saturates: a displacement beyond +-H (+-W) gives what +-H (+-W) gives, and the sum stays inside an int
        const int dy = min(max(d[0], -H), H), dx = min(max(d[1], -W), W);
        const uint8_t* __restrict__ fa = frames + (b * T + t) * frame;
        for (int e = threadIdx.x; e < BU_PATCH * BU_PATCH; e += BU_THREADS) {
            const int qy = bu_clamp(y0 - 2 + e / BU_PATCH, H - 1), qx = bu_clamp(x0 - 2 + e % BU_PATCH, W - 1);
            const int ay = bu_clamp(qy + dy, H - 1), ax = bu_clamp(qx + dx, W - 1);
            int sum = 0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const uint8_t a = fa[((int64_t)ay * W + ax) * C + c];
                alt_patch[e * C + c] = a;
                const int diff = (int)a - (int)ref_patch[e * C + c];
                sum += diff * diff;
            }
            sq_diff[e / BU_PATCH][e % BU_PATCH] = sum;           // <= 4 * 255^2
        }
        __syncthreads();
        for (int e = threadIdx.x; e < BU_PATCH * BU_TILE; e += BU_THREADS) {
            const int r = e >> 4, c = e & 15;
            row_sum[r][c] = sq_diff[r][c] + sq_diff[r][c + 1] + sq_diff[r][c + 2] + sq_diff[r][c + 3] + sq_diff[r][c + 4];
        }
        __syncthreads();
        if (inside) {
            const int D = row_sum[ty][tx] + row_sum[ty + 1][tx] + row_sum[ty + 2][tx] + row_sum[ty + 3][tx] + row_sum[ty + 4][tx];     // <= 25 * 4 * 255^2
            const int wgt = bu_weight(D, lo, hi, narrow);
#pragma unroll
            for (int c = 0; c < C; ++c) num[c] += wgt * (int)alt_patch[centre + c];
            den += wgt;
            sq += wgt * wgt;
        }
        __syncthreads();                                         // the next frame overwrites alt_patch, sq_diff and row_sum
    }
    if (!inside) return;
    const int64_t p = (b * H + y) * W + x;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float q = (float)__ddiv_rn((double)num[c], (double)den);          // 0 <= q <= 255
        if (out_u8) ((uint8_t*)out)[p * C + c] = (uint8_t)rintf(q);             // half to even
        else ((float*)out)[p * C + c] = q;
    }
    if (counts) {
        counts[2 * p] = den;
        counts[2 * p + 1] = sq;
    }
}

}  // namespace

extern "C" int64_t bf_burst_align_scratch_bytes(int B, int T, int H, int W, int C, int levels)
{
    BuLayout L;
    if (!bu_shape_ok(B, T, H, W, C) || !bu_layout(B, T, H, W, levels, L)) return BF_EINVAL;
    return L.bytes;
}

extern "C" int bf_burst_align(const uint8_t* frames, int B, int T, int H, int W, int C, int ref, int levels, int search, void* scratch,
                              int64_t scratch_bytes, int* field_out, void* stream)
{
    BuLayout L;
    if (!frames || !scratch || !field_out || !bu_shape_ok(B, T, H, W, C) || !bu_layout(B, T, H, W, levels, L)) return BF_EINVAL;
    if (ref < 0 || ref >= T || search < 1 || search > BU_MAXR) return BF_EINVAL;
    if (scratch_bytes < L.bytes || (uintptr_t)scratch % 16 || (uintptr_t)field_out % 4) return BF_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    uint8_t* base = (uint8_t*)scratch;
    const int64_t frames_n = (int64_t)B * T, pixels = frames_n * H * W;
    const dim3 grid0((unsigned)(((pixels + 3) / 4 + BU_THREADS - 1) / BU_THREADS));
    const int vec = (uintptr_t)frames % 4 == 0;                  // the level-0 luma starts the (16-byte aligned) scratch
    switch (C) {
    case 1: hipLaunchKernelGGL(burst_luma_kernel<1>, grid0, dim3(BU_THREADS), 0, s, frames, base + L.luma[0], pixels, vec); break;
    case 2: hipLaunchKernelGGL(burst_luma_kernel<2>, grid0, dim3(BU_THREADS), 0, s, frames, base + L.luma[0], pixels, vec); break;
    case 3: hipLaunchKernelGGL(burst_luma_kernel<3>, grid0, dim3(BU_THREADS), 0, s, frames, base + L.luma[0], pixels, vec); break;
    default: hipLaunchKernelGGL(burst_luma_kernel<4>, grid0, dim3(BU_THREADS), 0, s, frames, base + L.luma[0], pixels, vec); break;
    }
    for (int k = 1; k < levels; ++k) {
        const int blocks = bu_ceil_div(L.h[k] * L.w[k], BU_THREADS);
        hipLaunchKernelGGL(burst_down_kernel, dim3((unsigned)(frames_n * blocks)), dim3(BU_THREADS), 0, s, base + L.luma[k - 1],
                           base + L.luma[k], L.h[k - 1], L.w[k - 1], L.h[k], L.w[k], blocks);
    }
    for (int k = levels - 1; k >= 0; --k) {
        const bool top = k == levels - 1;
        const int* coarse = top ? nullptr : (const int*)(base + L.field[k + 1]);
        int* field = k ? (int*)(base + L.field[k]) : field_out;
        const dim3 grid((unsigned)(frames_n * L.gy[k] * bu_ceil_div(L.gx[k], BU_WAVES)));
        hipLaunchKernelGGL(burst_align_kernel, grid, dim3(BU_THREADS), 0, s, base + L.luma[k], coarse, field, T, ref, L.h[k], L.w[k],
                           L.gy[k], L.gx[k], top ? 0 : L.gy[k + 1], top ? 0 : L.gx[k + 1], search);
    }
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}

extern "C" int bf_op_burst_merge(const uint8_t* frames, const int* field, const int64_t* thresholds, int B, int T, int H, int W, int C,
                                 int ref, void* out, int out_is_u8, int* counts_or_null, void* stream)
{
    if (!frames || !field || !thresholds || !out || !bu_shape_ok(B, T, H, W, C) || ref < 0 || ref >= T) return BF_EINVAL;
    if (out == (const void*)frames || (uintptr_t)field % 4 || (uintptr_t)thresholds % 8 || (uintptr_t)counts_or_null % 4 ||
        (!out_is_u8 && (uintptr_t)out % 4))
        return BF_EINVAL;
    const int gy = bu_ceil_div(H, BU_TILE), gx = bu_ceil_div(W, BU_TILE);
    const dim3 grid((unsigned)((int64_t)B * gy * gx));
    const long long* thr = (const long long*)thresholds;
    hipStream_t s = (hipStream_t)stream;
    switch (C) {
    case 1: hipLaunchKernelGGL(burst_merge_kernel<1>, grid, dim3(BU_THREADS), 0, s, frames, field, thr, T, H, W, ref, gy, gx, out, out_is_u8, counts_or_null); break;
    case 2: hipLaunchKernelGGL(burst_merge_kernel<2>, grid, dim3(BU_THREADS), 0, s, frames, field, thr, T, H, W, ref, gy, gx, out, out_is_u8, counts_or_null); break;
    case 3: hipLaunchKernelGGL(burst_merge_kernel<3>, grid, dim3(BU_THREADS), 0, s, frames, field, thr, T, H, W, ref, gy, gx, out, out_is_u8, counts_or_null); break;
    default: hipLaunchKernelGGL(burst_merge_kernel<4>, grid, dim3(BU_THREADS), 0, s, frames, field, thr, T, H, W, ref, gy, gx, out, out_is_u8, counts_or_null); break;
    }
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}
