// Video: one step of the recursive motion-compensated temporal filter (bf_op_video_update).  The host side is
// blind_image_denoising_amd/video.py; the contract is in include/bfcnn_hip.h, the choices and the measurements are DESIGN.md 7.20.
// The alignment in front of it is bf_burst_align (burst.hip) on the pair (frame, image of the state).  Everything is integer
// arithmetic; scalars only: nothing is uploaded, allocated or synchronised.
//
// A workgroup owns one 16 x 16 tile, where the displacement is uniform, and a thread one pixel, as burst_merge_kernel does.  The
// frame's patch (20 x 20 x C bytes, coordinates clamped) and the displaced patch of the accumulated frame (20 x 20 x C halfwords,
// clamped twice) are staged in LDS once; the state's uint8 image is NOT read: it is (acc + 128) >> 8 of the staged halfwords, the
// same bits for 3 C bytes per pixel less traffic.  Squared differences summed over the channels, then the 5 x 5 box sum as a row
// pass and a column pass through LDS; the ramp divides in 32 bits when hi - lo < 2^23 and in 64 bits otherwise.
//
// Stores.  A pixel's accumulated value is 2 C bytes (6 at C = 3) and its image C bytes: stored by the pixel's thread a wave would
// write 64 pieces of 6 and of 3 bytes.  The new accumulated tile goes to LDS instead, and the three or four outputs are written from
// there as rows of the tile: 32 C, 16 C, 32 and (float32) 64 C contiguous bytes, a dword per lane wherever every row of the
// tensor starts on a dword (W C even for the halfwords, W C a multiple of 4 for the bytes: the host decides, `vec`), else a
// halfword or a byte per lane, still consecutive lanes on consecutive addresses.  The image and the float32 output are formed
// from the staged halfwords on the way out.
//
// Tile order.  Workgroup ids are dealt round-robin over the 8 XCDs; id g takes tile (g mod 8) ceil(n / 8) + g / 8, so that an XCD
// walks a contiguous eighth of the tiles and the two-pixel halo a tile reads of its neighbours (and the displaced patch, which
// neighbouring tiles with similar motion share) is found in that XCD's L2.
#include "bf_common.h"

namespace {

constexpr int VU_TILE = 16, VU_MAXC = 4, VU_THREADS = 256, VU_MAX_N = 64;
constexpr int VU_PATCH = VU_TILE + 4;                            // the 5 x 5 windows of a tile reach two pixels past it

__host__ __device__ inline int vu_ceil_div(int a, int b) { return (a + b - 1) / b; }
__device__ __forceinline__ int vu_clamp(int v, int last) { return min(max(v, 0), last); }

// lo < D < hi: ((hi - D) 256) / (hi - lo), in 32 bits when `narrow` (hi - lo < 2^23: the product is below 2^31)
__device__ __forceinline__ int vu_weight(int D, long long lo, long long hi, bool narrow)
{
    if (D <= lo) return 256;
    if (D >= hi) return 0;
    if (narrow) return (int)(((unsigned)(hi - D) << 8) / (unsigned)(hi - lo));
    return (int)(((hi - D) * 256) / (hi - lo));
}

// blockIdx.x = g, tile (g mod 8) per_xcd + g / 8 = (b gy + i) gx + j; thread (ty, tx) = pixel (16 i + ty, 16 j + tx)
template <int C>
__global__ __launch_bounds__(VU_THREADS) void video_update_kernel(const uint8_t* __restrict__ x, const uint16_t* __restrict__ acc_in,
                                                                  const uint16_t* __restrict__ cnt_in, const int* __restrict__ field,
                                                                  const long long* __restrict__ thresholds, int H, int W, int gy, int gx,
                                                                  int ntiles, int per_xcd, int n_cap, uint16_t* __restrict__ acc_out,
                                                                  uint16_t* __restrict__ cnt_out, uint8_t* __restrict__ image_out,
                                                                  float* __restrict__ out_f32, int vec2, int vec1)
{
    constexpr int ROW = VU_TILE * C;                             // values of a tile row
    __shared__ uint8_t x_patch[VU_PATCH * VU_PATCH * C];
    __shared__ uint16_t acc_patch[VU_PATCH * VU_PATCH * C];
    __shared__ int sq_diff[VU_PATCH][VU_PATCH], row_sum[VU_PATCH][VU_TILE];
    __shared__ __attribute__((aligned(4))) uint16_t new_acc[VU_TILE * ROW];
    __shared__ __attribute__((aligned(4))) uint16_t new_cnt[VU_TILE * VU_TILE];
    int g = (int)(blockIdx.x & 7u) * per_xcd + (int)(blockIdx.x >> 3);
    if (g >= ntiles) return;                                     // the whole workgroup: the grid is 8 per_xcd >= ntiles
    const int j = g % gx;
    g /= gx;
    const int i = g % gy;
    const int64_t b = g / gy;
    const int y0 = i * VU_TILE, x0 = j * VU_TILE;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int y = y0 + ty, xx = x0 + tx;
    const bool inside = y < H && xx < W;
    const int64_t frame = (int64_t)H * W;                        // pixels of an image
    const int* __restrict__ d = field + ((b * gy + i) * gx + j) * 2;
    // clamp(q + d) saturates: a displacement beyond +-H (+-W) gives what +-H (+-W) gives, and the sum stays inside an int
    const int dy = min(max(d[0], -H), H), dx = min(max(d[1], -W), W);
    const uint8_t* __restrict__ fx = x + b * frame * C;
    const uint16_t* __restrict__ fa = acc_in + b * frame * C;
    for (int e = threadIdx.x; e < VU_PATCH * VU_PATCH; e += VU_THREADS) {
        const int qy = vu_clamp(y0 - 2 + e / VU_PATCH, H - 1), qx = vu_clamp(x0 - 2 + e % VU_PATCH, W - 1);
        const int ay = vu_clamp(qy + dy, H - 1), ax = vu_clamp(qx + dx, W - 1);
        const uint8_t* __restrict__ px = fx + ((int64_t)qy * W + qx) * C;
        const uint16_t* __restrict__ pa = fa + ((int64_t)ay * W + ax) * C;
        int sum = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const uint8_t v = px[c];
            const uint16_t a = pa[c];
            x_patch[e * C + c] = v;
            acc_patch[e * C + c] = a;
            const int diff = (int)(((unsigned)a + 128u) >> 8) - (int)v;        // the state's image against the frame
            sum += diff * diff;
        }
        sq_diff[e / VU_PATCH][e % VU_PATCH] = sum;               // <= 4 * 256^2
    }
    const long long lo = thresholds[2 * b], hi = thresholds[2 * b + 1];
    const bool narrow = hi - lo < (1 << 23) && hi > lo;
    // the count travels with the pixel the accumulated value comes from
    const int n = inside ? min((int)cnt_in[b * frame + (int64_t)vu_clamp(y + dy, H - 1) * W + vu_clamp(xx + dx, W - 1)], n_cap) : 0;
    __syncthreads();
    for (int e = threadIdx.x; e < VU_PATCH * VU_TILE; e += VU_THREADS) {
        const int r = e >> 4, c = e & 15;
        row_sum[r][c] = sq_diff[r][c] + sq_diff[r][c + 1] + sq_diff[r][c + 2] + sq_diff[r][c + 3] + sq_diff[r][c + 4];
    }
    __syncthreads();
    if (inside) {
        const int D = row_sum[ty][tx] + row_sum[ty + 1][tx] + row_sum[ty + 2][tx] + row_sum[ty + 3][tx] + row_sum[ty + 4][tx];   // <= 25 * 4 * 256^2
        const unsigned m = ((unsigned)vu_weight(D, lo, hi, narrow) * (unsigned)n) >> 8;          // <= 256 (n_max - 1)
        const unsigned den = 256u + m;
        const int centre = ((ty + 2) * VU_PATCH + tx + 2) * C;
#pragma unroll
        for (int c = 0; c < C; ++c)                              // 65536 * 255 + 16128 * 65535 + 8192 < 2^31
            new_acc[ty * ROW + tx * C + c] = (uint16_t)((65536u * x_patch[centre + c] + m * acc_patch[centre + c] + (den >> 1)) / den);
        new_cnt[ty * VU_TILE + tx] = (uint16_t)den;
    }
    __syncthreads();

    // the outputs, row by row of the tile: th rows of tw pixels
    const int th = min(VU_TILE, H - y0), tw = min(VU_TILE, W - x0);
    const int64_t p0 = (b * H + y0) * W + x0;                    // the tile's first pixel
    const int nv = tw * C;                                       // values of a row that lie inside the frame
    {   // acc_out: halfwords
        uint16_t* __restrict__ dst = acc_out + p0 * C;
        const int pairs = vec2 ? nv >> 1 : 0;                    // dwords per row; the row's last halfword when nv is odd goes alone
        for (int e = threadIdx.x; e < th * pairs; e += VU_THREADS) {
            const int r = e / pairs, k = e - r * pairs;
            *reinterpret_cast<unsigned*>(dst + (int64_t)r * W * C + 2 * k) = *reinterpret_cast<const unsigned*>(new_acc + r * ROW + 2 * k);
        }
        const int rest = nv - 2 * pairs;
        for (int e = threadIdx.x; e < th * rest; e += VU_THREADS) {
            const int r = e / rest, k = 2 * pairs + e - r * rest;
            dst[(int64_t)r * W * C + k] = new_acc[r * ROW + k];
        }
    }
    {   // cnt_out: halfwords, one per pixel
        uint16_t* __restrict__ dst = cnt_out + p0;
        const bool v = vec2 && (W & 1) == 0;                     // every row of [B,H,W] starts on a dword
        const int pairs = v ? tw >> 1 : 0;
        for (int e = threadIdx.x; e < th * pairs; e += VU_THREADS) {
            const int r = e / pairs, k = e - r * pairs;
            *reinterpret_cast<unsigned*>(dst + (int64_t)r * W + 2 * k) = *reinterpret_cast<const unsigned*>(new_cnt + r * VU_TILE + 2 * k);
        }
        const int rest = tw - 2 * pairs;
        for (int e = threadIdx.x; e < th * rest; e += VU_THREADS) {
            const int r = e / rest, k = 2 * pairs + e - r * rest;
            dst[(int64_t)r * W + k] = new_cnt[r * VU_TILE + k];
        }
    }
    {   // image_out: bytes, (acc + 128) >> 8
        uint8_t* __restrict__ dst = image_out + p0 * C;
        const int quads = vec1 ? nv >> 2 : 0;
        for (int e = threadIdx.x; e < th * quads; e += VU_THREADS) {
            const int r = e / quads, k = e - r * quads;
            const uint16_t* __restrict__ s = new_acc + r * ROW + 4 * k;
            const unsigned lo2 = *reinterpret_cast<const unsigned*>(s), hi2 = *reinterpret_cast<const unsigned*>(s + 2);
            const unsigned packed = (((lo2 & 0xFFFFu) + 128u) >> 8) | ((((lo2 >> 16) + 128u) >> 8) << 8) |
                                    ((((hi2 & 0xFFFFu) + 128u) >> 8) << 16) | ((((hi2 >> 16) + 128u) >> 8) << 24);
            *reinterpret_cast<unsigned*>(dst + (int64_t)r * W * C + 4 * k) = packed;
        }
        const int rest = nv - 4 * quads;
        for (int e = threadIdx.x; e < th * rest; e += VU_THREADS) {
            const int r = e / rest, k = 4 * quads + e - r * rest;
            dst[(int64_t)r * W * C + k] = (uint8_t)(((unsigned)new_acc[r * ROW + k] + 128u) >> 8);
        }
    }
    if (out_f32) {                                               // acc / 256: exact
        float* __restrict__ dst = out_f32 + p0 * C;
        for (int e = threadIdx.x; e < th * nv; e += VU_THREADS) {
            const int r = e / nv, k = e - r * nv;
            dst[(int64_t)r * W * C + k] = (float)new_acc[r * ROW + k] * (1.0f / 256.0f);
        }
    }
}

bool vu_overlap(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}

}  // namespace

extern "C" int bf_op_video_update(const uint8_t* x, const uint16_t* acc_in, const uint16_t* cnt_in, const int* field,
                                  const int64_t* thresholds, int B, int H, int W, int C, int n_max, uint16_t* acc_out, uint16_t* cnt_out,
                                  uint8_t* image_out, float* out_f32_or_null, void* stream)
{
    if (!x || !acc_in || !cnt_in || !field || !thresholds || !acc_out || !cnt_out || !image_out) return BF_EINVAL;
    if (B <= 0 || H <= 0 || W <= 0 || C < 1 || C > VU_MAXC || n_max < 1 || n_max > VU_MAX_N) return BF_EINVAL;
    const int64_t frame = (int64_t)H * W;
    // one frame in 32-bit byte arithmetic; the grid below INT32_MAX workgroups: an image has
    // ceil(H / 16) ceil(W / 16) <= H W / 256 + H / 16 + W / 16 + 1 tiles
    if (frame * C > INT32_MAX / 4 || B > INT32_MAX / 4 || (frame / 16 + H + W + 1) * B > INT32_MAX / 4) return BF_EINVAL;
    if ((uintptr_t)acc_in % 2 || (uintptr_t)cnt_in % 2 || (uintptr_t)acc_out % 2 || (uintptr_t)cnt_out % 2 || (uintptr_t)field % 4 ||
        (uintptr_t)thresholds % 8 || (uintptr_t)out_f32_or_null % 4)
        return BF_EINVAL;
    // a tile reads its neighbours' frame and state: no output may lie over an input, nor over another output
    const int64_t n_px = (int64_t)B * frame;
    const void* ins[3] = {x, acc_in, cnt_in};
    const int64_t in_bytes[3] = {n_px * C, n_px * C * 2, n_px * 2};
    const void* outs[4] = {acc_out, cnt_out, image_out, out_f32_or_null};
    const int64_t out_bytes[4] = {n_px * C * 2, n_px * 2, n_px * C, n_px * C * 4};
    for (int o = 0; o < 4; ++o) {
        if (!outs[o]) continue;
        for (int k = 0; k < 3; ++k)
            if (vu_overlap(outs[o], out_bytes[o], ins[k], in_bytes[k])) return BF_EINVAL;
        for (int k = o + 1; k < 4; ++k)
            if (outs[k] && vu_overlap(outs[o], out_bytes[o], outs[k], out_bytes[k])) return BF_EINVAL;
    }
    const int gy = vu_ceil_div(H, VU_TILE), gx = vu_ceil_div(W, VU_TILE);
    const int ntiles = (int)((int64_t)B * gy * gx), per_xcd = vu_ceil_div(ntiles, 8);
    const dim3 grid((unsigned)(8 * per_xcd));
    const long long* thr = (const long long*)thresholds;
    const int n_cap = 256 * (n_max - 1);
    // a dword per lane where every row of the tensor starts on one: the tile's first column is a multiple of 16 pixels
    const int row = W * C;
    const int vec2 = (uintptr_t)acc_out % 4 == 0 && (uintptr_t)cnt_out % 4 == 0 && row % 2 == 0;
    const int vec1 = (uintptr_t)image_out % 4 == 0 && row % 4 == 0;
    hipStream_t s = (hipStream_t)stream;
#define VU_LAUNCH(CH)                                                                                                                    \
    hipLaunchKernelGGL(video_update_kernel<CH>, grid, dim3(VU_THREADS), 0, s, x, acc_in, cnt_in, field, thr, H, W, gy, gx, ntiles, per_xcd, \
                       n_cap, acc_out, cnt_out, image_out, out_f32_or_null, vec2, vec1)
    switch (C) {
    case 1: VU_LAUNCH(1); break;
    case 2: VU_LAUNCH(2); break;
    case 3: VU_LAUNCH(3); break;
    default: VU_LAUNCH(4); break;
    }
#undef VU_LAUNCH
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}
