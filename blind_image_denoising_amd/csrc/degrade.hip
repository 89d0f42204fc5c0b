// Blind degradations for training: a JPEG encode / decode round trip without entropy coding
// (bf_op_degrade_jpeg), a separable Gaussian blur (bf_op_degrade_blur) and clip + quantise + drop in one pass
// (bf_op_degrade_pointwise).  The contracts are in include/bfcnn_hip.h; all three are INTEGER arithmetic from the first clip on,
// so the result is the same bits whatever the launch geometry (tests/degrade_reference.py restates them in NumPy int64).
//
// Per-image parameters are device int32 arrays of B entries and one launch covers the batch.  A kernel never trusts them: a
// quality is clamped to 0..100, a radius to 0..DG_MAX_RADIUS, a step to 1..255 (the host side refuses such values; the clamp
// only keeps a wrong array from indexing outside LDS).  Every element offset is 64-bit.  No vector loads: a row of C = 3 samples
// has no alignment to rely on, and the same instructions run whatever the base pointer's alignment.
#include "bf_common.h"
#include "philox.h"

namespace {

constexpr int DG_THREADS = 256;
constexpr int DG_MAX_RADIUS = 12;
constexpr int DG_TAPS = 2 * DG_MAX_RADIUS + 1;

// the 8-bit code of a sample: round half to even (nothing happens to the integer-valued samples noise_augment produces), clip
__device__ __forceinline__ int dg_code(const void* __restrict__ src, int src_is_u8, int64_t i)
{
    if (src_is_u8) return ((const uint8_t*)src)[i];
    return (int)fminf(fmaxf(rintf(((const float*)src)[i]), 0.0f), 255.0f);          // NaN -> 0 (fmaxf returns the other operand)
}

__device__ __forceinline__ int dg_clip255(int v) { return min(max(v, 0), 255); }

// ---- JPEG ---------------------------------------------------------------------------------------------------------------------
// ISO/IEC 10918-1 Annex K.1 / K.2 in natural order (row = vertical frequency)
__constant__ uint8_t DG_BASE_TABLES[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// T[u][x] = rint(8192 c(u) / 2 cos((2 x + 1) u pi / 16)); the absolute values of a row or of a column sum to at most 23168
__constant__ short DG_DCT[64] = {
    2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896, 4017, 3406, 2276, 799, -799, -2276, -3406, -4017,
    3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784, 3406, -799, -4017, -2276, 2276, 4017, 799, -3406,
    2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896, 2276, -4017, 799, 3406, -3406, -799, 4017, -2276,
    1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567, 799, -2276, 3406, -4017, 4017, -3406, 2276, -799};

// One workgroup owns a 16 x 16 pixel tile of one image: 4 luminance blocks and, for colour, 2 (4:2:0) or 8 (4:4:4) chrominance
// blocks.  A quarter of the workgroup (64 threads, one per sample) takes one 8 x 8 block through DCT, quantiser and inverse DCT in
// LDS; the blocks of a tile go in rounds of four.  4:4:4 and grey tiles finish here (colour conversion, crop, float store); a
// 4:2:0 tile stores its decoded planes as bytes and jpeg_finish_420_kernel applies the triangle filter, which crosses tiles.
constexpr int JT = 16;                       // tile edge
struct JpegLds {
    int T[64];                               // DG_DCT
    int q[2][64];                            // the image's luminance / chrominance quantiser
    int plane[3][JT * JT];                   // Y, Cb, Cr codes of the tile; 4:2:0 keeps its 8 x 8 chroma in the first 64 entries
    int a[4][64], c[4][64];                  // per quarter: the two intermediates of a round trip
};

// 8 x 8 block at `blk` (row stride `stride`) of codes -> the decoded codes, in place; all 256 threads call it (barriers inside),
// `active` quarters work.  Range of the sums (int32 throughout): |p - 128| <= 128, so the row sums are <= 128 * 23168 < 2^22 and
// |a| <= 2897; column sums <= 2897 * 23168 < 2^27, |c8| <= 8193; |k q| <= (8193 + 4 q) / 8 <= 1152, so the inverse column
// sums are <= 1152 * 23168 < 2^25 and |a| <= 26071; inverse row sums <= 26071 * 23168 < 2^30.
__device__ __forceinline__ void dg_block_round_trip(JpegLds& s, int* blk, int stride, const int* q, bool active)
{
    const int quarter = threadIdx.x >> 6, l = threadIdx.x & 63, r = l >> 3, k = l & 7;
    int* a = s.a[quarter];
    int* c = s.c[quarter];
    if (active) {                                                    // rows: a[y][u] = (sum_x T[u][x] p[y][x] + 512) >> 10
        int sum = 0;
#pragma unroll
        for (int x = 0; x < 8; ++x) sum += s.T[k * 8 + x] * (blk[r * stride + x] - 128);
        a[l] = (sum + 512) >> 10;
    }
    __syncthreads();
    if (active) {                                                    // columns: c8[v][u] = (sum_y T[v][y] a[y][u] + 4096) >> 13
        int sum = 0;
#pragma unroll
        for (int y = 0; y < 8; ++y) sum += s.T[r * 8 + y] * a[y * 8 + k];
        const int c8 = (sum + 4096) >> 13, qq = q[l];
        const int level = (abs(c8) + 4 * qq) / (8 * qq);             // quantise: round half away from zero of c8 / (8 q)
        c[l] = (c8 < 0 ? -level : level) * qq;                       // dequantise
    }
    __syncthreads();
    if (active) {                                                    // inverse columns: a[y][u] = (sum_v T[v][y] c[v][u] + 512) >> 10
        int sum = 0;
#pragma unroll
        for (int v = 0; v < 8; ++v) sum += s.T[v * 8 + r] * c[v * 8 + k];
        a[l] = (sum + 512) >> 10;
    }
    __syncthreads();
    if (active) {                                                    // inverse rows: (sum_u T[u][x] a[y][u] + 32768) >> 16, + 128
        int sum = 0;
#pragma unroll
        for (int u = 0; u < 8; ++u) sum += s.T[u * 8 + k] * a[r * 8 + u];
        blk[r * stride + k] = dg_clip255(((sum + 32768) >> 16) + 128);
    }
    __syncthreads();
}

__device__ __forceinline__ void dg_store_rgb(float* __restrict__ dst, int64_t o, int Y, int Cb, int Cr)
{
    const int cb = Cb - 128, cr = Cr - 128;                          // |116130 cb| < 2^24
    dst[o] = (float)dg_clip255(Y + ((91881 * cr + 32768) >> 16));
    dst[o + 1] = (float)dg_clip255(Y + ((-22553 * cb - 46802 * cr + 32768) >> 16));
    dst[o + 2] = (float)dg_clip255(Y + ((116130 * cb + 32768) >> 16));
}

// MODE 0: grey, 1: 4:4:4, 2: 4:2:0 (planes: Y[B][Hp][Wp], Cb and Cr [B][Hp/2][Wp/2] bytes; Hp, Wp = H, W rounded up to 16)
template <int MODE>
__global__ __launch_bounds__(DG_THREADS) void jpeg_blocks_kernel(const void* __restrict__ src, int src_is_u8, float* __restrict__ dst,
                                                                 uint8_t* __restrict__ planes, int H, int W,
                                                                 const int* __restrict__ quality)
{
    constexpr int C = MODE == 0 ? 1 : 3;
    __shared__ JpegLds s;
    const int t = threadIdx.x, b = blockIdx.z;
    const int qual = min(max(quality[b], 0), 100);
    // the thread's pixel; padding = edge replication = the clamped coordinate
    const int ly = t >> 4, lx = t & 15, y = blockIdx.y * JT + ly, x = blockIdx.x * JT + lx;
    const int64_t pix = ((int64_t)b * H + min(y, H - 1)) * W + min(x, W - 1);
    if (qual == 0) {                                                 // the image is not encoded: its codes (the whole workgroup leaves)
        if (y < H && x < W)
            for (int c = 0; c < C; ++c) dst[pix * C + c] = (float)dg_code(src, src_is_u8, pix * C + c);
        return;
    }
    if (t < 64) s.T[t] = DG_DCT[t];
    if (t < 128) {
        const int scale = qual < 50 ? 5000 / qual : 200 - 2 * qual;
        s.q[t >> 6][t & 63] = min(max(((int)DG_BASE_TABLES[t >> 6][t & 63] * scale + 50) / 100, 1), 255);
    }
    if (MODE == 0) {
        s.plane[0][t] = dg_code(src, src_is_u8, pix);
    } else {
        const int R = dg_code(src, src_is_u8, pix * 3), G = dg_code(src, src_is_u8, pix * 3 + 1), Bl = dg_code(src, src_is_u8, pix * 3 + 2);
        s.plane[0][t] = (19595 * R + 38470 * G + 7471 * Bl + 32768) >> 16;                 // all three sums < 2^24 + 2^23
        s.plane[1][t] = (-11058 * R - 21710 * G + 32768 * Bl + (128 << 16) + 32767) >> 16;
        s.plane[2][t] = (32768 * R - 27439 * G - 5329 * Bl + (128 << 16) + 32767) >> 16;
    }
    __syncthreads();
    if (MODE == 2) {                                                 // 2 x 2 means, written over the head of the planes
        int m = 0;
        const int pl = 1 + (t >> 6), cy = (t >> 3) & 7, cx = t & 7;
        if (t < 128) {
            const int* p = s.plane[pl] + (2 * cy) * JT + 2 * cx;
            m = (p[0] + p[1] + p[JT] + p[JT + 1] + 2) >> 2;
        }
        __syncthreads();
        if (t < 128) s.plane[pl][cy * 8 + cx] = m;
        __syncthreads();
    }
    const int quarter = t >> 6;
    dg_block_round_trip(s, s.plane[0] + (quarter >> 1) * 8 * JT + (quarter & 1) * 8, JT, s.q[0], true);
    if (MODE == 1) {
        dg_block_round_trip(s, s.plane[1] + (quarter >> 1) * 8 * JT + (quarter & 1) * 8, JT, s.q[1], true);
        dg_block_round_trip(s, s.plane[2] + (quarter >> 1) * 8 * JT + (quarter & 1) * 8, JT, s.q[1], true);
    }
    if (MODE == 2) dg_block_round_trip(s, s.plane[1 + (quarter & 1)], 8, s.q[1], quarter < 2);

    if (MODE == 2) {
        const int Hp = gridDim.y * JT, Wp = gridDim.x * JT;          // the tile lies inside the padded planes
        uint8_t* __restrict__ img = planes + (int64_t)b * Hp * Wp * 3 / 2;
        img[(int64_t)y * Wp + x] = (uint8_t)s.plane[0][t];
        if (t < 128) {
            const int pl = t >> 6, cy = (t >> 3) & 7, cx = t & 7;
            uint8_t* __restrict__ ch = img + (int64_t)Hp * Wp + (int64_t)pl * (Hp / 2) * (Wp / 2);
            ch[(int64_t)(blockIdx.y * 8 + cy) * (Wp / 2) + blockIdx.x * 8 + cx] = (uint8_t)s.plane[1 + pl][cy * 8 + cx];
        }
    } else if (y < H && x < W) {                                     // crop
        const int64_t o = (((int64_t)b * H + y) * W + x) * C;
        if (MODE == 0) dst[o] = (float)s.plane[0][t];
        else dg_store_rgb(dst, o, s.plane[0][t], s.plane[1][t], s.plane[2][t]);
    }
}

// 4:2:0: triangle filter on the padded half-size planes (edges replicated), colour conversion, crop.  One thread per pixel.
// v <= 4 * 255, the horizontal sum <= 16 * 255.
__global__ __launch_bounds__(DG_THREADS) void jpeg_finish_420_kernel(const uint8_t* __restrict__ planes, float* __restrict__ dst, int H,
                                                                     int W, int Hp, int Wp, const int* __restrict__ quality)
{
    const int x = blockIdx.x * DG_THREADS + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= W || quality[b] <= 0) return;                           // quality 0: jpeg_blocks_kernel wrote the codes
    const int hc = Hp / 2, wc = Wp / 2;
    const uint8_t* __restrict__ img = planes + (int64_t)b * Hp * Wp * 3 / 2;
    const int i = y >> 1, j = x >> 1;
    const int i2 = (y & 1) ? min(i + 1, hc - 1) : max(i - 1, 0), j2 = (x & 1) ? min(j + 1, wc - 1) : max(j - 1, 0);
    int up[2];
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
        const uint8_t* __restrict__ c = img + (int64_t)Hp * Wp + (int64_t)pl * hc * wc;
        const int v_here = 3 * c[(int64_t)i * wc + j] + c[(int64_t)i2 * wc + j];
        const int v_side = 3 * c[(int64_t)i * wc + j2] + c[(int64_t)i2 * wc + j2];
        up[pl] = (3 * v_here + v_side + ((x & 1) ? 7 : 8)) >> 4;
    }
    dg_store_rgb(dst, (((int64_t)b * H + y) * W + x) * 3, img[(int64_t)y * Wp + x], up[0], up[1]);
}

// ---- blur ---------------------------------------------------------------------------------------------------------------------
// A workgroup owns BT_H x BT_W pixels of one image.  The codes of the tile and its halo go to LDS once (bytes), the horizontal pass
// writes h8 (<= 255 * 256: 16 bits) for the tile's rows and the vertical halo to LDS, the vertical pass reads it.  A row is indexed
// by SAMPLE (x C + c), so the neighbour k taps away is k C samples away and both passes walk consecutive LDS and global addresses.
constexpr int BT_H = 16, BT_W = 64;

template <int C>
__global__ __launch_bounds__(DG_THREADS) void blur_kernel(const void* __restrict__ src, int src_is_u8, float* __restrict__ dst, int H, int W,
                                                          const int* __restrict__ taps, const int* __restrict__ radius)
{
    constexpr int ROWS = BT_H + 2 * DG_MAX_RADIUS, IN_W = (BT_W + 2 * DG_MAX_RADIUS) * C, OUT_W = BT_W * C;
    __shared__ uint8_t in[ROWS * IN_W];
    __shared__ uint16_t h8[ROWS * OUT_W];
    __shared__ int w[DG_TAPS];
    const int t = threadIdx.x, b = blockIdx.z;
    const int r = min(max(radius[b], 0), DG_MAX_RADIUS);
    if (t <= 2 * r) w[t] = taps[b * DG_TAPS + t];
    const int y0 = blockIdx.y * BT_H, x0 = blockIdx.x * BT_W;
    const int rows = BT_H + 2 * r, in_w = (BT_W + 2 * r) * C;        // what this image's radius needs of the buffers
    // a wave per row, a lane per sample of it in steps of 64: the loads of a row are independent and go out together
    for (int ry = t >> 6; ry < rows; ry += DG_THREADS / 64) {
        const int64_t row = ((int64_t)b * H + min(max(y0 + ry - r, 0), H - 1)) * W;           // borders clamp
#pragma unroll
        for (int j = 0; j < (IN_W + 63) / 64; ++j) {
            const int rs = (t & 63) + 64 * j, rx = rs / C, c = rs - rx * C;
            if (rs < in_w) in[ry * IN_W + rs] = (uint8_t)dg_code(src, src_is_u8, (row + min(max(x0 + rx - r, 0), W - 1)) * C + c);
        }
    }
    __syncthreads();
    // both passes: a thread owns four outputs next to each other along the taps and slides a window over their inputs, one LDS
    // read of a sample and one of a tap for four products
    constexpr int HG = BT_W / 4 * C;                                 // horizontal groups of a row: (4 pixels, channel)
    for (int u = t; u < rows * HG; u += DG_THREADS) {                // h = sum w p <= 255 * 65536 < 2^24
        const int ry = u / HG, rem = u - ry * HG, g = rem / C, c = rem - g * C;
        const uint8_t* p = in + ry * IN_W + g * 4 * C + c;           // pixels 4 g .. 4 g + 3 + 2 r <= BT_W - 1 + 2 r of the row
        int a0 = p[0], a1 = p[C], a2 = p[2 * C], h0 = 0, h1 = 0, h2 = 0, h3 = 0;
        for (int k = 0; k <= 2 * r; ++k) {
            const int a3 = p[(k + 3) * C], wk = w[k];
            h0 += wk * a0; h1 += wk * a1; h2 += wk * a2; h3 += wk * a3;
            a0 = a1; a1 = a2; a2 = a3;
        }
        uint16_t* o = h8 + ry * OUT_W + g * 4 * C + c;
        o[0] = (uint16_t)((h0 + 128) >> 8); o[C] = (uint16_t)((h1 + 128) >> 8);
        o[2 * C] = (uint16_t)((h2 + 128) >> 8); o[3 * C] = (uint16_t)((h3 + 128) >> 8);
    }
    __syncthreads();
    for (int u = t; u < BT_H / 4 * OUT_W; u += DG_THREADS) {         // v = sum w h8 <= 255 * 256 * 65536 < 2^32: unsigned
        const int g = u / OUT_W, s = u - g * OUT_W, x = x0 + s / C;
        const uint16_t* p = h8 + g * 4 * OUT_W + s;                  // rows 4 g .. 4 g + 3 + 2 r <= BT_H - 1 + 2 r
        unsigned a0 = p[0], a1 = p[OUT_W], a2 = p[2 * OUT_W], v[4] = {0u, 0u, 0u, 0u};
        for (int k = 0; k <= 2 * r; ++k) {
            const unsigned a3 = p[(k + 3) * OUT_W], wk = (unsigned)w[k];
            v[0] += wk * a0; v[1] += wk * a1; v[2] += wk * a2; v[3] += wk * a3;
            a0 = a1; a1 = a2; a2 = a3;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int y = y0 + g * 4 + i;
            if (y < H && x < W) dst[(((int64_t)b * H + y) * W + x0) * C + s] = (float)((v[i] + (1u << 23)) >> 24);      // <= 0xFF800000
        }
    }
}

// ---- clip, quantise, drop -------------------------------------------------------------------------------------------------------
// one thread per pixel: the draw is the pixel's, its C samples share it
template <int C>
__global__ __launch_bounds__(DG_THREADS) void pointwise_kernel(const void* __restrict__ src, int src_is_u8, float* __restrict__ dst,
                                                               uint8_t* __restrict__ mask, int64_t npix, const int* __restrict__ step,
                                                               const int* __restrict__ threshold, uint32_t k0, uint32_t k1)
{
    const int b = blockIdx.y;
    const int q = min(max(step[b], 1), 255), half = q >> 1;
    const uint32_t thr = (uint32_t)max(threshold[b], 0);
    for (int64_t i = (int64_t)blockIdx.x * DG_THREADS + threadIdx.x; i < npix; i += (int64_t)gridDim.x * DG_THREADS) {
        bool dropped = false;
        if (thr > 0u) {
            uint32_t r[4];
            philox4x32_10((uint32_t)i, (uint32_t)((uint64_t)i >> 32), (uint32_t)b, 4u, k0, k1, r);
            dropped = (r[0] >> 8) < thr;
        }
        const int64_t o = ((int64_t)b * npix + i) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int p = dg_code(src, src_is_u8, o + c);            // (p + q / 2) / q * q <= 255 + 127
            dst[o + c] = dropped ? 0.0f : (float)min(255, (p + half) / q * q);
        }
        if (mask) mask[(int64_t)b * npix + i] = dropped ? 1 : 0;
    }
}

int dg_check(const void* src, const void* dst, int B, int H, int W, int C)
{
    if (!src || !dst || src == dst || B <= 0 || H <= 0 || W <= 0 || C < 1 || C > 4) return BF_EINVAL;
    if (B > 65535) return BF_EUNSUPPORTED;                           // the image is grid.y or grid.z
    return BF_OK;
}

inline int64_t dg_round_up(int64_t v, int m) { return (v + m - 1) / m * m; }

}  // namespace

extern "C" int64_t bf_op_degrade_jpeg_scratch_bytes(int B, int H, int W, int C, int subsampling)
{
    if (B <= 0 || H <= 0 || W <= 0 || (C != 1 && C != 3) || (subsampling != 444 && subsampling != 420)) return BF_EINVAL;
    if (C == 1 || subsampling == 444) return 0;
    return (int64_t)B * dg_round_up(H, JT) * dg_round_up(W, JT) * 3 / 2;
}

extern "C" int bf_op_degrade_jpeg(const void* src, int src_is_u8, float* dst, int B, int H, int W, int C, const int32_t* quality,
                                  int subsampling, void* scratch, int64_t scratch_bytes, void* stream)
{
    const int rc = dg_check(src, dst, B, H, W, C);
    if (rc != BF_OK) return rc;
    if (!quality || (C != 1 && C != 3) || (subsampling != 444 && subsampling != 420)) return BF_EINVAL;
    const int64_t need = bf_op_degrade_jpeg_scratch_bytes(B, H, W, C, subsampling);
    if (need > 0 && (!scratch || scratch_bytes < need)) return BF_EWORKSPACE;
    const int64_t tiles_y = dg_round_up(H, JT) / JT, tiles_x = dg_round_up(W, JT) / JT;
    if (tiles_y > 65535 || (int64_t)W > 65535 * (int64_t)DG_THREADS) return BF_EUNSUPPORTED;
    const dim3 grid((unsigned)tiles_x, (unsigned)tiles_y, (unsigned)B);
    hipStream_t s = (hipStream_t)stream;
    if (C == 1) {
        hipLaunchKernelGGL(jpeg_blocks_kernel<0>, grid, dim3(DG_THREADS), 0, s, src, src_is_u8, dst, (uint8_t*)nullptr, H, W, quality);
    } else if (subsampling == 444) {
        hipLaunchKernelGGL(jpeg_blocks_kernel<1>, grid, dim3(DG_THREADS), 0, s, src, src_is_u8, dst, (uint8_t*)nullptr, H, W, quality);
    } else {
        if (H > 65535) return BF_EUNSUPPORTED;
        hipLaunchKernelGGL(jpeg_blocks_kernel<2>, grid, dim3(DG_THREADS), 0, s, src, src_is_u8, dst, (uint8_t*)scratch, H, W, quality);
        if (hipGetLastError() != hipSuccess) return BF_EHIP;
        const dim3 fgrid((unsigned)((W + DG_THREADS - 1) / DG_THREADS), (unsigned)H, (unsigned)B);
        hipLaunchKernelGGL(jpeg_finish_420_kernel, fgrid, dim3(DG_THREADS), 0, s, (const uint8_t*)scratch, dst, H, W, (int)tiles_y * JT,
                           (int)tiles_x * JT, quality);
    }
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}

extern "C" int bf_op_degrade_blur(const void* src, int src_is_u8, float* dst, int B, int H, int W, int C, const int32_t* taps,
                                  const int32_t* radius, void* stream)
{
    const int rc = dg_check(src, dst, B, H, W, C);
    if (rc != BF_OK) return rc;
    if (!taps || !radius) return BF_EINVAL;
    const int64_t tiles_y = dg_round_up(H, BT_H) / BT_H, tiles_x = dg_round_up(W, BT_W) / BT_W;
    if (tiles_y > 65535 || tiles_x > INT32_MAX) return BF_EUNSUPPORTED;
    const dim3 grid((unsigned)tiles_x, (unsigned)tiles_y, (unsigned)B);
    hipStream_t s = (hipStream_t)stream;
    switch (C) {
    case 1: hipLaunchKernelGGL(blur_kernel<1>, grid, dim3(DG_THREADS), 0, s, src, src_is_u8, dst, H, W, taps, radius); break;
    case 2: hipLaunchKernelGGL(blur_kernel<2>, grid, dim3(DG_THREADS), 0, s, src, src_is_u8, dst, H, W, taps, radius); break;
    case 3: hipLaunchKernelGGL(blur_kernel<3>, grid, dim3(DG_THREADS), 0, s, src, src_is_u8, dst, H, W, taps, radius); break;
    default: hipLaunchKernelGGL(blur_kernel<4>, grid, dim3(DG_THREADS), 0, s, src, src_is_u8, dst, H, W, taps, radius); break;
    }
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}

extern "C" int bf_op_degrade_pointwise(const void* src, int src_is_u8, float* dst, uint8_t* mask, int B, int H, int W, int C,
                                       const int32_t* step, const int32_t* threshold, uint64_t seed, void* stream)
{
    const int rc = dg_check(src, dst, B, H, W, C);
    if (rc != BF_OK) return rc;
    if (!step || !threshold || (const void*)mask == src || (void*)mask == (void*)dst) return BF_EINVAL;
    const int64_t npix = (int64_t)H * W, blocks = (npix + DG_THREADS - 1) / DG_THREADS;
    const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096), (unsigned)B);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    switch (C) {
    case 1: hipLaunchKernelGGL(pointwise_kernel<1>, grid, dim3(DG_THREADS), 0, s, src, src_is_u8, dst, mask, npix, step, threshold, k0, k1); break;
    case 2: hipLaunchKernelGGL(pointwise_kernel<2>, grid, dim3(DG_THREADS), 0, s, src, src_is_u8, dst, mask, npix, step, threshold, k0, k1); break;
    case 3: hipLaunchKernelGGL(pointwise_kernel<3>, grid, dim3(DG_THREADS), 0, s, src, src_is_u8, dst, mask, npix, step, threshold, k0, k1); break;
    default: hipLaunchKernelGGL(pointwise_kernel<4>, grid, dim3(DG_THREADS), 0, s, src, src_is_u8, dst, mask, npix, step, threshold, k0, k1); break;
    }
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}
