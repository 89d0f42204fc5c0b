// Spatially correlated noise around a denoiser that was trained on white noise: how far the correlation reaches
// (bf_noise_correlation), pixel-shuffle down-sampling and its inverse (bf_op_pd_split_u8, bf_op_pd_merge; Zhou et al., "When
// AWGN-based denoiser meets real noises", AAAI 2020) and the random-replacing refinement (bf_op_pd_replace_u8, bf_op_pd_mean; Lee
// et al., AP-BSN, CVPR 2022).  The host side is blind_image_denoising_amd/pixel_shuffle.py; the formulas, the choices and the
// measurements are DESIGN.md 7.15.  Scalars only: nothing is uploaded, allocated or synchronised.
//
// Correlation.  q_s(y,x) = |x(y,x) - x(y,x+s) - x(y+s,x) + x(y+s,x+s)| at every position with y + s < H and x + s < W, s = 1..S,
// per image and channel, counted into an exact 511-bin histogram (the padded 512-bin layout of grouped_median.h), and
// sigma_s = the grouped-data median / 2 / 0.6745.  A workgroup (256 threads) owns PS_BAND = 32 rows x PS_PX = 64 pixel columns
// of positions and stages the (32 + S) x (64 + S) pixels they reach into LDS once, indexed by BYTE of a row so that the lanes
// touch consecutive addresses; a wave owns 8 rows and a lane one pixel column, as in noise_estimate.hip.  It then walks s = 1..S
// with ONE set of C histograms in LDS (8 KiB with the 11 KiB tile: eight workgroups fit a CU's LDS; S x C sets at once are 64 KiB
// at S = 8, C = 4 and leave two): after each s the set is merged into the 64-bit global bins with one vector atomic per non-empty
// bin and cleared.  Every count is an integer: the histograms do not depend on the order of the atomics, and an image inside a
// batch gets the counts of that image alone.
//
// Split and merge are data movement, one read and one write per sample.  A workgroup owns one row of the side that is strided
// (a destination row of the split: member (b, i, j = all), row u; an output row of the merge) and a piece of PD_PIXELS frame
// pixels of it; the contiguous side is read (split) or written (merge) by BYTE / by FLOAT of the row, and the other side per
// phase j, again contiguous: the stride lives in LDS alone.
//
// Replace and mean index an image by its flat pixel group / element: consecutive lanes, consecutive addresses.
#include "bf_common.h"
#include "grouped_median.h"
#include "philox.h"

namespace {

constexpr int PS_MAXC = 4, PS_MAXS = 8, PS_MAXT = 16;
constexpr int PS_PX = 64, PS_BAND = 32, PS_SUB = PS_BAND / 4;
constexpr int PS_BINS_PAD = BF_MEDIAN_BINS_PAD;                  // q is an integer in 0..510: bin 511 is padding
constexpr int PS_ROW_BYTES = (PS_PX + PS_MAXS) * PS_MAXC;        // LDS row pitch of the staged tile
constexpr int PS_THREADS = 256;
constexpr unsigned PS_PHILOX_STREAM = 5u;                        // counter word 3; 0 and 1: augment.hip, 2: risk.hip, 3: camera noise and
                                                                 // neighbor.hip, 4: degrade.hip, 6: restore.hip

struct PsTiles {
    int x, y;
    PsTiles(int H, int W) : x((W + PS_PX - 1) / PS_PX), y((H + PS_BAND - 1) / PS_BAND) {}
    int64_t per_image() const { return (int64_t)x * y; }
};

// ghist[image][channel][s - 1][512] += the histogram of q_s over the tile's positions
__global__ __launch_bounds__(PS_THREADS) void noise_correlation_tile_kernel(const uint8_t* __restrict__ img, int H, int W, int C, int S,
                                                                            int tiles_x, int tiles_y, unsigned long long* __restrict__ ghist)
{
    __shared__ uint8_t tile[PS_BAND + PS_MAXS][PS_ROW_BYTES];
    __shared__ unsigned hist[PS_MAXC][PS_BINS_PAD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int t = blockIdx.x;
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y, b = t / tiles_y;
    const int y0 = ty * PS_BAND, x0 = tx * PS_PX;
    const int rows = min(PS_BAND + S, H - y0), cols = min(PS_PX + S, W - x0);       // both >= 1: y0 < H, x0 < W
    const int row_bytes = cols * C;                                                 // <= PS_ROW_BYTES
    const uint8_t* __restrict__ src = img + (((int64_t)b * H + y0) * W + x0) * C;
    for (int e = threadIdx.x; e < rows * row_bytes; e += PS_THREADS) {
        const int r = e / row_bytes, cb = e - r * row_bytes;                        // r < rows: y0 + r < H; x0 C + cb < W C
        tile[r][cb] = src[(int64_t)r * W * C + cb];
    }
    for (int i = threadIdx.x; i < PS_MAXC * PS_BINS_PAD; i += PS_THREADS) hist[i / PS_BINS_PAD][i % PS_BINS_PAD] = 0u;
    __syncthreads();

    for (int s = 1; s <= S; ++s) {
        // positions (ly, lane) of this wave's rows whose far corner (ly + s, lane + s) is inside the staged tile, i.e. the image
        if (lane + s < cols)
            for (int ly = wave * PS_SUB; ly < wave * PS_SUB + PS_SUB && ly + s < rows; ++ly)
                for (int c = 0; c < C; ++c) {
                    const int a = lane * C + c, d = a + s * C;
                    const int q = (int)tile[ly][a] - (int)tile[ly][d] - (int)tile[ly + s][a] + (int)tile[ly + s][d];
                    atomicAdd(&hist[c][q < 0 ? -q : q], 1u);                        // |q| <= 510
                }
        __syncthreads();
        for (int i = threadIdx.x; i < C * PS_BINS_PAD; i += PS_THREADS) {
            const int c = i / PS_BINS_PAD, k = i % PS_BINS_PAD;
            const unsigned v = hist[c][k];
            if (v != 0u) {                                                          // k <= 510: bin 511 is never counted
                atomicAdd(&ghist[(((int64_t)b * C + c) * S + (s - 1)) * PS_BINS_PAD + k], (unsigned long long)v);
                hist[c][k] = 0u;
            }
        }
        __syncthreads();
    }
}

// sigma[image][channel][s - 1]: one workgroup per (image, channel, s)
__global__ __launch_bounds__(PS_THREADS) void noise_correlation_finalize_kernel(const unsigned long long* __restrict__ ghist,
                                                                                double* __restrict__ sigma)
{
    __shared__ unsigned long long cum[PS_BINS_PAD];
    const unsigned long long* g = ghist + (int64_t)blockIdx.x * PS_BINS_PAD;
    const unsigned long long hk[2] = {g[threadIdx.x], g[threadIdx.x + 256]};
    bf_grouped_median_sigma(hk, cum, sigma + blockIdx.x);
}

bool ps_correlation_shape_ok(int B, int H, int W, int C, int S)
{
    if (B <= 0 || C < 1 || C > PS_MAXC || S < 1 || S > PS_MAXS || H < S + 1 || W < S + 1) return false;
    return (int64_t)W * C <= INT32_MAX / 2 && PsTiles(H, W).per_image() * B <= INT32_MAX && (int64_t)B * C * S <= INT32_MAX;
}

// ---- pixel-shuffle down-sampling ---------------------------------------------------------------------------------------------

constexpr int PD_PIXELS = 512;                                   // frame pixels of a row that a workgroup owns: PD_PIXELS / s sub-image columns

__host__ __device__ inline int pd_cols(int s) { return PD_PIXELS / s; }

__host__ __device__ inline int pd_ceil_div(int a, int b) { return (a + b - 1) / b; }

// dst[(b s^2 + i s + j), u, v, :] = src[b, y, x, :], y = u s + i (- s when that is >= H), x = v s + j (- s when >= W).
// blockIdx.x = (b s + i) Hs + u, blockIdx.y = piece of pd_cols(s) columns v.  The piece is staged from one column of sub-image
// pixels (s frame pixels) in front of it, where the repeated last column of a phase comes from.
template <int C>
__global__ __launch_bounds__(PS_THREADS) void pd_split_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int W,
                                                                 int s, int Hs, int Ws)
{
    __shared__ uint8_t seg[(PD_PIXELS + PS_MAXS) * C];         // (nv + 1) s <= PD_PIXELS + s pixels
    int t = blockIdx.x;
    const int u = t % Hs;
    t /= Hs;
    const int i = t % s;
    const int64_t b = t / s;
    int y = u * s + i;
    if (y >= H) y -= s;                                          // u == Hs - 1 >= 1 there (H >= 2 s): y - s >= 0, the same phase
    const int v0 = blockIdx.y * pd_cols(s), nv = min(pd_cols(s), Ws - v0);
    const int xa = max(v0 - 1, 0) * s, xb = min((v0 + nv) * s, W);                  // frame columns [xa, xb) staged
    const uint8_t* __restrict__ row = src + ((b * H + y) * W + xa) * C;
    for (int e = threadIdx.x; e < (xb - xa) * C; e += PS_THREADS) seg[e] = row[e];
    __syncthreads();
    for (int j = 0; j < s; ++j) {
        uint8_t* __restrict__ d = dst + ((((b * s + i) * s + j) * Hs + u) * (int64_t)Ws + v0) * C;
        for (int e = threadIdx.x; e < nv * C; e += PS_THREADS) {
            const int v = e / C, ch = e - v * C;
            int x = (v0 + v) * s + j;
            if (x >= W) x -= s;                                  // v0 + v == Ws - 1 >= 1 there: x - s >= (v0 + v - 1) s >= xa
            d[e] = seg[(x - xa) * C + ch];
        }
    }
}

__device__ __forceinline__ uint8_t pd_to_u8(float q) { return (uint8_t)rintf(fminf(fmaxf(q, 0.f), 255.f)); }       // half to even

// out[b, y, x, :] = src[(b s^2 + (y mod s) s + (x mod s)), y div s, x div s, :]; blockIdx.x = b H + y, blockIdx.y = piece
template <int C>
__global__ __launch_bounds__(PS_THREADS) void pd_merge_kernel(const float* __restrict__ src, void* __restrict__ out, int out_u8, int H, int W,
                                                              int s, int Hs, int Ws)
{
    __shared__ float seg[PD_PIXELS * C];                         // nv s <= PD_PIXELS pixels
    const int64_t row = blockIdx.x;                              // b H + y
    const int64_t b = row / H;
    const int y = (int)(row - b * H);
    const int i = y % s, u = y / s;
    const int v0 = blockIdx.y * pd_cols(s), nv = min(pd_cols(s), Ws - v0);
    const int xa = v0 * s, xb = min((v0 + nv) * s, W);
    for (int j = 0; j < s; ++j) {
        const float* __restrict__ f = src + ((((b * s + i) * s + j) * Hs + u) * (int64_t)Ws + v0) * C;
        for (int e = threadIdx.x; e < nv * C; e += PS_THREADS) {
            const int v = e / C, ch = e - v * C;
            seg[(v * s + j) * C + ch] = f[e];                    // (v s + j) < nv s <= PD_PIXELS; columns past W are staged and not written
        }
    }
    __syncthreads();
    const int64_t o = (row * W + xa) * C;
    for (int e = threadIdx.x; e < (xb - xa) * C; e += PS_THREADS) {
        if (out_u8) ((uint8_t*)out)[o + e] = pd_to_u8(seg[e]);
        else ((float*)out)[o + e] = seg[e];
    }
}

int pd_check(int B, int H, int W, int C, int s, int& Hs, int& Ws)
{
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || s < 1) return BF_EINVAL;
    if (s > 1 && (H < 2 * s || W < 2 * s)) return BF_EINVAL;
    if (C > PS_MAXC || s > PS_MAXS) return BF_EUNSUPPORTED;
    Hs = pd_ceil_div(H, s);
    Ws = pd_ceil_div(W, s);
    // grid.x = B s Hs (split) or B H (merge), grid.y = pieces of a row; one row of the frame in 32-bit byte arithmetic
    if ((int64_t)B * s * Hs > INT32_MAX || (int64_t)B * H > INT32_MAX || pd_ceil_div(Ws, pd_cols(s)) > 65535) return BF_EUNSUPPORTED;
    if ((int64_t)(W + s) * C > INT32_MAX / 4) return BF_EUNSUPPORTED;
    return BF_OK;
}

// ---- random-replacing refinement ---------------------------------------------------------------------------------------------

// dst[(b T + t), p, :] = word (p & 3) of philox(p >> 2, t) < threshold ? noisy[b, p, :] : base[b, p, :].  One thread per group of
// four pixels (4 C bytes: C dwords when `vec`); blockIdx.x = b groups_x + piece.
template <int C>
__global__ __launch_bounds__(PS_THREADS) void pd_replace_u8_kernel(const uint8_t* __restrict__ base, const uint8_t* __restrict__ noisy,
                                                                   uint8_t* __restrict__ dst, int64_t pixels, int groups_x, int T,
                                                                   unsigned threshold, uint64_t seed, int vec)
{
    const int64_t b = blockIdx.x / groups_x;
    const int64_t g = (int64_t)(blockIdx.x % groups_x) * PS_THREADS + threadIdx.x, p = 4 * g;
    if (p >= pixels) return;
    const int64_t n = pixels * C, e = p * C;                     // bytes of an image, first byte of the group
    const bool whole = vec && p + 4 <= pixels;
    unsigned bw[C], nw[C];                                       // the group's 4 C bytes of both sources, little-endian dwords
#pragma unroll
    for (int k = 0; k < C; ++k) {
        if (whole) {
            bw[k] = *reinterpret_cast<const unsigned*>(base + b * n + e + 4 * k);
            nw[k] = *reinterpret_cast<const unsigned*>(noisy + b * n + e + 4 * k);
        } else {
            bw[k] = nw[k] = 0u;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (e + 4 * k + i < n) {
                    bw[k] |= (unsigned)base[b * n + e + 4 * k + i] << (8 * i);
                    nw[k] |= (unsigned)noisy[b * n + e + 4 * k + i] << (8 * i);
                }
        }
    }
    for (int t = 0; t < T; ++t) {
        uint32_t r[4];
        philox4x32_10((uint32_t)g, (uint32_t)((uint64_t)g >> 32), (uint32_t)t, PS_PHILOX_STREAM, (uint32_t)seed, (uint32_t)(seed >> 32), r);
        unsigned take[C];                                        // byte mask of the bytes that come from `noisy`
#pragma unroll
        for (int k = 0; k < C; ++k) take[k] = 0u;
#pragma unroll
        for (int px = 0; px < 4; ++px)
            if (r[px] < threshold)
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int byte = px * C + c;                 // compile-time after unrolling
                    take[byte >> 2] |= 0xFFu << (8 * (byte & 3));
                }
        uint8_t* __restrict__ d = dst + (b * T + t) * n + e;     // e + i < n below: inside member t of image b
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const unsigned v = (nw[k] & take[k]) | (bw[k] & ~take[k]);
            if (whole) *reinterpret_cast<unsigned*>(d + 4 * k) = v;
            else
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (e + 4 * k + i < n) d[4 * k + i] = (uint8_t)(v >> (8 * i));
        }
    }
}

// out[b, e] = (sum over t ascending of (double) src[(b T + t), e]) / T; one thread per element, blockIdx.y = b
__global__ __launch_bounds__(PS_THREADS) void pd_mean_kernel(const float* __restrict__ src, void* __restrict__ out, int out_u8, int64_t n, int T)
{
    const int64_t b = blockIdx.y;
    const int64_t e = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x;
    if (e >= n) return;
    const float* __restrict__ f = src + b * T * n + e;
    double sum = 0.0;
    for (int t = 0; t < T; ++t) sum += (double)f[(int64_t)t * n];
    const float q = (float)__ddiv_rn(sum, (double)T);
    if (out_u8) ((uint8_t*)out)[b * n + e] = pd_to_u8(q);
    else ((float*)out)[b * n + e] = q;
}

// pixels of an image, or 0 for a shape or a member count the two entries refuse
int64_t pd_refine_pixels(int B, int H, int W, int C, int T)
{
    if (B <= 0 || H <= 0 || W <= 0 || C < 1 || C > PS_MAXC || T < 1 || T > PS_MAXT) return 0;
    const int64_t pixels = (int64_t)H * W;
    if (pixels * C > INT32_MAX - 4096 || B > 65535) return 0;
    const int64_t groups_x = ((pixels + 3) / 4 + PS_THREADS - 1) / PS_THREADS;
    if (groups_x * B > INT32_MAX) return 0;
    return pixels;
}

}  // namespace

extern "C" int64_t bf_noise_correlation_scratch_bytes(int B, int H, int W, int C, int max_stride)
{
    if (!ps_correlation_shape_ok(B, H, W, C, max_stride)) return BF_EINVAL;
    return (int64_t)B * C * max_stride * PS_BINS_PAD * (int64_t)sizeof(unsigned long long);
}

extern "C" int bf_noise_correlation(const uint8_t* img, int B, int H, int W, int C, int max_stride, void* scratch, int64_t scratch_bytes,
                                    double* out_sigma, void* stream)
{
    if (!img || !scratch || !out_sigma || !ps_correlation_shape_ok(B, H, W, C, max_stride)) return BF_EINVAL;
    const int64_t need = bf_noise_correlation_scratch_bytes(B, H, W, C, max_stride);
    if (scratch_bytes < need || ((uintptr_t)scratch | (uintptr_t)out_sigma) % 8) return BF_EINVAL;
    const PsTiles tiles(H, W);
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* ghist = (unsigned long long*)scratch;
    if (hipMemsetAsync(ghist, 0, (size_t)need, s) != hipSuccess) return BF_EHIP;
    hipLaunchKernelGGL(noise_correlation_tile_kernel, dim3((unsigned)(tiles.per_image() * B)), dim3(PS_THREADS), 0, s, img, H, W, C,
                       max_stride, tiles.x, tiles.y, ghist);
    hipLaunchKernelGGL(noise_correlation_finalize_kernel, dim3((unsigned)(B * C * max_stride)), dim3(PS_THREADS), 0, s, ghist, out_sigma);
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}

extern "C" int bf_op_pd_split_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, int C, int stride, void* stream)
{
    if (!src || !dst || src == dst) return BF_EINVAL;
    int Hs = 0, Ws = 0;
    const int rc = pd_check(B, H, W, C, stride, Hs, Ws);
    if (rc != BF_OK) return rc;
    const dim3 grid((unsigned)(B * stride * Hs), (unsigned)pd_ceil_div(Ws, pd_cols(stride)));
    hipStream_t s = (hipStream_t)stream;
    switch (C) {
    case 1: hipLaunchKernelGGL(pd_split_u8_kernel<1>, grid, dim3(PS_THREADS), 0, s, src, dst, H, W, stride, Hs, Ws); break;
    case 2: hipLaunchKernelGGL(pd_split_u8_kernel<2>, grid, dim3(PS_THREADS), 0, s, src, dst, H, W, stride, Hs, Ws); break;
    case 3: hipLaunchKernelGGL(pd_split_u8_kernel<3>, grid, dim3(PS_THREADS), 0, s, src, dst, H, W, stride, Hs, Ws); break;
    default: hipLaunchKernelGGL(pd_split_u8_kernel<4>, grid, dim3(PS_THREADS), 0, s, src, dst, H, W, stride, Hs, Ws); break;
    }
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}

extern "C" int bf_op_pd_merge(const float* src, void* out, int out_is_u8, int B, int H, int W, int C, int stride, void* stream)
{
    if (!src || !out || out == (const void*)src || (uintptr_t)src % 4 || (!out_is_u8 && (uintptr_t)out % 4)) return BF_EINVAL;
    int Hs = 0, Ws = 0;
    const int rc = pd_check(B, H, W, C, stride, Hs, Ws);
    if (rc != BF_OK) return rc;
    const dim3 grid((unsigned)(B * H), (unsigned)pd_ceil_div(Ws, pd_cols(stride)));
    hipStream_t s = (hipStream_t)stream;
    switch (C) {
    case 1: hipLaunchKernelGGL(pd_merge_kernel<1>, grid, dim3(PS_THREADS), 0, s, src, out, out_is_u8, H, W, stride, Hs, Ws); break;
    case 2: hipLaunchKernelGGL(pd_merge_kernel<2>, grid, dim3(PS_THREADS), 0, s, src, out, out_is_u8, H, W, stride, Hs, Ws); break;
    case 3: hipLaunchKernelGGL(pd_merge_kernel<3>, grid, dim3(PS_THREADS), 0, s, src, out, out_is_u8, H, W, stride, Hs, Ws); break;
    default: hipLaunchKernelGGL(pd_merge_kernel<4>, grid, dim3(PS_THREADS), 0, s, src, out, out_is_u8, H, W, stride, Hs, Ws); break;
    }
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}

extern "C" int bf_op_pd_replace_u8(const uint8_t* base, const uint8_t* noisy, uint8_t* dst, int B, int H, int W, int C, int copies,
                                   unsigned threshold, uint64_t seed, void* stream)
{
    const int64_t pixels = pd_refine_pixels(B, H, W, C, copies);
    if (!base || !noisy || !dst || dst == base || dst == noisy || pixels == 0) return BF_EINVAL;
    const int groups_x = (int)(((pixels + 3) / 4 + PS_THREADS - 1) / PS_THREADS);
    // dword accesses: every image and every group of every tensor starts on a multiple of four bytes
    const int vec = (pixels * C) % 4 == 0 && ((uintptr_t)base | (uintptr_t)noisy | (uintptr_t)dst) % 4 == 0;
    const dim3 grid((unsigned)(groups_x * B));
    hipStream_t s = (hipStream_t)stream;
    switch (C) {
    case 1: hipLaunchKernelGGL(pd_replace_u8_kernel<1>, grid, dim3(PS_THREADS), 0, s, base, noisy, dst, pixels, groups_x, copies, threshold, seed, vec); break;
    case 2: hipLaunchKernelGGL(pd_replace_u8_kernel<2>, grid, dim3(PS_THREADS), 0, s, base, noisy, dst, pixels, groups_x, copies, threshold, seed, vec); break;
    case 3: hipLaunchKernelGGL(pd_replace_u8_kernel<3>, grid, dim3(PS_THREADS), 0, s, base, noisy, dst, pixels, groups_x, copies, threshold, seed, vec); break;
    default: hipLaunchKernelGGL(pd_replace_u8_kernel<4>, grid, dim3(PS_THREADS), 0, s, base, noisy, dst, pixels, groups_x, copies, threshold, seed, vec); break;
    }
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}

extern "C" int bf_op_pd_mean(const float* src, void* out, int out_is_u8, int B, int H, int W, int C, int copies, void* stream)
{
    const int64_t pixels = pd_refine_pixels(B, H, W, C, copies);
    if (!src || !out || out == (const void*)src || pixels == 0 || (uintptr_t)src % 4 || (!out_is_u8 && (uintptr_t)out % 4)) return BF_EINVAL;
    const int64_t n = pixels * C;
    const dim3 grid((unsigned)((n + PS_THREADS - 1) / PS_THREADS), (unsigned)B);
    hipLaunchKernelGGL(pd_mean_kernel, grid, dim3(PS_THREADS), 0, (hipStream_t)stream, src, out, out_is_u8, n, copies);
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}
