// Noise level statistics of one uint8 NHWC batch in one pass: the MAD estimator of noise_estimate.hip conditioned on the local
// intensity, for noise whose variance grows with the signal (var(y | x) = a x + b, shot noise plus read noise).  Per complete 2x2
// cell (the last odd row and column are dropped, as in noise_estimate.hip) and channel
//   q = |x00 - x01 - x10 + x11|  in 0..510      (twice the modulus of the orthonormal Haar HH coefficient)
//   s =  x00 + x01 + x10 + x11   in 0..1020     (twice the Haar LL coefficient)
// A cell with a sample equal to 0 or 255 is excluded and only counted.  Every other cell belongs to level l = s >> 6: NL_LEVELS =
// 16 levels, each 16 grey levels of cell mean wide.  LL and HH are orthogonal coefficients of the same four samples, so for
// independent noise conditioning on s does not bias q.  Per image, channel and level: the exact 511-bin histogram of q, the cell
// count n, the exact sum of s, and sigma_l = grouped median / 2 / 0.6745 (grouped_median.h, the rule of noise_estimate.hip); per
// image and channel the number of excluded cells.  The host side is blind_image_denoising_amd/noise_level.py; DESIGN.md 7.10.
//
// Layout.  As noise_estimate.hip a workgroup (4 waves) owns a tile of NL_BAND = 32 rows x NL_PX = 64 pixel columns and a wave
// NL_SUB = 8 of those rows, which start on an even row: a cell never crosses waves.  A wave's 8 x 64 pixels are 4 x 32 cells; lane
// (lane & 31, lane >> 5) owns cell column lane & 31 of the cell rows lane >> 5 and (lane >> 5) + 2, every channel of them.  The
// samples are read once, packed four to a register.  The histograms of ONE channel (16 levels x 512 bins x 4 B = 32 KB) live in
// LDS; the workgroup walks the channels over that one array: atomicAdd on unsigned, then one 64-bit vector atomic per non-empty
// bin into the global bins.  The s sums go through 32 LDS columns per level (one per cell column, so the lanes of a flat image do
// not meet on one address) and land in the padding bin 511 of the level's global histogram.
//
// Exactness.  Every quantity is an integer, added in 32 bits inside a workgroup (at most 512 cells: s sums below 2^20) and in 64
// bits across workgroups: the outputs do not depend on the order of the atomics.  Two calls return the same bits, and an image
// inside a batch the bits of that image alone.
#include "bf_common.h"
#include "block_reduce.h"
#include "grouped_median.h"

namespace {

constexpr int NL_MAXC = 4;
constexpr int NL_PX = 64;                 // pixel columns of a tile
constexpr int NL_BAND = 32;               // rows of a tile (a workgroup)
constexpr int NL_SUB = NL_BAND / 4;       // rows of a wave; even, so that a 2x2 cell stays inside one wave
constexpr int NL_LEVELS = 16;             // l = s >> 6
constexpr int NL_BINS = 511;              // q is an integer in 0..510
constexpr int NL_BINS_PAD = BF_MEDIAN_BINS_PAD;
constexpr int NL_SUM_BIN = NL_BINS;       // the padding bin of a level's global histogram holds its sum of s
constexpr int NL_PLANE = NL_LEVELS * NL_BINS_PAD;

struct NlTiles {
    int x, y;
    NlTiles(int H, int W) : x((W + NL_PX - 1) / NL_PX), y((H + NL_BAND - 1) / NL_BAND) {}
    int64_t per_image() const { return (int64_t)x * y; }
};

// ghist[image][channel][level][512] += the tile's histograms (bin 511: the sum of s); gexcl[image][channel] += its excluded cells
__global__ __launch_bounds__(256) void noise_level_tile_kernel(const uint8_t* __restrict__ img, int H, int W, int C, int tiles_x,
                                                               int tiles_y, unsigned long long* __restrict__ ghist,
                                                               unsigned long long* __restrict__ gexcl)
{
    __shared__ unsigned hist[NL_PLANE];
    __shared__ unsigned ssum[NL_LEVELS][32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int t = blockIdx.x;
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y, b = t / tiles_y;
    const int col = lane & 31;
    const int p = tx * NL_PX + 2 * col;                           // the cell's left pixel column
    const int y0 = ty * NL_BAND + wave * NL_SUB;                  // even
    const uint8_t* base = img + (int64_t)b * H * W * C;

    // the two cells of this lane: x[k][c] = x00 | x01 << 8 | x10 << 16 | x11 << 24
    unsigned x[2][NL_MAXC];
    bool valid[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int r = y0 + 2 * ((lane >> 5) + 2 * k);
        valid[k] = p + 1 < W && r + 1 < H;                        // the cell is complete: every index below is inside the image
        const uint8_t* top = base + ((int64_t)r * W + p) * C;
        const uint8_t* bot = top + (int64_t)W * C;
#pragma unroll
        for (int c = 0; c < NL_MAXC; ++c) {
            x[k][c] = 0u;
            if (valid[k] && c < C) x[k][c] = (unsigned)top[c] | (unsigned)top[C + c] << 8 | (unsigned)bot[c] << 16 | (unsigned)bot[C + c] << 24;
        }
    }

    unsigned excluded[NL_MAXC];
#pragma unroll
    for (int c = 0; c < NL_MAXC; ++c) {
        excluded[c] = 0u;
        if (c < C) {                                              // C is uniform: every thread meets the same barriers
            for (int i = tid; i < NL_PLANE; i += 256) hist[i] = 0u;
            for (int i = tid; i < NL_LEVELS * 32; i += 256) ssum[i >> 5][i & 31] = 0u;
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (valid[k]) {
                    const int x00 = x[k][c] & 255u, x01 = x[k][c] >> 8 & 255u, x10 = x[k][c] >> 16 & 255u, x11 = x[k][c] >> 24;
                    const bool sat = x00 == 0 || x00 == 255 || x01 == 0 || x01 == 255 || x10 == 0 || x10 == 255 || x11 == 0 || x11 == 255;
                    if (sat) ++excluded[c];
                    else {
                        const int d = x00 - x01 - x10 + x11, q = d < 0 ? -d : d, s = x00 + x01 + x10 + x11;      // s in 4..1016
                        atomicAdd(&hist[(s >> 6) * NL_BINS_PAD + q], 1u);
                        atomicAdd(&ssum[s >> 6][col], (unsigned)s);
                    }
                }
            __syncthreads();
            unsigned long long* g = ghist + ((int64_t)b * C + c) * NL_PLANE;
            for (int i = tid; i < NL_PLANE; i += 256) {
                const unsigned v = hist[i];
                if (v != 0u && (i & (NL_BINS_PAD - 1)) < NL_BINS) atomicAdd(&g[i], (unsigned long long)v);
            }
            if (tid < NL_LEVELS) {
                unsigned v = 0u;
                for (int i = 0; i < 32; ++i) v += ssum[tid][i];
                if (v != 0u) atomicAdd(&g[tid * NL_BINS_PAD + NL_SUM_BIN], (unsigned long long)v);
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int c = 0; c < NL_MAXC; ++c)
        if (c < C) {
            const unsigned w = bf_wave_sum(excluded[c]);          // all 64 lanes are here
            if (lane == 0 && w != 0u) atomicAdd(&gexcl[(int64_t)b * C + c], (unsigned long long)w);
        }
}

// levels[image][channel][level] = {n, sum of s, sigma_l}, excluded[image][channel]; one workgroup per (image, channel, level)
__global__ __launch_bounds__(256) void noise_level_finalize_kernel(const unsigned long long* __restrict__ ghist,
                                                                   const unsigned long long* __restrict__ gexcl,
                                                                   double* __restrict__ levels, double* __restrict__ excluded)
{
    __shared__ unsigned long long cum[NL_BINS_PAD];
    const int tid = threadIdx.x;
    const unsigned long long* g = ghist + (int64_t)blockIdx.x * NL_BINS_PAD;
    const unsigned long long hk[2] = {g[tid], tid + 256 < NL_BINS ? g[tid + 256] : 0ull};
    double* o = levels + (int64_t)blockIdx.x * 3;
    const unsigned long long n = bf_grouped_median_sigma(hk, cum, o + 2);
    if (tid == 0) {
        o[0] = (double)n;
        o[1] = (double)g[NL_SUM_BIN];
        if (blockIdx.x % NL_LEVELS == 0) excluded[blockIdx.x / NL_LEVELS] = (double)gexcl[blockIdx.x / NL_LEVELS];
    }
}

bool nl_shape_ok(int B, int H, int W, int C)
{
    if (B <= 0 || C < 1 || C > NL_MAXC || H < 3 || W < 3) return false;
    return (int64_t)W * C <= INT32_MAX - NL_PX * NL_MAXC && NlTiles(H, W).per_image() * B <= INT32_MAX &&
           (int64_t)B * C * NL_LEVELS <= INT32_MAX;
}

int64_t nl_hist_bytes(int B, int C) { return (int64_t)B * C * NL_PLANE * (int64_t)sizeof(unsigned long long); }

}  // namespace

extern "C" int64_t bf_noise_level_scratch_bytes(int B, int H, int W, int C)
{
    if (!nl_shape_ok(B, H, W, C)) return BF_EINVAL;
    return nl_hist_bytes(B, C) + (int64_t)B * C * (int64_t)sizeof(unsigned long long);
}

extern "C" int bf_noise_level(const uint8_t* img, int B, int H, int W, int C, void* scratch, int64_t scratch_bytes, double* out_levels,
                              double* out_excluded, void* stream)
{
    if (!img || !out_levels || !out_excluded || !scratch || !nl_shape_ok(B, H, W, C)) return BF_EINVAL;
    const int64_t need = bf_noise_level_scratch_bytes(B, H, W, C);
    if (scratch_bytes < need || ((uintptr_t)scratch | (uintptr_t)out_levels | (uintptr_t)out_excluded) % 8) return BF_EINVAL;
    const NlTiles tiles(H, W);
    unsigned long long* ghist = (unsigned long long*)scratch;
    unsigned long long* gexcl = (unsigned long long*)((char*)scratch + nl_hist_bytes(B, C));
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(scratch, 0, (size_t)need, s) != hipSuccess) return BF_EHIP;
    hipLaunchKernelGGL(noise_level_tile_kernel, dim3((unsigned)(tiles.per_image() * B)), dim3(256), 0, s, img, H, W, C, tiles.x, tiles.y,
                       ghist, gexcl);
    hipLaunchKernelGGL(noise_level_finalize_kernel, dim3((unsigned)(B * C * NL_LEVELS)), dim3(256), 0, s, ghist, gexcl, out_levels,
                       out_excluded);
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}
