// Non-local means (bf_op_nlm): every pixel becomes the mean of the pixels of its search window, weighted by how alike their
// patches are.  The host side is blind_image_denoising_amd/nlm.py; the definition is in include/bfcnn_hip.h, the choices and the
// measurements are DESIGN.md 7.18.  Integer arithmetic up to the one fp64 division; the weight comes from a table, no
// exponential is evaluated.  Scalars only: nothing is uploaded, allocated or synchronised.
//
// A workgroup owns a 32 x 32 tile of one image and a thread four adjacent pixels of one of its rows.  The tile and a halo of
// search + patch pixels go to LDS once, one dword per pixel (the channels in its bytes, zero above C), coordinates clamped:
// that is the edge replication.  With D = S(x) + S(q) - 2 X(x, q), S the patch sum of a pixel's own energy and X the patch sum
// of the products, S is a map made once per tile (in LDS, tile + search halo) and X costs one v_dot4_u32_u8 per pixel pair:
// the channel sum of a pair is one instruction, and its accumulator operand carries the sum down the patch's rows.  A thread
// keeps the (2 p + 1) x (4 + 2 p) dwords around its four pixels in registers for the whole launch; per candidate offset it
// reads the same block at the offset, forms 4 + 2 p column sums and slides the patch width over them: (2 p + 1)(4 + 2 p) / 4
// products per pixel and candidate instead of (2 p + 1)^2.  Rows of the LDS images are 61 and 53 dwords apart (= 1 mod 4): the
// 32 lanes of an LDS cycle -- eight column groups of four rows -- then read 32 different banks.
// Whether a candidate counts is decided by its coordinates; the staged values outside the frame are only ever patch borders.
#include "bf_common.h"

namespace {

constexpr int NL_TILE = 32, NL_COLS = 4, NL_THREADS = 256;
constexpr int NL_MAXP = 3, NL_MAXR = 10, NL_TABLE = 1024;
constexpr int NL_IMG_ROWS = NL_TILE + 2 * (NL_MAXR + NL_MAXP);       // 58
constexpr int NL_IMG_PITCH = 61;
constexpr int NL_S_ROWS = NL_TILE + 2 * NL_MAXR;                     // 52
constexpr int NL_S_PITCH = 53;
constexpr unsigned NL_MULT_OFF = 0xFFFFFFFFu;                        // the clamp of nlm_params: the filter is off
constexpr unsigned NL_MAX_D = 1u << 24;                             // D <= 255^2 * 4 * 49 < 2^24

__device__ __forceinline__ int nl_clamp(int v, int last) { return min(max(v, 0), last); }

// blockIdx.x = (b gy + i) gx + j; thread (ty, tx) = pixels (32 i + ty, 32 j + 4 tx .. + 3).  Three waves per SIMD is the register
// budget: at patch 3 the allocator otherwise stops at 128 VGPRs for a fourth wave that 29 KB of LDS per workgroup leave little room
// for, and the launch is slower for it
template <int P>
__global__ __launch_bounds__(NL_THREADS) __attribute__((amdgpu_waves_per_eu(3, 3))) void nlm_kernel(const uint8_t* __restrict__ images, const long long* __restrict__ params,
                                                         const int* __restrict__ table, int H, int W, int C, int R, int gy, int gx,
                                                         void* __restrict__ out, int out_u8, int* __restrict__ weights)
{
    constexpr int ROWS = 2 * P + 1, COLS = NL_COLS + 2 * P;
    __shared__ unsigned img[NL_IMG_ROWS * NL_IMG_PITCH];
    __shared__ unsigned energy[NL_S_ROWS * NL_S_PITCH];
    __shared__ int tab[NL_TABLE];
    int g = blockIdx.x;
    const int j0 = g % gx;
    g /= gx;
    const int i0 = g % gy;
    const int64_t b = g / gy;
    const int y0 = i0 * NL_TILE, x0 = j0 * NL_TILE;
    const int tx = threadIdx.x & 7, ty = threadIdx.x >> 3;
    const int y = y0 + ty, x = x0 + NL_COLS * tx;
    const uint8_t* __restrict__ im = images + b * H * W * C;
    // (offset, mult) clamped to [0, 2^24] and [0, 2^32 - 1], from their 32-bit halves: everything below is 32-bit arithmetic
    const int* __restrict__ prm = reinterpret_cast<const int*>(params + 2 * b);
    const unsigned off_lo = (unsigned)prm[0], mult_lo = (unsigned)prm[2];
    const int off_hi = prm[1], mult_hi = prm[3];
    const unsigned offset = off_hi < 0 ? 0u : (off_hi > 0 ? NL_MAX_D : min(off_lo, NL_MAX_D));
    const unsigned mult = mult_hi < 0 ? 0u : (mult_hi > 0 ? NL_MULT_OFF : mult_lo);
    const int64_t pix = (b * H + y) * W + x;                         // of the thread's first pixel

    if (mult == NL_MULT_OFF) {                                       // the whole workgroup: every weight is 0, w_c = 1
        if (y >= H) return;
        for (int k = 0; k < NL_COLS && x + k < W; ++k) {
            for (int c = 0; c < C; ++c) {
                const uint8_t v = im[((int64_t)y * W + x + k) * C + c];
                if (out_u8) ((uint8_t*)out)[(pix + k) * C + c] = v;
                else ((float*)out)[(pix + k) * C + c] = (float)v;
            }
            if (weights) weights[pix + k] = 1;
        }
        return;
    }

    const int halo = R + P, side = NL_TILE + 2 * halo;               // <= NL_IMG_ROWS
    for (int e = threadIdx.x; e < NL_TABLE; e += NL_THREADS) tab[e] = table[e];
    for (int e = threadIdx.x; e < side * side; e += NL_THREADS) {
        const int ly = e / side, lx = e - ly * side;
        const int qy = nl_clamp(y0 - halo + ly, H - 1), qx = nl_clamp(x0 - halo + lx, W - 1);
        const uint8_t* __restrict__ s = im + ((int64_t)qy * W + qx) * C;
        unsigned v = 0u;
        for (int c = 0; c < C; ++c) v |= (unsigned)s[c] << (8 * c);
        img[ly * NL_IMG_PITCH + lx] = v;
    }
    __syncthreads();
    const int sside = NL_TILE + 2 * R;                               // energy[ly][lx] = S of the staged pixel (ly + P, lx + P)
    for (int e = threadIdx.x; e < sside * sside; e += NL_THREADS) {
        const int ly = e / sside, lx = e - ly * sside;
        unsigned sum = 0u;
#pragma unroll
        for (int u = 0; u < ROWS; ++u)
#pragma unroll
            for (int v = 0; v < ROWS; ++v) {
                const unsigned q = img[(ly + u) * NL_IMG_PITCH + lx + v];
                sum = __builtin_amdgcn_udot4(q, q, sum, false);
            }
        energy[ly * NL_S_PITCH + lx] = sum;
    }
    __syncthreads();
    if (y >= H || x >= W) return;                                    // no barrier below

    // the top left corner of the patches of the thread's pixels: staged (ty + halo - P, 4 tx + halo - P)
    const unsigned* __restrict__ base = img + (ty + R) * NL_IMG_PITCH + NL_COLS * tx + R;
    const unsigned* __restrict__ sbase = energy + (ty + R) * NL_S_PITCH + NL_COLS * tx + R;
    unsigned refp[ROWS][COLS];
#pragma unroll
    for (int u = 0; u < ROWS; ++u)
#pragma unroll
        for (int k = 0; k < COLS; ++k) refp[u][k] = base[u * NL_IMG_PITCH + k];
    unsigned sx[NL_COLS], num[NL_COLS][4], den[NL_COLS], wmax[NL_COLS];
#pragma unroll
    for (int k = 0; k < NL_COLS; ++k) {
        sx[k] = sbase[k];
        den[k] = wmax[k] = 0u;
#pragma unroll
        for (int c = 0; c < 4; ++c) num[k][c] = 0u;
    }

    for (int dy = -R; dy <= R; ++dy) {
        if ((unsigned)(y + dy) >= (unsigned)H) continue;
        for (int dx = -R; dx <= R; ++dx) {
            if (dy == 0 && dx == 0) continue;
            const unsigned* __restrict__ cand = base + dy * NL_IMG_PITCH + dx;
            unsigned col[COLS], centre[NL_COLS];
#pragma unroll
            for (int k = 0; k < COLS; ++k) col[k] = 0u;
#pragma unroll
            for (int u = 0; u < ROWS; ++u)
#pragma unroll
                for (int k = 0; k < COLS; ++k) {
                    const unsigned q = cand[u * NL_IMG_PITCH + k];
                    col[k] = __builtin_amdgcn_udot4(refp[u][k], q, col[k], false);
                    if (u == P && k >= P && k < P + NL_COLS) centre[k - P] = q;
                }
            const unsigned* __restrict__ sq = sbase + dy * NL_S_PITCH + dx;
            unsigned X = 0u, idx[NL_COLS], w[NL_COLS];
#pragma unroll
            for (int k = 0; k < ROWS; ++k) X += col[k];
#pragma unroll
            for (int k = 0; k < NL_COLS; ++k) {
                if (k) X += col[k + 2 * P] - col[k - 1];
                const unsigned D = sx[k] + sq[k] - 2u * X;            // >= 0: a sum of squares
                const unsigned a = D > offset ? D - offset : 0u;
                idx[k] = min(__umulhi(a, mult), (unsigned)(NL_TABLE - 1));
            }
            // the four gathers go out together, whatever the frame says: a candidate outside it has an index like any other
#pragma unroll
            for (int k = 0; k < NL_COLS; ++k) w[k] = (unsigned)tab[idx[k]];
#pragma unroll
            for (int k = 0; k < NL_COLS; ++k) {
                w[k] = (unsigned)(x + k + dx) < (unsigned)W ? w[k] : 0u;
                wmax[k] = max(wmax[k], w[k]);
                den[k] += w[k];
#pragma unroll
                for (int c = 0; c < 4; ++c) num[k][c] += __umul24(w[k], (centre[k] >> (8 * c)) & 0xFFu);      // 13 x 8 bits
            }
        }
    }

#pragma unroll
    for (int k = 0; k < NL_COLS; ++k) {
        if (x + k >= W) break;
        const unsigned wc = max(wmax[k], 1u), own = refp[P][P + k], d = den[k] + wc;     // < 2^31 (bfcnn_hip.h)
        for (int c = 0; c < C; ++c) {
            const unsigned n = num[k][c] + wc * ((own >> (8 * c)) & 0xFFu);
            if (out_u8) ((uint8_t*)out)[(pix + k) * C + c] = (uint8_t)((2u * n + d) / (2u * d));
            else ((float*)out)[(pix + k) * C + c] = (float)__ddiv_rn((double)n, (double)d);
        }
        if (weights) weights[pix + k] = (int)d;
    }
}

}  // namespace

extern "C" int bf_op_nlm(const uint8_t* images, const int64_t* params, const int32_t* table, int B, int H, int W, int C, int patch,
                         int search, void* out, int cast_to_uint8, int32_t* weights_or_null, void* stream)
{
    if (!images || !params || !table || !out || B <= 0 || H <= 0 || W <= 0 || C < 1 || C > 4) return BF_EINVAL;
    if (patch < 1 || patch > NL_MAXP || search < 1 || search > NL_MAXR) return BF_EINVAL;
    if ((int64_t)B * H * W * C > INT32_MAX) return BF_EINVAL;
    if (out == (const void*)images || (uintptr_t)params % 8 || (uintptr_t)table % 4 || (uintptr_t)weights_or_null % 4 ||
        (!cast_to_uint8 && (uintptr_t)out % 4))
        return BF_EINVAL;
    const int gy = (H + NL_TILE - 1) / NL_TILE, gx = (W + NL_TILE - 1) / NL_TILE;
    const dim3 grid((unsigned)((int64_t)B * gy * gx));               // <= B H W
    const long long* prm = (const long long*)params;
    hipStream_t s = (hipStream_t)stream;
    switch (patch) {
    case 1: hipLaunchKernelGGL(nlm_kernel<1>, grid, dim3(NL_THREADS), 0, s, images, prm, table, H, W, C, search, gy, gx, out, cast_to_uint8, weights_or_null); break;
    case 2: hipLaunchKernelGGL(nlm_kernel<2>, grid, dim3(NL_THREADS), 0, s, images, prm, table, H, W, C, search, gy, gx, out, cast_to_uint8, weights_or_null); break;
    default: hipLaunchKernelGGL(nlm_kernel<3>, grid, dim3(NL_THREADS), 0, s, images, prm, table, H, W, C, search, gy, gx, out, cast_to_uint8, weights_or_null); break;
    }
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}
