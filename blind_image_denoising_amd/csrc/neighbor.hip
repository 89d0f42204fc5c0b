// Neighbor2Neighbor pairs (Huang et al., CVPR 2021): training a denoiser on noisy images alone.  From one noisy image y the sampler
// draws two half-resolution sub-images g1(y), g2(y) -- in every 2x2 cell two adjacent pixels at random -- and the network is trained
// to map g1(y) to g2(y); the paper's regulariser  gamma |f(g1(y)) - g2(y) - (g1(f(y)) - g2(f(y)))|^2  (f(y) under stop-gradient) folds,
// for a squared loss, into the target:  target = g2(y) + lambda (g1(f(y)) - g2(f(y))),  lambda = gamma / (1 + gamma).
//   bf_op_neighbor_pairs: one read of y (uint8 or float32) and optionally of f = f(y), both half-resolution float32 tensors written once.
// The host side is blind_image_denoising_amd/neighbor.py; the target identity and the measurements are DESIGN.md 7.9.
//
// Draw.  Cell (i, j) of image b (i < H/2, j < W2 = W/2) belongs to Philox group g = i ceil(W2 / 4) + (j >> 2) -- four consecutive
// cells of one row; a group never straddles a row -- and takes k = r[j & 3] >> 29 of
// philox4x32_10(counter = (lo32 g, hi32 g, b, 3), key = (lo32 seed, hi32 seed)).  The positions of a cell are 0 = (0,0), 1 = (0,1),
// 2 = (1,0), 3 = (1,1) (row, column); the ordered pair (p1, p2) = T[k], T = [(0,1),(0,2),(1,3),(2,3),(1,0),(2,0),(3,1),(3,2)]: the
// eight ordered 4-adjacent pairs.  All channels of a cell share k.
//
// Layout.  A thread owns one group: 8 C consecutive elements of two input rows, 4 C consecutive elements of each output row, so the
// lanes of a wave touch consecutive addresses.  With W2 a multiple of 4 and aligned bases the group's rows are loaded whole (16-byte
// loads; 8-byte loads for uint8 with an odd C, whose groups start on 8 bytes) and the pair is picked from registers by selects;
// every other shape -- and the tail group of a row -- reads the two chosen pixels of a cell directly.  Both paths form the same
// values from the same elements.  No LDS, no atomics; the grid depends on the shape alone.
#include <cmath>
#include "bf_common.h"
#include "philox.h"

namespace {

constexpr int NB_THREADS = 256, NB_MAXC = 4;
// T[k] as two bits per k: p1 = 0,0,1,2,1,2,3,3   p2 = 1,2,3,3,0,0,1,2
constexpr unsigned NB_P1 = 0u | 0u << 2 | 1u << 4 | 2u << 6 | 1u << 8 | 2u << 10 | 3u << 12 | 3u << 14;
constexpr unsigned NB_P2 = 1u | 2u << 2 | 3u << 4 | 3u << 6 | 0u << 8 | 0u << 10 | 1u << 12 | 2u << 14;

// one of the four positions of a cell, by selects (a dynamic index into a register array would go through scratch)
__device__ __forceinline__ float nb_pick(unsigned p, float v00, float v01, float v10, float v11)
{
    const float top = (p & 1u) ? v01 : v00, bottom = (p & 1u) ? v11 : v10;
    return (p & 2u) ? bottom : top;
}

// the 8 C elements of a group's row as floats: WORDS 32-bit words, loaded 16 bytes (or 8) at a time
template <bool U8, int C> struct NbRow {
    static constexpr int WORDS = U8 ? 2 * C : 8 * C;
    uint32_t w[WORDS];
    __device__ __forceinline__ void load(const void* __restrict__ p)
    {
        if constexpr (WORDS % 4 == 0) {
#pragma unroll
            for (int q = 0; q < WORDS / 4; ++q) {
                const uint4 v = reinterpret_cast<const uint4*>(p)[q];
                w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int q = 0; q < WORDS / 2; ++q) {
                const uint2 v = reinterpret_cast<const uint2*>(p)[q];
                w[2 * q] = v.x; w[2 * q + 1] = v.y;
            }
        }
    }
    __device__ __forceinline__ float at(int e) const         // e: a compile-time constant after unrolling
    {
        if constexpr (U8) return (float)(w[e >> 2] >> (8 * (e & 3)) & 255u);
        else return __uint_as_float(w[e]);
    }
};

template <bool U8> __device__ __forceinline__ float nb_read(const void* __restrict__ p, int64_t e)
{
    if constexpr (U8) return (float)static_cast<const uint8_t*>(p)[e];
    else return static_cast<const float*>(p)[e];
}

// input[b][i][j][c] = y[p1], target = y[p2] (+ lambda (f[p1] - f[p2])).  One thread per group of four cells of a row.
template <bool U8, int C>
__global__ __launch_bounds__(NB_THREADS) void neighbor_pairs_kernel(const void* __restrict__ y, const float* __restrict__ f, float lambda,
                                                                    float* __restrict__ input, float* __restrict__ target, int H2, int W2,
                                                                    int groups_row, int blocks_image, uint64_t seed, int vec)
{
    const int b = blockIdx.x / blocks_image;
    const int64_t g = (int64_t)(blockIdx.x % blocks_image) * NB_THREADS + threadIdx.x;
    if (g >= (int64_t)H2 * groups_row) return;
    const int i = (int)(g / groups_row), j0 = (int)(g % groups_row) * 4;
    uint32_t r[4];
    philox4x32_10((uint32_t)g, (uint32_t)((uint64_t)g >> 32), (uint32_t)b, 3u, (uint32_t)seed, (uint32_t)(seed >> 32), r);

    const int64_t pitch = (int64_t)2 * W2 * C;                                        // elements of an input row
    const int64_t row0 = ((int64_t)b * 2 * H2 + 2 * i) * pitch + (int64_t)2 * j0 * C;    // the group's first element, upper row
    const int64_t out0 = (((int64_t)b * H2 + i) * W2 + j0) * C;

    if (vec) {                                   // W2 % 4 == 0: the group is whole, its rows start on 16 (8) bytes
        float in[4 * C], tg[4 * C];
        {
            NbRow<U8, C> a, c;
            constexpr int64_t ESZ = U8 ? 1 : 4;
            a.load(static_cast<const char*>(y) + row0 * ESZ);
            c.load(static_cast<const char*>(y) + (row0 + pitch) * ESZ);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const unsigned k = r[t] >> 29, p1 = NB_P1 >> (2 * k) & 3u, p2 = NB_P2 >> (2 * k) & 3u;
#pragma unroll
                for (int ch = 0; ch < C; ++ch) {
                    const float v00 = a.at(2 * t * C + ch), v01 = a.at((2 * t + 1) * C + ch);
                    const float v10 = c.at(2 * t * C + ch), v11 = c.at((2 * t + 1) * C + ch);
                    in[t * C + ch] = nb_pick(p1, v00, v01, v10, v11);
                    tg[t * C + ch] = nb_pick(p2, v00, v01, v10, v11);
                }
            }
        }
        if (f) {
            NbRow<false, C> a, c;
            a.load(f + row0);
            c.load(f + row0 + pitch);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const unsigned k = r[t] >> 29, p1 = NB_P1 >> (2 * k) & 3u, p2 = NB_P2 >> (2 * k) & 3u;
#pragma unroll
                for (int ch = 0; ch < C; ++ch) {
                    const float v00 = a.at(2 * t * C + ch), v01 = a.at((2 * t + 1) * C + ch);
                    const float v10 = c.at(2 * t * C + ch), v11 = c.at((2 * t + 1) * C + ch);
                    const float d = nb_pick(p1, v00, v01, v10, v11) - nb_pick(p2, v00, v01, v10, v11);
                    tg[t * C + ch] = fmaf(lambda, d, tg[t * C + ch]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < C; ++q) {
            reinterpret_cast<float4*>(input + out0)[q] = make_float4(in[4 * q], in[4 * q + 1], in[4 * q + 2], in[4 * q + 3]);
            reinterpret_cast<float4*>(target + out0)[q] = make_float4(tg[4 * q], tg[4 * q + 1], tg[4 * q + 2], tg[4 * q + 3]);
        }
        return;
    }

#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (j0 + t >= W2) break;                 // the tail group of a row
        const unsigned k = r[t] >> 29, p1 = NB_P1 >> (2 * k) & 3u, p2 = NB_P2 >> (2 * k) & 3u;
        // both positions lie inside cell (i, j0 + t): rows 2 i, 2 i + 1 < H and columns 2 (j0 + t), 2 (j0 + t) + 1 < W
        const int64_t e1 = row0 + (p1 >> 1) * pitch + (int64_t)(2 * t + (p1 & 1u)) * C;
        const int64_t e2 = row0 + (p2 >> 1) * pitch + (int64_t)(2 * t + (p2 & 1u)) * C;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            float tg = nb_read<U8>(y, e2 + ch);
            if (f) tg = fmaf(lambda, f[e1 + ch] - f[e2 + ch], tg);
            input[out0 + t * C + ch] = nb_read<U8>(y, e1 + ch);
            target[out0 + t * C + ch] = tg;
        }
    }
}

bool nb_overlap(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}

template <bool U8>
void nb_launch(int C, dim3 grid, hipStream_t s, const void* y, const float* f, float lambda, float* input, float* target, int H2, int W2,
               int groups_row, int blocks_image, uint64_t seed, int vec)
{
#define NB_LAUNCH(CH)                                                                                                              \
    hipLaunchKernelGGL((neighbor_pairs_kernel<U8, CH>), grid, dim3(NB_THREADS), 0, s, y, f, lambda, input, target, H2, W2, groups_row, \
                       blocks_image, seed, vec)
    switch (C) {
    case 1: NB_LAUNCH(1); break;
    case 2: NB_LAUNCH(2); break;
    case 3: NB_LAUNCH(3); break;
    default: NB_LAUNCH(4); break;
    }
#undef NB_LAUNCH
}

}  // namespace

extern "C" int bf_op_neighbor_pairs(const void* y, int y_is_u8, const float* f, float lambda, float* input, float* target, int B, int H,
                                    int W, int C, uint64_t seed, void* stream)
{
    if (!y || !input || !target || B <= 0 || H < 2 || W < 2 || (H & 1) || (W & 1) || C < 1 || C > NB_MAXC) return BF_EINVAL;
    if (!std::isfinite(lambda) || lambda < 0.f || lambda >= 1.f) return BF_EINVAL;
    const int H2 = H / 2, W2 = W / 2, groups_row = (W2 + 3) / 4;
    const int64_t n = (int64_t)B * H * W * C;                            // elements of y (and f)
    const int64_t blocks_image = ((int64_t)H2 * groups_row + NB_THREADS - 1) / NB_THREADS;
    if (n > ((int64_t)1 << 40) || blocks_image * B > INT32_MAX) return BF_EINVAL;
    const int64_t y_bytes = n * (y_is_u8 ? 1 : 4), f_bytes = n * 4, out_bytes = n;     // n / 4 floats
    if ((uintptr_t)input % 4 || (uintptr_t)target % 4 || (uintptr_t)f % 4 || (!y_is_u8 && (uintptr_t)y % 4)) return BF_EINVAL;
    if (nb_overlap(input, out_bytes, target, out_bytes) || nb_overlap(input, out_bytes, y, y_bytes) ||
        nb_overlap(target, out_bytes, y, y_bytes))
        return BF_EINVAL;
    if (f && (nb_overlap(input, out_bytes, f, f_bytes) || nb_overlap(target, out_bytes, f, f_bytes))) return BF_EINVAL;
    // whole groups from aligned rows: a group's row starts 8 C elements after its neighbour's, a row W C = 8 C (W2 / 4) after the last
    const uintptr_t y_align = !y_is_u8 || C % 2 == 0 ? 16 : 8;
    const int vec = W2 % 4 == 0 && (uintptr_t)y % y_align == 0 && (uintptr_t)f % 16 == 0 && ((uintptr_t)input | (uintptr_t)target) % 16 == 0;
    const dim3 grid((unsigned)(blocks_image * B));
    if (y_is_u8) nb_launch<true>(C, grid, (hipStream_t)stream, y, f, lambda, input, target, H2, W2, groups_row, (int)blocks_image, seed, vec);
    else nb_launch<false>(C, grid, (hipStream_t)stream, y, f, lambda, input, target, H2, W2, groups_row, (int)blocks_image, seed, vec);
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}
