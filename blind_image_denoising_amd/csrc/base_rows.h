// The base convolution's matrix-core formulation (header of base_rows.hip), shared by its two users: base_conv_rows_kernel
// (base_rows.hip, a kernel of its own) and the producer hook of fused_block2_h3w_kernel (fused_h3w.hip, the first pair launch of a
// forward computes its x0 rows itself).  Both must produce the SAME bits, so the weights, their scale, the A operands and the
// input records exist here and nowhere else.
#pragma once
#include "bf_common.h"
#include "h3_core.h"
#include "h3_weights.h"

// element (tap, c, m) of the 3x3 x [r, g, b, 1_inside] x 16 weight tensor: w / 255 for a colour, -0.5 sum_c w for the indicator
__device__ __forceinline__ float br_wval(const float* __restrict__ w, const int tap, const int c, const int m)
{
    if (c < 3) return w[(tap * 3 + c) * 16 + m] / 255.0f;
    return -0.5f * (w[(tap * 3 + 0) * 16 + m] + w[(tap * 3 + 1) * 16 + m] + w[(tap * 3 + 2) * 16 + m]);
}

// the weight scale of the largest entry (h3_weights.h); all threads of the workgroup call it; red: >= blockDim.x floats of LDS.
// Only the first 256 threads' partial maxima enter the tree -- they cover all 576 entries (a maximum has no order).
__device__ __forceinline__ float br_weight_scale(const float* __restrict__ w, float* red)
{
    return bf_h3_block_weight_scale<256>([&](const int i) { return br_wval(w, i / 64, (i >> 4) & 3, i & 15); }, 9 * 4 * 16, red);
}

// A operand of vertical tap dy for lane (n = lane & 15: output channel, q = lane >> 4): k-slot 8 (q & 1) + j of the half (q >> 1):
// slots 0..3 = tap dx 0, 4..7 = dx 1, 8..11 = dx 2, 12..15 = unused; half 0 = hi, 1 = lo of w * s
__device__ __forceinline__ h8 br_operand(const float* __restrict__ w, const float s, const int dy, const int lane)
{
    const int n = lane & 15, q = lane >> 4;
    h8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int slot = 8 * (q & 1) + j, dx = slot >> 2, c = slot & 3;
        float v = 0.f;
        if (dx < 3) v = br_wval(w, dy * 3 + dx, c, n) * s;
        _Float16 hi, lo;
        bf_h3_split(v, hi, lo);
        r[j] = (q >> 1) ? lo : hi;
    }
    return r;
}

// where a pixel of input row yy, column x stands: the [r, g, b, 1_inside] record is all zero outside the padded H x W frame, the
// indicator is 1 inside it, and the colours are read (three bytes at the returned address) only inside Hs x Ws
struct BrPixel {
    bool inside, colour;
};
__device__ __forceinline__ BrPixel br_pixel(const int yy, const int x, const int H, const int W, const int Hs, const int Ws)
{
    BrPixel p;
    p.inside = yy >= 0 && yy < H && x >= 0 && x < W;
    p.colour = p.inside && yy < Hs && x < Ws;
    return p;
}
__device__ __forceinline__ h4 br_record(const BrPixel p, const unsigned r, const unsigned g, const unsigned b)
{
    h4 v = {(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
    if (p.inside) v[3] = (_Float16)1.f;                // carries the -0.5 of the normalisation
    if (p.colour) {
        v[0] = (_Float16)(float)r;                     // a uint8 value is exact in f16
        v[1] = (_Float16)(float)g;
        v[2] = (_Float16)(float)b;
    }
    return v;
}
