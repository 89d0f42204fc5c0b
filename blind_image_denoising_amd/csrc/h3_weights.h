// Weight preparation shared by every split-f16 ("f16x3") operator: the power-of-two scale, the hi / lo split and
// the decode of the row-streaming A-operand image.  A weight v is carried as hi = f16(v s), lo = f16(v s - hi); the scale s keeps
// lo a NORMAL f16 number, so every split-f16 result of the project depends on the rule below.  It exists here and nowhere else.
#pragma once
#include "block_reduce.h"
#include <math.h>

// The rule: the power of two s that puts max_abs * s in [2^13, 2^14), with the exponent of max_abs clamped to +-100;
// s = 1 for a zero, negative or non-finite maximum.  Host and device evaluate the same expression (bf_debug_h3_weight_scale).
__host__ __device__ inline float bf_h3_weight_scale(const float max_abs)
{
    if (!(max_abs > 0.f) || !isfinite(max_abs)) return 1.f;
    int ex;
    (void)frexpf(max_abs, &ex);                              // max_abs = f 2^ex, f in [0.5, 1)
    ex = ex < -100 ? -100 : (ex > 100 ? 100 : ex);
    return ldexpf(1.f, 14 - ex);
}

// The rule applied to max |value_of_i(i)| over i < n, by a workgroup of NT threads; every thread gets s.  red = NT floats of LDS,
// free again on return.
template <int NT, typename F>
__device__ __forceinline__ float bf_h3_block_weight_scale(F&& value_of_i, const int n, float* red)
{
    float m = 0.f;
    for (int i = threadIdx.x; i < n; i += NT) m = fmaxf(m, fabsf(value_of_i(i)));
    return bf_h3_weight_scale(bf_block_reduce<NT, BfMax>(red, (int)threadIdx.x, m));
}

// v ~ hi + lo (22 mantissa bits).  The eight-wide forms are h3_split (h3_core.h) and uh_split8 (unet_h3_core.h).
__device__ __forceinline__ void bf_h3_split(const float v, _Float16& hi, _Float16& lo)
{
    hi = (_Float16)v;
    lo = (_Float16)(v - (float)hi);
}

// Element idx of the row-streaming A-operand images [i][lane][8 x f16] of a 3x3, 16 -> 16 convolution (fused_h3*.hip and the
// training kernels read them): which weight it holds.
//   i = dy * 4 + {0: pair (dy,0)|(dy,1) hi, 1: pair lo, 2: single (dy,2) [hi | hi], 3: single [lo | 0]};
//   lane l: output channel l & 15, k-slots 8 (l >> 4) .. + 7 (k-slot < 16: first tap of the pair, >= 16: second tap; input
//   channel = k-slot & 15).
// tap = 3 dy + dx; part = 0: the hi half, 1: the lo half, 2: zero.  For the 13th image (i = 12, not a weight image) only cin and
// cout mean something.
__device__ __forceinline__ void bf_h3_row_operand(const int idx, int& tap, int& part, int& cin, int& cout)
{
    const int i = idx >> 9, l = (idx >> 3) & 63, j = idx & 7;
    const int kslot = 8 * (l >> 4) + j, half = kslot >> 4;
    cout = l & 15;
    cin = kslot & 15;
    const int dy = i >> 2, kind = i & 3;
    if (kind == 0) { tap = dy * 3 + half; part = 0; }
    else if (kind == 1) { tap = dy * 3 + half; part = 1; }
    else if (kind == 2) { tap = dy * 3 + 2; part = 0; }                  // [w_hi | w_hi] x [x_hi | x_lo]
    else { tap = dy * 3 + 2; part = half ? 2 : 1; }                        // [w_lo | 0]    x [x_hi | x_lo]
}
