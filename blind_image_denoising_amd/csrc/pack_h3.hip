// Inference weight packs of the split-f16 fused blocks (fused_h3.hip, fused_h3v.hip, fused_h3w.hip read them).
#include "bf_common.h"

// ------------------------------------------------------------------------------------------
// One workgroup per (layer, conv).  dst per block (BF_H3_BLOCK_FLOATS): [aux 64 floats][w1r][w2r] with, per convolution,
// thirteen A-operand register images [i][lane][8 x f16] in the row-streaming layout:
//   i = dy*4 + {0: pair (dy,0)|(dy,1) hi, 1: pair lo, 2: single (dy,2) [hi | hi], 3: single [lo | 0]}, i = 12: sr * identity;
//   lane l: output channel l & 15, k-slots 8*(l >> 4) .. +7 (k-slot < 16: first tap of the pair, >= 16: second tap; input
//   channel = k-slot & 15).
// The weights are pre-scaled by a power of two sr (max |w * fold| * sr in [2^13, 2^14)) so that w_lo stays a normal f16 number.
// conv2 (which == 1): the folded BN scale is multiplied INTO the weights (per output channel) and the kernels add the
// residual as (sr * I) x [x_hi | x_lo] on the matrix pipe, so sr must itself be an f16 number: sr <= 2^15.
// aux[0..15] = 1/s1, aux[32..47] = folded BN shift, aux[48..63] = 1/s2 (aux[16..31] is not used).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pack_h3_kernel(const float* __restrict__ params, const float* __restrict__ state,
                                                      int64_t p_blocks, int64_t p_stride, float* __restrict__ dst,
                                                      int64_t d_stride, int use_bn, float eps,
                                                      const float* __restrict__ ext_scale, const float* __restrict__ ext_shift)
{
    __shared__ float red[256];
    const int layer = blockIdx.x >> 1, which = blockIdx.x & 1;
    const float* w = params + p_blocks + layer * p_stride + which * 2304;      // HWIO [3][3][16][16]
    __shared__ float s_fold[16];
    __shared__ float s_scale_r;
    if (threadIdx.x < 16) {
        float f = 1.f;
        if (which == 1) {
            if (ext_scale) f = ext_scale[threadIdx.x];
            else if (use_bn) f = params[p_blocks + layer * p_stride + 4608 + threadIdx.x] / sqrtf(state[layer * 32 + 16 + threadIdx.x] + eps);
        }
        s_fold[threadIdx.x] = f;
    }
    __syncthreads();
    float m = 0.f;
    for (int i = threadIdx.x; i < 2304; i += 256) m = fmaxf(m, fabsf(w[i] * s_fold[i & 15]));
    red[threadIdx.x] = m;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + st]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float sr = 1.f;
        const float mx = red[0];
        if (mx > 0.f && mx < 3.0e38f) {
            int ex;
            (void)frexpf(mx, &ex);                   // mx = f * 2^ex, f in [0.5, 1)
            ex = max(-100, min(100, ex));
            sr = ldexpf(1.f, 14 - ex);               // mx * sr in [2^13, 2^14)
        }
        if (which == 1) sr = fminf(sr, 32768.f);
        s_scale_r = sr;
    }
    __syncthreads();
    const float sr = s_scale_r;
    _Float16* orow = reinterpret_cast<_Float16*>(dst + layer * d_stride + 64 + which * BF_H3R_WPACK_FLOATS);
    for (int idx = threadIdx.x; idx < 13 * 64 * 8; idx += 256) {
        const int i = idx >> 9, l = (idx >> 3) & 63, j = idx & 7;
        const int cout = l & 15, kslot = 8 * (l >> 4) + j, half = kslot >> 4, cin = kslot & 15;
        if (i == 12) {
            orow[idx] = (which == 1 && cin == cout) ? (_Float16)sr : (_Float16)0.f;
            continue;
        }
        const int dy = i >> 2, kind = i & 3;
        int tap, part;
        if (kind == 0) { tap = dy * 3 + half; part = 0; }
        else if (kind == 1) { tap = dy * 3 + half; part = 1; }
        else if (kind == 2) { tap = dy * 3 + 2; part = 0; }                 // [w_hi | w_hi] x [x_hi | x_lo]
        else { tap = dy * 3 + 2; part = half ? 2 : 1; }                       // [w_lo | 0]    x [x_hi | x_lo]
        const float ws = w[(tap * 16 + cin) * 16 + cout] * s_fold[cout] * sr;
        const _Float16 hi = (_Float16)ws;
        const _Float16 lo = (_Float16)(ws - (float)hi);
        orow[idx] = part == 0 ? hi : (part == 1 ? lo : (_Float16)0.f);
    }
    float* aux = dst + layer * d_stride;
    if (threadIdx.x < 16) {
        const int c = threadIdx.x;
        if (which == 0) {
            aux[c] = 1.0f / sr;                       // conv1 folds nothing
        } else {
            float sc = 1.f, sh = 0.f;
            if (ext_scale) {                          // debug entry: caller's scale (folded above) / shift
                sh = ext_shift[c];
            } else if (use_bn) {     // keras BatchNormalization(training=False): gamma*(x-mean)*rsqrt(var+eps)
                const float g = params[p_blocks + layer * p_stride + 4608 + c];
                const float mean = state[layer * 32 + c], var = state[layer * 32 + 16 + c];
                sc = g / sqrtf(var + eps);
                sh = -sc * mean;
            }
            aux[32 + c] = sh;
            aux[48 + c] = 1.0f / sr;                  // scale folded into the weights
        }
    }
}

hipError_t bf_launch_pack_h3(const float* params, const float* state, int64_t p_blocks, int64_t p_stride, float* dst,
                             int64_t d_stride, int layers, int use_bn, float eps, const float* ext_scale,
                             const float* ext_shift, hipStream_t s)
{
    if (layers <= 0) return hipSuccess;
    hipLaunchKernelGGL(pack_h3_kernel, dim3(layers * 2), dim3(256), 0, s, params, state, p_blocks, p_stride, dst, d_stride,
                       use_bn, eps, ext_scale, ext_shift);
    return hipGetLastError();
}
