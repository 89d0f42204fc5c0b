// Inference weight packs of the split-f16 fused blocks (fused_h3.hip, fused_h3v.hip, fused_h3w.hip read them).
#include "bf_common.h"
#include "h3_weights.h"

// ------------------------------------------------------------------------------------------
// One workgroup per (layer, conv).  dst per block (BF_H3_BLOCK_FLOATS): [aux 64 floats][w1r][w2r] with, per convolution,
// thirteen A-operand register images [i][lane][8 x f16] in the row-streaming layout: twelve weight images (bf_h3_row_operand,
// h3_weights.h) and i = 12: sr * identity.
// The weights are pre-scaled by the power of two sr of max |w * fold| (the rule of h3_weights.h).
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
    if (threadIdx.x < 16) {
        float f = 1.f;
        if (which == 1) {
            if (ext_scale) f = ext_scale[threadIdx.x];
            else if (use_bn) f = params[p_blocks + layer * p_stride + 4608 + threadIdx.x] / sqrtf(state[layer * 32 + 16 + threadIdx.x] + eps);
        }
        s_fold[threadIdx.x] = f;
    }
    __syncthreads();
    float sr = bf_h3_block_weight_scale<256>([&](const int i) { return w[i] * s_fold[i & 15]; }, 2304, red);
    if (which == 1) sr = fminf(sr, 32768.f);         // conv2: sr itself is an f16 operand (sr * I carries the residual)
    _Float16* orow = reinterpret_cast<_Float16*>(dst + layer * d_stride + 64 + which * BF_H3R_WPACK_FLOATS);
    for (int idx = threadIdx.x; idx < 13 * 64 * 8; idx += 256) {
        int tap, part, cin, cout;
        bf_h3_row_operand(idx, tap, part, cin, cout);
        if (idx >> 9 == 12) {
            orow[idx] = (which == 1 && cin == cout) ? (_Float16)sr : (_Float16)0.f;
            continue;
        }
        _Float16 hi, lo;
        bf_h3_split(w[(tap * 16 + cin) * 16 + cout] * s_fold[cout] * sr, hi, lo);
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
