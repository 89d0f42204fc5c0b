// Variance stabilisation around a Gaussian denoiser: the generalised Anscombe transform of a uint8 image whose
// noise variance grows with the signal, var(y | x) = gain x + offset, and its inverse (algebraic, or the exact unbiased inverse
// of Makitalo & Foi, IEEE TIP 2013, in closed form).  Per image b and channel c, with a = gain[b][c], o = offset[b][c] read from
// DEVICE memory (what bf_noise_level's fit leaves there) and sanitised where they are used:
//   a = a finite and > 0 ? min(a, 64) : 0        o = o finite ? clamp(o, 1/12, 65025) : 1/12        c = 3/8 a^2 + o, rc = sqrt(c)
//   forward   u(y) = 2 y / (sqrt(a y + c) + rc), s = 255 / u(255), v = rint(s u(y))          (0 -> 0, 255 -> 255, identity for a = 0)
//   inverse   u = clamp(w, 0, 255) / s, x = rc u + a u^2 / 4 [+ a / 4 + a (K1 d - K2 d^2 + K3 d^3), d = a / (a u + 2 rc)]
// The forward map is a table of 256 C bytes per image, built in fp64 in LDS by every workgroup that serves a span of that image;
// the inverse takes its per-plane constants from fp64 and works in float32.  Both are pure streams over the flat elements of an
// image, e = (h W + w) C + c, channel = e mod C: an image gets the same bits alone or inside a batch.  No atomics.
#include "bf_common.h"
#include <type_traits>

#define VST_THREADS 256
#define VST_FWD_ITERS 16         // dwords per thread of the forward kernel: 16 KiB of an image per workgroup and table
#define VST_INV_ITERS 4          // groups of four floats per thread of the inverse kernel: 16 KiB in per workgroup

struct VstPlane { double a, c, rc; };

__device__ __forceinline__ VstPlane vst_plane(const double gain, const double offset)
{
#pragma clang fp contract(off)
    VstPlane p;
    p.a = (isfinite(gain) && gain > 0.0) ? fmin(gain, 64.0) : 0.0;
    const double o = isfinite(offset) ? fmin(fmax(offset, 1.0 / 12.0), 65025.0) : 1.0 / 12.0;
    p.c = 0.375 * (p.a * p.a) + o;
    p.rc = sqrt(p.c);
    return p;
}

// the generalised Anscombe transform minus its value at 0, in the form that stays finite as a -> 0; no contraction, so that
// an fp64 restatement that rounds every operation gets the same bits
__device__ __forceinline__ double vst_u(const VstPlane& p, const double y)
{
#pragma clang fp contract(off)
    return (2.0 * y) / (sqrt(p.a * y + p.c) + p.rc);
}

// Elements of an image are served in groups of four: group g holds elements 4 g - head .. 4 g - head + 3, head = the image
// base's distance from the group alignment of BOTH pointers (0 when they disagree: then no group is moved as a whole).
// A group that lies inside the image and whose pointers agree is one vector access; the others go element by element.
__global__ __launch_bounds__(VST_THREADS) void vst_forward_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                     int64_t n, int C, const double* __restrict__ gain,
                                                                     const double* __restrict__ offset)
{
    __shared__ uint8_t table[4 * 256];
    __shared__ VstPlane planes[4];
    __shared__ double scale[4];
    const int b = blockIdx.y;
    if ((int)threadIdx.x < C) {                                             // the plane's constants once, not once per entry
#pragma clang fp contract(off)
        const VstPlane p = vst_plane(gain[b * C + threadIdx.x], offset[b * C + threadIdx.x]);
        planes[threadIdx.x] = p;
        scale[threadIdx.x] = 255.0 / vst_u(p, 255.0);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 256 * C; i += VST_THREADS) {
#pragma clang fp contract(off)
        const int c = i >> 8;
        table[i] = (uint8_t)fmin(fmax(rint(scale[c] * vst_u(planes[c], (double)(i & 255))), 0.0), 255.0);
    }
    __syncthreads();
    const uint8_t* __restrict__ s = src + (int64_t)b * n;
    uint8_t* __restrict__ d = dst + (int64_t)b * n;
    const int head_s = (int)((uintptr_t)s & 3), head_d = (int)((uintptr_t)d & 3);
    const bool agree = head_s == head_d;
    const int head = agree ? head_s : 0;
    const int64_t g0 = (int64_t)blockIdx.x * (VST_THREADS * VST_FWD_ITERS) + threadIdx.x;
    const int64_t first = 4 * (g0 - threadIdx.x) - head;                    // the workgroup's span: [first, first + 4 groups)
    if (agree && first >= 0 && first + 4 * VST_THREADS * VST_FWD_ITERS <= n) {
        // every group of the span is whole: all loads first (a thread keeps VST_FWD_ITERS dwords in flight), then the table
        unsigned x4[VST_FWD_ITERS];
#pragma unroll
        for (int it = 0; it < VST_FWD_ITERS; ++it)
            x4[it] = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(s + 4 * (g0 + it * VST_THREADS) - head));
        const int step = 4 * VST_THREADS % C;                               // channel of a thread's next group
        int c0 = (int)((4 * g0 - head + 4 * C) % C);
#pragma unroll
        for (int it = 0; it < VST_FWD_ITERS; ++it) {
            unsigned y4 = 0u;
            int c = c0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                y4 |= (unsigned)table[c * 256 + (x4[it] >> (8 * i) & 255u)] << (8 * i);
                c = c + 1 == C ? 0 : c + 1;
            }
            *reinterpret_cast<unsigned*>(d + 4 * (g0 + it * VST_THREADS) - head) = y4;
            c0 = c0 + step >= C ? c0 + step - C : c0 + step;
        }
        return;
    }
    for (int it = 0; it < VST_FWD_ITERS; ++it) {                            // the first and the last span of an image, and spans whose pointers disagree
        const int64_t e0 = 4 * (g0 + (int64_t)it * VST_THREADS) - head;
        if (e0 >= n) break;
        const bool whole = agree && e0 >= 0 && e0 + 4 <= n;
        unsigned x4 = 0u, y4 = 0u;
        if (whole) x4 = *reinterpret_cast<const unsigned*>(s + e0);
        else
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (e0 + i >= 0 && e0 + i < n) x4 |= (unsigned)s[e0 + i] << (8 * i);
        int c = (int)((e0 + 4 * C) % C);                                    // e0 >= -3
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            y4 |= (unsigned)table[c * 256 + (x4 >> (8 * i) & 255u)] << (8 * i);
            c = c + 1 == C ? 0 : c + 1;
        }
        if (whole) *reinterpret_cast<unsigned*>(d + e0) = y4;
        else
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (e0 + i >= 0 && e0 + i < n) d[e0 + i] = (uint8_t)(y4 >> (8 * i));
    }
}

static bool vst_shape_ok(int B, int H, int W, int C, int64_t* n, int64_t* groups)
{
    if (B <= 0 || H <= 0 || W <= 0 || C < 1 || C > 4 || B > 65535) return false;         // the image is the grid's y
    *n = (int64_t)H * W * C;
    *groups = (*n + 3) / 4 + 1;                                                         // + 1: a head splits one group in two
    return *n <= INT32_MAX - 4096;
}

extern "C" int bf_op_vst_forward_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, int C, const double* gain,
                                    const double* offset, void* stream)
{
    int64_t n, groups;
    if (!src || !dst || !gain || !offset || ((uintptr_t)gain | (uintptr_t)offset) % 8 != 0) return BF_EINVAL;
    if (!vst_shape_ok(B, H, W, C, &n, &groups)) return BF_EINVAL;
    const int64_t per_wg = VST_THREADS * VST_FWD_ITERS;
    hipLaunchKernelGGL(vst_forward_u8_kernel, dim3((unsigned)((groups + per_wg - 1) / per_wg), (unsigned)B), dim3(VST_THREADS), 0,
                       (hipStream_t)stream, src, dst, n, C, gain, offset);
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}

// ---- inverse: float32 in the stabilised domain -> float32 or uint8 grey levels ----
// per plane, folded in fp64 and rounded once: x = u (rc + a4 u) [+ a4 + d (k1 + d (d k3 - k2)), d = a rcp(a u + rc2)]
struct VstInverse { float inv_s, rc, a4, a, rc2, k1, k2, k3; };

template <bool EXACT>
__device__ __forceinline__ float vst_inverse_one(const VstInverse& k, float w)
{
    w = fminf(fmaxf(w, 0.0f), 255.0f);                                      // NaN -> 0
    const float u = w * k.inv_s;
    float x = u * (k.rc + k.a4 * u);
    if (EXACT) {
        // 1 / D, D the Anscombe value.  The divisor lies in [2 rc, 2 rc + a u(255)], within [0.57, 1e3]: v_rcp_f32 is good to 1 ulp
        // there, 1e-7 of a term of at most a K1 d < 16.  A correctly rounded division and unfolded constants: 40.6 us against 36.8
        // on 25 M samples
        const float d = k.a * __builtin_amdgcn_rcpf(k.a * u + k.rc2);
        x += k.a4 + d * (k.k1 + d * (d * k.k3 - k.k2));
    }
    return fminf(fmaxf(x, 0.0f), 255.0f);
}

template <bool EXACT, bool U8>
__global__ __launch_bounds__(VST_THREADS) void vst_inverse_kernel(const float* __restrict__ src, void* __restrict__ dst_, int64_t n,
                                                                  int C, const double* __restrict__ gain,
                                                                  const double* __restrict__ offset)
{
    __shared__ VstInverse planes[4];
    const int b = blockIdx.y;
    if ((int)threadIdx.x < C) {
#pragma clang fp contract(off)
        const VstPlane p = vst_plane(gain[b * C + threadIdx.x], offset[b * C + threadIdx.x]);
        planes[threadIdx.x] = {(float)(vst_u(p, 255.0) / 255.0), (float)p.rc, (float)(0.25 * p.a), (float)p.a, (float)(2.0 * p.rc),
                               (float)(p.a * 0.30618621784789724), (float)(p.a * 1.375), (float)(p.a * 0.76546554461974314)};
    }
    __syncthreads();
    typedef typename std::conditional<U8, uint8_t, float>::type out_t;
    const float* __restrict__ s = src + (int64_t)b * n;
    out_t* __restrict__ d = reinterpret_cast<out_t*>(dst_) + (int64_t)b * n;
    const int head_s = (int)((uintptr_t)s >> 2 & 3), head_d = (int)((uintptr_t)d / sizeof(out_t) & 3);
    const bool agree = head_s == head_d;
    const int head = agree ? head_s : 0;
    const int64_t g0 = (int64_t)blockIdx.x * (VST_THREADS * VST_INV_ITERS) + threadIdx.x;
    const int64_t first = 4 * (g0 - threadIdx.x) - head;                    // the workgroup's span: [first, first + 4 groups)
    const bool interior = agree && first >= 0 && first + 4 * VST_THREADS * VST_INV_ITERS <= n;
    f32x4 w[VST_INV_ITERS];
    if (interior)                                                           // every group is whole: all loads first
#pragma unroll
        for (int it = 0; it < VST_INV_ITERS; ++it)
            w[it] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(s + 4 * (g0 + it * VST_THREADS) - head));
#pragma unroll
    for (int it = 0; it < VST_INV_ITERS; ++it) {
        const int64_t e0 = 4 * (g0 + (int64_t)it * VST_THREADS) - head;
        if (e0 >= n) break;
        const bool whole = interior || (agree && e0 >= 0 && e0 + 4 <= n);
        if (!interior) {
            if (whole) w[it] = *reinterpret_cast<const f32x4*>(s + e0);
            else
#pragma unroll
                for (int i = 0; i < 4; ++i) w[it][i] = (e0 + i >= 0 && e0 + i < n) ? s[e0 + i] : 0.0f;
        }
        float x[4];
        int c = (int)((e0 + 4 * C) % C);                                    // e0 >= -3
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[i] = vst_inverse_one<EXACT>(planes[c], w[it][i]);
            if (U8) x[i] = rintf(x[i]);                                     // half to even
            c = c + 1 == C ? 0 : c + 1;
        }
        if (whole) {
            if (U8)
                *reinterpret_cast<unsigned*>(d + e0) = (unsigned)x[0] | (unsigned)x[1] << 8 | (unsigned)x[2] << 16 | (unsigned)x[3] << 24;
            else
                *reinterpret_cast<f32x4*>(d + e0) = (f32x4){x[0], x[1], x[2], x[3]};
        } else
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (e0 + i >= 0 && e0 + i < n) d[e0 + i] = (out_t)x[i];
    }
}

extern "C" int bf_op_vst_inverse(const float* src, void* dst, int B, int H, int W, int C, const double* gain, const double* offset,
                                 int exact, int cast_to_uint8, void* stream)
{
    int64_t n, groups;
    if (!src || !dst || !gain || !offset || ((uintptr_t)gain | (uintptr_t)offset) % 8 != 0) return BF_EINVAL;
    if ((uintptr_t)src % 4 != 0 || (!cast_to_uint8 && (uintptr_t)dst % 4 != 0)) return BF_EINVAL;
    if ((const void*)src == dst && cast_to_uint8) return BF_EINVAL;         // bytes over their own floats: not in place
    if (!vst_shape_ok(B, H, W, C, &n, &groups)) return BF_EINVAL;
    const int64_t per_wg = VST_THREADS * VST_INV_ITERS;
    const dim3 grid((unsigned)((groups + per_wg - 1) / per_wg), (unsigned)B), block(VST_THREADS);
    const hipStream_t st = (hipStream_t)stream;
    if (exact && cast_to_uint8) hipLaunchKernelGGL((vst_inverse_kernel<true, true>), grid, block, 0, st, src, dst, n, C, gain, offset);
    else if (exact) hipLaunchKernelGGL((vst_inverse_kernel<true, false>), grid, block, 0, st, src, dst, n, C, gain, offset);
    else if (cast_to_uint8) hipLaunchKernelGGL((vst_inverse_kernel<false, true>), grid, block, 0, st, src, dst, n, C, gain, offset);
    else hipLaunchKernelGGL((vst_inverse_kernel<false, false>), grid, block, 0, st, src, dst, n, C, gain, offset);
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}
