// DepthwiseConv2D 7 x 7 (SAME, zero padding; w [7][7][C]) -> [LayerNormalization(center=False, eps) * gamma] -> [activation]:
// the first layer of the reference's ConvNeXt block (bfcnn/backbone_convnext.py:108-113; backbone_blocks.py:174-189), the k = 7
// instance of bf_op_dwconv_ln (unet_ops.hip dispatches here).  fp32 NHWC, out != in, C in {32, 64, 128}.
//
// The column-walking form of uo_dwconv_ln_rows_kernel (a lane owns 4 channels of an image column and walks down a strip of rows;
// every input row is multiplied into the 7 output rows it touches, held as 7 rotating accumulators) keeps its k * k tap vectors
// in registers: at k = 7 that is 49 f32x4 = 196 VGPRs before the accumulators and the prefetched row.  Here
//   * the 49 tap vectors live in LDS ([tap][C / 4] f32x4, 6 / 12 / 24 KiB), read with ds_read_b128: the C / 4 lanes of a pixel read
//     consecutive 16-byte slots, lanes of different pixels the same ones (broadcast), so the reads are conflict-free;
//   * a lane owns TWO adjacent columns: a tap vector read from LDS feeds two multiply-adds, and an input row costs 8 loads for two
//     outputs (7 for one in the k <= 5 kernel).  With one LDS read per multiply-add the LDS (4 cycles per ds_read_b128 per wave,
//     shared by the CU's four SIMDs) would need more cycles than the multiply-adds themselves;
//   * registers: 14 accumulators + 8 current + 8 prefetched input vectors = 120 VGPRs + taps in flight; the compiler's 162 to 166
//     VGPRs leave three waves per SIMD.
// Each input row is requested one row step (about 400 vector instructions) ahead of its use; two rows ahead was measured and is
// slower, because its 200 VGPRs leave two waves per SIMD.  HBM traffic: the input once plus 6 halo rows per
// strip (from L2 where the neighbouring strip is resident), the output once.
//
// Summation order of an output: tap rows top to bottom, taps left to right, one fp32 accumulator -- fixed, independent of the strip
// an output row falls in, so the result is deterministic and does not depend on the strip height.  Rows and columns outside the
// image are loaded from the clamped coordinate and replaced by zero (a select, not a multiply: no 0 * inf), so H, W < 7 are fine.
#include "bf_common.h"
#include <math.h>

namespace {

constexpr int K = 7, RAD = 3, P = 2, NV = K + P - 1;      // P columns per lane, NV input vectors per row step

template <int CTRL>
__device__ __forceinline__ float d7_dpp_add(float v)
{
    const int t = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true);
    return v + __builtin_bit_cast(float, t);
}
// sum over the LPP = C / 4 consecutive lanes of a pixel, result in all of them (the butterfly of unet_ops.hip: uo_pixel_sum)
template <int LPP>
__device__ __forceinline__ float d7_pixel_sum(float v)
{
    v = d7_dpp_add<0xB1>(v);                      // quad_perm [1,0,3,2]
    v = d7_dpp_add<0x4E>(v);                      // quad_perm [2,3,0,1]
    if (LPP >= 8) v = d7_dpp_add<0x141>(v);       // row_half_mirror
    if (LPP >= 16) v = d7_dpp_add<0x140>(v);      // row_mirror
    if (LPP >= 32) v += __shfl_xor(v, 16, 64);
    return v;
}
__device__ __forceinline__ float d7_act(float v, int act, float alpha)
{
    switch (act) {
    case 1: return fmaxf(v, 0.f);
    case 2: return v > 0.f ? v : alpha * v;
    case 3: return bf_gelu(v);
    case 4: return tanhf(v);
    default: return v;
    }
}

// grid (column groups of P * 256 / (C / 4) columns, strips of R rows, batch)
template <int C>
__global__ __launch_bounds__(256, 2) void d7_dwconv_ln_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                              const float* __restrict__ w, const float* __restrict__ gamma, int H,
                                                              int W, int R, float eps, int act, float alpha)
{
    constexpr int LPP = C / 4, PPB = 256 / LPP;
    __shared__ f32x4 wl[K * K * LPP];
    for (int i = threadIdx.x; i < K * K * LPP; i += 256) wl[i] = reinterpret_cast<const f32x4*>(w)[i];
    __syncthreads();
    const int cl = threadIdx.x % LPP, pl = threadIdx.x / LPP;
    const int c0 = 4 * cl;
    const int x0 = (blockIdx.x * PPB + pl) * P;
    const int y0 = blockIdx.y * R;
    const int yend = min(y0 + R, H);
    const int64_t img = (int64_t)blockIdx.z * H * W;
    f32x4 gm = {1.f, 1.f, 1.f, 1.f};
    if (gamma) gm = *reinterpret_cast<const f32x4*>(gamma + c0);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    // the NV input columns x0 - 3 .. x0 + P + 2 (clamped into the image; the ones outside are replaced by zero)
    int xo[NV];
    bool xin[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int xx = x0 + j - RAD;
        xin[j] = xx >= 0 && xx < W;
        xo[j] = min(max(xx, 0), W - 1) * C + c0;
    }
    auto load_row = [&](int yi, f32x4 (&v)[NV]) {
        const float* row = in + (img + (int64_t)min(max(yi, 0), H - 1) * W) * C;
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] = *reinterpret_cast<const f32x4*>(row + xo[j]);
    };
    f32x4 acc[K][P];
#pragma unroll
    for (int ky = 0; ky < K; ++ky)
#pragma unroll
        for (int p = 0; p < P; ++p) acc[ky][p] = zero;
    f32x4 nxt[NV];
    load_row(y0 - RAD, nxt);
    for (int yi = y0 - RAD; yi < yend + RAD; ++yi) {
        const bool yin = yi >= 0 && yi < H;                       // the same for the whole workgroup
        f32x4 v[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] = (yin && xin[j]) ? nxt[j] : zero;
        load_row(yi + 1, nxt);                                      // in flight while this row is multiplied
        if (yin) {
            // input row yi is tap row ky of output row yi - ky + RAD = accumulator ky
#pragma unroll
            for (int ky = 0; ky < K; ++ky)
#pragma unroll
                for (int kx = 0; kx < K; ++kx) {
                    const f32x4 wv = wl[(ky * K + kx) * LPP + cl];
#pragma unroll
                    for (int p = 0; p < P; ++p) acc[ky][p] += wv * v[kx + p];
                }
        }
        const int yo = yi - RAD;                                    // acc[K - 1] is complete (yo < yend by the loop bound)
        if (yo >= y0) {
#pragma unroll
            for (int p = 0; p < P; ++p) {
                f32x4 r = acc[K - 1][p];
                if (gamma) {
                    const float mean = d7_pixel_sum<LPP>(r[0] + r[1] + r[2] + r[3]) * (1.f / C);
                    const f32x4 dd = r - mean;
                    const float var = d7_pixel_sum<LPP>(dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2] + dd[3] * dd[3]) * (1.f / C);
                    r = dd * (gm * rsqrtf(var + eps));
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) r[j] = d7_act(r[j], act, alpha);
                if (x0 + p < W) *reinterpret_cast<f32x4*>(out + ((img + (int64_t)yo * W) + x0 + p) * C + c0) = r;
            }
        }
#pragma unroll
        for (int ky = K - 1; ky > 0; --ky)
#pragma unroll
            for (int p = 0; p < P; ++p) acc[ky][p] = acc[ky - 1][p];
#pragma unroll
        for (int p = 0; p < P; ++p) acc[0][p] = zero;
    }
}

// rows per workgroup: 6 halo rows are re-read and re-multiplied per strip (32 rows: 19 % more multiply-adds than outputs, 8 rows:
// 75 %); inputs that would give fewer than two workgroups per CU (512) with 32-row strips take 8-row strips, as bf_op_dwconv_ln
// does for k <= 5.  64-row strips (9 %) were measured at 32 x 256 x 256 and are no faster: at 64 channels they
// leave 1024 workgroups for the 768 the chip holds at once.  The height is a kernel argument.
int d7_strip_rows(int B, int H, int W, int C)
{
    const int cols = P * 256 / (C / 4);
    const int64_t wgs = (int64_t)B * ((W + cols - 1) / cols) * ((H + 31) / 32);
    return (wgs >= 512 || (H + 7) / 8 > 65535) ? 32 : 8;
}

}  // namespace

int bf_dwconv7_ln(const float* in, float* out, const float* w, const float* ln_gamma, int B, int H, int W, int C, float eps, int act,
                  float alpha, hipStream_t s)
{
    if (C != 32 && C != 64 && C != 128) return BF_EUNSUPPORTED;
    const int R = d7_strip_rows(B, H, W, C);
    const int cols = P * 256 / (C / 4);
    if (B > 65535 || (H + R - 1) / R > 65535) return BF_EUNSUPPORTED;
    const dim3 grid((W + cols - 1) / cols, (H + R - 1) / R, B);
    if (C == 32) hipLaunchKernelGGL(d7_dwconv_ln_kernel<32>, grid, dim3(256), 0, s, in, out, w, ln_gamma, H, W, R, eps, act, alpha);
    else if (C == 64) hipLaunchKernelGGL(d7_dwconv_ln_kernel<64>, grid, dim3(256), 0, s, in, out, w, ln_gamma, H, W, R, eps, act, alpha);
    else hipLaunchKernelGGL(d7_dwconv_ln_kernel<128>, grid, dim3(256), 0, s, in, out, w, ln_gamma, H, W, R, eps, act, alpha);
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}
