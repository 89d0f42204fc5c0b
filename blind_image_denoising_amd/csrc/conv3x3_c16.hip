// 3x3, 16 -> 16 channel, stride-1 SAME convolutions on the gfx950 matrix cores.
//
// Reference semantics: keras Conv2D(3x3, use_bias=False, padding="same") inside conv2d_wrapper
// (bfcnn/utilities.py:196) as the resnet blocks call it (bfcnn/backbone_blocks.py:174-196), the
// BatchNormalization / activation that follow it (utilities.py:207-215) and the residual Add
// (backbone_blocks.py:242).
//
// GEMM view per tap: D[cout][pixel] += W[cout][cin] * X[cin][pixel], exact fp32 on
// v_mfma_f32_16x16x4_f32 (bitwise an fmaf chain).  The weights are the A operand and live in 36
// VGPRs per lane for the whole kernel; the activations are the B operand, one ds_read_b128 per
// tap and 16-pixel group feeds four MFMAs (k-slot q of MFMA kk carries cin = 4q+kk).  The D
// fragment leaves every lane with 4 consecutive output channels of one pixel, so stores are
// 16 B per lane, 1 KiB contiguous per wave-instruction in NHWC.
#include "bf_common.h"

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// ------------------------------------------------------------------------------------------
// weight packing: HWIO [3,3,16,16] -> wpack[(tap*4+kk)*64 + lane] = W[tap][4*(lane>>4)+kk][lane&15]
// transpose_flip = 1 packs the data-gradient kernel W'[tap][ci][co] = W[8-tap][co][ci].
// ------------------------------------------------------------------------------------------
__global__ void pack_conv_kernel(const float* __restrict__ w, float* __restrict__ wpack, int transpose_flip)
{
    for (int idx = threadIdx.x; idx < BF_WPACK_FLOATS; idx += blockDim.x) {
        const int i = idx >> 6, l = idx & 63;
        const int tap = i >> 2, kk = i & 3;
        const int cin = 4 * (l >> 4) + kk, cout = l & 15;
        wpack[idx] = transpose_flip ? w[((8 - tap) * 16 + cout) * 16 + cin]
                                    : w[(tap * 16 + cin) * 16 + cout];
    }
}

hipError_t bf_launch_pack_conv(const float* w_hwio, float* wpack, int transpose_flip, hipStream_t s)
{
    hipLaunchKernelGGL(pack_conv_kernel, dim3(1), dim3(256), 0, s, w_hwio, wpack, transpose_flip);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// generic single convolution with selectable epilogue
// ------------------------------------------------------------------------------------------
constexpr int CT_H = 16, CT_W = 32;            // output tile
constexpr int CT_IH = CT_H + 2, CT_IW = CT_W + 2;

template <int EPI>
__global__ __launch_bounds__(256) void conv3x3_c16_kernel(ConvArgs a)
{
    __shared__ __attribute__((aligned(16))) float tile[CT_IH * CT_IW * 16];   // 39,168 B
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles_x = (a.W + CT_W - 1) / CT_W, tiles_y = (a.H + CT_H - 1) / CT_H;
    int t = blockIdx.x;
    const int tx = t % tiles_x; t /= tiles_x;
    const int ty = t % tiles_y;
    const int b = t / tiles_y;
    const int y0 = ty * CT_H, x0 = tx * CT_W;
    const size_t img = (size_t)b * a.H * a.W * 16;
    const float* inb = a.in + img;

    for (int n = tid; n < CT_IH * CT_IW * 4; n += 256) {
        const int row = n / (CT_IW * 4);
        const int rem = n - row * (CT_IW * 4);
        const int gy = y0 - 1 + row, gx = x0 - 1 + (rem >> 2);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W)
            v = *reinterpret_cast<const float4*>(inb + ((size_t)gy * a.W + gx) * 16 + (rem & 3) * 4);
        *reinterpret_cast<float4*>(tile + n * 4) = v;
    }
    float w[36];
#pragma unroll
    for (int i = 0; i < 36; ++i) w[i] = a.wpack[i * 64 + lane];
    __syncthreads();

    const int p = lane & 15, q = lane >> 4;
    f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
    if (EPI & EPI_AFFINE) {
        sc = *reinterpret_cast<const f32x4*>(a.scale + q * 4);
        sh = *reinterpret_cast<const f32x4*>(a.shift + q * 4);
    }
    f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int half = 0; half < 2; ++half) {
        f32x4 acc[4];
        int base[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const int gi = half * 4 + j;
            const int r = 4 * wave + (gi >> 1), xo = (gi & 1) * 16;
            base[j] = (r * CT_IW + xo + p) * 16 + q * 4;
        }
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int off = ((tap / 3) * CT_IW + (tap % 3)) * 16;
            f32x4 bv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) bv[j] = *reinterpret_cast<const f32x4*>(tile + base[j] + off);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = MFMA(w[tap * 4 + kk], bv[j][kk], acc[j]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gi = half * 4 + j;
            const int gy = y0 + 4 * wave + (gi >> 1), gx = x0 + (gi & 1) * 16 + p;
            if (gy < a.H && gx < a.W) {
                const size_t idx = img + ((size_t)gy * a.W + gx) * 16 + q * 4;
                f32x4 v = bf_acc_ready(acc[j]);
                if (EPI & EPI_STATS) { s1 += v; s2 += v * v; }
                if (EPI & EPI_AFFINE) v = v * sc + sh;
                if (EPI & EPI_RELU) {
                    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                }
                if (EPI & EPI_MASK) {
                    const f32x4 m = *reinterpret_cast<const f32x4*>(a.mask + idx);
                    v.x = m.x > 0.f ? v.x : 0.f; v.y = m.y > 0.f ? v.y : 0.f;
                    v.z = m.z > 0.f ? v.z : 0.f; v.w = m.w > 0.f ? v.w : 0.f;
                }
                if (EPI & EPI_RES) v += *reinterpret_cast<const f32x4*>(a.res + idx);
                *reinterpret_cast<f32x4*>(a.out + idx) = v;
            }
        }
    }

    if (EPI & EPI_STATS) {
        // reduce over the 16 pixel lanes that share a channel quad, then over the 4 waves
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                s1[c] += __shfl_xor(s1[c], m);
                s2[c] += __shfl_xor(s2[c], m);
            }
        }
        __syncthreads();                       // tile no longer needed
        float* red = tile;                     // [4 waves][32]
        if (p == 0) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                red[wave * 32 + q * 4 + c] = s1[c];
                red[wave * 32 + 16 + q * 4 + c] = s2[c];
            }
        }
        __syncthreads();
        if (tid < 32)
            a.stats[(size_t)blockIdx.x * 32 + tid] = (red[tid] + red[32 + tid]) + (red[64 + tid] + red[96 + tid]);
    }
}

int bf_conv3x3_c16_grid(int B, int H, int W)
{
    return B * ((H + CT_H - 1) / CT_H) * ((W + CT_W - 1) / CT_W);
}

hipError_t bf_launch_conv3x3_c16(const ConvArgs& a, int epi, hipStream_t s)
{
    const dim3 grid(bf_conv3x3_c16_grid(a.B, a.H, a.W)), block(256);
#define BF_CASE(E) case E: hipLaunchKernelGGL(conv3x3_c16_kernel<E>, grid, block, 0, s, a); break;
    switch (epi) {
        BF_CASE(0)
        BF_CASE(EPI_RELU)
        BF_CASE(EPI_STATS)
        BF_CASE(EPI_AFFINE | EPI_RES)
        BF_CASE(EPI_AFFINE)
        BF_CASE(EPI_AFFINE | EPI_RELU)
        BF_CASE(EPI_RES)
        BF_CASE(EPI_MASK)
        default: return hipErrorInvalidValue;
    }
#undef BF_CASE
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// fused residual block (inference): out = x + scale * conv2(act(conv1(x))) + shift
// One HBM read and one HBM write of the 16-channel activation per BLOCK (72 FLOP/B instead of
// 36); the intermediate activation only ever exists in LDS.  Tile 14x32 outputs: input tile
// 18x36 px (41,472 B) + intermediate 16x34 px (34,816 B) = 76,288 B LDS -> two 4-wave
// workgroups per CU.  Workgroups are persistent: weights (72 VGPRs) are fetched once; consecutive
// tiles of one XCD-label (blockIdx % 8) are neighbours in the image so halos are L2 hits.
// ------------------------------------------------------------------------------------------
// Tile geometry is a template parameter (TH x TW outputs, NW waves per workgroup).  TW is a multiple
// of 16, so an output row is TW/16 MFMA groups.  The intermediate region is (TH+2) x (TW+2): per row
// TW/16 "row groups" (columns 0..TW-1) and the two remaining columns of every 8 rows form one "strip
// group" (lane p -> row 8s + p/2, column TW + p%2).
template <int TH_, int TW_, int NW_>
struct FusedCfg {
    static constexpr int TH = TH_, TW = TW_, NW = NW_, NT = NW_ * 64;
    static constexpr int MH = TH + 2, MW = TW + 2;        // intermediate region
    static constexpr int IH = TH + 4, IW = TW + 4;        // input region
    static constexpr int GPR = TW / 16;                   // groups per row
    static constexpr int RG = MH * GPR;                   // conv1 row groups
    static constexpr int SG = (MH + 7) / 8;               // conv1 strip groups
    static constexpr int OG = TH * GPR;                   // conv2 groups
    static constexpr int IN4 = IH * IW * 4;               // float4 per input tile
    static constexpr int PF = (IN4 + NT - 1) / NT;        // float4 per lane in the prefetch
    static_assert(TW % 16 == 0, "output rows must be whole MFMA groups");
};

template <int NG>
__device__ __forceinline__ void conv_groups(const float* __restrict__ src, const int (&base)[NG],
                                            const int row_pitch, const float (&w)[36], f32x4 (&acc)[NG])
{
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int off = ((tap / 3) * row_pitch + (tap % 3)) * 16;
        f32x4 bv[NG];
#pragma unroll
        for (int j = 0; j < NG; ++j) bv[j] = *reinterpret_cast<const f32x4*>(src + base[j] + off);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int j = 0; j < NG; ++j) acc[j] = MFMA(w[tap * 4 + kk], bv[j][kk], acc[j]);
    }
}

struct FusedTile {
    int y0, x0;
    size_t img;
};

template <class Cfg>
__device__ __forceinline__ FusedTile fused_tile(const FusedBlockArgs& a, int t)
{
    FusedTile r;
    const int tx = t % a.tiles_x;
    t /= a.tiles_x;
    const int ty = t % a.tiles_y;
    const int b = t / a.tiles_y;
    r.y0 = ty * Cfg::TH;
    r.x0 = tx * Cfg::TW;
    r.img = (size_t)b * a.H * a.W * 16;
    return r;
}

// a tile whose whole input region lies inside the image needs no bounds check anywhere
template <class Cfg>
__device__ __forceinline__ bool tile_interior(const FusedBlockArgs& a, const FusedTile& t)
{
    return t.y0 >= 2 && t.y0 + Cfg::TH + 2 <= a.H && t.x0 >= 2 && t.x0 + Cfg::TW + 2 <= a.W;
}

// ---- v4: LDS-DMA + immediate-offset addressing ------------------------------------------------------
// Measured on MI355X (profiles/, tools/exp): a non-MFMA VALU instruction costs ~7 SIMD cycles of matrix
// throughput, and the register-prefetch kernel executes 0.74 of them per MFMA (tile fetch address math,
// LDS staging, pass prologues/epilogues) -- that, not barriers or tiling, held it at 61 %.  This variant
// removes them structurally:
//   * wave w owns groups g = w + NW*k.  With RG % NW == 0 and NW % GPR == 0 the group's row is
//     (w/GPR) + (NW/GPR)*k and its column (w%GPR)*16, so every LDS address is ONE per-wave VGPR constant
//     plus a compile-time immediate (ds_read/ds_write offset field); global addresses are a scalar base
//     plus one per-wave VGPR constant.  A pass needs no address VALU at all.
//   * the next tile goes global -> LDS by DMA (global_load_lds_dwordx4) with per-lane constant offsets:
//     no VGPR staging, no ds_write pass, no fetch address math; it is issued after the conv1 -> conv2
//     barrier (the residual is re-read from global/L2) and lands while conv2 runs.  Two barriers per tile.
template <class Cfg>
struct V4 {
    static_assert(Cfg::RG % Cfg::NW == 0 && Cfg::NW % Cfg::GPR == 0, "v4 addressing needs RG % NW == 0 and NW % GPR == 0");
    static constexpr int RSTEP = Cfg::NW / Cfg::GPR;              // rows between a wave's consecutive groups
    static constexpr int K1R = Cfg::RG / Cfg::NW;                  // conv1 row groups per wave
    static constexpr int K1S = (Cfg::SG + Cfg::NW - 1) / Cfg::NW;  // conv1 strip-group slots per wave
    static constexpr int K2 = Cfg::OG / Cfg::NW;                   // conv2 groups per wave (OG % NW == 0 follows)
    static_assert(Cfg::OG % Cfg::NW == 0, "conv2 groups must divide evenly");
    static constexpr int TIN_PAD_FLOATS = Cfg::PF * Cfg::NT * 4;
    static constexpr int TMID_FLOATS = Cfg::MH * Cfg::MW * 16;
    static constexpr int LDS_BYTES = (TMID_FLOATS + TIN_PAD_FLOATS) * 4;
};

struct V4Lane {
    int in_c;        // float offset in the input tile of this wave's row-group pixel (k = 0)
    int mid_c;       // float offset in the intermediate tile (k = 0): conv1 writes, conv2 reads
    int strip_in;    // float offset in the input tile of this wave's strip-group pixel (slot 0)
    int strip_mid;   // float offset in the intermediate tile of this wave's strip-group pixel
    unsigned glob_c; // byte offset in the image of this wave's output pixel (k = 0) relative to the tile origin
    int px;          // column of the lane's pixel inside the tile for row groups: (w%GPR)*16 + p
    int sp;          // p (strip groups: row 8s + p/2, column TW + p%2)
};

// K consecutive groups of this wave starting at slot K0: conv1 (+activation) -> intermediate tile
template <class Cfg, int NG, int K0, bool INTERIOR>
__device__ __forceinline__ void v4_conv1_rows(const FusedBlockArgs& a, const float* __restrict__ tin, float* __restrict__ tmid,
                                              const float (&w1)[36], const V4Lane& L, const FusedTile& t, const int wrow)
{
    constexpr int RS = V4<Cfg>::RSTEP;
    int base[NG];
    f32x4 acc[NG];
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        base[j] = L.in_c + (K0 + j) * RS * Cfg::IW * 16;            // VGPR + immediate
        acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    conv_groups<NG>(tin, base, Cfg::IW, w1, acc);
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        f32x4 v = bf_acc_ready(acc[j]);
        if (a.act1_relu) {
            v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
        }
        if (!INTERIOR) {
            // conv2 must see ZERO padding outside the image, not conv1 evaluated there
            const int gy = t.y0 - 1 + wrow + (K0 + j) * RS;         // scalar
            const int gx = t.x0 - 1 + L.px;
            if (gy < 0 || gy >= a.H || gx < 0 || gx >= a.W) v = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        *reinterpret_cast<f32x4*>(tmid + L.mid_c + (K0 + j) * RS * Cfg::MW * 16) = v;
    }
}

template <class Cfg, bool INTERIOR>
__device__ __forceinline__ void v4_conv1_strip(const FusedBlockArgs& a, const float* __restrict__ tin, float* __restrict__ tmid,
                                               const float (&w1)[36], const V4Lane& L, const FusedTile& t, const int s)
{
    // strip group s: rows 8s .. 8s+7 (clamped to MH-1 in a partial last group), columns TW, TW+1
    int base[1];
    f32x4 acc[1] = {(f32x4){0.f, 0.f, 0.f, 0.f}};
    int my = 8 * s + (L.sp >> 1);
    int dst;
    if (Cfg::MH % 8 == 0 || 8 * s + 8 <= Cfg::MH) {
        base[0] = L.strip_in;
        dst = L.strip_mid;
    } else {
        my = min(my, Cfg::MH - 1);
        base[0] = (my * Cfg::IW + Cfg::TW + (L.sp & 1)) * 16 + (L.in_c & 12);
        dst = (my * Cfg::MW + Cfg::TW + (L.sp & 1)) * 16 + (L.in_c & 12);
    }
    conv_groups<1>(tin, base, Cfg::IW, w1, acc);
    f32x4 v = bf_acc_ready(acc[0]);
    if (a.act1_relu) {
        v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    }
    if (!INTERIOR) {
        const int gy = t.y0 - 1 + my, gx = t.x0 - 1 + Cfg::TW + (L.sp & 1);
        if (gy < 0 || gy >= a.H || gx < 0 || gx >= a.W) v = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    *reinterpret_cast<f32x4*>(tmid + dst) = v;
}

// conv2 + folded BN + residual (from global) of NG groups starting at slot K0
template <class Cfg, int NG, int K0, bool INTERIOR>
__device__ __forceinline__ void v4_conv2(const FusedBlockArgs& a, const float* __restrict__ tmid, const char* __restrict__ in_tile,
                                         char* __restrict__ out_tile, const float (&w2)[36], const f32x4 sc, const f32x4 sh,
                                         const V4Lane& L, const FusedTile& t, const int wrow)
{
    constexpr int RS = V4<Cfg>::RSTEP;
    int base[NG];
    f32x4 acc[NG], res[NG];
    const size_t rowstep = (size_t)a.W * 64;                         // bytes per image row
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        base[j] = L.mid_c + (K0 + j) * RS * Cfg::MW * 16;
        acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        res[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const int gy = t.y0 + wrow + (K0 + j) * RS;                  // scalar
        if (INTERIOR || (gy < a.H && t.x0 + L.px < a.W))
            res[j] = *reinterpret_cast<const f32x4*>(in_tile + (K0 + j) * RS * rowstep + L.glob_c);
    }
    conv_groups<NG>(tmid, base, Cfg::MW, w2, acc);
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        const int gy = t.y0 + wrow + (K0 + j) * RS;
        if (INTERIOR || (gy < a.H && t.x0 + L.px < a.W)) {
            const f32x4 v = bf_acc_ready(acc[j]) * sc + sh + res[j];
            *reinterpret_cast<f32x4*>(out_tile + (K0 + j) * RS * rowstep + L.glob_c) = v;
        }
    }
}

template <class Cfg, int K0, bool INTERIOR>
__device__ __forceinline__ void v4_conv1_all(const FusedBlockArgs& a, const float* __restrict__ tin, float* __restrict__ tmid,
                                             const float (&w1)[36], const V4Lane& L, const FusedTile& t, const int wrow)
{
    constexpr int K = V4<Cfg>::K1R;
    if constexpr (K0 < K) {
        constexpr int NG = K - K0 >= 4 ? (K - K0 == 4 || K - K0 >= 7 ? 4 : 3) : K - K0;   // 8 -> 4+4, 9 -> 3+3+3, 6 -> 3+3, 5 -> 3+2
        const bool needed = INTERIOR || (t.y0 - 1 + wrow + K0 * V4<Cfg>::RSTEP <= a.H);  // rows beyond H+1 are never read
        if (needed) v4_conv1_rows<Cfg, NG, K0, INTERIOR>(a, tin, tmid, w1, L, t, wrow);
        v4_conv1_all<Cfg, K0 + NG, INTERIOR>(a, tin, tmid, w1, L, t, wrow);
    }
}

template <class Cfg, int K0, bool INTERIOR>
__device__ __forceinline__ void v4_conv2_all(const FusedBlockArgs& a, const float* __restrict__ tmid, const char* __restrict__ in_tile,
                                             char* __restrict__ out_tile, const float (&w2)[36], const f32x4 sc, const f32x4 sh,
                                             const V4Lane& L, const FusedTile& t, const int wrow)
{
    constexpr int K = V4<Cfg>::K2;
    if constexpr (K0 < K) {
        constexpr int NG = K - K0 >= 4 ? (K - K0 == 4 || K - K0 >= 7 ? 4 : 3) : K - K0;   // 7 -> 4+3
        const bool needed = INTERIOR || (t.y0 + wrow + K0 * V4<Cfg>::RSTEP < a.H);
        if (needed) v4_conv2<Cfg, NG, K0, INTERIOR>(a, tmid, in_tile, out_tile, w2, sc, sh, L, t, wrow);
        v4_conv2_all<Cfg, K0 + NG, INTERIOR>(a, tmid, in_tile, out_tile, w2, sc, sh, L, t, wrow);
    }
}

// DMA of a tile: interior = per-lane constant offsets from the tile origin, nothing else
template <class Cfg, bool INTERIOR>
__device__ __forceinline__ void v4_dma(const FusedBlockArgs& a, const FusedTile& t, float* __restrict__ tin, int tid, int wave,
                                       const unsigned (&pfoff)[Cfg::PF])
{
    const char* origin = reinterpret_cast<const char*>(a.in + t.img) + ((ptrdiff_t)(t.y0 - 2) * a.W + (t.x0 - 2)) * 64;
    constexpr int RW = Cfg::IW * 4;
    int row = tid / RW, rem = tid - row * RW;
#pragma unroll
    for (int i = 0; i < Cfg::PF; ++i) {
        const char* src = origin + pfoff[i];
        if (!INTERIOR || (i + 1) * Cfg::NT > Cfg::IN4) {
            const bool in_tile = (i + 1) * Cfg::NT <= Cfg::IN4 || tid + i * Cfg::NT < Cfg::IN4;
            bool inside = true;
            if (!INTERIOR) {
                const int gy = t.y0 - 2 + row, gx = t.x0 - 2 + (rem >> 2);
                inside = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
                rem += Cfg::NT % RW;
                row += Cfg::NT / RW;
                if (rem >= RW) { rem -= RW; ++row; }
            }
            if (!(in_tile && inside)) src = reinterpret_cast<const char*>(a.zeros);
        }
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(tin + (i * Cfg::NT + wave * 64) * 4),
                                         16, 0, 0);
    }
}

template <class Cfg>
__global__ __launch_bounds__(Cfg::NT, 2) void fused_block_v4_kernel(FusedBlockArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* tmid = lds;                                       // [MH][MW][16]
    float* tin = lds + V4<Cfg>::TMID_FLOATS;                 // [IH][IW][16] + pad to whole wave-instructions
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int p = lane & 15, q = lane >> 4;
    const int wrow = wave / Cfg::GPR, wcol = (wave % Cfg::GPR) * 16;

    V4Lane L0;
    L0.in_c = (wrow * Cfg::IW + wcol + p) * 16 + q * 4;
    L0.mid_c = (wrow * Cfg::MW + wcol + p) * 16 + q * 4;
    L0.strip_in = ((8 * wave + (p >> 1)) * Cfg::IW + Cfg::TW + (p & 1)) * 16 + q * 4;     // strip slot 0: s = wave
    L0.strip_mid = ((8 * wave + (p >> 1)) * Cfg::MW + Cfg::TW + (p & 1)) * 16 + q * 4;
    L0.glob_c = ((unsigned)(wrow * a.W + wcol + p) * 16u + (unsigned)q * 4u) * 4u;
    L0.px = wcol + p;
    L0.sp = p;
    unsigned pfoff[Cfg::PF];
    {
        constexpr int RW = Cfg::IW * 4;
        int row = tid / RW, rem = tid - row * RW;
#pragma unroll
        for (int i = 0; i < Cfg::PF; ++i) {
            pfoff[i] = ((unsigned)(row * a.W + (rem >> 2)) * 16u + (unsigned)(rem & 3) * 4u) * 4u;
            rem += Cfg::NT % RW;
            row += Cfg::NT / RW;
            if (rem >= RW) { rem -= RW; ++row; }
        }
    }

    float w1[36], w2[36];
#pragma unroll
    for (int i = 0; i < 36; ++i) { w1[i] = a.w1pack[i * 64 + lane]; w2[i] = a.w2pack[i * 64 + lane]; }
    const f32x4 sc = *reinterpret_cast<const f32x4*>(a.scale + q * 4);
    const f32x4 sh = *reinterpret_cast<const f32x4*>(a.shift + q * 4);

    const int nxcd = gridDim.x >= 8 ? 8 : 1;
    const int label = blockIdx.x % nxcd, slot = blockIdx.x / nxcd;
    const int per_label = gridDim.x / nxcd;
    const int chunk = (a.ntiles + nxcd - 1) / nxcd;
    const int t_begin = label * chunk;
    const int t_end = min(a.ntiles, t_begin + chunk);
    int t = t_begin + slot;
    if (t >= t_end) return;

    FusedTile cur = fused_tile<Cfg>(a, t);
    v4_dma<Cfg, false>(a, cur, tin, tid, wave, pfoff);
    __syncthreads();                                         // drains the DMA (vmcnt(0)) and publishes tin

    for (; t < t_end; t += per_label) {
        const int tn = t + per_label;
        const bool has_next = tn < t_end;
        FusedTile nxt = cur;
        if (has_next) nxt = fused_tile<Cfg>(a, tn);
        V4Lane L = L0;
        // opaque inside the loop body: keeps LICM from hoisting every (constant + immediate) address
        asm volatile("" : "+v"(L.in_c), "+v"(L.mid_c), "+v"(L.glob_c));
        const bool interior = tile_interior<Cfg>(a, cur);
        const char* in_tile = reinterpret_cast<const char*>(a.in + cur.img) + ((size_t)cur.y0 * a.W + cur.x0) * 64;
        char* out_tile = reinterpret_cast<char*>(a.out + cur.img) + ((size_t)cur.y0 * a.W + cur.x0) * 64;

        // ---- conv1: input tile -> intermediate tile -------------------------------------------
        if (interior) v4_conv1_all<Cfg, 0, true>(a, tin, tmid, w1, L, cur, wrow);
        else v4_conv1_all<Cfg, 0, false>(a, tin, tmid, w1, L, cur, wrow);
#pragma unroll
        for (int ks = 0; ks < V4<Cfg>::K1S; ++ks) {
            const int s = wave + Cfg::NW * ks;               // strip group index
            if (s < Cfg::SG) {
                V4Lane Ls = L;
                Ls.strip_in = L.strip_in + ks * Cfg::NW * 8 * Cfg::IW * 16;
                Ls.strip_mid = L.strip_mid + ks * Cfg::NW * 8 * Cfg::MW * 16;
                if (interior) v4_conv1_strip<Cfg, true>(a, tin, tmid, w1, Ls, cur, s);
                else if (cur.y0 - 1 + 8 * s <= a.H && cur.x0 - 1 + Cfg::TW <= a.W) v4_conv1_strip<Cfg, false>(a, tin, tmid, w1, Ls, cur, s);
            }
        }
        __syncthreads();                                     // tmid complete; tin is dead (residual comes from global)

        if (has_next) {
            if (tile_interior<Cfg>(a, nxt)) v4_dma<Cfg, true>(a, nxt, tin, tid, wave, pfoff);
            else v4_dma<Cfg, false>(a, nxt, tin, tid, wave, pfoff);
        }
        // ---- conv2 + folded BN + residual -> global ---------------------------------------------
        if (interior) v4_conv2_all<Cfg, 0, true>(a, tmid, in_tile, out_tile, w2, sc, sh, L, cur, wrow);
        else v4_conv2_all<Cfg, 0, false>(a, tmid, in_tile, out_tile, w2, sc, sh, L, cur, wrow);
        __syncthreads();                                     // drains the DMA; tin = next tile, tmid free
        cur = nxt;
    }
}

template <class Cfg>
static hipError_t launch_fused_v4(FusedBlockArgs a, int wgs_per_cu, hipStream_t s)
{
    if (!a.zeros) return hipErrorInvalidValue;
    a.tiles_x = (a.W + Cfg::TW - 1) / Cfg::TW;
    a.tiles_y = (a.H + Cfg::TH - 1) / Cfg::TH;
    a.ntiles = a.B * a.tiles_x * a.tiles_y;
    {
        const hipError_t ea = bf_set_max_lds(reinterpret_cast<const void*>(fused_block_v4_kernel<Cfg>), V4<Cfg>::LDS_BYTES);      // once per device
        if (ea != hipSuccess) return ea;
    }
    const int resident = 256 * wgs_per_cu;
    int grid = a.ntiles < resident ? a.ntiles : resident;
    if (grid >= 8) grid -= grid % 8;
    hipLaunchKernelGGL(fused_block_v4_kernel<Cfg>, dim3(grid), dim3(Cfg::NT), V4<Cfg>::LDS_BYTES, s, a);
    return hipGetLastError();
}

// bf_set_option("fused_tile") once chose between this kernel (4) and its predecessors (0-2 register prefetch in three tile
// geometries, 3 LDS-DMA without immediate-offset addressing; DESIGN.md 4 keeps their measurements).  The option stays and
// succeeds for every integer; every value runs fused_block_v4_kernel on 14x32 tiles x 4 waves, two workgroups per CU.
void bf_set_fused_tile(int) {}

// name of the kernel bf_launch_fused_block launches (bench.py looks its counter traffic up by this name)
const char* bf_fused_block_kernel_name() { return "fused_block_v4_kernel"; }

hipError_t bf_launch_fused_block(const FusedBlockArgs& a, hipStream_t s) { return launch_fused_v4<FusedCfg<14, 32, 4>>(a, 2, s); }

// ------------------------------------------------------------------------------------------
// weight gradient of the 3x3 16->16 convolution:
//   dW[tap][ci][co] = sum over pixels of X[pixel + tap][ci] * dY[pixel][co]
// GEMM view: M = ci, N = co, K = pixels (4 per MFMA; k-slot q of MFMA kk is pixel 4kk+q of a
// 16-pixel group, which keeps the ds_read_b32 of both operands bank-conflict free).  One dY
// fragment is shared by the nine taps (nine accumulators = 36 VGPRs).  Persistent workgroups
// keep their partial dW in registers across tiles; partials are reduced in a fixed order
// (no float atomics -> bitwise reproducible).
// ------------------------------------------------------------------------------------------
constexpr int WG_TH = 16, WG_TW = 32;
constexpr int WG_IH = WG_TH + 2, WG_IW = WG_TW + 2;

__global__ __launch_bounds__(256, 2) void wgrad3x3_c16_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                              float* __restrict__ partial, int B, int H, int W,
                                                              int tiles_x, int tiles_y, int ntiles)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* tx_ = lds;                               // [18][34][16]  x with halo
    float* td = lds + WG_IH * WG_IW * 16;           // [16][32][16]  dy
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = lane & 15, q = lane >> 4;
    f32x4 acc[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int tt = t;
        const int txi = tt % tiles_x; tt /= tiles_x;
        const int tyi = tt % tiles_y;
        const int b = tt / tiles_y;
        const int y0 = tyi * WG_TH, x0 = txi * WG_TW;
        const size_t img = (size_t)b * H * W * 16;
        for (int n = tid; n < WG_IH * WG_IW * 4; n += 256) {
            const int row = n / (WG_IW * 4);
            const int rem = n - row * (WG_IW * 4);
            const int gy = y0 - 1 + row, gx = x0 - 1 + (rem >> 2);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gy >= 0 && gy < H && gx >= 0 && gx < W)
                v = *reinterpret_cast<const float4*>(x + img + ((size_t)gy * W + gx) * 16 + (rem & 3) * 4);
            *reinterpret_cast<float4*>(tx_ + n * 4) = v;
        }
        for (int n = tid; n < WG_TH * WG_TW * 4; n += 256) {
            const int row = n / (WG_TW * 4);
            const int rem = n - row * (WG_TW * 4);
            const int gy = y0 + row, gx = x0 + (rem >> 2);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gy < H && gx < W)
                v = *reinterpret_cast<const float4*>(dy + img + ((size_t)gy * W + gx) * 16 + (rem & 3) * 4);
            *reinterpret_cast<float4*>(td + n * 4) = v;
        }
        __syncthreads();
        // wave handles rows 4w..4w+3 of the tile: 8 groups of 16 pixels
        for (int gi = 0; gi < 8; ++gi) {
            const int r = 4 * wave + (gi >> 1), xo = (gi & 1) * 16;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int px = xo + 4 * kk + q;
                const float bv = td[(r * WG_TW + px) * 16 + p];
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const float av = tx_[((r + tap / 3) * WG_IW + px + tap % 3) * 16 + p];
                    acc[tap] = MFMA(av, bv, acc[tap]);
                }
            }
        }
        __syncthreads();
    }
    // cross-wave reduction through LDS: [4][9][256]
    float* red = lds;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            red[(wave * 9 + tap) * 256 + (4 * q + j) * 16 + p] = acc[tap][j];
    __syncthreads();
    for (int i = tid; i < 2304; i += 256)
        partial[(size_t)blockIdx.x * 2304 + i] = (red[i] + red[2304 + i]) + (red[2 * 2304 + i] + red[3 * 2304 + i]);
}

int bf_wgrad_grid(int B, int H, int W)
{
    const int ntiles = B * ((H + WG_TH - 1) / WG_TH) * ((W + WG_TW - 1) / WG_TW);
    return ntiles < 512 ? ntiles : 512;
}

hipError_t bf_launch_wgrad3x3_c16(const float* x, const float* dy, float* partial, float* dw,
                                  int B, int H, int W, hipStream_t s)
{
    const int tiles_x = (W + WG_TW - 1) / WG_TW, tiles_y = (H + WG_TH - 1) / WG_TH;
    const int ntiles = B * tiles_x * tiles_y;
    const int grid = bf_wgrad_grid(B, H, W);
    constexpr int lds_bytes = (WG_IH * WG_IW + WG_TH * WG_TW) * 16 * 4;   // 71,936
    {
        const hipError_t ea = bf_set_max_lds(reinterpret_cast<const void*>(wgrad3x3_c16_kernel), lds_bytes);      // once per device
        if (ea != hipSuccess) return ea;
    }
    hipLaunchKernelGGL(wgrad3x3_c16_kernel, dim3(grid), dim3(256), lds_bytes, s, x, dy, partial, B, H, W,
                       tiles_x, tiles_y, ntiles);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return bf_launch_reduce_partials(partial, grid, 2304, dw, 1.0f, s);
}
