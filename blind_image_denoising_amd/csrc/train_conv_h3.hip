// Training convolutions with the split-f16 ("f16x3") arithmetic on fp32 NHWC tensors: the single 3x3 16->16 convolution
// (forward conv1 / conv2, data gradients), its weight packs and the weight gradient.  Arithmetic, K packing and the
// row-streaming inner loop (h3_rows.h) are those of the inference kernel: see the header of fused_h3.hip.
#include "bf_common.h"
#include "h3_core.h"
#include "h3_rows.h"
#include "h3_weights.h"

// ==========================================================================================================
// Single 3x3 16->16 convolution on fp32 NHWC tensors with the split-f16 arithmetic and the row-streaming inner loop of
// the fused inference kernels (fused_h3.hip): the training convolutions (forward conv1 / conv2, data gradients) -- same epilogue stages
// as conv3x3_c16_kernel ([ReLU] [mask] [+residual] [BN statistics]), same 16x32 tiles and grid, so it is a drop-in.
// The fp32 tile is split into hi / lo f16 planes while it is staged into LDS (8 vector instructions per 4 values);
// a wave streams 8 rows of one 16-column strip; the fp32 result goes straight from the accumulator to HBM.
// 15 MFMAs of 16 cycles per 16 pixels instead of 36 MFMAs of 32 cycles.
// ==========================================================================================================
struct ConvH3Geom {
    static constexpr int TH = 16, TW = 32, IH = TH + 2, IW = TW + 2, R = 8;
    static constexpr int PLANE = (IH * IW * 16 + 255) / 256 * 256;
    static constexpr int LDS_BYTES = 4 * PLANE;
};

template <int EPI, bool PRE = false>
__global__ __launch_bounds__(256, 2) void conv3x3_h3_kernel(ConvArgs a)
{
    using G = ConvH3Geom;
    __shared__ __attribute__((aligned(16))) char tile[G::LDS_BYTES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, q = lane >> 4;
    const int tiles_x = (a.W + G::TW - 1) / G::TW, tiles_y = (a.H + G::TH - 1) / G::TH;
    int t = a.reverse ? (int)gridDim.x - 1 - (int)blockIdx.x : (int)blockIdx.x;
    const int tx = t % tiles_x; t /= tiles_x;
    const int ty = t % tiles_y;
    const int b = t / tiles_y;
    const int y0 = ty * G::TH, x0 = tx * G::TW;
    const size_t img = (size_t)b * a.H * a.W * 16;

    // weights: 12 A-operand images + 1/s (pack_h3_train_kernel)
    h8 w[13];
#pragma unroll
    for (int i = 0; i < 12; ++i) w[i] = reinterpret_cast<const h8*>(a.wpack)[i * 64 + lane];
    w[12] = w[0];
    const float inv_s = a.wpack[BF_H3R_WPACK_FLOATS];

    // stage: fp32 NHWC (1-pixel halo, zero outside the image) -> hi / lo planes [4][IH][IW][8 x f16].  All the loads of a
    // thread are issued before the first one is consumed (a rolled load -> split -> store loop pays one memory round trip
    // per element: hipcc does not pipeline it)
    {
        constexpr int NX = (G::IH * G::IW * 4 + 255) / 256;
        f32x4 rx[NX], rc[PRE ? NX : 1];
        f32x4 psc = {0.f, 0.f, 0.f, 0.f}, psh = {0.f, 0.f, 0.f, 0.f};
        if (PRE) {                              // tid & 3 is the channel quad of every element this thread stages
            psc = *reinterpret_cast<const f32x4*>(a.pre_scale + (tid & 3) * 4);
            psh = *reinterpret_cast<const f32x4*>(a.pre_shift + (tid & 3) * 4);
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const int e = tid + i * 256;
            const int px = e >> 2, quad = e & 3;
            const int row = px / G::IW, col = px - row * G::IW;
            const int gy = y0 - 1 + row, gx = x0 - 1 + col;
            rx[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (PRE) rc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (e < G::IH * G::IW * 4 && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
                const size_t idx = img + ((size_t)gy * a.W + gx) * 16 + quad * 4;
                rx[i] = *reinterpret_cast<const f32x4*>(a.in + idx);
                if (PRE) rc[i] = *reinterpret_cast<const f32x4*>(a.pre_c + idx);
            }
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const int e = tid + i * 256;
            if (e < G::IH * G::IW * 4) {
                const int px = e >> 2, quad = e & 3;
                f32x4 v = rx[i];
                if (PRE) {
                    // y = x + (scale * c + shift) as affine_add_kernel rounds it; 0 outside the image (SAME padding); the tile's
                    // own pixels (not the halo, which the neighbours own) go back to HBM: the block input the backward pass needs
                    const int row = px / G::IW, col = px - row * G::IW;
                    const int gy = y0 - 1 + row, gx = x0 - 1 + col;
                    const bool in = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = in ? rx[i][k] + fmaf(psc[k], rc[i][k], psh[k]) : 0.f;
                    if (in && row >= 1 && row <= G::TH && col >= 1 && col <= G::TW)
                        *reinterpret_cast<f32x4*>(a.pre_out + img + ((size_t)gy * a.W + gx) * 16 + quad * 4) = v;
                }
                h4 hi, lo;
                h3_split(v, hi, lo);
                char* p = tile + (quad >> 1) * G::PLANE + px * 16 + (quad & 1) * 8;
                *reinterpret_cast<h4*>(p) = hi;
                *reinterpret_cast<h4*>(p + 2 * G::PLANE) = lo;
            }
        }
    }
    __syncthreads();

    const int strip = wave & 1, half = wave >> 1;
    const int px_l = strip * 16 + n;                              // column inside the tile
    const int o0 = half * G::R;                                   // first output row of this wave
    const int b1 = (q & 1) * G::PLANE + (o0 * G::IW + px_l) * 16;
    const int gx = x0 + px_l;
    struct Epi {
        struct Pre {};
        enum { EXTRA_MFMA = 0 };
        const ConvArgs& a; size_t base; int gy0, gx, q; float inv_s; f32x4 sc, sh;
        f32x4* s1; f32x4* s2;
        __device__ __forceinline__ Pre pre(const int) const { return Pre{}; }
        __device__ __forceinline__ f32x4 finish(const int, const f32x4 acc, const Pre&) const { return acc; }
        __device__ __forceinline__ void operator()(const int o, const f32x4 acc) const
        {
            if (gy0 + o < a.H && gx < a.W) {
                const size_t idx = base + (size_t)o * a.W * 16;
                f32x4 v = acc * inv_s;
                if (EPI & EPI_STATS) { *s1 += v; *s2 += v * v; }
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
                if (EPI & EPI_BNBWD) { *s1 += v; *s2 += v * *reinterpret_cast<const f32x4*>(a.bnc + idx); }
                *reinterpret_cast<f32x4*>(a.out + idx) = v;
            }
        }
    };
    f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
    f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
    if (EPI & EPI_AFFINE) {
        sc = *reinterpret_cast<const f32x4*>(a.scale + q * 4);
        sh = *reinterpret_cast<const f32x4*>(a.shift + q * 4);
    }
    const Epi epi{a, img + ((size_t)(y0 + o0) * a.W + gx) * 16 + q * 4, y0 + o0, gx, q, inv_s, sc, sh, &s1, &s2};
    h3r_rows<G::R, G::IW * 16, 2 * G::PLANE>(tile, b1 + (q >> 1) * 16, b1 + 32 + (q >> 1) * 2 * G::PLANE, w, epi, H3NoHook{});

    if (EPI & (EPI_STATS | EPI_BNBWD)) {
        // reduce over the 16 pixel lanes that share a channel quad, then over the 4 waves (fixed order)
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                s1[c] += __shfl_xor(s1[c], m);
                s2[c] += __shfl_xor(s2[c], m);
            }
        }
        __syncthreads();                       // tile no longer needed
        float* red = reinterpret_cast<float*>(tile);      // [4 waves][32]
        if (n == 0) {
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

hipError_t bf_launch_conv3x3_h3(const ConvArgs& a, int epi, hipStream_t s)
{
    const dim3 grid(bf_conv3x3_c16_grid(a.B, a.H, a.W)), block(256);
    if (a.pre_c) {
        // affine + add on load: in front of a block's first convolution only ([activation] epilogue)
        if (!a.pre_scale || !a.pre_shift || !a.pre_out || a.pre_out == a.in || a.pre_out == a.pre_c) return hipErrorInvalidValue;
        if (epi == EPI_RELU) hipLaunchKernelGGL((conv3x3_h3_kernel<EPI_RELU, true>), grid, block, 0, s, a);
        else if (epi == 0) hipLaunchKernelGGL((conv3x3_h3_kernel<0, true>), grid, block, 0, s, a);
        else return hipErrorInvalidValue;
        return hipGetLastError();
    }
#define BF_CASE(E) case E: hipLaunchKernelGGL(conv3x3_h3_kernel<E>, grid, block, 0, s, a); break;
    switch (epi) {
        BF_CASE(0)
        BF_CASE(EPI_RELU)
        BF_CASE(EPI_STATS)
        BF_CASE(EPI_RES)
        BF_CASE(EPI_RES | EPI_BNBWD)
        BF_CASE(EPI_MASK)
        default: return hipErrorInvalidValue;
    }
#undef BF_CASE
    return hipGetLastError();
}

// training packs: one workgroup per (layer, which) with which = 0 w1 forward, 1 w2 forward, 2 w1 data gradient,
// 3 w2 data gradient (W'[tap][ci][co] = W[8-tap][co][ci]); row layout of the fused kernels without BN folding or
// identity; dst = [12 x 64 x 16 B][1/s broadcast x 64 floats]
__global__ __launch_bounds__(256) void pack_h3_train_kernel(const float* __restrict__ params, int64_t p_blocks, int64_t p_stride,
                                                            float* __restrict__ dst, int64_t d_stride, int nconv, int unit)
{
    // blockIdx.x = layer * 2 * nconv + which ; which < nconv: forward pack of convolution `which`, else the data-gradient pack
    // of convolution which - nconv.  Convolution j of a block sits at j * 2304 (+ (j - 1) * 16 behind the gammas: unit = 2320)
    __shared__ float red[256];
    const int per = 2 * nconv;
    const int layer = blockIdx.x / per, which = blockIdx.x % per;
    const int cj = which % nconv;
    const float* w = params + p_blocks + layer * p_stride + (cj == 0 ? 0 : 2304 + (int64_t)(cj - 1) * unit);
    const int tf = which / nconv;
    const float sr = bf_h3_block_weight_scale<256>([&](const int i) { return w[i]; }, 2304, red);
    float* out = dst + ((int64_t)layer * per + which) * d_stride;
    _Float16* orow = reinterpret_cast<_Float16*>(out);
    for (int idx = threadIdx.x; idx < 12 * 64 * 8; idx += 256) {
        int tap, part, cin, cout;
        bf_h3_row_operand(idx, tap, part, cin, cout);
        const float wv = tf ? w[((8 - tap) * 16 + cout) * 16 + cin] : w[(tap * 16 + cin) * 16 + cout];
        _Float16 hi, lo;
        bf_h3_split(wv * sr, hi, lo);
        orow[idx] = part == 0 ? hi : (part == 1 ? lo : (_Float16)0.f);
    }
    for (int idx = 12 * 64 * 8 + threadIdx.x; idx < 13 * 64 * 8; idx += 256) orow[idx] = (_Float16)0.f;     // unused 13th image
    if (threadIdx.x < 64) out[BF_H3R_WPACK_FLOATS + threadIdx.x] = 1.0f / sr;
}

hipError_t bf_launch_pack_h3_train(const float* params, int64_t p_blocks, int64_t p_stride, float* dst, int layers, int nconv,
                                   int unit, hipStream_t s)
{
    if (layers <= 0) return hipSuccess;
    hipLaunchKernelGGL(pack_h3_train_kernel, dim3(layers * 2 * nconv), dim3(256), 0, s, params, p_blocks, p_stride, dst,
                       (int64_t)BF_H3_TRAIN_PACK_FLOATS, nconv, unit);
    return hipGetLastError();
}

// ==========================================================================================================
// Weight gradient of the 3x3 16->16 convolution with the split-f16 arithmetic:
//   dW[tap][ci][co] = sum over pixels of X[pixel + tap][ci] * dY[pixel][co]
//                   ~ X_hi.dY_hi + X_lo.dY_hi + X_hi.dY_lo                       (fp32 accumulation)
// GEMM view per tap: M = ci, N = co, K = pixels, 32 pixels (one tile row) per v_mfma_f32_16x16x32_f16.  Both operands
// need the PIXEL index along K while the tiles are pixel-major in memory: the LDS images stay [pixel][16 channels]
// (32 B per pixel, written with 8-byte stores while the fp32 tile is split) and ds_read_b64_tr_b16 delivers them
// transposed -- lane 16g+i receives channel i of pixels 4g..4g+3 -- two reads per operand and K chunk (k-slots 0..3 of
// lane group g = pixels 4g..4g+3, k-slots 4..7 = pixels 16+4g..16+4g+3: the two 32-lane halves of a read touch
// disjoint 256-B windows, no bank conflicts).  27 MFMAs of 16 cycles per 32 pixels instead of 72 of 32 cycles, and 40
// LDS reads instead of 80.  Nine accumulators stay in registers across the tiles of a persistent workgroup; partials
// are reduced in a fixed order (no float atomics -> bitwise reproducible), exactly as wgrad3x3_c16_kernel does.
// ==========================================================================================================
typedef __fp16 fp16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));

struct WgradH3Geom {
    static constexpr int TH = 16, TW = 32, IH = TH + 2, IW = TW + 2;
    static constexpr int X_IMG = IH * IW * 32, D_IMG = TH * TW * 32;       // bytes per f16 image
    static constexpr int LDS_BYTES = 2 * X_IMG + 2 * D_IMG;                // 71,936
};

__device__ __forceinline__ h8 h3_tr_operand(const char* img, const int addr)
{
    typedef unsigned u2 __attribute__((ext_vector_type(2)));
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    const fp16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4*)(img + addr));
    const fp16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4*)(img + addr + 16 * 32));
    const u2 ua = __builtin_bit_cast(u2, a), ub = __builtin_bit_cast(u2, b);
    return __builtin_bit_cast(h8, (u4){ua[0], ua[1], ub[0], ub[1]});
}

__global__ __launch_bounds__(256, 2) void wgrad3x3_h3_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                             float* __restrict__ partial, int B, int H, int W, int tiles_x,
                                                             int tiles_y, int ntiles)
{
    using G = WgradH3Geom;
    extern __shared__ __attribute__((aligned(16))) char wg_lds[];
    char* xh = wg_lds;                      // [IH][IW][16] f16 hi
    char* xl = wg_lds + G::X_IMG;           // lo
    char* dh = wg_lds + 2 * G::X_IMG;       // [TH][TW][16] f16 hi
    char* dl = dh + G::D_IMG;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // transposed-read address of this lane inside a 32-pixel row chunk: pixel 4g + q', channels 4p'..4p'+3
    const int tr_off = (4 * (lane >> 4) + ((lane & 15) >> 2)) * 32 + (lane & 3) * 8;
    f32x4 acc[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // The fp32 elements of a tile are fetched into registers one tile ahead (NX + ND 16-byte loads per thread) and split /
    // written to LDS after the matrix work of the previous tile: the global-memory latency of tile t+1 hides behind the
    // MFMAs of tile t inside the workgroup, instead of relying on the second workgroup of the CU alone.
    constexpr int NX = (G::IH * G::IW * 4 + 255) / 256, ND = G::TH * G::TW * 4 / 256;
    f32x4 rx[NX], rd[ND];
    auto fetch = [&](const int t) {
        int tt = t;
        const int txi = tt % tiles_x; tt /= tiles_x;
        const int tyi = tt % tiles_y;
        const int b = tt / tiles_y;
        const int y0 = tyi * G::TH, x0 = txi * G::TW;
        const size_t img = (size_t)b * H * W * 16;
#pragma unroll
        for (int i = 0; i < NX; ++i) {                     // x with a 1-pixel halo (zero outside the image)
            const int e = tid + i * 256;
            const int px = e >> 2, quad = e & 3;
            const int row = px / G::IW, col = px - row * G::IW;
            const int gy = y0 - 1 + row, gx = x0 - 1 + col;
            rx[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (e < G::IH * G::IW * 4 && gy >= 0 && gy < H && gx >= 0 && gx < W)
                rx[i] = *reinterpret_cast<const f32x4*>(x + img + ((size_t)gy * W + gx) * 16 + quad * 4);
        }
#pragma unroll
        for (int i = 0; i < ND; ++i) {                     // dy (zero outside the image)
            const int e = tid + i * 256;
            const int px = e >> 2, quad = e & 3;
            const int row = px / G::TW, col = px - row * G::TW;
            const int gy = y0 + row, gx = x0 + col;
            rd[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (gy < H && gx < W) rd[i] = *reinterpret_cast<const f32x4*>(dy + img + ((size_t)gy * W + gx) * 16 + quad * 4);
        }
    };
    if ((int)blockIdx.x < ntiles) fetch(blockIdx.x);
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        // split + store the prefetched tile
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const int e = tid + i * 256;
            if (e < G::IH * G::IW * 4) {
                h4 hi, lo;
                h3_split(rx[i], hi, lo);
                *reinterpret_cast<h4*>(xh + (e >> 2) * 32 + (e & 3) * 8) = hi;
                *reinterpret_cast<h4*>(xl + (e >> 2) * 32 + (e & 3) * 8) = lo;
            }
        }
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            const int e = tid + i * 256;
            h4 hi, lo;
            h3_split(rd[i], hi, lo);
            *reinterpret_cast<h4*>(dh + (e >> 2) * 32 + (e & 3) * 8) = hi;
            *reinterpret_cast<h4*>(dl + (e >> 2) * 32 + (e & 3) * 8) = lo;
        }
        __syncthreads();
        if (t + (int)gridDim.x < ntiles) fetch(t + gridDim.x);
        // wave handles rows 4w .. 4w+3 of the tile: four K chunks of 32 pixels
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int r = 4 * wave + rr;
            const h8 bh = h3_tr_operand(dh, r * G::TW * 32 + tr_off);
            const h8 bl = h3_tr_operand(dl, r * G::TW * 32 + tr_off);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int ax = ((r + tap / 3) * G::IW + tap % 3) * 32 + tr_off;
                const h8 ah = h3_tr_operand(xh, ax);
                const h8 al = h3_tr_operand(xl, ax);
                acc[tap] = MFMA_H(ah, bh, acc[tap]);
                acc[tap] = MFMA_H(al, bh, acc[tap]);
                acc[tap] = MFMA_H(ah, bl, acc[tap]);
            }
        }
        __syncthreads();
    }
    // cross-wave reduction through LDS: [4][9][256], D[ci = 4q + j][co = p] per lane
    float* red = reinterpret_cast<float*>(wg_lds);
    const int p = lane & 15, q = lane >> 4;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const f32x4 v = bf_acc_ready(acc[tap]);
#pragma unroll
        for (int j = 0; j < 4; ++j) red[(wave * 9 + tap) * 256 + (4 * q + j) * 16 + p] = v[j];
    }
    __syncthreads();
    for (int i = tid; i < 2304; i += 256)
        partial[(size_t)blockIdx.x * 2304 + i] = (red[i] + red[2304 + i]) + (red[2 * 2304 + i] + red[3 * 2304 + i]);
}

hipError_t bf_launch_wgrad3x3_h3(const float* x, const float* dy, float* partial, float* dw, int B, int H, int W, hipStream_t s)
{
    using G = WgradH3Geom;
    const int tiles_x = (W + G::TW - 1) / G::TW, tiles_y = (H + G::TH - 1) / G::TH;
    const int ntiles = B * tiles_x * tiles_y;
    const int grid = bf_wgrad_grid(B, H, W);
    {
        const hipError_t ea = bf_set_max_lds(reinterpret_cast<const void*>(wgrad3x3_h3_kernel), G::LDS_BYTES);      // once per device
        if (ea != hipSuccess) return ea;
    }
    hipLaunchKernelGGL(wgrad3x3_h3_kernel, dim3(grid), dim3(256), G::LDS_BYTES, s, x, dy, partial, B, H, W, tiles_x, tiles_y, ntiles);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return bf_launch_reduce_partials(partial, grid, 2304, dw, 1.0f, s);
}
