// Single-kernel entry points for tests/ and the timing tools (include/bfcnn_hip_debug.h).  They take no handle and need nothing from
// the engine: each packs its own weights into the caller's scratch buffer and calls one launcher of bf_common.h.
#include "bf_common.h"
#include "h3_weights.h"
#include <cstring>

// ------------------------------------------------------------------------------------------
// diagnostics used by tests/ (single-kernel entry points; not part of the drop-in surface)
// ------------------------------------------------------------------------------------------
extern "C" int bf_debug_conv3x3(const float* in, const float* w_hwio, float* out, const float* scale, const float* shift,
                                const float* res, const float* mask, float* stats, float* wpack_scratch, int B, int H, int W,
                                int epi, int transpose_flip, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (bf_launch_pack_conv(w_hwio, wpack_scratch, transpose_flip, s) != hipSuccess) return BF_EHIP;
    ConvArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.in = in; ca.out = out; ca.wpack = wpack_scratch; ca.scale = scale; ca.shift = shift; ca.res = res; ca.mask = mask;
    ca.stats = stats; ca.B = B; ca.H = H; ca.W = W;
    return bf_launch_conv3x3_c16(ca, epi, s) == hipSuccess ? BF_OK : BF_EHIP;
}

static unsigned long long* g_fused_dbg = nullptr;
// diagnostic builds (H3_ABLATE=32, tools/stamp_h3.py and its siblings): device buffer of 512*8*8 u64 that receives per-wave phase cycle sums
extern "C" int bf_debug_set_fused_dbg(void* buf) { g_fused_dbg = (unsigned long long*)buf; return BF_OK; }

extern "C" int bf_debug_conv3x3_grid(int B, int H, int W) { return bf_conv3x3_c16_grid(B, H, W); }

extern "C" int bf_debug_fused_block(const float* in, const float* w1_hwio, const float* w2_hwio, const float* scale,
                                    const float* shift, float* out, float* wpack_scratch, int B, int H, int W, int act1_relu,
                                    void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (bf_launch_pack_conv(w1_hwio, wpack_scratch, 0, s) != hipSuccess) return BF_EHIP;
    if (bf_launch_pack_conv(w2_hwio, wpack_scratch + BF_WPACK_FLOATS, 0, s) != hipSuccess) return BF_EHIP;
    if (bf_launch_zero(wpack_scratch + 2 * BF_WPACK_FLOATS, 64, s) != hipSuccess) return BF_EHIP;
    FusedBlockArgs fa;
    fa.zeros = wpack_scratch + 2 * BF_WPACK_FLOATS;
    fa.in = in; fa.out = out; fa.w1pack = wpack_scratch; fa.w2pack = wpack_scratch + BF_WPACK_FLOATS; fa.scale = scale;
    fa.shift = shift; fa.B = B; fa.H = H; fa.W = W; fa.tiles_x = fa.tiles_y = fa.ntiles = 0; fa.act1_relu = act1_relu;
    return bf_launch_fused_block(fa, s) == hipSuccess ? BF_OK : BF_EHIP;
}

// split-f16 fused block on fp32 NHWC tensors: convert in, run, convert out.  scratch: float buffer of at least
// 2 * B*H*W*16 + BF_H3_BLOCK_FLOATS + 4608 + 32 + 64 + 128 floats (two split-planar activations, packed weights,
// the two HWIO kernels + gamma-free BN stand-in, zero line, dump line).
extern "C" int64_t bf_debug_fused_block_h3_scratch_floats(int B, int H, int W)
{
    return 2 * (int64_t)B * H * W * 16 + BF_H3_BLOCK_FLOATS + 4608 + 16 + 32 + 64 + 256;
}

extern "C" int bf_debug_fused_block_h3(const float* in, const float* w1_hwio, const float* w2_hwio, const float* scale,
                                       const float* shift, float* out, float* scratch, int B, int H, int W, int act1_relu,
                                       void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const int64_t act = (int64_t)B * H * W * 16;
    float* xa = scratch;
    float* ya = scratch + act;
    float* pk = ya + act;                          // BF_H3_BLOCK_FLOATS
    float* params = pk + BF_H3_BLOCK_FLOATS;       // [w1 2304][w2 2304][gamma 16]
    float* state = params + 4608 + 16;             // [mean 16][var 16]
    float* zeros = state + 32;                     // 64
    float* dump = zeros + 64;                      // 256
    // the caller's scale / shift stand in for the folded BN (ext_scale / ext_shift of the pack kernel)
    if (hipMemcpyAsync(params, w1_hwio, 2304 * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return BF_EHIP;
    if (hipMemcpyAsync(params + 2304, w2_hwio, 2304 * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return BF_EHIP;
    if (bf_launch_zero(zeros, 64, s) != hipSuccess) return BF_EHIP;
    if (bf_launch_pack_h3(params, state, 0, 4608 + 16, pk, BF_H3_BLOCK_FLOATS, 1, 0, 0.f, scale, shift, s) != hipSuccess) return BF_EHIP;
    if (bf_launch_h3_from_f32(in, xa, B, H, W, s) != hipSuccess) return BF_EHIP;
    FusedH3Args fa;
    fa.in = xa; fa.out = ya; fa.aux = pk;
    fa.w1r = fa.aux + 64; fa.w2r = fa.aux + 64 + BF_H3R_WPACK_FLOATS;
    fa.B = B; fa.H = H; fa.W = W; fa.tiles_x = fa.tiles_y = fa.ntiles = 0; fa.rows_per_tile = 0; fa.variant = -1; fa.reverse_tiles = 0; fa.act1_relu = act1_relu;
    fa.zeros = zeros; fa.dump = dump; fa.dbg = g_fused_dbg;
    fa.head_wh = nullptr; fa.head_out = nullptr; fa.head_u8 = 0; fa.Ho = fa.Wo = 0; fa.denormalize = 0; fa.v_min = fa.v_max = 0.f;
    fa.status = nullptr;
    if (bf_launch_fused_block_h3(fa, s) != hipSuccess) return BF_EHIP;
    return bf_launch_h3_to_f32(ya, out, B, H, W, s) == hipSuccess ? BF_OK : BF_EHIP;
}

// TWO split-f16 fused blocks in one launch (fused_h3w.hip) on fp32 NHWC tensors: convert in, run, convert out.
// w_hwio = [4][3][3][16][16] (conv1a, conv2a, conv1b, conv2b), scale / shift = [2][16] (block a, b).
extern "C" int64_t bf_debug_fused_block2_h3_scratch_floats(int B, int H, int W)
{
    return 2 * (int64_t)B * H * W * 16 + 2 * (int64_t)BF_H3_BLOCK_FLOATS + 2 * (4608 + 16) + 32 + 64;
}

extern "C" int bf_debug_fused_block2_h3(const float* in, const float* w_hwio, const float* scale, const float* shift, float* out,
                                        float* scratch, int B, int H, int W, int act1_relu, int reverse, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (!in || !w_hwio || !scale || !shift || !out || !scratch || B <= 0 || H <= 0 || W <= 0) return BF_EINVAL;
    const int64_t act = (int64_t)B * H * W * 16;
    float* xa = scratch;
    float* ya = scratch + act;
    float* pk = ya + act;                              // 2 x BF_H3_BLOCK_FLOATS
    float* params = pk + 2 * BF_H3_BLOCK_FLOATS;       // 2 x [w1 2304][w2 2304][gamma 16]
    float* state = params + 2 * (4608 + 16);           // [mean 16][var 16] (unused: the caller's scale / shift stand in)
    float* zeros = state + 32;                         // 64
    if (hipMemcpyAsync(params, w_hwio, 4608 * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return BF_EHIP;
    if (hipMemcpyAsync(params + 4608 + 16, w_hwio + 4608, 4608 * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return BF_EHIP;
    if (bf_launch_zero(zeros, 64, s) != hipSuccess) return BF_EHIP;
    for (int b = 0; b < 2; ++b)
        if (bf_launch_pack_h3(params + b * (4608 + 16), state, 0, 4608 + 16, pk + b * BF_H3_BLOCK_FLOATS, BF_H3_BLOCK_FLOATS, 1, 0,
                              0.f, scale + 16 * b, shift + 16 * b, s) != hipSuccess) return BF_EHIP;
    if (bf_launch_h3_from_f32(in, xa, B, H, W, s) != hipSuccess) return BF_EHIP;
    FusedH3WArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.in = xa; fa.out = ya;
    for (int b = 0; b < 2; ++b) {
        const float* aux = pk + b * BF_H3_BLOCK_FLOATS;
        fa.aux[b] = aux; fa.w1r[b] = aux + 64; fa.w2r[b] = aux + 64 + BF_H3R_WPACK_FLOATS;
    }
    fa.B = B; fa.H = H; fa.W = W; fa.reverse_tiles = reverse ? 1 : 0; fa.act1_relu = act1_relu;
    fa.zeros = zeros; fa.dbg = g_fused_dbg;
    if (bf_launch_fused_block2_h3w(fa, s) != hipSuccess) return BF_EHIP;
    return bf_launch_h3_to_f32(ya, out, B, H, W, s) == hipSuccess ? BF_OK : BF_EHIP;
}

extern "C" int bf_debug_set_h3_variant(int variant)
{
    bf_set_h3_variant(variant);
    return BF_OK;
}

// single split-f16 3x3 convolution on fp32 NHWC (the training convolution); scratch = 4 * BF_H3_TRAIN_PACK floats + 2304
extern "C" int64_t bf_debug_conv3x3_h3_scratch_floats(void) { return 4 * (int64_t)BF_H3_TRAIN_PACK_FLOATS + 2 * 2304 + 16; }
extern "C" int bf_debug_conv3x3_h3(const float* in, const float* w_hwio, float* out, const float* res, const float* mask,
                                   float* stats, float* scratch, int B, int H, int W, int epi, int transpose_flip, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    float* params = scratch + 4 * BF_H3_TRAIN_PACK_FLOATS;        // [w 2304][unused 2304][gamma 16]: one "layer"
    if (hipMemcpyAsync(params, w_hwio, 2304 * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return BF_EHIP;
    if (hipMemcpyAsync(params + 2304, w_hwio, 2304 * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return BF_EHIP;
    if (bf_launch_pack_h3_train(params, 0, 4608 + 16, scratch, 1, 2, 2320, s) != hipSuccess) return BF_EHIP;
    ConvArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.in = in; ca.out = out; ca.wpack = scratch + (transpose_flip ? 2 : 0) * BF_H3_TRAIN_PACK_FLOATS;
    ca.res = res; ca.mask = mask; ca.stats = stats; ca.B = B; ca.H = H; ca.W = W;
    return bf_launch_conv3x3_h3(ca, epi, s) == hipSuccess ? BF_OK : BF_EHIP;
}

// conv3x3_h3 with "affine + add on load": y = in + pre_scale * pre_c + pre_shift -> pre_out ; out = [relu] conv(y)
extern "C" int bf_debug_conv3x3_h3_pre(const float* in, const float* pre_c, const float* pre_scale, const float* pre_shift,
                                       float* pre_out, const float* w_hwio, float* out, float* scratch, int B, int H, int W, int relu,
                                       int reverse, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    float* params = scratch + 4 * BF_H3_TRAIN_PACK_FLOATS;
    if (hipMemcpyAsync(params, w_hwio, 2304 * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return BF_EHIP;
    if (hipMemcpyAsync(params + 2304, w_hwio, 2304 * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return BF_EHIP;
    if (bf_launch_pack_h3_train(params, 0, 4608 + 16, scratch, 1, 2, 2320, s) != hipSuccess) return BF_EHIP;
    ConvArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.in = in; ca.out = out; ca.wpack = scratch; ca.B = B; ca.H = H; ca.W = W; ca.reverse = reverse;
    ca.pre_c = pre_c; ca.pre_scale = pre_scale; ca.pre_shift = pre_shift; ca.pre_out = pre_out;
    return bf_launch_conv3x3_h3(ca, relu ? EPI_RELU : 0, s) == hipSuccess ? BF_OK : BF_EHIP;
}

// the training-mode forward of one [3,3] block in one kernel (train_fwd_h3t.hip): a_out = x + pre_scale * pre_c + pre_shift (pre_c
// given), t_out = [relu] conv_0(a) (t_out given), c_out = conv_1(t), stats[32] = per-channel sum | sum of squares of c_out.
// scratch: bf_debug_fwd_block_h3t_scratch_floats(B, H, W) floats
extern "C" int64_t bf_debug_fwd_block_h3t_scratch_floats(int B, int H, int W)
{
    return 4 * (int64_t)BF_H3_TRAIN_PACK_FLOATS + 2 * 2304 + 16 + (int64_t)bf_fwd_block_h3t_grid(B, H, W) * 32;
}
extern "C" int bf_debug_fwd_block_h3t(const float* x, const float* pre_c, const float* pre_scale, const float* pre_shift,
                                      const float* w0_hwio, const float* w1_hwio, float* a_out, float* t_out, float* c_out, float* stats,
                                      float* scratch, int B, int H, int W, int relu, int reverse, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (!bf_fwd_block_h3t_supports(H, W)) return BF_EUNSUPPORTED;
    float* params = scratch + 4 * BF_H3_TRAIN_PACK_FLOATS;
    if (hipMemcpyAsync(params, w0_hwio, 2304 * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return BF_EHIP;
    if (hipMemcpyAsync(params + 2304, w1_hwio, 2304 * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return BF_EHIP;
    if (bf_launch_pack_h3_train(params, 0, 4608 + 16, scratch, 1, 2, 2320, s) != hipSuccess) return BF_EHIP;
    float* partial = params + 2 * 2304 + 16;
    FwdBlockH3Args fa;
    memset(&fa, 0, sizeof(fa));
    fa.x = x; fa.pre_c = pre_c; fa.pre_scale = pre_scale; fa.pre_shift = pre_shift; fa.a_out = a_out; fa.t_out = t_out; fa.c_out = c_out;
    fa.wpack0 = scratch; fa.wpack1 = scratch + BF_H3_TRAIN_PACK_FLOATS; fa.stats = partial;
    fa.B = B; fa.H = H; fa.W = W; fa.reverse = reverse; fa.act_relu = relu;
    if (bf_launch_fwd_block_h3t(fa, s) != hipSuccess) return BF_EHIP;
    return bf_launch_reduce_partials(partial, bf_fwd_block_h3t_grid(B, H, W), 32, stats, 1.0f, s) == hipSuccess ? BF_OK : BF_EHIP;
}

// the backward of one [3,3] block in one kernel with T recomputed (train_bwd_h3t.hip): dc = k1 g + k2 c + k3 (coef = k1 | k2 | k3),
// T = [relu] conv_0(a), dw1 = T^T dc, dT = dgrad_1(dc) [* (T > 0)], dw0 = a^T dT, out = dgrad_0(dT) + g, stats[32] = sums of out |
// out * bnc (bnc given).  scratch: bf_debug_bwd_block_h3t_scratch_floats(B, H, W) floats
extern "C" int64_t bf_debug_bwd_block_h3t_scratch_floats(int B, int H, int W)
{
    return 4 * (int64_t)BF_H3_TRAIN_PACK_FLOATS + 2 * 2304 + 16 + (int64_t)bf_bwd_block_h3t_grid(B, H, W) * (2 * 2304 + 32);
}
extern "C" int bf_debug_bwd_block_h3t(const float* a_in, const float* g, const float* c, const float* coef, const float* w0_hwio,
                                      const float* w1_hwio, const float* bnc, float* out, float* dw1, float* dw0, float* stats,
                                      float* scratch, int B, int H, int W, int relu, int reverse, void* stream)
{
    // reverse: bit 0 = walk the bands bottom-up; bit 1 = the KERNEL ALONE (weights packed by an earlier call with the same scratch, no
    // reduction of the partials: bench.py's live timing of the launch)
    hipStream_t s = (hipStream_t)stream;
    if (!bf_bwd_block_h3t_supports(H, W)) return BF_EUNSUPPORTED;
    const bool alone = (reverse & 2) != 0;
    reverse &= 1;
    float* params = scratch + 4 * BF_H3_TRAIN_PACK_FLOATS;
    if (!alone) {
        if (hipMemcpyAsync(params, w0_hwio, 2304 * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return BF_EHIP;
        if (hipMemcpyAsync(params + 2304, w1_hwio, 2304 * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return BF_EHIP;
        if (bf_launch_pack_h3_train(params, 0, 4608 + 16, scratch, 1, 2, 2320, s) != hipSuccess) return BF_EHIP;
    }
    const int grid = bf_bwd_block_h3t_grid(B, H, W);
    float* wp1 = params + 2 * 2304 + 16;
    float* wp0 = wp1 + (int64_t)grid * 2304;
    float* st = wp0 + (int64_t)grid * 2304;
    BwdBlockH3Args fa;
    memset(&fa, 0, sizeof(fa));
    fa.a = a_in; fa.g = g; fa.c = c; fa.coef = coef; fa.bnc = bnc; fa.out = out;
    fa.wfwd0 = scratch; fa.wdg0 = scratch + 2 * BF_H3_TRAIN_PACK_FLOATS; fa.wdg1 = scratch + 3 * BF_H3_TRAIN_PACK_FLOATS;
    fa.wpartial1 = wp1; fa.wpartial0 = wp0; fa.stats = st;
    fa.B = B; fa.H = H; fa.W = W; fa.reverse = reverse; fa.act_relu = relu; fa.dbg = g_fused_dbg;
    if (bf_launch_bwd_block_h3t(fa, s) != hipSuccess) return BF_EHIP;
    if (alone) return BF_OK;
    if (bf_launch_reduce_partials(wp1, grid, 2304, dw1, 1.0f, s) != hipSuccess) return BF_EHIP;
    if (bf_launch_reduce_partials(wp0, grid, 2304, dw0, 1.0f, s) != hipSuccess) return BF_EHIP;
    if (bnc && stats && bf_launch_reduce_partials(st, grid, 32, stats, 1.0f, s) != hipSuccess) return BF_EHIP;
    return BF_OK;
}

// the fused backward kernel of one convolution (train_bwd_h3.hip): dw = x^T g', dx = dgrad(g') [* (x > 0) | + res], with
// g' = k1 g + k2 c + k3 when coef is given; stats (EPI_BNBWD): [grid][32] partials of (sum dx, sum dx * bnc).
// scratch: bf_debug_bwd3x3_h3_scratch_floats(B, H, W) floats
extern "C" int64_t bf_debug_bwd3x3_h3_scratch_floats(int B, int H, int W)
{
    return bf_debug_conv3x3_h3_scratch_floats() + (int64_t)bf_bwd3x3_h3_grid(B, H, W) * (2304 + 32);
}
extern "C" int bf_debug_bwd3x3_h3_grid(int B, int H, int W) { return bf_bwd3x3_h3_grid(B, H, W); }
// (dbuf selected the retired 512-thread form of the kernel: accepted and ignored, as is bit 1 of `reverse` below)
extern "C" int bf_debug_bwd3x3_h3_grid_ex(int B, int H, int W, int) { return bf_bwd3x3_h3_grid(B, H, W); }
extern "C" int bf_debug_bwd3x3_h3(const float* x, const float* g, const float* c, const float* coef, const float* w_hwio, float* out,
                                  const float* res, const float* bnc, float* dw, float* stats, float* scratch, int B, int H, int W,
                                  int epi, int reverse, int repack, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (repack) {
        float* params = scratch + 4 * BF_H3_TRAIN_PACK_FLOATS;
        if (hipMemcpyAsync(params, w_hwio, 2304 * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return BF_EHIP;
        if (hipMemcpyAsync(params + 2304, w_hwio, 2304 * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return BF_EHIP;
        if (bf_launch_pack_h3_train(params, 0, 4608 + 16, scratch, 1, 2, 2320, s) != hipSuccess) return BF_EHIP;
    }
    float* partial = scratch + bf_debug_conv3x3_h3_scratch_floats();
    BwdH3Args a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.g = g; a.c = c; a.coef = coef; a.wpack = scratch + 2 * BF_H3_TRAIN_PACK_FLOATS; a.out = out; a.res = res; a.bnc = bnc;
    a.wpartial = partial; a.stats = partial + (int64_t)bf_bwd3x3_h3_grid(B, H, W) * 2304;
    a.B = B; a.H = H; a.W = W; a.reverse = reverse & 1;                                    // reverse: bit 0 walk direction, bit 1 ignored
    if (bf_launch_bwd3x3_h3(a, epi, dw, s) != hipSuccess) return BF_EHIP;
    if (stats && (epi & EPI_BNBWD) &&
        hipMemcpyAsync(stats, a.stats, (size_t)bf_bwd3x3_h3_grid(B, H, W) * 32 * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
        return BF_EHIP;
    return BF_OK;
}

extern "C" int64_t bf_debug_wgrad_partial_floats(int B, int H, int W) { return (int64_t)bf_wgrad_grid(B, H, W) * 2304; }

extern "C" int bf_debug_wgrad3x3_h3(const float* x, const float* dy, float* partial, float* dw, int B, int H, int W, void* stream)
{
    return bf_launch_wgrad3x3_h3(x, dy, partial, dw, B, H, W, (hipStream_t)stream) == hipSuccess ? BF_OK : BF_EHIP;
}

extern "C" int bf_debug_wgrad3x3(const float* x, const float* dy, float* partial, float* dw, int B, int H, int W, void* stream)
{
    return bf_launch_wgrad3x3_c16(x, dy, partial, dw, B, H, W, (hipStream_t)stream) == hipSuccess ? BF_OK : BF_EHIP;
}

// the split-f16 weight scale as the kernels evaluate it (h3_weights.h), on the host
extern "C" float bf_debug_h3_weight_scale(float max_abs) { return bf_h3_weight_scale(max_abs); }

// raw MFMA layout probe: D = A(16x4) * B(4x16) with A[m][k] = a_in[m*4+k], B[k][n] = b_in[k*16+n]
__global__ void mfma_probe_kernel(const float* a_in, const float* b_in, float* d_out)
{
    const int l = threadIdx.x;
    const float a = a_in[(l & 15) * 4 + (l >> 4)];
    const float b = b_in[(l >> 4) * 16 + (l & 15)];
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) d_out[((l >> 4) * 4 + j) * 16 + (l & 15)] = acc[j];
}

extern "C" int bf_debug_mfma_probe(const float* a, const float* b, float* d, void* stream)
{
    hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a, b, d);
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}
