// Inference half of the C-ABI engine: the packed-weight images (bf_pack_inference), the forward plan -- every choice a forward
// makes, made once per call by host arithmetic alone -- and the launcher that carries a plan out (bf_forward_*).
#include "engine.h"
#include <cstdio>
#include <cstring>

// ---- tiny pack kernels ---------------------------------------------------------------------
__global__ void pack_all_convs_kernel(const float* __restrict__ params, int64_t p_blocks, int64_t p_stride, float* __restrict__ dst,
                                      int64_t d_stride, int with_dgrad, int nconv, int unit)
{
    // blockIdx.x = layer * (with_dgrad ? 2 : 1) * nconv + which ; which < nconv: forward pack of convolution `which`, else the
    // data-gradient pack of convolution which - nconv (convolution j of a block at j * 2304, + (j - 1) * 16 behind gammas)
    const int per = (with_dgrad ? 2 : 1) * nconv;
    const int layer = blockIdx.x / per, which = blockIdx.x % per;
    const int cj = which % nconv;
    const float* w = params + p_blocks + layer * p_stride + (cj == 0 ? 0 : 2304 + (int64_t)(cj - 1) * unit);
    float* o = dst + layer * d_stride + which * (with_dgrad ? (int64_t)BF_TRAIN_PACK_STRIDE : (int64_t)BF_WPACK_FLOATS);
    const int tf = which / nconv;
    for (int idx = threadIdx.x; idx < BF_WPACK_FLOATS; idx += blockDim.x) {
        const int i = idx >> 6, l = idx & 63;
        const int tap = i >> 2, kk = i & 3;
        const int cin = 4 * (l >> 4) + kk, cout = l & 15;
        o[idx] = tf ? w[((8 - tap) * 16 + cout) * 16 + cin] : w[(tap * 16 + cin) * 16 + cout];
    }
}

// one workgroup per (layer, pack): layers * nconv forward packs, and as many data-gradient packs with with_dgrad
hipError_t bf_launch_pack_all_convs(const float* params, int64_t p_blocks, int64_t p_stride, float* dst, int64_t d_stride, int layers,
                                    int with_dgrad, int nconv, int unit, hipStream_t s)
{
    hipLaunchKernelGGL(pack_all_convs_kernel, dim3(layers * (with_dgrad ? 2 : 1) * nconv), dim3(256), 0, s, params, p_blocks, p_stride, dst,
                       d_stride, with_dgrad, nconv, unit);
    return hipGetLastError();
}

// folded inference BN: keras BatchNormalization(training=False): gamma*(x-mean)*rsqrt(var+eps)
__global__ void fold_bn_kernel(const float* __restrict__ params, const float* __restrict__ state, int64_t p_blocks, int64_t p_stride,
                               float* __restrict__ packed, int64_t k_blocks, int64_t k_stride, int layers, int use_bn, float eps)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= layers * 16) return;
    const int layer = i / 16, c = i % 16;
    float sc = 1.f, sh = 0.f;
    if (use_bn) {
        const float g = params[p_blocks + layer * p_stride + 4608 + c];
        const float mean = state[layer * 32 + c], var = state[layer * 32 + 16 + c];
        sc = g / sqrtf(var + eps);
        sh = -sc * mean;
    }
    float* o = packed + k_blocks + layer * k_stride + 2 * BF_WPACK_FLOATS;
    o[c] = sc;
    o[16 + c] = sh;
}

__global__ void pack_edges_kernel(const float* __restrict__ params, float* __restrict__ packed, int64_t p_base, int64_t n_base,
                                  int64_t p_head0, int64_t p_head1, int hf, int co, int64_t k_base, int64_t k_w0, int64_t k_w1,
                                  int64_t k_wh)
{
    for (int i = threadIdx.x; i < n_base; i += blockDim.x) packed[k_base + i] = params[p_base + i];
    for (int i = threadIdx.x; i < 16 * hf; i += blockDim.x) packed[k_w0 + i] = params[p_head0 + i];
    for (int i = threadIdx.x; i < hf * co; i += blockDim.x) packed[k_w1 + i] = params[p_head1 + i];
    if (threadIdx.x < 64) {
        const int c = threadIdx.x >> 2, o = threadIdx.x & 3;
        float s = 0.f;
        if (o < co)
            for (int j = 0; j < hf; ++j) s = fmaf(params[p_head0 + c * hf + j], params[p_head1 + j * co + o], s);
        packed[k_wh + threadIdx.x] = s;
        packed[k_wh + 64 + threadIdx.x] = 0.f;     // k_zero line (directly behind k_wh)
    }
}

// block_kernels of length 1 or 3: per block [nb weight images][nb x (scale16, shift16)]
__global__ void pack_generic_blocks_kernel(const float* __restrict__ params, const float* __restrict__ state, int64_t p_blocks,
                                           int64_t p_stride, float* __restrict__ dst, int64_t d_stride, int nb, int use_bn, float eps)
{
    const int layer = blockIdx.x / nb, j = blockIdx.x % nb;
    const int64_t conv_off = (int64_t)j * 2304 + (use_bn && j >= 2 ? (j - 1) * 16 : 0);   // gamma j-1 sits before conv j (j >= 2)
    const float* w = params + p_blocks + layer * p_stride + conv_off;
    float* o = dst + layer * d_stride + (int64_t)j * BF_WPACK_FLOATS;
    for (int idx = threadIdx.x; idx < BF_WPACK_FLOATS; idx += blockDim.x) {
        const int i = idx >> 6, l = idx & 63;
        const int tap = i >> 2, kk = i & 3;
        const int cin = 4 * (l >> 4) + kk, cout = l & 15;
        o[idx] = w[(tap * 16 + cin) * 16 + cout];
    }
    if (threadIdx.x < 16) {
        const int c = threadIdx.x;
        float sc = 1.f, sh = 0.f;
        if (use_bn && j >= 1) {
            const float g = w[2304 + c];                                   // gamma follows its convolution
            const float* st = state + ((int64_t)layer * (nb - 1) + (j - 1)) * 32;
            sc = g / sqrtf(st[16 + c] + eps);
            sh = -sc * st[c];
        }
        float* aff = dst + layer * d_stride + (int64_t)nb * BF_WPACK_FLOATS + j * 32;
        aff[c] = sc;
        aff[16 + c] = sh;
    }
}

extern "C" int bf_pack_inference(bf_handle h, const float* params, const float* state, void* packed, void* stream)
{
    if (!h) return BF_EINVAL;
    if (!params || !packed || (h->n_state > 0 && !state)) return fail(h, BF_EINVAL, "bf_pack_inference: NULL buffer");
    if ((uintptr_t)packed % 16) return fail(h, BF_EWORKSPACE, "packed buffer must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    float* pk = (float*)packed;
    const bf_resnet_desc& d = h->d;
    if (d.no_layers > 0 && d.block_convs != 2) {
        hipLaunchKernelGGL(pack_generic_blocks_kernel, dim3(d.no_layers * d.block_convs), dim3(256), 0, s, params, state, h->p_blocks,
                           h->p_block_stride, pk + h->k_blocks, h->k_block_stride, d.block_convs, d.use_bn, d.bn_eps);
        BF_HIP(hipGetLastError(), "pack_generic_blocks");
    } else if (d.no_layers > 0) {
        BF_HIP(bf_launch_pack_all_convs(params, h->p_blocks, h->p_block_stride, pk + h->k_blocks, h->k_block_stride, d.no_layers, 0, 2,
                                        2320, s), "pack_all_convs");
        hipLaunchKernelGGL(fold_bn_kernel, dim3((d.no_layers * 16 + 255) / 256), dim3(256), 0, s, params, state, h->p_blocks,
                           h->p_block_stride, pk, h->k_blocks, h->k_block_stride, d.no_layers, d.use_bn, d.bn_eps);
        BF_HIP(hipGetLastError(), "fold_bn");
        BF_HIP(bf_launch_pack_h3(params, state, h->p_blocks, h->p_block_stride, pk + h->k_h3, BF_H3_BLOCK_FLOATS, d.no_layers,
                                 d.use_bn, d.bn_eps, nullptr, nullptr, s), "pack_h3");
    }
    hipLaunchKernelGGL(pack_edges_kernel, dim3(1), dim3(256), 0, s, params, pk, h->p_base, h->n_base, h->p_head0, h->p_head1,
                       d.head_filters, d.out_channels, h->k_base, h->k_w0, h->k_w1, h->k_wh);
    BF_HIP(hipGetLastError(), "pack_edges");
    return BF_OK;
}

// ------------------------------------------------------------------------------------------
// inference: the plan
// ------------------------------------------------------------------------------------------
// The five ways a forward runs residual blocks; each has one launcher below.
enum class StepKind {
    Pair,           // two split-f16 blocks in one launch (fused_h3w.hip)
    H3Single,       // one split-f16 block (fused_h3.hip / fused_h3v.hip: ForwardStep::h3)
    Fp32Fused,      // one exact-fp32 fused block (conv3x3_c16.hip)
    GeneralConvs,   // a block of 1 or 3 convolutions, one launch each
    Unfused,        // a [3,3] block as two convolution launches
};
constexpr int STEP_KINDS = 5;

struct ForwardStep {
    int first, blocks;      // runs blocks [first, first + blocks)
    int launches;           // kernel launches it makes
    StepKind kind;
    H3Kernel h3;            // H3Single: the kernel chosen for exactly this launch
    bool reverse;           // split-f16 kernels: walk the bands last to first
    bool head;              // the launch also runs the head (always the last step)
    const char* kernel_name() const
    {
        switch (kind) {
        case StepKind::Pair: return "fused_block2_h3w_kernel";
        case StepKind::H3Single: return bf_fused_block_h3_kernel_name(h3);
        case StepKind::Fp32Fused: return bf_fused_block_kernel_name();
        default: return "conv3x3_c16_kernel";
        }
    }
};

// Everything a forward of B images of H x W (padded size) decides, from the model, the handle's options and the shape alone.
// A value: no pointer into the call, no allocation.  The steps are a function of the block index (next), so any depth fits.
struct ForwardPlan {
    int N = 0, block_convs = 2;
    bool h3 = false;            // split-f16 blocks: the activations are split-planar between the base convolution and the head
    bool compact = false;       // ... in the compact layout: every block runs the full-row streaming kernel
    bool pair_ok = false;       // consecutive blocks run two per launch
    bool head_in_block = false; // the last block's epilogue runs the head
    bool head_in_pair = false;  // the last pair launch runs the head
    int split = 0;              // BaseConvArgs::out_split = HeadArgs::feat_split: 0 fp32, 1 split-planar, 2 compact
    bool zigzag = false;
    StepKind single_kind = StepKind::H3Single;  // how a block that is not in a pair runs
    H3Choice single = {H3Kernel::Tiles32, false}, last_single = {H3Kernel::Tiles32, false};   // H3Single: a block alone / carrying the head
    int launches = 0;           // block launches of the forward and the kernel that runs most of its blocks (bf_get_block_kernel)
    const char* dominant = "";

    bool head_kernel() const { return !head_in_block && !head_in_pair; }
    // the step that starts at block i, the forward having made `launch` block launches before it
    ForwardStep next(int i, int launch) const
    {
        ForwardStep st;
        st.first = i; st.blocks = 1; st.launches = 1; st.kind = single_kind; st.h3 = single.kernel; st.reverse = false; st.head = false;
        const bool zz = zigzag && (launch & 1);
        // an odd block count runs its single block FIRST, so that the last launch is a pair and can carry the head; the block in
        // front of one that carries the head itself stays single
        if (pair_ok && i + 1 < N && !(head_in_block && i + 1 == N - 1) && !(i == 0 && (N & 1))) {
            st.blocks = 2; st.kind = StepKind::Pair; st.reverse = zz; st.head = head_in_pair && i + 2 == N;
        } else if (single_kind == StepKind::H3Single) {
            st.head = head_in_block && i == N - 1;
            const H3Choice& c = st.head ? last_single : single;
            st.h3 = c.kernel; st.reverse = zz || c.bottom_up;
        } else if (single_kind == StepKind::GeneralConvs) {
            st.launches = block_convs;
        } else if (single_kind == StepKind::Unfused) {
            st.launches = 2;
        }
        return st;
    }
};

static ForwardPlan make_forward_plan(bf_handle h, int B, int H, int W)
{
    const bf_resnet_desc& d = h->d;
    ForwardPlan p;
    p.N = d.no_layers; p.block_convs = d.block_convs; p.zigzag = h->h3_zigzag != 0;
    p.h3 = h->fused_blocks && h->arith == 1 && d.no_layers > 0 && d.block_convs == 2;
    p.single_kind = d.block_convs != 2 ? StepKind::GeneralConvs
                    : p.h3             ? StepKind::H3Single
                    : h->fused_blocks  ? StepKind::Fp32Fused : StepKind::Unfused;
    if (p.h3) {
        const bool head_fits = d.head_activation == BF_ACT_LINEAR && d.out_channels == 3;      // the folded head: linear, 3 channels
        // the head epilogue exists in the row-streaming tile kernel only: asking for it selects that kernel for the last block
        p.head_in_block = h->fused_head && head_fits;
        const H3Request plain = {B, H, W, h->h3_variant, false, false};
        p.single = bf_select_fused_block_h3(plain);
        // compact layout (48 instead of 64 bytes per pixel between the launches): when every block runs the full-row streaming kernel
        p.compact = h->h3_compact && !p.head_in_block && p.single.kernel == H3Kernel::FullRow;
        if (p.compact) p.single = bf_select_fused_block_h3({B, H, W, h->h3_variant, false, true});
        if (p.head_in_block) p.last_single = bf_select_fused_block_h3({B, H, W, 1, true, false});
        // two blocks per launch (fused_h3w.hip) wherever the one-block streaming kernel would run: x1 and both intermediate
        // activations stay in LDS, 128 instead of 256 bytes per pixel through HBM for a pair
        p.pair_ok = h->h3_pair && !p.compact && (h->h3_pair == 2 || bf_fused_block_h3_use_pairs(plain)) &&
                    bf_fused_block2_h3w_supports(H, W);                                         // 2: A/B only
        p.head_in_pair = p.pair_ok && !p.head_in_block && h->h3_pair_head && d.no_layers >= 2 && head_fits;
        p.split = p.compact ? 2 : 1;
    }
    // the totals: which kernel runs how many of the blocks (a launch counts for the blocks it runs, a block of several launches once
    // per launch; among equals the one that ran first)
    const char* name[STEP_KINDS + 1] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int count[STEP_KINDS + 1] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < p.N;) {
        const ForwardStep st = p.next(i, p.launches);
        const char* nm = st.kernel_name();
        for (int k = 0; k < STEP_KINDS + 1; ++k) {
            if (name[k] == nullptr) name[k] = nm;
            if (!strcmp(name[k], nm)) { count[k] += st.blocks > 1 ? st.blocks : st.launches; break; }
        }
        p.launches += st.launches;
        i += st.blocks;
    }
    for (int k = 0, best = 0; k < STEP_KINDS + 1 && name[k]; ++k)
        if (count[k] > best) { best = count[k]; p.dominant = name[k]; }
    return p;
}

// One line of text for a plan (grammar: include/bfcnn_hip_debug.h, bf_debug_forward_plan).  Returns the characters written, or -1
// when they do not fit.
static int print_forward_plan(const ForwardPlan& p, char* out, int out_bytes)
{
    int n = snprintf(out, out_bytes, "%s", p.split == 2 ? "compact" : (p.split == 1 ? "split" : "f32"));
    for (int i = 0, launch = 0; i < p.N && n < out_bytes;) {
        const ForwardStep st = p.next(i, launch);
        for (int j = 0; j < st.launches && n < out_bytes; ++j) {
            n += snprintf(out + n, out_bytes - n, " %s:%d", st.kernel_name(), st.first);
            if (n < out_bytes && st.blocks == 2) n += snprintf(out + n, out_bytes - n, "+%d", st.first + 1);
            if (n < out_bytes && st.launches > 1) n += snprintf(out + n, out_bytes - n, ".%d", j);
            if (n < out_bytes && st.kind == StepKind::H3Single && st.h3 == H3Kernel::Tiles16) n += snprintf(out + n, out_bytes - n, ",t16");
            if (n < out_bytes && st.reverse) n += snprintf(out + n, out_bytes - n, ",rev");
            if (n < out_bytes && st.head) n += snprintf(out + n, out_bytes - n, ",head");
        }
        launch += st.launches;
        i += st.blocks;
    }
    if (n < out_bytes && p.head_kernel()) n += snprintf(out + n, out_bytes - n, " head");
    return n < out_bytes ? n : -1;
}

extern "C" int bf_debug_forward_plan(bf_handle h, int B, int H, int W, int pad_pow2, char* out, int out_bytes)
{
    if (!h || !out || out_bytes <= 0) return BF_EINVAL;
    if (B <= 0 || H <= 0 || W <= 0) return fail(h, BF_EINVAL, "batch/height/width must be positive (got %d,%d,%d)", B, H, W);
    const ForwardPlan p = pad_pow2 ? make_forward_plan(h, B, pow2_target(H), pow2_target(W)) : make_forward_plan(h, B, H, W);
    if (print_forward_plan(p, out, out_bytes) < 0) {
        out[0] = 0;
        return fail(h, BF_EINVAL, "bf_debug_forward_plan: the plan does not fit %d bytes", out_bytes);
    }
    return p.launches;
}

// ------------------------------------------------------------------------------------------
// inference: the launcher.  Nothing below chooses: each function turns one planned step into its launch(es).
// ------------------------------------------------------------------------------------------
// what the steps of one forward share: the problem, the packed weights, the three activation buffers and the one that is current
struct ForwardRun {
    bf_handle h;
    hipStream_t s;
    const float* pk;
    int B, H, W, Hs, Ws;    // activations are [B, H, W, 16]; the images are [B, Hs, Ws, .]
    float* buf[3];
    int cur;
    int* status;
    void* out;
    int out_is_u8;
    const BaseConvArgs* base;   // not NULL: the first step (a pair) computes the base convolution itself
};

// The three ways a forward runs its base convolution (bf_debug_base_path reports them by these numbers).
enum BasePath { BaseVector = 0, BaseRows = 1, BaseInPair = 2 };

// Inside the first launch when that launch is a pair that neither carries the head nor walks last to first, and
// base_conv_rows_kernel is the kernel that would run (the launch computes that kernel's bits, not the vector kernel's: where the
// selection prefers the vector kernel a forward keeps its bits too); else whichever kernel bf_launch_base_conv picks.
static BasePath base_path(bf_handle h, const ForwardPlan& p, const BaseConvArgs& ba)
{
    if (!bf_base_conv_runs_rows(ba)) return BaseVector;
    if (h->h3_pair_base && p.N > 0) {
        const ForwardStep st = p.next(0, 0);
        if (st.kind == StepKind::Pair && !st.head && !st.reverse) return BaseInPair;
    }
    return BaseRows;
}

static BaseConvArgs base_conv_args(bf_handle h, const ForwardPlan& p, int B, int Hs, int Ws, int H, int W, int in_is_u8)
{
    const bf_resnet_desc& d = h->d;
    BaseConvArgs ba;
    ba.in = nullptr; ba.out = nullptr; ba.w = nullptr;
    ba.B = B; ba.Hs = Hs; ba.Ws = Ws; ba.H = H; ba.W = W; ba.cin = d.in_channels; ba.k = d.kernel_size;
    ba.in_is_u8 = in_is_u8; ba.act_relu = d.base_activation == BF_ACT_RELU;
    ba.v_min = d.v_min; ba.v_max = d.v_max;
    // split-f16 blocks keep the activations split-planar between base conv and head (same bytes as fp32)
    ba.out_split = p.split;
    ba.status = nullptr;
    return ba;
}

extern "C" int bf_debug_base_path(bf_handle h, int B, int H, int W, int pad_pow2, int in_is_u8)
{
    if (!h) return BF_EINVAL;
    if (B <= 0 || H <= 0 || W <= 0) return fail(h, BF_EINVAL, "batch/height/width must be positive (got %d,%d,%d)", B, H, W);
    const int Hp = pad_pow2 ? pow2_target(H) : H, Wp = pad_pow2 ? pow2_target(W) : W;
    const ForwardPlan p = make_forward_plan(h, B, Hp, Wp);
    return base_path(h, p, base_conv_args(h, p, B, H, W, Hp, Wp, in_is_u8 != 0));
}

static int run_pair(ForwardRun& r, const ForwardStep& st)
{
    bf_handle h = r.h;
    const bf_resnet_desc& d = h->d;
    FusedH3WArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.in = r.buf[r.cur]; fa.out = r.buf[r.cur ^ 1];
    for (int b = 0; b < 2; ++b) {
        const float* aux = r.pk + h->k_h3 + (int64_t)(st.first + b) * BF_H3_BLOCK_FLOATS;
        fa.aux[b] = aux; fa.w1r[b] = aux + 64; fa.w2r[b] = aux + 64 + BF_H3R_WPACK_FLOATS;
    }
    fa.B = r.B; fa.H = r.H; fa.W = r.W;
    fa.reverse_tiles = st.reverse;
    fa.act1_relu = d.activation == BF_ACT_RELU; fa.zeros = r.pk + h->k_zero; fa.dbg = nullptr;
    if (st.head) {                                           // last pair: the linear head rides in its store step
        fa.head_wh = r.pk + h->k_wh; fa.head_out = r.out; fa.head_u8 = r.out_is_u8; fa.Ho = r.Hs; fa.Wo = r.Ws;
        fa.denormalize = d.denormalize; fa.v_min = d.v_min; fa.v_max = d.v_max; fa.status = r.status;
    }
    if (r.base && st.first == 0) {                           // first launch: x0 is computed in it, from the images
        fa.in = nullptr; fa.base_u8 = r.base->in; fa.base_w = r.base->w; fa.Hs = r.base->Hs; fa.Ws = r.base->Ws;
        fa.base_relu = r.base->act_relu; fa.status = r.status;
    }
    BF_HIP(bf_launch_fused_block2_h3w(fa, r.s), "fused_block2_h3w");
    r.cur ^= 1;
    return BF_OK;
}

static int run_h3_single(ForwardRun& r, const ForwardStep& st, bool compact)
{
    bf_handle h = r.h;
    const bf_resnet_desc& d = h->d;
    FusedH3Args fa;
    fa.in = r.buf[r.cur]; fa.out = r.buf[r.cur ^ 1];
    fa.aux = r.pk + h->k_h3 + (int64_t)st.first * BF_H3_BLOCK_FLOATS;
    fa.w1r = fa.aux + 64; fa.w2r = fa.aux + 64 + BF_H3R_WPACK_FLOATS;
    fa.B = r.B; fa.H = r.H; fa.W = r.W; fa.tiles_x = fa.tiles_y = fa.ntiles = 0; fa.rows_per_tile = 0; fa.variant = h->h3_variant;
    // consecutive blocks walk the batch in opposite directions: a block starts on the bands the previous one wrote
    // last, which are the ones still in the 256 MB Infinity Cache
    fa.reverse_tiles = st.reverse;
    fa.act1_relu = d.activation == BF_ACT_RELU; fa.zeros = r.pk + h->k_zero; fa.dump = (char*)r.status + 1024; fa.dbg = nullptr;
    fa.head_wh = nullptr; fa.head_out = nullptr; fa.head_u8 = 0; fa.Ho = fa.Wo = 0; fa.denormalize = 0;
    fa.v_min = fa.v_max = 0.f; fa.status = nullptr; fa.compact = compact;
    if (st.head) {                                           // last block: linear head in its epilogue, no head kernel
        fa.variant = 1;
        fa.head_wh = r.pk + h->k_wh; fa.head_out = r.out; fa.head_u8 = r.out_is_u8; fa.Ho = r.Hs; fa.Wo = r.Ws;
        fa.denormalize = d.denormalize; fa.v_min = d.v_min; fa.v_max = d.v_max; fa.status = r.status;
    }
    BF_HIP(bf_launch_fused_block_h3_as(fa, st.h3, r.s), "fused_block_h3");
    r.cur ^= 1;
    return BF_OK;
}

static int run_fp32_fused(ForwardRun& r, const ForwardStep& st)
{
    bf_handle h = r.h;
    const bf_resnet_desc& d = h->d;
    const float* blk = r.pk + h->k_blocks + st.first * h->k_block_stride;
    FusedBlockArgs fa;
    fa.in = r.buf[r.cur]; fa.out = r.buf[r.cur ^ 1];
    fa.w1pack = blk; fa.w2pack = blk + BF_WPACK_FLOATS;
    fa.scale = blk + 2 * BF_WPACK_FLOATS; fa.shift = fa.scale + 16;
    fa.B = r.B; fa.H = r.H; fa.W = r.W; fa.tiles_x = fa.tiles_y = fa.ntiles = 0;
    fa.act1_relu = d.activation == BF_ACT_RELU; fa.zeros = r.pk + h->k_zero;
    BF_HIP(bf_launch_fused_block(fa, r.s), "fused_block");
    r.cur ^= 1;
    return BF_OK;
}

static int run_general_convs(ForwardRun& r, const ForwardStep& st)
{
    bf_handle h = r.h;
    const bf_resnet_desc& d = h->d;
    const float* blk = r.pk + h->k_blocks + st.first * h->k_block_stride;
    const int cur = r.cur;
    // general block: conv1 (no BN) + act, [conv2 + BN + act,] conv_last + BN + linear, + skip (backbone_blocks.py:174-242;
    // a one-convolution block is conv (no BN, linear) + skip: the last activation is forced to base_activation)
    const int nbk = d.block_convs;
    const float* aff = blk + (int64_t)nbk * BF_WPACK_FLOATS;
    int src = cur;
    for (int j = 0; j < nbk; ++j) {
        const bool last = j == nbk - 1;
        int dst = (src + 1) % 3;
        if (dst == cur) dst = (dst + 1) % 3;                 // the block input stays alive for the skip
        ConvArgs ca;
        memset(&ca, 0, sizeof(ca));
        ca.in = r.buf[src]; ca.out = r.buf[dst]; ca.wpack = blk + (int64_t)j * BF_WPACK_FLOATS; ca.B = r.B; ca.H = r.H; ca.W = r.W;
        ca.scale = aff + j * 32; ca.shift = ca.scale + 16; ca.res = r.buf[cur];
        const bool relu = !last && d.activation == BF_ACT_RELU;
        int epi = (j >= 1 ? EPI_AFFINE : 0) | (relu ? EPI_RELU : 0) | (last ? EPI_RES : 0);
        BF_HIP(bf_launch_conv3x3_c16(ca, epi, r.s), "block conv");
        src = dst;
    }
    r.cur = src;
    return BF_OK;
}

static int run_unfused(ForwardRun& r, const ForwardStep& st)
{
    bf_handle h = r.h;
    const bf_resnet_desc& d = h->d;
    const float* blk = r.pk + h->k_blocks + st.first * h->k_block_stride;
    const int cur = r.cur;
    // unfused: T = act(conv1 x) ; y = x + scale*conv2(T) + shift
    const int t = (cur + 1) % 3, y = (cur + 2) % 3;
    ConvArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.in = r.buf[cur]; ca.out = r.buf[t]; ca.wpack = blk; ca.B = r.B; ca.H = r.H; ca.W = r.W;
    BF_HIP(bf_launch_conv3x3_c16(ca, d.activation == BF_ACT_RELU ? EPI_RELU : 0, r.s), "conv1");
    ca.in = r.buf[t]; ca.out = r.buf[y]; ca.wpack = blk + BF_WPACK_FLOATS;
    ca.scale = blk + 2 * BF_WPACK_FLOATS; ca.shift = ca.scale + 16; ca.res = r.buf[cur];
    BF_HIP(bf_launch_conv3x3_c16(ca, EPI_AFFINE | EPI_RES, r.s), "conv2");
    r.cur = y;
    return BF_OK;
}

static int run_step(ForwardRun& r, const ForwardStep& st, const ForwardPlan& p)
{
    switch (st.kind) {
    case StepKind::Pair: return run_pair(r, st);
    case StepKind::H3Single: return run_h3_single(r, st, p.compact);
    case StepKind::Fp32Fused: return run_fp32_fused(r, st);
    case StepKind::GeneralConvs: return run_general_convs(r, st);
    default: return run_unfused(r, st);
    }
}

// workspace check, base convolution, the planned steps, head
static int run_forward(bf_handle h, const float* pk, const void* in, int in_is_u8, void* out, int out_is_u8, int B, int Hs,
                          int Ws, int H, int W, void* ws, int64_t ws_bytes, hipStream_t s)
{
    const bf_resnet_desc& d = h->d;
    const int64_t act_bytes = (int64_t)B * H * W * 16 * 4;
    if (!ws || (uintptr_t)ws % 16) return fail(h, BF_EWORKSPACE, "workspace must be a 16-byte aligned device buffer");
    if (ws_bytes < act_bytes * 3 + BF_STATUS_BYTES)
        return fail(h, BF_EWORKSPACE, "workspace too small: %lld < %lld bytes", (long long)ws_bytes,
                    (long long)(act_bytes * 3 + BF_STATUS_BYTES));
    const ForwardPlan p = make_forward_plan(h, B, H, W);
    ForwardRun r;
    r.h = h; r.s = s; r.pk = pk; r.B = B; r.H = H; r.W = W; r.Hs = Hs; r.Ws = Ws;
    r.buf[0] = (float*)ws; r.buf[1] = (float*)((char*)ws + act_bytes); r.buf[2] = (float*)((char*)ws + 2 * act_bytes);
    r.cur = 0;
    r.status = (int*)((char*)ws + (ws_bytes - BF_STATUS_BYTES) / 4 * 4);
    r.out = out; r.out_is_u8 = out_is_u8;

    BaseConvArgs ba = base_conv_args(h, p, B, Hs, Ws, H, W, in_is_u8);
    ba.in = in; ba.out = r.buf[0]; ba.w = pk + h->k_base;
    ba.status = r.status;
    r.base = base_path(h, p, ba) == BaseInPair ? &ba : nullptr;
    if (!r.base) BF_HIP(bf_launch_base_conv(ba, s), "base_conv");

    if (h->timing) BF_HIP(h->timed.begin(s), "hipEventRecord");
    for (int i = 0, launch = 0; i < p.N;) {
        const ForwardStep st = p.next(i, launch);
        const int rc = run_step(r, st, p);
        if (rc != BF_OK) return rc;
        launch += st.launches;
        i += st.blocks;
    }
    if (h->timing) BF_HIP(h->timed.end(s, p.launches, TimingRing::Forward), "hipEventRecord");
    h->block_launches = p.launches;
    h->block_kernel = p.dominant;
    if (!p.head_kernel()) return BF_OK;
    HeadArgs ha;
    ha.feat = r.buf[r.cur];
    ha.w0 = pk + h->k_w0; ha.w1 = pk + h->k_w1;
    ha.wh = d.head_activation == BF_ACT_LINEAR ? pk + h->k_wh : nullptr;
    ha.out = out;
    ha.B = B; ha.H = H; ha.W = W; ha.Ho = Hs; ha.Wo = Ws; ha.hf = d.head_filters; ha.cout = d.out_channels;
    ha.act = d.head_activation; ha.out_is_u8 = out_is_u8; ha.denormalize = d.denormalize;
    ha.v_min = d.v_min; ha.v_max = d.v_max; ha.leaky_alpha = d.leaky_alpha;
    ha.feat_split = p.split;
    ha.status = r.status;
    BF_HIP(bf_launch_head(ha, s), "head");
    return BF_OK;
}

static int check_dims(bf_handle h, const void* packed, const void* in, const void* out, int B, int H, int W)
{
    if (!packed || !in || !out) return fail(h, BF_EINVAL, "NULL tensor pointer");
    if (B <= 0 || H <= 0 || W <= 0) return fail(h, BF_EINVAL, "batch/height/width must be positive (got %d,%d,%d)", B, H, W);
    if ((int64_t)B * H * W * 16 >= ((int64_t)1 << 40)) return fail(h, BF_EINVAL, "tensor too large");
    return BF_OK;
}

extern "C" int bf_forward_u8(bf_handle h, const void* packed, const uint8_t* in, uint8_t* out, int B, int H, int W, void* ws,
                             int64_t ws_bytes, void* stream)
{
    if (!h) return BF_EINVAL;
    int rc = check_dims(h, packed, in, out, B, H, W);
    if (rc) return rc;
    return run_forward(h, (const float*)packed, in, 1, out, 1, B, H, W, pow2_target(H), pow2_target(W), ws, ws_bytes,
                          (hipStream_t)stream);
}

// DenoiserModule(cast_to_uint8=False): the same chain as bf_forward_u8 without the final round + cast
extern "C" int bf_forward_u8_f32(bf_handle h, const void* packed, const uint8_t* in, float* out, int B, int H, int W, void* ws,
                                 int64_t ws_bytes, void* stream)
{
    if (!h) return BF_EINVAL;
    int rc = check_dims(h, packed, in, out, B, H, W);
    if (rc) return rc;
    return run_forward(h, (const float*)packed, in, 1, out, 0, B, H, W, pow2_target(H), pow2_target(W), ws, ws_bytes,
                          (hipStream_t)stream);
}

extern "C" int bf_forward_f32(bf_handle h, const void* packed, const float* in, float* out, int B, int H, int W, void* ws,
                              int64_t ws_bytes, void* stream)
{
    if (!h) return BF_EINVAL;
    int rc = check_dims(h, packed, in, out, B, H, W);
    if (rc) return rc;
    return run_forward(h, (const float*)packed, in, 0, out, 0, B, H, W, H, W, ws, ws_bytes, (hipStream_t)stream);
}
