// Training half of the C-ABI engine: bf_train_step = train_step_single_gpu (forward in training mode, head + loss, backward,
// regularisers) as one stream-ordered launch sequence, and the small kernels only the step launches.
#include "engine.h"
#include "block_reduce.h"
#include <cstring>
#include <cmath>

// ------------------------------------------------------------------------------------------
// workspace layout
// ------------------------------------------------------------------------------------------
struct TrainLayout {
    int64_t wpack, wh, bn_scale, bn_meaninv, coef, stage1, partial, wslots, acts, extra, total;   // float offsets
    int64_t act_floats, partial_floats, wslot_floats;
};

static int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }

static TrainLayout train_layout(bf_handle h, int B, int H, int W)
{
    TrainLayout L;
    const int N = h->d.no_layers;
    int64_t o = 0;
    const int nb = h->d.block_convs;                       // convolutions per block: forward + data-gradient pack each
    L.wpack = o; o += (int64_t)N * 2 * nb * BF_TRAIN_PACK_STRIDE;
    L.wh = o; o += 64;
    L.bn_scale = o; o += (int64_t)N * (nb > 1 ? nb - 1 : 1) * 32 + 32;
    L.bn_meaninv = o; o += (int64_t)N * (nb > 1 ? nb - 1 : 1) * 32 + 32;
    L.coef = o; o += 64;
    L.stage1 = o; o += 64 * 32 * 2;            // doubles
    int64_t pf = (int64_t)bf_conv3x3_c16_grid(B, H, W) * 32;
    pf = max64(pf, 4096 * 32);
    pf = max64(pf, (int64_t)bf_wgrad_grid(B, H, W) * 2304);
    pf = max64(pf, (int64_t)bf_bwd3x3_h3_grid(B, H, W) * (2304 + 32));
    pf = max64(pf, 2 * align_up((int64_t)bf_fwd_block_h3t_grid(B, H, W) * 32, 64));  // two sets of BatchNorm sums in turn (train_forward)
    pf = max64(pf, (int64_t)bf_bwd_block_h3t_grid(B, H, W) * (2304 + 64));           // + two sets of BatchNorm sums in turn
    pf = max64(pf, (int64_t)bf_base_wgrad_grid(B, H, W) * h->n_base);
    pf = max64(pf, (int64_t)bf_head_train_grid(B, H, W) * 80);
    L.partial_floats = align_up(pf, 64);
    L.partial = o; o += L.partial_floats + 256;     // +256: reduced head sums / scratch
    // one weight-gradient partial slot per block convolution (fused backward kernel): summed by ONE launch at the end of the step
    L.wslot_floats = max64(bf_bwd3x3_h3_grid(B, H, W), bf_bwd_block_h3t_grid(B, H, W)) * 2304;
    L.wslots = o; o += L.wslot_floats * N * nb;
    o = align_up(o, 64);
    L.act_floats = (int64_t)B * H * W * 16;
    // A_0..A_N, per block and convolution j >= 1 its input T_j and its raw output C_j, dA + two more gradient buffers (the
    // fused backward kernel reads its operands with a halo, so it never writes over one of them)
    L.acts = o; o += L.act_floats * ((int64_t)N * (2 * (nb - 1) + 1) + 4);
    // RMSE / SSIM loss terms (loss_terms.hip): prediction, extra gradient, three window maps (4 channels at most), partials
    L.extra = o; o += (int64_t)B * H * W * 4 * 5 + 4096 + align_up(B, 64) + 64;
    L.total = o;
    return L;
}

int64_t bf_train_workspace_floats(bf_handle h, int B, int H, int W) { return train_layout(h, B, H, W).total; }

// ------------------------------------------------------------------------------------------
// training
// ------------------------------------------------------------------------------------------
// reduces the head partials and writes the head gradients + the data-term losses
//   partial rows: [0,64) M | 64 sum|e| | 65 hinge sum | 66 per-block sum e^2 (blocks of one image are contiguous)
__global__ __launch_bounds__(1024) void head_finalize_kernel(const float* __restrict__ partial, int nblk, int blocks_per_image, int B,
                                                             double numel, double per_image, const float* __restrict__ w0,
                                                             const float* __restrict__ w1, int hf, int co, float* __restrict__ g0,
                                                             float* __restrict__ g1, float* __restrict__ losses,
                                                             float mae_multiplier, float depth_weight)
{
    constexpr int NS = 15;                     // 66 columns x 15 row stripes = 990 threads
    __shared__ double M[64];
    __shared__ double sums[2];
    __shared__ double rm[1024];
    __shared__ double part[NS][66];
    const int tid = threadIdx.x;
    // (one thread per column walked all B*64 rows alone: 540 us per step; 3 stripes on 198 threads: 61 us), fixed order
    if (tid < 66 * NS) {
        const int col = tid % 66, stripe = tid / 66;
        double s = 0.0;
        // loads issued eight at a time (a rolled load -> add loop waits out one L2 round trip per row); same add order
        int r = stripe;
        for (; r + 7 * NS < nblk; r += 8 * NS) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = partial[(size_t)(r + NS * u) * 80 + col];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += (double)v[u];
        }
        for (; r < nblk; r += NS) s += (double)partial[(size_t)r * 80 + col];
        part[stripe][col] = s;
    }
    __syncthreads();
    if (tid < 66) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < NS; ++k) s += part[k][tid];
        if (tid < 64) M[tid] = s; else sums[tid - 64] = s;
    }
    // rmse: mean over images of sqrt(mean_sq + DEFAULT_EPSILON)   (loss.py:92-113, constants.py:7)
    double acc = 0.0;
    for (int b = tid; b < B; b += 1024) {
        double sq = 0.0;
        int k = 0;
        for (; k + 7 < blocks_per_image; k += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = partial[(size_t)(b * blocks_per_image + k + u) * 80 + 66];
#pragma unroll
            for (int u = 0; u < 8; ++u) sq += (double)v[u];
        }
        for (; k < blocks_per_image; ++k) sq += (double)partial[(size_t)(b * blocks_per_image + k) * 80 + 66];
        acc += sqrt(sq / per_image + 1e-3);
    }
    const double rm_sum = bf_block_reduce<1024, BfSum>(rm, tid, acc);
    // dW0[c][j] = sum_o M[c][o] * W1[j][o] ; dW1[j][o] = sum_c W0[c][j] * M[c][o]
    for (int i = tid; i < 16 * hf; i += 1024) {
        const int c = i / hf, j = i % hf;
        double s = 0.0;
        for (int o = 0; o < co; ++o) s += M[c * 4 + o] * (double)w1[j * co + o];
        g0[i] = (float)s;
    }
    for (int i = tid; i < hf * co; i += 1024) {
        const int j = i / co, o = i % co;
        double s = 0.0;
        for (int c = 0; c < 16; ++c) s += (double)w0[c * hf + j] * M[c * 4 + o];
        g1[i] = (float)s;
    }
    if (tid == 0) {
        const double mae_actual = sums[0] / numel;
        const double mae_loss = mae_multiplier > 0.f ? sums[1] / numel : 0.0;
        losses[BF_LOSS_MAE] = (float)mae_actual;
        losses[BF_LOSS_MSE] = (float)(rm_sum / (double)B);
        losses[BF_LOSS_SSIM] = 0.f;
        losses[BF_LOSS_DENOISER_TOTAL] = (float)(mae_loss * mae_multiplier);
        losses[BF_LOSS_TOTAL] = (float)(mae_loss * mae_multiplier * depth_weight);     // + model loss added by reg kernel
    }
}

// regularisers (keras "l1" -> 0.01*sum|w|, "l2" -> 0.01*sum w^2; bfcnn/loss.py:181-187):
// adds d(reg*regularization)/dw to grads; per-workgroup fp64 partial sums (fixed order), finished by
// regularizer_finalize_kernel.  (One workgroup walking all 84 k parameters alone took 50 us of a step.)
constexpr int REG_GRID = 64;
__global__ __launch_bounds__(1024) void regularizer_kernel(const float* __restrict__ params, float* __restrict__ grads, int64_t n,
                                                           int64_t n_base, int64_t p_blocks, int64_t p_stride, int64_t p_head0,
                                                           int reg_base, int reg_block, int reg_head, float regularization,
                                                           double* __restrict__ wg_sums, int unit)
{
    __shared__ double red[1024];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x; i < n; i += (int64_t)REG_GRID * 1024) {
        int reg;
        if (i < n_base) reg = reg_base;
        else if (i >= p_head0) reg = reg_head;
        else {      // block: conv0 [2304], then per further convolution its kernel [2304] and (with BatchNorm) its gamma [16]
            const unsigned r = (unsigned)(i - p_blocks) % (unsigned)p_stride;
            reg = (r < 2304u || ((r - 2304u) % (unsigned)unit) < 2304u) ? reg_block : BF_REG_NONE;
        }
        const float w = params[i];
        if (reg == BF_REG_L1) {
            acc += 0.01 * fabs((double)w);
            grads[i] = grads[i] + regularization * 0.01f * (w > 0.f ? 1.f : (w < 0.f ? -1.f : 0.f));
        } else if (reg == BF_REG_L2) {
            acc += 0.01 * (double)w * (double)w;
            grads[i] = grads[i] + regularization * 0.02f * w;
        }
    }
    const double sum = bf_block_reduce<1024, BfSum>(red, (int)threadIdx.x, acc);
    if (threadIdx.x == 0) wg_sums[blockIdx.x] = sum;
}

__global__ void regularizer_finalize_kernel(const double* __restrict__ wg_sums, float regularization, float* __restrict__ losses)
{
    if (threadIdx.x == 0) {
        double r = 0.0;
        for (int k = 0; k < REG_GRID; ++k) r += wg_sums[k];
        losses[BF_LOSS_REGULARIZATION] = (float)r;
        losses[BF_LOSS_MODEL_TOTAL] = (float)(r * regularization);
        losses[BF_LOSS_TOTAL] = losses[BF_LOSS_TOTAL] + (float)(r * regularization);
        losses[BF_LOSS_GRAD_NORM] = 0.f;
    }
}

__global__ void premultiply_head_kernel(const float* __restrict__ w0, const float* __restrict__ w1, int hf, int co, float* __restrict__ wh)
{
    if (threadIdx.x < 64) {
        const int c = threadIdx.x >> 2, o = threadIdx.x & 3;
        float s = 0.f;
        if (o < co)
            for (int j = 0; j < hf; ++j) s = fmaf(w0[c * hf + j], w1[j * co + o], s);
        wh[threadIdx.x] = s;
    }
}

__global__ void scale_range_kernel(float* __restrict__ p, int64_t n, float f)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] *= f;
}

__global__ void fill_identity_affine_kernel(float* scale_shift)
{
    if (threadIdx.x < 16) { scale_shift[threadIdx.x] = 1.f; scale_shift[16 + threadIdx.x] = 0.f; }
}

// What the three phases of a training step share: the problem, the workspace and its buffer map, the kernel-selection predicates
// and the walking direction of the next tile kernel.
struct TrainStep {
    bf_handle h;
    hipStream_t s;
    int B, H, W, N, nb, unit;       // nb: block = conv_0 [+ act] , conv_j + BN [+ act] (j >= 1), last one linear, + skip
                                    // unit: floats from convolution kernel j >= 1 of a block to the next (gamma in between)
    int64_t npix;
    double count;
    TrainLayout L;
    float* w;                       // workspace
    float* partial;
    double* stage1;
    bool h3t;                       // split-f16 arithmetic (train_arith)
    bool fwd_block, bwd_block;      // whole blocks in one kernel (train_fwd_h3t.hip / train_bwd_h3t.hip)
    bool fused_bwd;                 // weight + data gradient of a convolution in one kernel (train_bwd_h3.hip)
    bool bfold;                     // bwd_block with the BatchNorm-backward finalisation in the next launch's prologue
    int launch_no;

    float* ACT(int64_t i) const { return w + L.acts + i * L.act_floats; }
    // buffer map: A_i = ACT(i) (i = 0..N: block inputs / outputs) ; T(i,j) = input of convolution j >= 1 of block i (the
    // activated output of convolution j-1) ; C(i,j) = raw output of convolution j >= 1 (in front of its BatchNorm)
    float* A(int i) const { return ACT(i); }
    float* T(int i, int j) const { return ACT(N + 1 + (int64_t)i * (nb - 1) + (j - 1)); }
    float* C(int i, int j) const { return ACT(N + 1 + (int64_t)N * (nb - 1) + (int64_t)i * (nb - 1) + (j - 1)); }
    // gradient buffers: 0 = dA (the head's output) and two spares; the fused kernels ping-pong between them
    float* gbuf(int k) const { return ACT(N + 1 + k + 2 * (int64_t)N * (nb - 1)); }
    // a gradient buffer that is neither g nor dA (the fused backward kernels read their operands with a halo: never in place)
    float* spare_gbuf(const float* g, const float* dA) const
    {
        for (int k = 0; k < 3; ++k)
            if (gbuf(k) != g && gbuf(k) != dA) return gbuf(k);
        return nullptr;
    }
    int64_t conv_off(int j) const { return j == 0 ? (int64_t)0 : 2304 + (int64_t)(j - 1) * unit; }     // inside a block's parameters
    int64_t bn_idx(int i, int j) const { return (int64_t)i * (nb - 1) + (j - 1); }                       // BatchNorm of convolution j >= 1
    int bwd_grid() const { return bwd_block ? bf_bwd_block_h3t_grid(B, H, W) : bf_bwd3x3_h3_grid(B, H, W); }

    // every tile kernel of the step reads what the one before it wrote: alternate the walking direction (train_zigzag)
    int next_reverse() { return h->train_zigzag ? (launch_no++ & 1) : 0; }
    hipError_t conv(ConvArgs& ca, int epi)
    {
        if (!h3t) return bf_launch_conv3x3_c16(ca, epi, s);
        ca.reverse = next_reverse();
        return bf_launch_conv3x3_h3(ca, epi, s);
    }
    hipError_t wgrad(const float* xx, const float* dyy, float* dw) const
    {
        return h3t ? bf_launch_wgrad3x3_h3(xx, dyy, partial, dw, B, H, W, s) : bf_launch_wgrad3x3_c16(xx, dyy, partial, dw, B, H, W, s);
    }
};

static TrainStep make_train_step(bf_handle h, int B, int H, int W, const TrainLayout& L, void* ws, hipStream_t s)
{
    const bf_resnet_desc& d = h->d;
    TrainStep t;
    t.h = h; t.s = s; t.B = B; t.H = H; t.W = W; t.N = d.no_layers; t.nb = d.block_convs; t.unit = d.use_bn ? 2320 : 2304;
    t.npix = (int64_t)B * H * W; t.count = (double)t.npix;
    t.L = L; t.w = (float*)ws; t.partial = t.w + L.partial;
    t.stage1 = reinterpret_cast<double*>(t.w + L.stage1);     // (offset is a multiple of 2 floats: 8-byte aligned)
    t.h3t = h->train_arith == 1;
    t.launch_no = 0;
    // whole blocks in one kernel (train_fwd_h3t.hip): [3,3] blocks, BatchNorm on the second convolution, the split-f16 arithmetic,
    // images up to 256 columns, and a forward of enough rows that its bands (rows + 6 steps each) keep 256 workgroups busy
    t.fwd_block = t.h3t && h->train_fwd_block && h->train_fused_fwd && t.nb == 2 && d.use_bn && bf_fwd_block_h3t_supports(H, W) &&
                  (h->train_fwd_block == 2 || (int64_t)B * H >= 4096);
    // the whole backward of a block in one kernel that RECOMPUTES T_i from A_i (train_bwd_h3t.hip): same kind of block, any width
    t.bwd_block = t.h3t && h->train_bwd_block && h->train_fused_bwd && t.nb == 2 && d.use_bn && bf_bwd_block_h3t_supports(H, W) &&
                  (h->train_bwd_block == 2 || bf_bwd_block_h3t_strip_rows(B, H, W) >= 8192);
    t.fused_bwd = t.h3t && h->train_fused_bwd;
    // train_fold_finalize with the block backward kernel: launch i reads the sums launch i + 1 wrote and finalises them in its prologue,
    // so the sums go to two buffers in turn (both behind the weight-gradient slots inside `partial`)
    const int64_t bg = t.bwd_grid();
    t.bfold = t.bwd_block && h->train_fold_finalize != 0 && bg * 2304 + 2 * bg * 32 <= L.partial_floats;
    return t;
}

// "fwd: <kernels>; bwd: <kernels>" of bf_get_train_kernels
static std::string train_kernel_names(const TrainStep& t)
{
    const bf_engine& e = *t.h;
    const char* fwd = t.fwd_block ? "fwd_block_h3t_kernel"
                      : !t.h3t    ? "conv3x3_c16_kernel"
                      : e.train_fused_fwd && t.nb >= 2 && e.d.use_bn ? "conv3x3_h3_kernel<.., PRE> + conv3x3_h3_kernel" : "conv3x3_h3_kernel";
    const char* bwd = t.bwd_block   ? "bwd_block_h3t_kernel"
                      : t.fused_bwd ? "bwd3x3_h3_kernel<true, 8> + bwd3x3_h3_kernel<false, 36>"
                      : t.h3t       ? "wgrad3x3_h3_kernel + conv3x3_h3_kernel" : "wgrad3x3_c16_kernel + conv3x3_c16_kernel";
    return std::string("fwd: ") + fwd + "; bwd: " + bwd;
}

// ---- forward, training mode (hydra(noisy, training=True), train_loop.py:249-251, 277) ----
static int train_forward(TrainStep& t, const float* params, float* state, const float* noisy)
{
    bf_handle h = t.h;
    const bf_resnet_desc& d = h->d;
    const TrainLayout& L = t.L;
    hipStream_t s = t.s;
    float* w = t.w;
    const int B = t.B, H = t.H, W = t.W, N = t.N, nb = t.nb;
    BaseConvArgs ba;
    ba.in = noisy; ba.out = t.A(0); ba.w = params + h->p_base;
    ba.B = B; ba.Hs = H; ba.Ws = W; ba.H = H; ba.W = W; ba.cin = d.in_channels; ba.k = d.kernel_size; ba.in_is_u8 = 0;
    ba.act_relu = 0; ba.v_min = d.v_min; ba.v_max = d.v_max; ba.out_split = 0; ba.status = nullptr;
    BF_HIP(bf_launch_base_conv(ba, s), "base_conv");
    const int conv_grid = bf_conv3x3_c16_grid(B, H, W);
    const bool relu = d.activation == BF_ACT_RELU;
    bool pending_affine = false;
    const bool need_t = !t.bwd_block;                       // the per-convolution backward kernels read T_i
    for (int i = 0; i < N; ++i) {
        const float* wp = w + L.wpack + (int64_t)i * 2 * nb * BF_TRAIN_PACK_STRIDE;        // forward packs 0..nb-1, then data-gradient packs
        if (t.fwd_block) {
            // A_i = A_{i-1} + bn(C_{i-1}) on load ; T_i = act(conv_0 A_i) ; C_i = conv_1 T_i + its batch statistics.
            // train_fold_finalize: the BatchNorm finalisation of block i - 1 runs in THIS launch's prologue (every workgroup sums that
            // block's partials itself; two partial buffers in turn), so a forward is one launch per block instead of two
            const int fgrid = bf_fwd_block_h3t_grid(B, H, W);
            const int64_t pp = align_up((int64_t)fgrid * 32, 64);
            const bool fold = h->train_fold_finalize != 0 && 2 * pp <= L.partial_floats;
            float* part_i = fold ? t.partial + (i & 1) * pp : t.partial;
            FwdBlockH3Args fa;
            memset(&fa, 0, sizeof(fa));
            fa.B = B; fa.H = H; fa.W = W; fa.reverse = t.next_reverse(); fa.act_relu = relu;
            fa.x = t.A(i);
            if (pending_affine) {
                fa.x = t.A(i - 1); fa.pre_c = t.C(i - 1, 1); fa.a_out = t.A(i);
                fa.pre_scale = w + L.bn_scale + t.bn_idx(i - 1, 1) * 32; fa.pre_shift = fa.pre_scale + 16;
                if (fold) {
                    fa.fin_partial = t.partial + ((i - 1) & 1) * pp; fa.fin_nblk = fgrid; fa.fin_count = t.count;
                    fa.fin_gamma = params + h->p_blocks + (i - 1) * h->p_block_stride + t.conv_off(1) + 2304;
                    fa.fin_mm = state + t.bn_idx(i - 1, 1) * 32; fa.fin_mv = fa.fin_mm + 16;
                    fa.fin_eps = d.bn_eps; fa.fin_momentum = d.bn_momentum;
                    fa.fin_scale = w + L.bn_scale + t.bn_idx(i - 1, 1) * 32; fa.fin_meaninv = w + L.bn_meaninv + t.bn_idx(i - 1, 1) * 32;
                }
                pending_affine = false;
            }
            fa.t_out = need_t ? t.T(i, 1) : nullptr; fa.c_out = t.C(i, 1);
            fa.wpack0 = wp; fa.wpack1 = wp + BF_TRAIN_PACK_STRIDE; fa.stats = part_i;
            BF_HIP(bf_launch_fwd_block_h3t(fa, s), "fwd_block_h3t");
            if (fold && i + 1 < N) {
                pending_affine = true;                              // block i + 1 finalises this BatchNorm itself
                continue;
            }
            float* scale = w + L.bn_scale + t.bn_idx(i, 1) * 32;
            BF_HIP(bf_launch_bn_finalize(part_i, fgrid, t.count, params + h->p_blocks + i * h->p_block_stride + t.conv_off(1) + 2304,
                                         state + t.bn_idx(i, 1) * 32, state + t.bn_idx(i, 1) * 32 + 16, d.bn_eps, d.bn_momentum, scale,
                                         scale + 16, w + L.bn_meaninv + t.bn_idx(i, 1) * 32, t.stage1, s), "bn_finalize");
            if (i + 1 < N) pending_affine = true;
            else BF_HIP(bf_launch_affine_add(t.A(i), t.C(i, 1), scale, scale + 16, t.A(i + 1), t.npix, s), "affine_add");
            continue;
        }
        for (int j = 0; j < nb; ++j) {
            const bool last = j == nb - 1, bn = j >= 1 && d.use_bn;
            ConvArgs ca;
            memset(&ca, 0, sizeof(ca));
            ca.B = B; ca.H = H; ca.W = W;
            ca.in = j == 0 ? t.A(i) : t.T(i, j); ca.wpack = wp + (int64_t)j * BF_TRAIN_PACK_STRIDE;
            if (j == 0 && pending_affine) {
                // A(i) = A(i-1) + scale * C(i-1, last) + shift has not been formed yet: this convolution does it on load
                ca.in = t.A(i - 1); ca.pre_c = t.C(i - 1, nb - 1); ca.pre_out = t.A(i);
                ca.pre_scale = w + L.bn_scale + t.bn_idx(i - 1, nb - 1) * 32; ca.pre_shift = ca.pre_scale + 16;
                pending_affine = false;
            }
            if (bn) {
                // conv -> BatchNorm (batch statistics ride in the convolution's epilogue) -> [activation | + skip]
                float* scale = w + L.bn_scale + t.bn_idx(i, j) * 32;
                ca.out = t.C(i, j); ca.stats = t.partial;
                BF_HIP(t.conv(ca, EPI_STATS), "conv + statistics");
                BF_HIP(bf_launch_bn_finalize(t.partial, conv_grid, t.count, params + h->p_blocks + i * h->p_block_stride + t.conv_off(j) + 2304,
                                             state + t.bn_idx(i, j) * 32, state + t.bn_idx(i, j) * 32 + 16, d.bn_eps, d.bn_momentum, scale,
                                             scale + 16, w + L.bn_meaninv + t.bn_idx(i, j) * 32, t.stage1, s), "bn_finalize");
                // block i+1's conv_0 forms A(i+1) on load.  (The head kernel doing the same for the last block was tried: its register
                // count went past 256, one wave per SIMD, +105 us in the head for the 79 us of affine_add.)
                if (last && t.h3t && h->train_fused_fwd && i + 1 < N && nb >= 2) pending_affine = true;
                else if (last) BF_HIP(bf_launch_affine_add(t.A(i), t.C(i, j), scale, scale + 16, t.A(i + 1), t.npix, s), "affine_add");
                else BF_HIP(bf_launch_affine_act(t.C(i, j), scale, scale + 16, t.T(i, j + 1), relu, t.npix, s), "affine_act");
            } else if (last) {
                // no BatchNorm on the block's last convolution (one-convolution block, or use_bn off): linear, + skip
                ca.out = t.A(i + 1); ca.res = t.A(i);
                BF_HIP(t.conv(ca, EPI_RES), "conv + skip");
            } else {
                ca.out = t.T(i, j + 1);
                BF_HIP(t.conv(ca, relu ? EPI_RELU : 0), "conv + activation");
            }
        }
    }
    return BF_OK;
}

// ---- head forward + loss + head backward: dL/dA_N * S to gbuf(0), the head's gradients and the data-term losses; *grad_unscale = 1 / S ----
static int train_head_and_loss(TrainStep& t, const float* params, const float* gt, const bf_loss_desc* loss, float* predictions,
                               float* grads, float* losses, float* grad_unscale)
{
    bf_handle h = t.h;
    const bf_resnet_desc& d = h->d;
    hipStream_t s = t.s;
    const int B = t.B, H = t.H, W = t.W;
    const bool extra_terms = loss->ssim_multiplier > 0.f || loss->mse_multiplier > 0.f;     // use_ssim / use_mse (loss.py:174-179)
    const double numel = (double)t.npix * d.out_channels;
    HeadTrainArgs ta;
    ta.feat = t.A(t.N); ta.wh = t.w + t.L.wh;
    ta.gt = gt; ta.pred = predictions; ta.dfeat = t.gbuf(0); ta.partial = t.partial; ta.dextra = nullptr;
    ta.B = B; ta.H = H; ta.W = W; ta.cout = d.out_channels; ta.denormalize = d.denormalize;
    ta.v_min = d.v_min; ta.v_max = d.v_max; ta.hinge = loss->hinge; ta.cutoff = loss->cutoff;
    ta.dscale = loss->mae_multiplier > 0.f ? (float)((double)loss->mae_multiplier * loss->depth_weight / numel) : 0.f;
    // Gradient scaling of the split-f16 backward.  dL/dprediction is O(1 / numel): 5e-8 at 32 x 256 x 256 x 3.  The data-
    // and weight-gradient kernels split every dy into two f16 numbers while they stage it; below 2^-14 the split keeps an
    // ABSOLUTE floor of 2^-25, so unscaled gradients lost most of their bits -- the larger the batch the more (bf_train_step
    // against itself on a batch that repeats two images: weight gradients 0.3 % off at 32 x 64 x 64, 12 % at 32 x 256 x 256;
    // tools/exp/train_batch_rep.py).  The head hands the blocks dfeat * S, S the power of two next to numel / (multiplier *
    // depth_weight); every backward operator is linear in dy, and the block / base gradients are multiplied by 1 / S (exact)
    // before the regularisers are added.  The exact-fp32 arithmetic runs with S = 1 as before.
    *grad_unscale = 1.0f;
    ta.dfeat_scale = 1.0f;
    if (t.h3t) {
        const double per = (loss->mae_multiplier > 0.f ? (double)loss->mae_multiplier : 1.0) * (loss->depth_weight > 0.f ? loss->depth_weight : 1.0) / numel;
        int ex = 0;
        (void)frexp(1.0 / per, &ex);
        ex = ex - 1 < 0 ? 0 : (ex - 1 > 40 ? 40 : ex - 1);
        ta.dfeat_scale = ldexpf(1.0f, ex);
        *grad_unscale = ldexpf(1.0f, -ex);
    }
    const int hgrid = bf_head_train_grid(B, H, W);
    float* scal = nullptr;
    if (extra_terms) {
        // pass A: prediction + per-image sums; then the additive gradient of the RMSE / SSIM terms; pass B below adds it
        const int64_t pe = t.npix * d.out_channels;
        float* ex = t.w + t.L.extra;
        float* predbuf = predictions ? predictions : ex;
        float *dextra = ex + pe, *maps = ex + 2 * pe, *ssim_partial = ex + 5 * (int64_t)t.npix * 4;
        float* coef = ssim_partial + 4096;
        scal = coef + align_up(B, 64);
        ta.pred = predbuf;
        BF_HIP(bf_launch_head_train(ta, hgrid, s), "head_train (prediction pass)");
        BF_HIP(bf_launch_loss_extra(predbuf, gt, B, H, W, d.out_channels, t.partial, hgrid / B, loss->hinge, loss->cutoff,
                                    loss->mse_multiplier > 0.f ? loss->mse_multiplier : 0.f,
                                    loss->ssim_multiplier > 0.f ? loss->ssim_multiplier : 0.f, loss->depth_weight, 255.0f, maps,
                                    ssim_partial, coef, scal, dextra, s), "loss_extra");
        ta.pred = nullptr;
        ta.dextra = dextra;
    }
    BF_HIP(bf_launch_head_train(ta, hgrid, s), "head_train");
    hipLaunchKernelGGL(head_finalize_kernel, dim3(1), dim3(1024), 0, s, t.partial, hgrid, hgrid / B, B, numel,
                       (double)H * W * d.out_channels, params + h->p_head0, params + h->p_head1, d.head_filters, d.out_channels,
                       grads + h->p_head0, grads + h->p_head1, losses, loss->mae_multiplier, loss->depth_weight);
    BF_HIP(hipGetLastError(), "head_finalize");
    if (extra_terms)
        BF_HIP(bf_launch_loss_extra_finalize(scal, B, H, W, d.out_channels, loss->mse_multiplier > 0.f ? loss->mse_multiplier : 0.f,
                                             loss->ssim_multiplier > 0.f ? loss->ssim_multiplier : 0.f, loss->depth_weight, losses, s),
               "loss_extra_finalize");
    return BF_OK;
}

// ---- backward through the blocks: block weight / gamma gradients to grads, *dA_out = the buffer that holds dL/dA_0 -------------
// g = dL/d(block output) arrives in dA = gbuf(0).  Per convolution j = nb-1 .. 0: [BatchNorm backward: g -> dc, dgamma] ; weight
// gradient from (input of conv j, dc) ; data gradient through conv j -- for j >= 1 written over T(i,j) with the ReLU mask
// of the activation that produced T(i,j), for j = 0 added to dA (the skip).
static int train_backward(TrainStep& t, const float* params, float* grads, float** dA_out)
{
    bf_handle h = t.h;
    const bf_resnet_desc& d = h->d;
    const TrainLayout& L = t.L;
    hipStream_t s = t.s;
    float* w = t.w;
    float* partial = t.partial;
    const int B = t.B, H = t.H, W = t.W, N = t.N, nb = t.nb;
    const bool h3t = t.h3t, fused_bwd = t.fused_bwd, bfold = t.bfold;
    const bool relu = d.activation == BF_ACT_RELU;
    const int conv_grid = bf_conv3x3_c16_grid(B, H, W);
    const int64_t n4 = t.npix * 4;
    const int bgrid = (int)((n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048);
    const int bwd_grid = t.bwd_grid();
    float* bwd_stats = partial + (int64_t)bwd_grid * 2304;
    auto bstats = [&](int i) { return bfold ? bwd_stats + (int64_t)(i & 1) * bwd_grid * 32 : bwd_stats; };
    float* dA = t.gbuf(0);
    for (int i = N - 1; i >= 0; --i) {
        const float* wp = w + L.wpack + (int64_t)i * 2 * nb * BF_TRAIN_PACK_STRIDE;
        float* gblk = grads + h->p_blocks + i * h->p_block_stride;
        const float* g = dA;
        for (int j = nb - 1; j >= 0; --j) {
            const bool last = j == nb - 1, bn = j >= 1 && d.use_bn;
            const float* dy = g;
            if (bn) {
                // sum dy, sum dy*c: for the block's last BatchNorm they come from the data-gradient kernel of the block above
                // when it produced dA (split-f16 path: its epilogue accumulates them), else from the reduction kernel
                const bool fused_sums = h3t && last && i < N - 1;
                if (!fused_sums) BF_HIP(bf_launch_bn_bwd_reduce(g, t.C(i, j), partial, t.npix, bgrid, s), "bn_bwd_reduce");
                if (!(bfold && fused_sums))
                BF_HIP(bf_launch_bn_bwd_finalize(fused_sums && fused_bwd ? bstats(i + 1) : partial,
                                                 fused_sums ? (fused_bwd ? bwd_grid : conv_grid) : bgrid, t.count,
                                                 params + h->p_blocks + i * h->p_block_stride + t.conv_off(j) + 2304,
                                                 w + L.bn_meaninv + t.bn_idx(i, j) * 32, w + L.coef, gblk + t.conv_off(j) + 2304, t.stage1, s),
                       "bn_bwd_finalize");
                if (!fused_bwd) {
                    BF_HIP(bf_launch_bn_bwd_apply(g, t.C(i, j), w + L.coef, t.C(i, j), t.npix, s), "bn_bwd_apply");
                    dy = t.C(i, j);
                }
            }
            if (t.bwd_block) {
                // one row-streaming kernel for the whole block, T recomputed from A(i): dc = k1 g + k2 c + k3 ; T = act(conv_0 A) ;
                // dw1 = T^T dc ; dT = dgrad_1(dc) * (T > 0) ; dw0 = A^T dT ; dA' = dgrad_0(dT) + g [+ the sums of the BatchNorm in front]
                BwdBlockH3Args fa;
                memset(&fa, 0, sizeof(fa));
                fa.B = B; fa.H = H; fa.W = W; fa.act_relu = relu; fa.reverse = t.next_reverse();
                fa.a = t.A(i); fa.g = g; fa.c = t.C(i, 1); fa.coef = w + L.coef;
                if (bfold && i < N - 1) {                           // the sums came from launch i + 1: finalised in this launch's prologue
                    fa.fin_partial = bstats(i + 1); fa.fin_nblk = bwd_grid; fa.fin_count = t.count;
                    fa.fin_gamma = params + h->p_blocks + i * h->p_block_stride + t.conv_off(1) + 2304;
                    fa.fin_meaninv = w + L.bn_meaninv + t.bn_idx(i, 1) * 32;
                    fa.fin_dgamma = gblk + t.conv_off(1) + 2304;
                }
                fa.wfwd0 = wp; fa.wdg0 = wp + (int64_t)nb * BF_TRAIN_PACK_STRIDE; fa.wdg1 = wp + (int64_t)(nb + 1) * BF_TRAIN_PACK_STRIDE;
                fa.wpartial1 = w + L.wslots + ((int64_t)i * nb + 1) * L.wslot_floats;
                fa.wpartial0 = w + L.wslots + ((int64_t)i * nb + 0) * L.wslot_floats;
                fa.stats = bstats(i);
                if (i > 0) fa.bnc = t.C(i - 1, nb - 1);
                float* out = t.spare_gbuf(g, dA);                   // (g == dA here)
                fa.out = out;
                // option "timing": one HIP-event pair around EVERY launch of this kernel (ring of BF_TIMING_RING pairs; bf_get_timing
                // returns their sum and count: bench.py's live roofline of the training step, measured inside real steps)
                if (h->timing) BF_HIP(h->timed.begin(s), "hipEventRecord");
                BF_HIP(bf_launch_bwd_block_h3t(fa, s), "bwd_block_h3t");
                if (h->timing) BF_HIP(h->timed.end(s, 1, TimingRing::TrainBlock), "hipEventRecord");
                g = out;
                dA = out;
                break;                                              // both convolutions done
            }
            if (fused_bwd) {
                // one kernel: [dc = k1 g + k2 c + k3] ; dw = x^T dc ; dx = dgrad(dc) [* mask | + skip]
                BwdH3Args fa;
                memset(&fa, 0, sizeof(fa));
                fa.B = B; fa.H = H; fa.W = W;
                fa.x = j == 0 ? t.A(i) : t.T(i, j);
                fa.g = g;
                if (bn) { fa.c = t.C(i, j); fa.coef = w + L.coef; }
                fa.wpack = wp + (int64_t)(nb + j) * BF_TRAIN_PACK_STRIDE;
                fa.wpartial = w + L.wslots + ((int64_t)i * nb + j) * L.wslot_floats; fa.stats = bwd_stats; fa.reverse = t.next_reverse();
                float* out = t.spare_gbuf(g, dA);
                int epi;
                if (j > 0) {
                    epi = relu ? EPI_MASK : 0;
                } else {
                    fa.res = dA;
                    if (g != dA) out = dA;                          // in place over the skip gradient (read at the same element only)
                    epi = EPI_RES;
                    if (d.use_bn && nb >= 2 && i > 0) { fa.bnc = t.C(i - 1, nb - 1); epi |= EPI_BNBWD; }
                }
                fa.out = out;
                BF_HIP(bf_launch_bwd3x3_h3(fa, epi, nullptr, s), "bwd3x3_h3");
                g = out;
                if (j == 0) dA = out;                               // (one-convolution block: another buffer than before)
                continue;
            }
            BF_HIP(t.wgrad(j == 0 ? t.A(i) : t.T(i, j), dy, gblk + t.conv_off(j)), "wgrad");
            ConvArgs ca;
            memset(&ca, 0, sizeof(ca));
            ca.B = B; ca.H = H; ca.W = W;
            ca.in = dy; ca.wpack = wp + (int64_t)(nb + j) * BF_TRAIN_PACK_STRIDE;
            if (j > 0) {
                ca.out = t.T(i, j); ca.mask = t.T(i, j);
                BF_HIP(t.conv(ca, relu ? EPI_MASK : 0), "dgrad");
                g = t.T(i, j);
            } else {
                ca.out = dA; ca.res = dA;
                if (h3t && d.use_bn && nb >= 2 && i > 0) {       // dA becomes dy of block i-1's last BatchNorm: its sums ride along
                    ca.bnc = t.C(i - 1, nb - 1); ca.stats = partial;
                    BF_HIP(t.conv(ca, EPI_RES | EPI_BNBWD), "dgrad + skip");
                } else {
                    BF_HIP(t.conv(ca, EPI_RES), "dgrad + skip");
                }
            }
        }
    }
    if (fused_bwd && N > 0)
        BF_HIP(bf_launch_reduce_wgrad_slots(w + L.wslots, L.wslot_floats, bwd_grid, grads + h->p_blocks, h->p_block_stride, N, nb, t.unit, s),
               "reduce_wgrad_slots");
    *dA_out = dA;
    return BF_OK;
}

extern "C" int bf_train_step(bf_handle h, const float* params, float* state, const float* gt, const float* noisy, int B, int H,
                             int W, const bf_loss_desc* loss, float* predictions, float* grads, float* losses, void* ws,
                             int64_t ws_bytes, void* stream)
{
    if (!h) return BF_EINVAL;
    const bf_resnet_desc& d = h->d;
    if (!params || !gt || !noisy || !loss || !grads || !losses || (h->n_state > 0 && !state))
        return fail(h, BF_EINVAL, "bf_train_step: NULL argument");
    if (loss->struct_size != (int32_t)sizeof(bf_loss_desc)) return fail(h, BF_EINVAL, "bf_loss_desc struct_size mismatch");
    if (B <= 0 || H <= 0 || W <= 0) return fail(h, BF_EINVAL, "batch/height/width must be positive");
    if (loss->ssim_multiplier > 0.f && (H < 7 || W < 7)) return fail(h, BF_EINVAL, "SSIM needs images of at least 7x7");
    if (loss->ssim_multiplier > 0.f && !d.denormalize)
        return fail(h, BF_EUNSUPPORTED, "SSIM term (max_val 255) is built for the denormalised hydra output");
    if (d.head_activation != BF_ACT_LINEAR) return fail(h, BF_EUNSUPPORTED, "training is built for the linear denoiser head");
    if (d.block_convs < 1 || d.block_convs > 3) return fail(h, BF_EUNSUPPORTED, "training is built for blocks of 1 to 3 convolutions (got %d)", d.block_convs);
    if (d.out_channels != d.in_channels) return fail(h, BF_EINVAL, "gt/prediction channel mismatch");
    const TrainLayout L = train_layout(h, B, H, W);
    if (!ws || (uintptr_t)ws % 16) return fail(h, BF_EWORKSPACE, "workspace must be a 16-byte aligned device buffer");
    if (ws_bytes < L.total * 4) return fail(h, BF_EWORKSPACE, "workspace too small: %lld < %lld bytes", (long long)ws_bytes,
                                            (long long)(L.total * 4));
    hipStream_t s = (hipStream_t)stream;
    TrainStep t = make_train_step(h, B, H, W, L, ws, s);
    if (t.N > 0) {
        if (t.h3t) {
            BF_HIP(bf_launch_pack_h3_train(params, h->p_blocks, h->p_block_stride, t.w + L.wpack, t.N, t.nb, t.unit, s), "pack_h3_train");
        } else {
            BF_HIP(bf_launch_pack_all_convs(params, h->p_blocks, h->p_block_stride, t.w + L.wpack, (int64_t)2 * t.nb * BF_TRAIN_PACK_STRIDE,
                                            t.N, 1, t.nb, t.unit, s), "pack_all_convs");
        }
    }
    hipLaunchKernelGGL(premultiply_head_kernel, dim3(1), dim3(64), 0, s, params + h->p_head0, params + h->p_head1, d.head_filters,
                       d.out_channels, t.w + L.wh);
    BF_HIP(hipGetLastError(), "premultiply_head");

    int rc = train_forward(t, params, state, noisy);
    if (rc != BF_OK) return rc;
    float grad_unscale = 1.0f;
    rc = train_head_and_loss(t, params, gt, loss, predictions, grads, losses, &grad_unscale);
    if (rc != BF_OK) return rc;
    h->train_kernels = train_kernel_names(t);
    float* dA = nullptr;                            // dL/dA_0 after the backward pass
    rc = train_backward(t, params, grads, &dA);
    if (rc != BF_OK) return rc;

    BF_HIP(bf_launch_base_wgrad(noisy, dA, t.partial, grads + h->p_base, B, H, W, d.in_channels, d.kernel_size, d.v_min, d.v_max, s),
           "base_wgrad");
    if (grad_unscale != 1.0f) {
        // base + block gradients (everything in front of the head's tensors) back to the loss's own scale
        hipLaunchKernelGGL(scale_range_kernel, dim3(64), dim3(256), 0, s, grads, h->p_head0, grad_unscale);
        BF_HIP(hipGetLastError(), "grad_unscale");
    }
    hipLaunchKernelGGL(regularizer_kernel, dim3(REG_GRID), dim3(1024), 0, s, params, grads, h->n_params, h->n_base, h->p_blocks,
                       h->p_block_stride, h->p_head0, d.reg_base, d.reg_block, d.reg_head, loss->regularization, t.stage1,
                       t.unit);
    hipLaunchKernelGGL(regularizer_finalize_kernel, dim3(1), dim3(64), 0, s, t.stage1, loss->regularization, losses);
    BF_HIP(hipGetLastError(), "regularizer");
    return BF_OK;
}
