// C-ABI engine: validates the model description, lays out parameters exactly as keras creates
// the trainable variables, and turns DenoiserModule.__call__ / hydra() / train_step_single_gpu /
// apply_grads into stream-ordered launch sequences of the gfx950 kernels.
// The library owns no device memory and never synchronises (include/bfcnn_hip.h).
// This unit: the handle, the tensor inventory, the options, the reports and the size queries (engine.h names the other three).
#include "engine.h"
#include <cstdarg>
#include <cstdio>
#include <cstring>

static thread_local std::string g_create_error;

int fail(bf_handle h, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_create_error = buf;
    return code;
}

int hip_fail(bf_handle h, hipError_t e, const char* what)
{
    return fail(h, BF_EHIP, "%s: %s", what, hipGetErrorString(e));
}

extern "C" int bf_abi_version(void) { return BFCNN_ABI_VERSION; }

extern "C" const char* bf_last_error(bf_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

static void add_tensor(std::vector<bf_tensor_info>& v, const char* name, int64_t& off, int rank, int s0, int s1, int s2,
                       int s3, int kind, int reg)
{
    bf_tensor_info t;
    memset(&t, 0, sizeof(t));
    snprintf(t.name, sizeof(t.name), "%s", name);
    t.offset = off;
    t.rank = rank;
    t.shape[0] = s0; t.shape[1] = s1; t.shape[2] = s2; t.shape[3] = s3;
    t.kind = kind;
    t.regularizer = reg;
    int64_t n = 1;
    for (int i = 0; i < rank; ++i) n *= t.shape[i];
    off += n;
    v.push_back(t);
}

// model_builder (bfcnn/model.py:58-162) -> backbone_resnet.builder (backbone_resnet.py:19-298)
// argument checks, restricted to the configurations the gfx950 kernels are built for.
extern "C" int bf_create(const bf_resnet_desc* d, bf_handle* out)
{
    if (out) *out = nullptr;
    if (!d || !out) return fail(nullptr, BF_EINVAL, "bf_create: desc/out must not be NULL");
    if (d->struct_size != (int32_t)sizeof(bf_resnet_desc))
        return fail(nullptr, BF_EINVAL, "bf_create: struct_size %d != %d (ABI mismatch)", d->struct_size, (int)sizeof(bf_resnet_desc));
    if (d->no_layers < 0) return fail(nullptr, BF_EINVAL, "no_layers must be >= 0");              // backbone_blocks.py:122
    if (d->block_convs <= 0) return fail(nullptr, BF_EINVAL, "len(block_kernels) must be >= 0 "); // backbone_resnet.py:111
    if (d->block_convs > 3) return fail(nullptr, BF_EINVAL, "len(block_kernels) must be <= 3");   // backbone_resnet.py:113
    if (d->in_channels != 1 && d->in_channels != 3)
        return fail(nullptr, BF_EUNSUPPORTED, "in_channels %d: only 1 and 3 are built", d->in_channels);
    if (d->filters != BF_C) return fail(nullptr, BF_EUNSUPPORTED, "filters %d: the MFMA path is built for 16", d->filters);
    if (d->kernel_size != 1 && d->kernel_size != 3 && d->kernel_size != 5 && d->kernel_size != 7)
        return fail(nullptr, BF_EUNSUPPORTED, "base kernel_size %d: only 1,3,5,7", d->kernel_size);
    // [3,3] is the fused / trainable path; [3] and [3,3,3] (conv1 no-BN+act, conv2 BN+act, conv3 BN+linear, backbone_blocks.py:
    // 174-213) run inference through the single-convolution kernel with the general epilogue [affine][ReLU][+residual]
    if (d->block_kernel != 3)
        return fail(nullptr, BF_EUNSUPPORTED, "block_kernels must be 3x3 (got %d convs of %d)", d->block_convs, d->block_kernel);
    if (d->activation != BF_ACT_RELU && d->activation != BF_ACT_LINEAR)
        return fail(nullptr, BF_EUNSUPPORTED, "block activation must be relu or linear");
    if (d->base_activation != BF_ACT_LINEAR)
        return fail(nullptr, BF_EUNSUPPORTED, "base_activation must be linear");
    if (d->head_filters < 1 || d->head_filters > 64) return fail(nullptr, BF_EUNSUPPORTED, "head filters must be in 1..64");
    if (d->out_channels < 1 || d->out_channels > 4) return fail(nullptr, BF_EUNSUPPORTED, "output_channels must be in 1..4");
    if (!(d->v_max > d->v_min)) return fail(nullptr, BF_EINVAL, "value_range must have max > min");

    bf_engine* h = new bf_engine();
    h->d = *d;
    const int k = d->kernel_size, cin = d->in_channels, hf = d->head_filters, co = d->out_channels;
    int64_t off = 0;
    h->p_base = off;
    add_tensor(h->tensors, "base/kernel", off, 4, k, k, cin, BF_C, BF_KIND_CONV, d->reg_base);
    h->n_base = off;
    h->p_blocks = off;
    const int nb = d->block_convs;
    h->p_block_stride = nb * 2304 + (d->use_bn ? (nb - 1) * 16 : 0);
    char name[64];
    for (int i = 0; i < d->no_layers; ++i) {
        for (int j = 0; j < nb; ++j) {             // keras creation order: conv j, then its BN gamma (first conv has no BN)
            snprintf(name, sizeof(name), "block%d/conv%d/kernel", i, j);
            add_tensor(h->tensors, name, off, 4, 3, 3, BF_C, BF_C, BF_KIND_CONV, d->reg_block);
            if (j >= 1 && d->use_bn) {
                snprintf(name, sizeof(name), "block%d/bn%d/gamma", i, j);
                add_tensor(h->tensors, name, off, 1, BF_C, 0, 0, 0, BF_KIND_GAMMA, BF_REG_NONE);
            }
        }
    }
    h->p_head0 = off;
    add_tensor(h->tensors, "head/conv0/kernel", off, 4, 1, 1, BF_C, hf, BF_KIND_CONV, d->reg_head);
    h->p_head1 = off;
    add_tensor(h->tensors, "head/conv1/kernel", off, 4, 1, 1, hf, co, BF_KIND_CONV, d->reg_head);
    h->n_params = off;
    int64_t soff = 0;
    if (d->use_bn) {
        for (int i = 0; i < d->no_layers; ++i)
            for (int j = 1; j < nb; ++j) {
                snprintf(name, sizeof(name), "block%d/bn%d/moving_mean", i, j);
                add_tensor(h->states, name, soff, 1, BF_C, 0, 0, 0, BF_KIND_MOVING_MEAN, BF_REG_NONE);
                snprintf(name, sizeof(name), "block%d/bn%d/moving_variance", i, j);
                add_tensor(h->states, name, soff, 1, BF_C, 0, 0, 0, BF_KIND_MOVING_VAR, BF_REG_NONE);
            }
    }
    h->n_state = soff;
    // packed layout
    int64_t ko = 0;
    h->k_base = ko; ko += align_up(h->n_base, 64);
    // per block: nb weight images, then one folded (scale, shift) pair per convolution (identity for the BN-less first one)
    h->k_blocks = ko; h->k_block_stride = nb == 2 ? 2 * BF_WPACK_FLOATS + 32 : nb * (BF_WPACK_FLOATS + 32);
    ko += h->k_block_stride * d->no_layers;
    h->k_w0 = ko; ko += align_up(16 * hf, 64);
    h->k_w1 = ko; ko += align_up(hf * co, 64);
    h->k_wh = ko; ko += 64;
    h->k_zero = ko; ko += 64;
    h->k_h3 = ko; ko += (int64_t)BF_H3_BLOCK_FLOATS * d->no_layers;
    h->k_total = ko;
    *out = h;
    return BF_OK;
}

extern "C" void bf_destroy(bf_handle h)
{
    if (!h) return;
    for (hipEvent_t e : h->timed.ev) (void)hipEventDestroy(e);
    delete h;
}
extern "C" int64_t bf_param_count(bf_handle h) { return h ? h->n_params : -1; }
extern "C" int64_t bf_state_count(bf_handle h) { return h ? h->n_state : -1; }
extern "C" int bf_tensor_count(bf_handle h, int state) { return h ? (int)(state ? h->states.size() : h->tensors.size()) : -1; }

extern "C" int bf_tensor_at(bf_handle h, int state, int index, bf_tensor_info* out)
{
    if (!h || !out) return BF_EINVAL;
    const auto& v = state ? h->states : h->tensors;
    if (index < 0 || index >= (int)v.size()) return fail(h, BF_EINVAL, "tensor index %d out of range", index);
    *out = v[index];
    return BF_OK;
}

extern "C" int bf_set_option(bf_handle h, const char* key, int value)
{
    if (!h || !key) return BF_EINVAL;
    if (!strcmp(key, "fused_blocks")) { h->fused_blocks = value ? 1 : 0; return BF_OK; }
    if (!strcmp(key, "fused_tile")) { bf_set_fused_tile(value); return BF_OK; }
    if (!strcmp(key, "h3_variant")) { h->h3_variant = value; return BF_OK; }      // per handle; < 0 = library default
    if (!strcmp(key, "h3_zigzag")) { h->h3_zigzag = value ? 1 : 0; return BF_OK; }
    if (!strcmp(key, "h3_compact")) { h->h3_compact = value ? 1 : 0; return BF_OK; }
    if (!strcmp(key, "h3_pair")) { h->h3_pair = value == 2 ? 2 : (value ? 1 : 0); return BF_OK; }
    if (!strcmp(key, "base_rows")) { bf_set_base_conv_rows(value); return BF_OK; }       // process-wide (A/B only)
    if (!strcmp(key, "h3_pair_head")) { h->h3_pair_head = value ? 1 : 0; return BF_OK; }
    if (!strcmp(key, "h3_pair_base")) { h->h3_pair_base = value ? 1 : 0; return BF_OK; }
    if (!strcmp(key, "fused_head")) { h->fused_head = value ? 1 : 0; return BF_OK; }
    if (!strcmp(key, "train_zigzag")) { h->train_zigzag = value ? 1 : 0; return BF_OK; }
    if (!strcmp(key, "train_fused_fwd")) { h->train_fused_fwd = value ? 1 : 0; return BF_OK; }
    if (!strcmp(key, "train_fused_bwd")) { h->train_fused_bwd = value ? 1 : 0; return BF_OK; }
    if (!strcmp(key, "train_bwd_block")) { h->train_bwd_block = value < 0 ? 1 : (value > 2 ? 2 : value); return BF_OK; }
    if (!strcmp(key, "train_fwd_block")) { h->train_fwd_block = value < 0 ? 1 : (value > 2 ? 2 : value); return BF_OK; }
    // retired A/B options (their kernels lost and were removed): accepted and ignored
    if (!strcmp(key, "train_fused_bwd2") || !strcmp(key, "train_bwd_dbuf")) return BF_OK;
    if (!strcmp(key, "train_fold_finalize")) { h->train_fold_finalize = value ? 1 : 0; return BF_OK; }
    if (!strcmp(key, "train_arith")) { h->train_arith = value < 0 ? 1 : (value ? 1 : 0); return BF_OK; }
    if (!strcmp(key, "arith")) { h->arith = value < 0 ? 1 : (value ? 1 : 0); return BF_OK; }
    if (!strcmp(key, "timing")) {
        h->timing = value ? 1 : 0;
        h->timed.restart();                         // (re)setting the option restarts the measurement window
        if (h->timing && h->timed.ev.empty()) {
            h->timed.ev.resize(2 * BF_TIMING_RING, nullptr);
            for (hipEvent_t& e : h->timed.ev)
                if (hipEventCreate(&e) != hipSuccess) return fail(h, BF_EHIP, "hipEventCreate failed");
        }
        return BF_OK;
    }
    return fail(h, BF_EINVAL, "unknown option [%s]", key);
}

// sum of the elapsed ms of the event pairs of the current window (TimingRing, engine.h: the brackets of the forwards, or of the
// block-backward launches of the training steps, since the option was set or the other kind was last timed) and the number of
// kernel launches inside them.  The caller must have synchronised the stream.
extern "C" int bf_get_timing(bf_handle h, float* ms, int* launches)
{
    if (!h || !ms || !launches) return BF_EINVAL;
    const TimingRing& t = h->timed;
    if (!h->timing || t.ev.empty()) return fail(h, BF_EINVAL, "timing option is off");
    const int64_t n = t.n < BF_TIMING_RING ? t.n : BF_TIMING_RING;
    if (n == 0) return fail(h, BF_EINVAL, "no forward has run since the timing option was set");
    double total = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        float one = 0.f;
        hipError_t e = hipEventElapsedTime(&one, t.ev[2 * i], t.ev[2 * i + 1]);
        if (e != hipSuccess) return hip_fail(h, e, "hipEventElapsedTime");
        total += one;
    }
    *ms = (float)total;
    *launches = (int)(t.launches_in_pair * n);
    return BF_OK;
}

// name of the kernel that ran most of the residual-block launches of the last forward, and how many launches one forward made
extern "C" const char* bf_get_block_kernel(bf_handle h, int* launches_per_forward)
{
    if (!h) return "";
    if (launches_per_forward) *launches_per_forward = h->block_launches;
    return h->block_kernel;
}

// the kernels that ran the residual blocks of the handle's LAST bf_train_step: "fwd: <kernels>; bwd: <kernels>" ("" before the first)
extern "C" const char* bf_get_train_kernels(bf_handle h) { return h ? h->train_kernels.c_str() : ""; }

extern "C" int64_t bf_packed_bytes(bf_handle h) { return h ? h->k_total * 4 : -1; }

extern "C" int64_t bf_workspace_bytes(bf_handle h, int mode, int B, int H, int W)
{
    if (!h || B <= 0 || H <= 0 || W <= 0) return -1;
    if (mode == BF_MODE_INFERENCE) {
        const int Hp = pow2_target(H), Wp = pow2_target(W);      // u8 path pads; f32 path needs <= this
        return (int64_t)B * Hp * Wp * 16 * 4 * 3 + BF_STATUS_BYTES;
    }
    return bf_train_workspace_floats(h, B, H, W) * 4;
}
