/*
 * bfcnn_hip.h -- C ABI of the MI355X (gfx950) engine for the bfcnn resnet-denoiser hot path.
 *
 * The reference (NikolasMarkou/blind_image_denoising, bfcnn 3.2.0) is pure Python on
 * TensorFlow/Keras: it has no FFI of its own.  These entry points are what a binding for
 * its hot path replaces; every declaration cites the reference interface (file:line under
 * the reference root) whose behaviour it reproduces.  The reference-side stub a maintainer
 * would add is shown in INTEGRATION.md (ctypes, because the reference host is Python).
 *
 * Conventions
 *   - plain C types only; no torch / HIP types in signatures (a stream is passed as void*
 *     = hipStream_t, NULL = the null stream);
 *   - every tensor pointer is DEVICE memory on the handle's device unless the name ends in
 *     `_host`; activations are NHWC, contiguous; kernels are HWIO ([kh,kw,cin,cout]) exactly
 *     as keras stores them;
 *   - the caller owns every buffer, including the workspace (size from bf_workspace_bytes);
 *     the library never allocates device memory, never synchronises and spawns no threads:
 *     all work is enqueued on the given stream (graph-capturable);
 *   - return value 0 = BF_OK, negative = error; text via bf_last_error().
 */
#ifndef BFCNN_HIP_H
#define BFCNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BFCNN_ABI_VERSION 1

typedef struct bf_engine* bf_handle;

enum bf_status {
    BF_OK = 0,
    BF_EINVAL = -1,       /* bad argument (reference raises ValueError)            */
    BF_EUNSUPPORTED = -2, /* config outside the hot path (NotImplementedError)     */
    BF_EWORKSPACE = -3,   /* workspace / packed buffer too small or misaligned     */
    BF_EHIP = -4          /* HIP runtime error on launch                           */
};

enum bf_activation { BF_ACT_LINEAR = 0, BF_ACT_RELU = 1, BF_ACT_LEAKY_RELU = 2 };
enum bf_regularizer { BF_REG_NONE = 0, BF_REG_L1 = 1, BF_REG_L2 = 2 };
enum bf_mode { BF_MODE_INFERENCE = 0, BF_MODE_TRAIN = 1 };
enum bf_tensor_kind { BF_KIND_CONV = 0, BF_KIND_GAMMA = 1, BF_KIND_MOVING_MEAN = 2, BF_KIND_MOVING_VAR = 3 };

/* The arguments of bfcnn/backbone_resnet.py:19-50 (builder) and bfcnn/model.py:251-275
 * (model_denoiser_builder) that the hot path uses.  The host parses the reference's
 * pipeline JSON (bfcnn/utilities.py:59-96) into this struct. */
typedef struct bf_resnet_desc {
    int32_t struct_size;      /* = sizeof(bf_resnet_desc)                                   */
    int32_t in_channels;      /* input_shape[-1], 1..4                                       */
    int32_t filters;          /* `filters`; the MFMA path is built for 16                    */
    int32_t kernel_size;      /* base conv kernel_size: 1,3,5,7                              */
    int32_t no_layers;        /* number of residual blocks                                   */
    int32_t block_convs;      /* len(block_kernels); 2 (fused, trainable) | 1 | 3 (inference)  */
    int32_t block_kernel;     /* block_kernels[*]; 3                                         */
    int32_t activation;       /* bf_activation of the first block conv                       */
    int32_t base_activation;  /* bf_activation of base conv and last block conv (linear)     */
    int32_t use_bn;           /* BatchNormalization(scale=True, center=False) after conv2    */
    int32_t head_filters;     /* denoiser `filters` (default 32), <= 64                      */
    int32_t head_activation;  /* denoiser `activation` (default linear)                      */
    int32_t out_channels;     /* denoiser `output_channels`, 1..4                            */
    int32_t denormalize;      /* 1: always denormalise; 0: literal snapshot graph (model.py:110-116) */
    int32_t reg_base;         /* bf_regularizer: kernel_regularizer of the base conv         */
    int32_t reg_block;        /* block_regularizer                                           */
    int32_t reg_head;         /* denoiser kernel_regularizer                                 */
    float v_min, v_max;       /* value_range                                                 */
    float bn_eps, bn_momentum;/* constants.py:9,11                                           */
    float leaky_alpha;        /* slope when an activation is BF_ACT_LEAKY_RELU               */
} bf_resnet_desc;

/* bfcnn/loss.py:162-179 + the depth weight of train_loop.py:284-285. */
typedef struct bf_loss_desc {
    int32_t struct_size;
    float hinge, cutoff;
    float mae_multiplier;
    float mse_multiplier;     /* > 0: + rmse(hinge, cutoff^2) * this (loss.py:228-235)       */
    float ssim_multiplier;    /* > 0: + (1 - mean tf.image.ssim(7x7, max 255)) * this (:219-227) */
    float regularization;
    float depth_weight;
} bf_loss_desc;

/* losses written by bf_train_step, device float[BF_LOSS_COUNT] (keys of constants.py:35-50). */
enum bf_loss_slot {
    BF_LOSS_TOTAL = 0,          /* p_total_loss (train_loop.py:299-301)                      */
    BF_LOSS_DENOISER_TOTAL = 1, /* denoiser_loss[total_loss]                                 */
    BF_LOSS_MAE = 2,            /* mae_loss (no hinge)                                       */
    BF_LOSS_MSE = 3,            /* mse_loss = rmse (no hinge)                                */
    BF_LOSS_SSIM = 4,           /* ssim_loss = 1 - mean ssim (0 when the term is off)        */
    BF_LOSS_REGULARIZATION = 5, /* model_loss[regularization_loss]                           */
    BF_LOSS_MODEL_TOTAL = 6,    /* model_loss[total_loss]                                    */
    BF_LOSS_GRAD_NORM = 7,      /* global L2 norm of the last gradient given to bf_adam_step */
    BF_LOSS_COUNT = 8
};

typedef struct bf_tensor_info {
    char name[64];
    int64_t offset;           /* element offset in the flat params (or state) buffer         */
    int32_t rank;
    int32_t shape[4];
    int32_t kind;             /* bf_tensor_kind                                              */
    int32_t regularizer;      /* bf_regularizer                                              */
} bf_tensor_info;

/* ---- lifetime ----------------------------------------------------------------------- */

int bf_abi_version(void);

/* model_builder(config) (bfcnn/model.py:58-162): validates the description and builds the
 * launch plan.  No device memory is touched.  *out = NULL on failure; bf_last_error(NULL)
 * then holds the reason. */
int bf_create(const bf_resnet_desc* desc, bf_handle* out);
void bf_destroy(bf_handle h);
const char* bf_last_error(bf_handle h);

/* ---- parameter inventory (keras trainable_variables / non-trainable BN stats) -------- */

int64_t bf_param_count(bf_handle h);   /* trainable floats: conv kernels + BN gammas         */
int64_t bf_state_count(bf_handle h);   /* BN moving_mean / moving_variance floats            */
int bf_tensor_count(bf_handle h, int state);
int bf_tensor_at(bf_handle h, int state, int index, bf_tensor_info* out);

/* ---- inference ---------------------------------------------------------------------- */

int64_t bf_packed_bytes(bf_handle h);
int64_t bf_workspace_bytes(bf_handle h, int mode, int batch, int height, int width);

/* Re-lays the weights for the kernels (MFMA operand images, BN folded to scale/shift with
 * the inference formula of keras BatchNormalization: gamma*(x-moving_mean)*rsqrt(var+eps)).
 * Call after every change of params/state. */
int bf_pack_inference(bf_handle h, const float* params, const float* state, void* packed, void* stream);

/* DenoiserModule.__call__ (bfcnn/module_denoiser.py:46-75): uint8 [B,H,W,C] -> uint8 [B,H,W,Cout]:
 * cast, pad_to_power_of_2 (utilities.py:736-751), hydra, remove_padding, round-half-even, cast. */
int bf_forward_u8(bf_handle h, const void* packed, const uint8_t* in, uint8_t* out,
                  int batch, int height, int width, void* workspace, int64_t workspace_bytes, void* stream);

/* DenoiserModule(cast_to_uint8=False).__call__ (bfcnn/module_denoiser.py:66-75 without the cast branch): the same chain,
 * float32 [B,H,W,Cout] out, not rounded. */
int bf_forward_u8_f32(bf_handle h, const void* packed, const uint8_t* in, float* out,
                      int batch, int height, int width, void* workspace, int64_t workspace_bytes, void* stream);

/* hydra(x, training=False) (bfcnn/model.py:91-151; test_step train_loop.py:253-257):
 * float32 [B,H,W,C] in value_range -> float32 [B,H,W,Cout].  No power-of-two padding. */
int bf_forward_f32(bf_handle h, const void* packed, const float* in, float* out,
                   int batch, int height, int width, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- training ----------------------------------------------------------------------- */

/* train_step_single_gpu (bfcnn/train_loop.py:259-312) for the single-output resnet hydra:
 * training-mode forward (BN batch statistics, moving stats updated in `state`), L1 loss with
 * hinge/cutoff (loss.py:40-65,190-247) * depth_weight + regularisation (loss.py:181-187),
 * gradients of the total w.r.t. every trainable variable into `grads` (flat, same layout as
 * params).  `predictions` may be NULL.  `losses` = device float[BF_LOSS_COUNT]. */
int bf_train_step(bf_handle h, const float* params, float* state, const float* gt, const float* noisy,
                  int batch, int height, int width, const bf_loss_desc* loss,
                  float* predictions, float* grads, float* losses,
                  void* workspace, int64_t workspace_bytes, void* stream);

/* apply_grads (bfcnn/train_loop.py:314-321) with the optimizer of bfcnn/optimizer.py:190-206:
 * keras-2.13 Adam, optional global_clipnorm (<=0 disables), grads pre-scaled by grad_scale
 * (1/world_size after a sum all-reduce).  `iterations` = optimizer.iterations before the step;
 * `lr` = schedule(iterations) evaluated by the host.  losses[BF_LOSS_GRAD_NORM] receives the
 * (scaled) global norm when `losses` is not NULL.  scratch = device float[>=2] (may alias
 * the workspace). */
int bf_adam_step(bf_handle h, float* params, const float* grads, float* m, float* v,
                 int64_t iterations, float lr, float beta_1, float beta_2, float epsilon,
                 float global_clipnorm, float grad_scale, float* losses, float* scratch, void* stream);

/* The same with keras' other two clipping modes (optimizer.py:165-169): clipnorm = tf.clip_by_norm on every gradient tensor,
 * clipvalue = clip_by_value; precedence as keras 2.13: clipnorm, else global_clipnorm, else clipvalue (<= 0 disables each).
 * tensor_offsets = device int64[n_tensors + 1]: offsets of the trainable tensors in the flat vector, last = parameter
 * count (bf_tensor_info order); tensor_scratch = device float[n_tensors]. */
int bf_adam_step_ex(bf_handle h, float* params, const float* grads, float* m, float* v,
                    int64_t iterations, float lr, float beta_1, float beta_2, float epsilon,
                    float global_clipnorm, float clipnorm, float clipvalue, const int64_t* tensor_offsets, int n_tensors,
                    float* tensor_scratch, float grad_scale, float* losses, float* scratch, void* stream);

/* ---- pyramid / resampling (bfcnn/pyramid.py, upsampling.py, downsampling.py) ---------- */

/* AveragePooling2D(pool_size=(kh,kw), strides=2, padding="same") (pyramid.py:266-270,374-378). */
int bf_avgpool_s2_same(const float* in, float* out, int batch, int height, int width, int channels,
                       int kh, int kw, void* stream);
/* tf.nn.avg_pool2d(2x2, stride 2, VALID) [+clip 0..255][+round] (utilities.py:642-672). */
int bf_avgpool2_valid(const float* in, float* out, int batch, int height, int width, int channels,
                      int clip_values, int round_values, void* stream);
/* UpSampling2D(2, "bilinear"|"nearest") (pyramid.py:319-325; upsampling.py:65,105):
 * out = up(in) [+ add][- sub...]: out = alpha*up(in) + beta*other (other may be NULL). */
int bf_upsample2x(const float* in, const float* other, float* out, int batch, int height, int width,
                  int channels, int bilinear, float alpha, float beta, void* stream);
/* one level of the Laplacian split in ONE kernel (bfcnn/pyramid.py:374-385): down = AveragePooling2D((kh,kw), strides 2, same)(in)
 * [B,H/2,W/2,C] and lap = in - UpSampling2D(2, bilinear)(down) [B,H,W,C]; x is read once (2.25 n floats of traffic instead of the
 * 3.5 n of bf_avgpool_s2_same + bf_upsample2x) and the results are bitwise those of the two calls.  Returns BF_EUNSUPPORTED
 * without launching anything for shapes it does not take (odd H or W, W*C not a multiple of 4, C a multiple of 4, kh not in
 * {3,5,7}, unaligned tensors): the caller then makes the two calls. */
int bf_laplacian_split(const float* in, float* down, float* lap, int batch, int height, int width, int channels, int kh, int kw,
                       void* stream);
/* x[:, ::2, ::2, :] (downsampling.py:61). */
int bf_strided_slice2(const float* in, float* out, int batch, int height, int width, int channels, void* stream);

/* prepare_data_fn of bfcnn/dataset.py:126-239 on a device batch [B,H,W,C] of floats in value range (not in place):
 *   out_clean = round(flip(in))                               (geometric_augmentation_fn :131-159, tf.round :234)
 *   out_noisy = round(out_clean * (1 + mult_std * tn) + add_std * tn')   (noise_augmentation_fn :161-230)
 * tn, tn' = standard normals truncated at +-2 (tf.random.truncated_normal re-picks outside 2 sigma), drawn per element
 * from Philox4x32-10 (counter = element index, key = seed).  The per-BATCH random choices of the reference -- the two
 * flips (flip_mask bit 0 left-right, bit 1 up-down), whether each noise is applied (std = 0 disables it) and the
 * standard deviations ~ U[min,max] -- are the caller's (blind_image_denoising_amd.dataset draws them on the host).
 * out_clean may be NULL. */
int bf_noise_augment(const float* in, float* out_clean, float* out_noisy, int batch, int height, int width, int channels,
                     int flip_mask, float mult_std, float add_std, uint64_t seed, void* stream);

/* Image-quality sums of two device batches a, b [batch,height,width,channels] (NHWC, both uint8 or both float32: `dtype`), what
 * tf.image.psnr / tf.image.ssim and a mean absolute error are formed from (the acceptance check of the reference's
 * tests/bfcnn/test_pretrained.py:62-78; blind_image_denoising_amd/metrics.py is the host side).  out = device double[batch][4]:
 *   out[i][0] = sum (a - b)^2, out[i][1] = sum |a - b| over image i (uint8 inputs: exact integers),
 *   out[i][2] = sum over all VALID windows and channels of the SSIM map of TF 2.13's _ssim_per_channel (window = softmax over
 *               the filter_size x filter_size grid of -(i^2 + j^2) / (2 filter_sigma^2), c1 = (k1 max_val)^2, c2 = (k2 max_val)^2),
 *   out[i][3] = the number of those terms, (height - filter_size + 1) * (width - filter_size + 1) * channels,
 * so mse = out[0] / (H W C), mae = out[1] / (H W C), psnr = 20 log10(max_val) - 10 log10(mse), ssim = out[2] / out[3].
 * filter_size odd in 3..11, height and width >= filter_size, channels in 1..4; no padding and no float copy of the images.
 * Sums are carried in fp64 and reduced in a fixed order (per-workgroup partials in `scratch`, then one workgroup per image):
 * repeated calls return the same bits.  bf_image_metrics_scratch_bytes: the scratch one call needs (BF_EINVAL for a shape the
 * call refuses); BF_EINVAL for NULL, a bad shape, dtype or window, or too little scratch. */
enum bf_dtype { BF_DTYPE_U8 = 0, BF_DTYPE_F32 = 1 };
int64_t bf_image_metrics_scratch_bytes(int batch, int height, int width, int channels, int filter_size);
int bf_image_metrics(const void* a, const void* b, int dtype, int batch, int height, int width, int channels, double max_val,
                     int filter_size, double filter_sigma, double k1, double k2, double* out, void* scratch, int64_t scratch_bytes,
                     void* stream);

/* No-reference noise statistics of one NHWC batch (dtype: bf_dtype; csrc/noise_estimate.hip) in one pass, for images that have
 * no clean counterpart.  out = double[batch][channels][4], per image and channel:
 *   out[..][0] = S = sum |L| over the (height-2)(width-2) interior pixels, L = image (*) [[1,-2,1],[-2,4,-2],[1,-2,1]]
 *   out[..][1] = sigma_fast = sqrt(pi/2) / 6 * S / ((height-2)(width-2))                 (Immerkaer 1996)
 *   out[..][2] = sigma_mad = med / 2 / 0.6745, med = the grouped-data median of q = |x00 - x01 - x10 + x11| over the complete
 *                2x2 cells (q = twice the modulus of the orthonormal Haar HH coefficient; Donoho's MAD rule).  Bin 0 of the
 *                511-bin histogram covers [0, 1/2), bin k >= 1 covers [k - 1/2, k + 1/2), the bin that holds the n/2-th of the n
 *                cells is interpolated linearly; 0 when every cell is zero.  uint8 only: NaN for float32.
 *   out[..][3] = the number of samples equal to 0 or 255 (saturation biases both estimators low).  uint8 only: NaN for float32.
 * uint8: S, the histogram and the count are 64-bit integer sums, exact in any order.  float32: L and S in fp64, reduced in a
 * fixed order.  Either way repeated calls return the same bits, and a plane inside a batch the bits of that plane alone.
 * height and width >= 3, channels in 1..4.  `scratch`: bf_noise_estimate_scratch_bytes bytes, 8-byte aligned, zeroed by the call
 * on `stream`; nothing is allocated and nothing synchronises.  BF_EINVAL for NULL, a bad shape or dtype, or short or misaligned
 * scratch. */
int64_t bf_noise_estimate_scratch_bytes(int batch, int height, int width, int channels);
int bf_noise_estimate(const void* img, int dtype, int batch, int height, int width, int channels, void* scratch,
                      int64_t scratch_bytes, double* out, void* stream);

/* Noise level statistics of one uint8 NHWC batch in one pass (csrc/noise_level.hip): the MAD estimator above conditioned on the
 * local intensity, for noise whose variance grows with the signal (var(y | x) = a x + b).  Per complete 2x2 cell and channel:
 * q = |x00 - x01 - x10 + x11| (0..510) and s = x00 + x01 + x10 + x11 (0..1020); a cell with a sample equal to 0 or 255 is excluded
 * and only counted; every other cell belongs to level l = s >> 6 (16 levels, each 16 grey levels of cell mean wide).
 *   out_levels   = double[batch][channels][16][3] = (n, the sum of s, sigma_l) per level: n cells, sigma_l = med / 2 / 0.6745 with
 *                  med the grouped-data median of the level's 511-bin histogram of q, by the rule of bf_noise_estimate (0 for an
 *                  empty level or when every cell is zero)
 *   out_excluded = double[batch][channels], the number of excluded cells
 * Everything is a 64-bit integer sum, exact in any order: repeated calls return the same bits, and an image inside a batch the
 * bits of that image alone.  height and width >= 3, channels in 1..4.  `scratch`: bf_noise_level_scratch_bytes bytes, 8-byte
 * aligned, zeroed by the call on `stream`; nothing is allocated and nothing synchronises.  BF_EINVAL for NULL, a bad shape, or
 * short or misaligned scratch. */
int64_t bf_noise_level_scratch_bytes(int batch, int height, int width, int channels);
int bf_noise_level(const uint8_t* img, int batch, int height, int width, int channels, void* scratch, int64_t scratch_bytes,
                   double* out_levels, double* out_excluded, void* stream);

/* Signal-dependent (Poisson-Gaussian) camera noise on a uint8 NHWC batch (csrc/augment.hip), channels in 1..4, H W C < 2^31 - 4096:
 *   dst = clip(rint(src + sqrt(gain[c] src + read_sigma[c]^2) z), 0, 255), in float32, z an untruncated standard normal:
 *   z = sqrt(-2 ln u1) cos(2 pi u2), u1 = ((r[0] >> 8) + 1) / 2^24, u2 = (r[1] >> 8) / 2^24, r = philox4x32_10(counter = (lo32 e,
 *   hi32 e, 0, 3), key = (lo32 seed, hi32 seed)), e = (h W + w) C + c inside the image: an image gets the same bits alone or inside
 *   a batch.  `gain` and `read_sigma` are HOST arrays of `channels` floats, read by the call and passed to the kernel by value.
 * dst may be src.  One launch, no allocation, no synchronisation.  BF_EINVAL for NULL, a bad shape, or a gain or read_sigma that is
 * negative or not finite. */
int bf_op_camera_noise_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, int C, const float* gain, const float* read_sigma,
                          uint64_t seed, void* stream);

/* Variance stabilisation of a uint8 NHWC batch whose noise variance is gain x + offset, and the way back (csrc/vst.hip; DESIGN.md
 * 7.11).  `gain` and `offset` are DEVICE arrays double[B][C] (what the fit of bf_noise_level leaves on the device), 8-byte aligned;
 * per image and channel, sanitised where they are used: a = gain finite and > 0 ? min(gain, 64) : 0, o = offset finite ?
 * clamp(offset, 1/12, 65025) : 1/12, c = 3/8 a^2 + o, rc = sqrt(c).
 *   forward: dst = rint(s u(src)), u(y) = 2 y / (sqrt(a y + c) + rc) (the generalised Anscombe transform minus its value at 0),
 *     s = 255 / u(255), in fp64 through a table per image: 0 -> 0, 255 -> 255, noise of standard deviation s everywhere, the
 *     identity for a = 0.  dst may be src.
 *   inverse: src = float32 in the stabilised domain, clamped to [0, 255]; u = src / s, x = rc u + a u^2 / 4, and with exact != 0
 *     the exact unbiased inverse of Makitalo & Foi (2013): x += a / 4 + a (K1 d - K2 d^2 + K3 d^3), d = a / (a u + 2 rc), K1 =
 *     sqrt(3/2) / 4, K2 = 11/8, K3 = 5 sqrt(3/2) / 8.  float32 arithmetic (the reciprocal to 1 ulp) on constants folded in fp64,
 *     within 1e-3 of the fp64 value (measured: 5.5e-5); dst = x clipped to [0, 255]
 *     as float32, or with cast_to_uint8 != 0 rounded half to even to uint8.  A float32 dst may be src.
 * Flat per image, channel = element index mod C: an image gets the same bits alone or inside a batch.  C in 1..4, B <= 65535,
 * H W C < 2^31 - 4096.  One launch, no atomics, no allocation, no synchronisation.  BF_EINVAL for NULL, a misaligned pointer
 * (gain, offset: 8 bytes; float32 images: 4 bytes), a bad shape, or a uint8 dst on top of its float32 src. */
int bf_op_vst_forward_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, int C, const double* gain, const double* offset,
                         void* stream);
int bf_op_vst_inverse(const float* src, void* dst, int B, int H, int W, int C, const double* gain, const double* offset, int exact,
                      int cast_to_uint8, void* stream);

/* ---- unet_laplacian backbone operators (BASELINE.json configs[4]) ------------------------------
 * What bfcnn/backbone_unet_laplacian.py:281-606 builds from keras layers, as fp32 NHWC device operators; the host
 * (blind_image_denoising_amd/unet_laplacian.py) chains them as the reference builder chains its layers.
 * All pointers are 16-byte aligned device buffers; activation codes: BF_ACT_LINEAR 0, BF_ACT_RELU 1, 2 leaky relu
 * (slope `alpha`), 3 gelu (erf form), 4 tanh.  Unsupported channel counts return BF_EUNSUPPORTED. */

/* weights of a 1x1 Conv2D [cin][cout] (HWIO) -> matrix-core operand order; cin, cout multiples of 16. */
int bf_op_pack_pointwise(const float* w, float* wp, int cin, int cout, void* stream);
/* Conv2D 1x1, use_bias=False (utilities.py:196): out = res + mult * act(in . w); mult [cout] / res [npix][cout] may be NULL. */
int bf_op_pointwise(const float* in, float* out, const float* wp, const float* mult, const float* res, int64_t npix,
                    int cin, int cout, int act, float alpha, void* stream);
/* Conv2D kh x kw, strides s, padding="same" (utilities.py:196): out = res + act(conv(in) + bias), bias [cout] (a folded
 * BatchNorm shift) / res may be NULL; wp = kh*kw
 * tap matrices [cin][cout], each packed by bf_op_pack_pointwise, tap-major; cin, cout in {32, 64, 128}.  Serves the
 * "conv2d" downsample (2x2 stride 2, downsampling.py:45-55) and the 3x3 convolution of upsample_bilinear_conv2d /
 * upsample_nearest_conv2d (upsampling.py:52-72). */
int bf_op_conv2d(const float* in, float* out, const float* wp, const float* res, const float* bias, int batch, int height,
                 int width, int cin, int cout, int kh, int kw, int stride, int act, float alpha, void* stream);
/* The decoder entry of the plain unet (bfcnn/backbone_blocks.py:383-396) in one kernel: out [B,H,W,cout] = res + act(conv_kxk(
 * Concatenate([UpSampling2D(2, nearest)(up), skip])) + bias), padding="same", stride 1, up [B,H/2,W/2,c_up], skip [B,H,W,c_skip];
 * neither the upsampled tensor nor the concat is written.  wp = the (c_up + c_skip) -> cout kernel packed as for bf_op_conv2d;
 * bias / res may be NULL.  Built for c_up = c_skip = cout in {32, 64, 128}, k in {1, 3, 5} (else BF_EUNSUPPORTED); H, W even.
 * Bitwise equal to bf_upsample2x + bf_op_concat_channels + bf_op_conv2d. */
int bf_op_upcat_conv2d(const float* up, const float* skip, float* out, const float* wp, const float* res, const float* bias,
                       int batch, int height, int width, int c_up, int c_skip, int cout, int k, int act, float alpha, void* stream);
/* DepthwiseConv2D k x k, depth_multiplier m (output channel c*m + j), padding="same", + bias[C*m] (folded BatchNorm shift,
 * may be NULL) + activation (backbone_resnet.py:165-176, block_depthwise); w [k][k][C][m]. */
int bf_op_dwconv_mult(const float* in, float* out, const float* w, const float* bias, int batch, int height, int width,
                      int channels, int multiplier, int k, int act, float alpha, void* stream);
/* bf_op_dwconv_mult followed by a 1x1 convolution cin*m -> cout (wp packed by bf_op_pack_pointwise) in one kernel:
 * out = res + act2(act1(dw(in) + bias1) . w + bias2); the cin*m-wide tensor is never written (the bottleneck tail of the
 * shipped resnet config: depthwise 3x3 x4 -> BN -> ReLU -> grouped 1x1 -> BN -> Add). */
int bf_op_dwmult_pointwise(const float* in, float* out, const float* wd, const float* bias1, int act1, float alpha1,
                           const float* wp, const float* bias2, int act2, float alpha2, const float* res, int batch, int height,
                           int width, int cin, int multiplier, int k, int cout, void* stream);
/* The whole bottleneck block of the shipped resnet config (resnet_color_1x6_bn_32x128x32_1x3x1.json; backbone_resnet.py:149-178,
 * backbone_blocks.py:160-243) in one kernel, its two 1x1 convolutions on the f16 matrix cores with split-f16 operands (hi + lo, three
 * products, fp32 accumulation -- DESIGN.md 4.2):
 *   out = [x +] act2(act1(depthwise3x3_x4(act0(x . w0 + shift0)) + shift1) . w2 + shift2)        32 -> 32 -> 128 -> 32 channels
 * replaces bf_op_pointwise followed by bf_op_dwmult_pointwise.  w0 [32][32], wd [3][3][32][4], w2 [128][32] (grouped 1x1 as a block-
 * diagonal dense matrix), BatchNorm scales folded into wd / w2 and offsets passed as shift0 [32] / shift1 [128] / shift2 [32] (or NULL).
 * Activations: 0 linear, 1 relu, 2 leaky relu (0 <= alpha <= 1); BF_EUNSUPPORTED for others.  out != x. */
int64_t bf_op_bneck_h3_pack_bytes(void);
int bf_op_pack_bneck_h3(const float* w0, const float* wd, const float* w2, void* packed, void* stream);
int bf_op_bneck_block_h3(const float* x, float* out, const void* packed, const float* shift0, int act0, float alpha0,
                         const float* shift1, int act1, float alpha1, const float* shift2, int act2, float alpha2, int add_res,
                         int batch, int height, int width, void* stream);
/* MaxPooling2D(2, 2, padding="same") (downsampling.py:56-58). */
int bf_op_maxpool2(const float* in, float* out, int batch, int height, int width, int channels, void* stream);
/* The same 1x1 convolution with the epilogues of AdditiveAttentionGate (custom_layers.py:805-832):
 * mode 0 = bf_op_pointwise;  mode 1: out = act(in . w + res);  mode 2: out = res * sigmoid(4 * mult * (in . w)) + add;
 * mode 3: out = act(in . w + mult) + res (mult = per-channel bias: a convolution with a folded BatchNorm). */
int bf_op_pointwise_ex(const float* in, float* out, const float* wp, const float* mult, const float* res, const float* add,
                       int64_t npix, int cin, int cout, int act, float alpha, int mode, void* stream);
/* ConvNextBlock conv_2 -> activation -> conv_3 -> ChannelLearnableMultiplier -> Add(skip, .) (custom_layers.py:990-1008;
 * backbone_unet_laplacian.py:351-354): out = skip + mult * (act(in . w1) . w2), w1 [C][4C], w2 [4C][C] packed as above. */
int bf_op_convnext_mlp(const float* in, const float* skip, float* out, const float* w1p, const float* w2p, const float* mult,
                       int64_t npix, int channels, int act, float alpha, void* stream);
/* The same operator on the f16 matrix cores with split-f16 operands (hi + lo f16 pairs, three products, fp32
 * accumulation: ~22 mantissa bits; needs |activation| < 65504): w1 [C][4C], w2 [4C][C] fp32 are packed once into
 * bf_op_mlp_h3_pack_bytes(C) bytes; C = 32 or 64. */
int64_t bf_op_mlp_h3_pack_bytes(int channels);
int bf_op_pack_mlp_h3(const float* w1, const float* w2, void* packed, int channels, void* stream);
int bf_op_convnext_mlp_h3(const float* in, const float* skip, float* out, const void* packed, const float* mult,
                          int64_t npix, int channels, int act, float alpha, void* stream);
/* A whole ConvNextBlock whose depthwise convolution is 1x1 (decoder_kernel_size 1) plus the residual Add, one kernel:
 * out = x + mult * (act(LayerNormalization(x * dw) * ln_gamma . w1) . w2); dw [C], ln_gamma [C] or NULL. */
int bf_op_convnext_block1_h3(const float* x, float* out, const float* dw, const float* ln_gamma, float eps, const void* packed,
                             const float* mult, int64_t npix, int channels, int act, float alpha, void* stream);
/* The first decoder block of a level with the node in front of it formed while its pixels are loaded (32 channels, 1x1 depthwise):
 * x = enc + act_up(UpSampling2D(2, "bilinear")(low)); out = x + ConvNextBlock(x)  (backbone_unet_laplacian.py:438-568, upsampling.py:80-90:
 * replaces bf_op_upsample_act_add followed by bf_op_convnext_block1_h3, bit for bit).  enc, out [B, OH, OW, 32]; low [B, OH/2, OW/2, 32];
 * OH, OW even; act_up 0 linear / 1 relu / 2 leaky relu (alpha_up).  BF_EUNSUPPORTED for other channel counts or odd sizes. */
int bf_op_convnext_block1_up_h3(const float* enc, const float* low, float* out, const float* dw, const float* ln_gamma, float eps,
                                const void* packed, const float* mult, int batch, int out_height, int out_width, int channels, int act,
                                float alpha, int act_up, float alpha_up, void* stream);
/* A CHAIN of 1..3 pixel-wise ConvNext blocks (1x1 depthwise: decoder_kernel_size 1, 32 channels) in one kernel -- the `width` decoder
 * blocks of a level (backbone_unet_laplacian.py:538-560) without a round trip through memory between them:
 *   for b in 0 .. nblocks-1:  x = x + mult[b] * (act(LayerNormalization(x * dw[b]) * gamma[b] . w1[b]) . w2[b])
 * low != NULL: the first block's input is x + act_up(UpSampling2D(2, "bilinear")(low)) (x = the encoder's skip map [B, OH, OW, 32], low
 * [B, OH/2, OW/2, 32]; OH, OW even) -- bf_op_convnext_block1_up_h3 followed by nblocks - 1 times bf_op_convnext_block1_h3.  The arrays
 * are HOST arrays of nblocks device pointers; packed[b] from bf_op_pack_mlp_h3_chain (the operand of bf_op_pack_mlp_h3 with the first
 * kernel's rows in the order the chain kernel holds a pixel's channels; same size); gamma[b] / mult[b] may be NULL.  out may alias x. */
int bf_op_pack_mlp_h3_chain(const float* w1, const float* w2, void* packed, int channels, void* stream);
int bf_op_convnext_chain32_h3(const float* x, const float* low, float* out, int nblocks, const void* const* packed,
                              const float* const* dw, const float* const* ln_gamma, const float* const* mult, float eps, int batch,
                              int out_height, int out_width, int act, float alpha, int act_up, float alpha_up, void* stream);
/* A whole encoder ConvNextBlock (k x k depthwise, k = 3 or 5, 32 channels) plus the residual Add, one kernel
 * (custom_layers.py:975-1008; backbone_unet_laplacian.py:336-354):
 * out = x + mult * (act(LayerNormalization(DepthwiseConv2D_kxk(x)) * ln_gamma . w1) . w2); dw [k][k][C]; out != x. */
int bf_op_convnext_block_h3(const float* x, float* out, const float* dw, int k, const float* ln_gamma, float eps,
                            const void* packed, const float* mult, int batch, int height, int width, int channels, int act,
                            float alpha, void* stream);
/* A/B switch between kernel variants of one operator (process-wide; tests and tools only): key "enc32":
 * 2 = wave-specialised encoder block kernel with the producers' row walk unrolled (default), 1 = wave-specialised,
 * 0 = the single-role one, 3 = two workgroups per CU, 4 = 2 with two consumer waves per SIMD (k = 3 only; k = 5 runs 2). */
int bf_op_set_variant(const char* key, int value);
/* DepthwiseConv2D k x k (SAME, zero pad; w [k][k][C]; k = 0: none) -> LayerNormalization(center=False, epsilon) * gamma
 * (ln_gamma NULL: none) -> activation   (custom_layers.py:979-988; backbone_unet_laplacian.py:355-360; the first layer of the
 * ConvNeXt block, backbone_convnext.py:108-113).  fp32 NHWC, out != in.  Built: k in {0, 1, 3, 5} for channels in {32, 64, 128,
 * 256}; k = 7 for channels in {32, 64, 128} (its own kernel, dwconv7_ln.hip: the 49 tap vectors in LDS, two columns per lane);
 * every other (channels, k) returns BF_EUNSUPPORTED.  H, W smaller than k are fine.  Deterministic: a fixed summation order. */
int bf_op_dwconv_ln(const float* in, float* out, const float* w, const float* ln_gamma, int batch, int height, int width,
                    int channels, int k, float eps, int act, float alpha, void* stream);
/* Laplacian split between levels (backbone_unet_laplacian.py:366-386): smooth = AveragePooling2D(k, strides 1, same) or,
 * with gauss [k][k], GaussianFilter; lap = in - smooth; down = smooth[:, ::2, ::2, :] (downsampling.py:61). */
int bf_op_smooth_split(const float* in, float* lap, float* down, const float* gauss, int batch, int height, int width,
                       int channels, int k, int down_stride /* 2: the slice above; 1: the whole smooth map */, void* stream);
/* The same split with the level's output normalisation in front, one kernel (backbone_unet_laplacian.py:355-386):
 * y = act(LayerNormalization(in) * ln_gamma) (ln_gamma NULL: y = act(in)) is never written; lap = y - smooth(y),
 * down = smooth(y)[:, ::2, ::2, :]; k = 3 or 5. */
int bf_op_norm_smooth_split(const float* in, const float* ln_gamma, float eps, int act, float alpha, const float* gauss,
                            float* lap, float* down, int batch, int height, int width, int channels, int k, void* stream);
/* out = other + act(UpSampling2D(2, "bilinear")(in)) (upsampling.py:80-102 + the decoder Add). */
int bf_op_upsample_act_add(const float* in, const float* other, float* out, int batch, int height, int width, int channels,
                           int act, float alpha, void* stream);
/* tf.image.resize(BILINEAR, antialias=False), half-pixel centres (custom_layers.py:1328-1334, 1351-1357). */
int bf_op_resize_bilinear(const float* in, float* out, int batch, int height, int width, int channels, int out_height,
                          int out_width, void* stream);
/* keras.layers.Attention(use_scale=False, score_mode="dot") on [query, value, key] (custom_layers.py:1345): [B][T][A], A = 32,
 * out = softmax(q k^T) v per sequence.  batch = number of sequences (images, or image rows for rank-4 inputs: keras then
 * attends along the last-but-one axis only); any length (16 queries per wave, keys walked 16 at a time). */
int bf_op_attention(const float* q, const float* v, const float* k, float* out, int batch, int tokens, int channels, void* stream);
/* The same with q / v / k rows `ld` floats apart (ld >= channels, a multiple of 4): the three projections written side by
 * side by ONE 1x1 convolution with 3 * channels outputs (q = base, the others at base + channels, base + 2 * channels). */
int bf_op_attention_ld(const float* q, const float* v, const float* k, float* out, int batch, int tokens, int channels, int ld,
                       void* stream);
/* first Conv2D k x k cin(<=4) -> cout on the (optionally) normalised image; the [Hs,Ws] source (u8 or f32) is zero-padded
 * to [H,W] before normalisation as pad_to_power_of_2 does (utilities.py:736-751; model.py:100-102). */
int bf_op_first_conv(const void* in, int in_is_u8, float* out, const float* w, int batch, int src_height, int src_width,
                     int height, int width, int cin, int cout, int k, int normalize, float v_min, float v_max, int act,
                     float alpha, void* stream);
/* The same for the one shape the unet_laplacian builder emits (5 x 5, 3 -> 32) on the f16 matrix cores with split-f16
 * operands (three products, fp32 accumulation: the arithmetic of bf_op_convnext_mlp_h3). */
int bf_op_first_conv_h3(const void* in, int in_is_u8, float* out, const float* w, int batch, int src_height, int src_width,
                        int height, int width, int normalize, float v_min, float v_max, int act, float alpha, void* stream);
/* The same for kernel sizes 3, 5 and 7 (the base convolution of the resnet configs: kernel_size 7). */
int bf_op_first_conv_h3k(const void* in, int in_is_u8, float* out, const float* w, int batch, int src_height, int src_width,
                         int height, int width, int k, int normalize, float v_min, float v_max, int act, float alpha, void* stream);
/* last Conv2D 1x1 of a denoiser head + tanh(2x)*0.51 [+ denormalise][+ round, uint8], cropped to [Ho,Wo]
 * (model.py:321-342, 136-139; module_denoiser.py:62-73). */
int bf_op_head_out(const float* in, const float* w, void* out, int out_is_u8, int batch, int height, int width, int out_height,
                   int out_width, int head_filters, int cout, int denormalize, float v_min, float v_max, int* status, void* stream);
/* A whole denoiser head in one kernel: [LayerNormalization(in) * ln_gamma (the backbone's output normalisation,
 * backbone_unet_laplacian.py:547-551; NULL: none)] -> Conv2D 1x1 cin -> 32 (w0p packed by bf_op_pack_pointwise) ->
 * activation -> Conv2D 1x1 32 -> cout (w1 [32][cout]) -> tanh(2x)*0.51 [-> denormalise][-> round, uint8], cropped. */
int bf_op_head_fused(const float* in, const float* ln_gamma, float eps, const float* w0p, int act, float alpha, const float* w1,
                     void* out, int out_is_u8, int batch, int height, int width, int out_height, int out_width, int cin,
                     int head_filters, int cout, int denormalize, float v_min, float v_max, int* status, void* stream);
/* The same head with its first 1x1 on the f16 matrix cores (split-f16 operands, three products, fp32 accumulation) for cin = 32 / 64;
 * same arguments, same operand from bf_op_pack_pointwise; BF_EUNSUPPORTED for other channel counts. */
int bf_op_head_fused_h3(const float* in, const float* ln_gamma, float eps, const float* w0p, int act, float alpha, const float* w1,
                        void* out, int out_is_u8, int batch, int height, int width, int out_height, int out_width, int cin, int hf,
                        int cout, int denormalize, float v_min, float v_max, int* status, void* stream);
/* status (both heads above; may be NULL): int32 on the device, |= BF_STATUS_F16_RANGE when the value in front of the tanh is
 * not finite -- an activation left the f16 range inside a split-f16 operator upstream; clear it with bf_op_fill32. */
int bf_op_fill32(void* p, int value, int64_t n, void* stream);
/* Conv2DTranspose k x k, stride s, padding "same", no bias (upsample_type "conv2d_transpose": bfcnn/upsampling.py:37-48,
 * utilities.py:200-202): in [B,H,W,cin] -> out [B,H*s,W*s,cout]; w [k,k,cout,cin] (keras kernel layout); act as
 * bf_op_pointwise. */
int bf_op_conv2d_transpose(const float* in, const float* w, float* out, int batch, int height, int width, int cin, int cout,
                           int k, int stride, int act, float alpha, void* stream);
/* mult[c] = tanh(relu(1 + w[c])) (ChannelLearnableMultiplier, custom_layers.py:304-306). */
int bf_op_channel_multiplier(const float* w, float* mult, int n, void* stream);

/* bf_adam_step_ex for a flat parameter vector no handle describes (models assembled from bf_op_*: unet_laplacian) */
int bf_op_adam_step(float* params, const float* grads, float* m, float* v, int64_t n, int64_t iterations, float lr, float beta_1,
                    float beta_2, float epsilon, float global_clipnorm, float clipnorm, float clipvalue,
                    const int64_t* tensor_offsets, int n_tensors, float* tensor_scratch, float grad_scale, float* losses,
                    float* scratch, void* stream);

/* ---- backward primitives of the operator library (train_prims.hip) --------------------------------------------------------
 * What `unet_laplacian` training needs beyond the forward operators (bfcnn/train_loop.py:259-312 with the multi-output hydra;
 * tf.GradientTape does this in the reference): exact fp32, NHWC, reductions through caller-supplied scratch (fixed order).
 * act codes as bf_op_pointwise (0 linear, 1 relu, 2 leaky relu(alpha), 3 exact-erf gelu). */
/* dx = dy * act'(.) ; ref = the activation's input, or (ref_is_output, relu / leaky relu / tanh (4) only) its output */
int bf_op_act_bwd(const float* ref, const float* dy, float* dx, int64_t n, int act, float alpha, int ref_is_output, void* stream);
/* 1x1 convolution weight gradient dW[cin][cout] = sum_p x[p][cin] dy[p][cout]; scratch >= cin*cout floats (more = more splits) */
int bf_op_matmul_wgrad(const float* x, const float* dy, float* dw, int64_t npix, int cin, int cout, float* scratch,
                       int64_t scratch_floats, void* stream);
/* DepthwiseConv2D k x k (same) weight gradient dw[k][k][C]; scratch >= k*k*C floats */
int bf_op_dwconv_wgrad(const float* x, const float* dy, float* dw, int batch, int height, int width, int channels, int k,
                       float* scratch, int64_t scratch_floats, void* stream);
/* LayerNormalization(center=False) backward: dx and dgamma from the layer's input x; scratch >= C floats */
int bf_op_layernorm_bwd(const float* x, const float* gamma, const float* dy, float* dx, float* dgamma, int64_t npix, int channels,
                        float eps, float* scratch, int64_t scratch_floats, void* stream);
/* out = res + t * m[c] * s[b] (ChannelLearnableMultiplier value m, StochasticDepth sample scale s, skip Add; each optional) */
int bf_op_scale_add(const float* res, const float* t, const float* m, const float* sample_scale, float* out, int batch, int64_t hw,
                    int channels, void* stream);
int bf_op_scale_add_bwd(const float* t, const float* m, const float* sample_scale, const float* dy, float* dt, float* dm, int batch,
                        int64_t hw, int channels, float* scratch, int64_t scratch_floats, void* stream);
/* ChannelLearnableMultiplier m = tanh(relu(1 + w)) (custom_layers.py:304-306): dw from dm */
int bf_op_multiplier_bwd(const float* w, const float* dm, float* dw, int n, void* stream);
/* adjoint of bf_op_smooth_split (gauss NULL: AveragePooling2D with the in-bounds divisor): dx from (dlap, ddown) */
int bf_op_smooth_split_bwd(const float* dlap, const float* ddown, const float* gauss, float* dx, int batch, int height, int width,
                           int channels, int k, void* stream);
/* the same with ddown the gradient of the full-resolution smooth map (down_stride 1: conv2d / maxpool down-sampling) or of
   smooth[:, ::2, ::2] (2); averaging or Gaussian windows of any size k <= 7 (TF same padding: the extra tap after for even k) */
int bf_op_smooth_split_bwd_ex(const float* dlap, const float* ddown, const float* gauss, float* dx, int batch, int height, int width,
                              int channels, int k, int down_stride, void* stream);
/* adjoint of MaxPooling2D(2, 2, same) (bfcnn/downsampling.py:56-68): dx [B,H,W,C] = dy [B,ceil(H/2),ceil(W/2),C] at each window's
   first maximum, 0 elsewhere */
int bf_op_maxpool2_bwd(const float* x, const float* dy, float* dx, int batch, int height, int width, int channels, void* stream);
/* adjoint of UpSampling2D(2, bilinear | nearest): dx [B,H,W,C] from dy [B,2H,2W,C] */
int bf_op_upsample2x_bwd(const float* dy, float* dx, int batch, int height, int width, int channels, int bilinear, void* stream);
/* k x k convolution (same, stride 1) weight gradient for the first convolution; x = the raw image, normalised as the forward does */
int bf_op_conv2d_wgrad(const void* x, int x_is_u8, const float* dy, float* dw, int batch, int height, int width, int cin, int cout,
                       int k, int normalize, float v_min, float v_max, float* scratch, int64_t scratch_floats, void* stream);
/* last stage of a denoiser head backward (model.py:321-342): h [npix,hf] activated hidden layer, w1 [hf,cout], dL/dpred ->
 * dh, dw1 (tanh(2x)*0.51, clip, denormalise differentiated) */
int bf_op_head_out_bwd(const float* h, const float* w1, const float* dpred, float* dh, float* dw1, int64_t npix, int head_filters,
                       int cout, int denormalize, float v_min, float v_max, float* scratch, int64_t scratch_floats, void* stream);
/* denoiser_loss of ONE output scale (loss.py:190-247) and d(total * depth_weight)/dpred; losses[BF_LOSS_COUNT] */
int64_t bf_op_denoiser_loss_scratch_floats(int batch, int height, int width, int channels);
int bf_op_denoiser_loss(const float* pred, const float* gt, int batch, int height, int width, int channels, const bf_loss_desc* loss,
                        float* dpred, float* losses, float* scratch, int64_t scratch_floats, void* stream);
/* dot-product attention for training: out = (softmax(q k^T) * pscale) v with P = softmax kept ([B,T,T]; pscale = dropout
 * keep-mask / keep-probability or NULL), and its backward (dS_scratch [B,T,T]) */
int bf_op_attention_train(const float* q, const float* v, const float* k, const float* pscale, float* out, float* P, int batch,
                          int tokens, int channels, void* stream);
int bf_op_attention_bwd(const float* q, const float* v, const float* k, const float* pscale, const float* P, const float* dout,
                        float* dq, float* dv, float* dk, float* dS_scratch, int batch, int tokens, int channels, void* stream);
/* adjoint of bf_op_resize_bilinear; scratch: B*H*out_width*C floats */
int bf_op_resize_bilinear_bwd(const float* dy, float* dx, int batch, int height, int width, int channels, int out_height,
                              int out_width, float* scratch, void* stream);
/* regularisers: value[0] += term, grad += grad_scale * d(term)/dw (bf_op_reg_elementwise: grad may be NULL, the value alone).
 * kind BF_REG_L1 / BF_REG_L2 with coefficient coef;
 * SoftOrthonormalConstraintRegularizer (regularizers.py:283-338) on a 1x1 kernel [cin][cout], scratch 2*cout*cout floats */
int bf_op_reg_elementwise(const float* w, float* grad, int64_t n, int kind, float coef, float grad_scale, float* value, void* stream);
int bf_op_reg_soft_orthonormal(const float* w, float* grad, int cin, int cout, float lambda, float l1, float l2, float grad_scale,
                               float* value, float* scratch, void* stream);
/* the same with grad NULL allowed (the value alone) and mask_diagonal 1 = SoftOrthogonalConstraintRegularizer (regularizers.py:208-280:
   the terms on W^T W with its diagonal zeroed); w is any [rows][cout] matrix: an HWIO kernel [k,k,cin,cout] with rows = k k cin */
int bf_op_reg_soft_orthogonal_ex(const float* w, float* grad, int cin, int cout, float lambda, float l1, float l2, float grad_scale,
                                 float* value, float* scratch, int mask_diagonal, void* stream);
/* weight re-layouts for the data gradients: spatial flip of [k][k][inner]; transpose of [a][b] */
/* ---- training-mode operators of the resnet builder outside the 16-filter 3x3 engine (csrc/train_generic.hip) ----
   BatchNormalization(center=False) with batch statistics, bfcnn/utilities.py:204-206 under training=True: y = act(gamma (x - mean)
   / sqrt(var + eps)); save [2C] = mean | 1 / sqrt(var + eps) for the backward; moving statistics (may be NULL) updated with
   `momentum` and the Bessel-corrected variance (fused-kernel semantics).  channels must divide 256.  Backward: dx, dgamma from dy
   (the gradient at the BatchNorm's output, in front of the activation). */
int64_t bf_op_bn_train_scratch_floats(int channels);
int bf_op_bn_train_fwd(const float* x, const float* gamma, float* y, float* save, float* moving_mean, float* moving_var, int64_t npix,
                       int channels, float eps, float momentum, int act, float alpha, float* scratch, int64_t scratch_floats,
                       void* stream);
int bf_op_bn_train_bwd(const float* x, const float* gamma, const float* save, const float* dy, float* dx, float* dgamma, int64_t npix,
                       int channels, float* scratch, int64_t scratch_floats, void* stream);
/* channel gate of add_gates (bfcnn/backbone_blocks.py:199-208): g = hard_sigmoid(relu(mean_hw(x) W0) W1), out = x * g [+ res];
   w0 [C][C8], w1 [C8][C] (keras Dense kernels, no bias), C8 <= 32; save: bf_op_gate_save_floats floats kept for the backward.
   Backward: dy = gradient at x * g; dx = gradient at x through the multiply AND the mean; dw0 / dw1 overwritten. */
int64_t bf_op_gate_save_floats(int batch, int channels, int squeeze);
int64_t bf_op_gate_scratch_floats(int batch, int channels);
int bf_op_gate_fwd(const float* x, const float* w0, const float* w1, const float* res, float* out, float* save, int batch, int64_t hw,
                   int channels, int squeeze, float* scratch, int64_t scratch_floats, void* stream);
int bf_op_gate_bwd(const float* x, const float* w0, const float* w1, const float* save, const float* dy, float* dx, float* dw0,
                   float* dw1, int batch, int64_t hw, int channels, int squeeze, float* scratch, int64_t scratch_floats, void* stream);
/* the gate's relatives on the same kernels.  m = mean_hw(sel) [B, sel_channels]; h = act0(m W0 + b0) (act0 1 relu, 2 leaky relu
   with alpha0; biases may be NULL); p = h W1 + b1; g = F(p) with mode 0 hard_sigmoid(p), 1 sigmoid(p), 2 hard_sigmoid(2.5 - relu(p)),
   3 sigmoid(2.5 - relu(p)); out = x g [+ x2 (1 - g)] [+ res].
     squeeze_and_excite_block (bfcnn/backbone_blocks.py:251-313): sel = x, act0 2 / alpha0 0.1, mode 1 (default), 0 (hard_sigmoid_version),
       2 (+ learn_to_turn_off);  selector_block, scale_type GLOBAL (custom_layers_selector.py:268-283, 316-330): sel = the selector
       layer, x = input_1, x2 = input_2, mode 2 (HARD) / 3 (SOFT).
   bf_op_selector_mix: the per-pixel form of the same mix for scale_type LOCAL (u >= 0 the up-sampled selector map):
     s = F(2.5 - u), out = x1 s + x2 (1 - s).  bf_op_avgpool_same: AveragePooling2D(pool, strides, padding "same"), any sizes,
     divisor = taps inside the image (custom_layers_selector.py:196-201). */
int64_t bf_op_channel_gate_save_floats(int batch, int sel_channels, int channels, int squeeze);
int bf_op_channel_gate_ex(const float* sel, const float* x, const float* x2, const float* res, float* out, const float* w0,
                          const float* b0, const float* w1, const float* b1, float* save, int batch, int64_t hw, int sel_channels,
                          int channels, int squeeze, int act0, float alpha0, int mode, float* scratch, int64_t scratch_floats,
                          void* stream);
int bf_op_dense2(const float* in, const float* w0, const float* b0, const float* w1, const float* b1, float* out, int64_t n,
                 int in_channels, int channels, int squeeze, int act0, float alpha0, int mode, void* stream);   /* rows of [n][in_channels]; mode 4 = relu */
int bf_op_selector_mix(const float* x1, const float* x2, const float* u, float* out, int64_t n, int soft, void* stream);
int bf_op_avgpool_same(const float* in, float* out, int batch, int height, int width, int channels, int pool_h, int pool_w,
                       int stride_h, int stride_w, void* stream);
/* add_concat_input (bfcnn/backbone_resnet.py:277-279): out [B,H,W,out_channels] = feat [channels] | normalise(x) [in_channels] | 0 ...,
   x the raw image [B,Hs,Ws,in_channels] (u8 or f32), zero-padded to [H,W] before normalisation as the first convolution sees it */
int bf_op_concat_input(const float* feat, const void* x, int x_is_u8, float* out, int batch, int height, int width, int src_height,
                       int src_width, int channels, int in_channels, int out_channels, float v_min, float v_max, void* stream);
/* selector_block's optional pre-filters (bfcnn/custom_layers_selector.py:160-185; utilities.py:566-620).  local_normalization =
   bf_op_avgpool_same (strides 1) + bf_op_center_scale (var NULL: out = (x - mean)^2; else out = (x - mean) / sqrt(var + eps));
   global_normalization = bf_op_bn_train_fwd per sample with gamma 1; lowpass / highpass: out = x (1 - tanh(a x)^b) / x tanh(a x)^b */
int bf_op_center_scale(const float* x, const float* mean, const float* var, float* out, int64_t n, float eps, void* stream);
int bf_op_pass_filter(const float* x, float* out, int64_t n, float a, int b, int highpass, void* stream);
/* their adjoints: dx of the pass filters; for y = (x - m) / sqrt(v + eps): dd = dy / sqrt(v + eps) and dv = d y / d v (bf_op_center_scale_bwd),
   then out = dd + 2 (x - m) t with t = the pooling's adjoint of dv (bf_op_center_sq_bwd); dx = out - pooling adjoint of out */
int bf_op_pass_filter_bwd(const float* x, const float* dy, float* dx, int64_t n, float a, int b, int highpass, void* stream);
int bf_op_center_scale_bwd(const float* x, const float* mean, const float* var, const float* dy, float* dd, float* dv, int64_t n, float eps,
                           void* stream);
int bf_op_center_sq_bwd(const float* x, const float* mean, const float* t, const float* dd, float* out, int64_t n, void* stream);
/* selector_block in training: adjoints of bf_op_selector_mix (dx1, dx2, du from dy), bf_op_avgpool_same (dx [B,H,W,C] from the pooled
   map's gradient; accumulate != 0: added to dx), bf_op_dense2 in its selector form (no biases, act0 = leaky ReLU alpha0, final ReLU:
   din, dw0 [in_channels][squeeze], dw1 [squeeze][channels]; scratch: bf_op_dense2_bwd_scratch_floats), and the channel slice
   dst[r][0:channels] = src[r][offset:offset+channels] that undoes bf_op_concat_channels */
int bf_op_selector_mix_bwd(const float* x1, const float* x2, const float* u, const float* dy, float* dx1, float* dx2, float* du, int64_t n,
                           int soft, void* stream);
int bf_op_avgpool_same_bwd(const float* dpooled, float* dx, int batch, int height, int width, int channels, int pool_h, int pool_w,
                           int stride_h, int stride_w, int accumulate, void* stream);
int64_t bf_op_dense2_bwd_scratch_floats(int64_t n, int channels, int squeeze);
int bf_op_dense2_bwd(const float* in, const float* w0, const float* w1, const float* dout, float* din, float* dw0, float* dw1, int64_t n,
                     int in_channels, int channels, int squeeze, float alpha0, float* scratch, int64_t scratch_floats, void* stream);
int bf_op_slice_channels(const float* src, float* dst, int64_t rows, int src_channels, int offset, int channels, void* stream);
/* selector_block's MIXED / MULTISCALE inputs (custom_layers_selector.py:203-262): keras Concatenate on the channel axis of up to
   three [rows][C*] tensors; the per-sample channel mean of x [B][hw][C] broadcast to out [B][rows_out][C]
   (tf.reduce_mean(x, axis=[1, 2], keepdims=True) added to a zeroed pooled map); scratch: bf_op_gate_scratch_floats(B, C) */
int bf_op_concat_channels(const float* a, const float* b, const float* c, float* out, int64_t rows, int ca, int cb, int cc, void* stream);
int bf_op_channel_mean_broadcast(const float* x, float* out, int batch, int64_t hw, int channels, int64_t rows_out, float* scratch,
                                 int64_t scratch_floats, void* stream);
/* the last stage of AdditiveAttentionGate (bfcnn/custom_layers.py:826-832) with the Add behind it, for training:
   out = enc * sigmoid(4 o) [+ up]; backward: denc = dy * s, do = dy * enc * 4 s (1 - s) */
int bf_op_sigmoid_gate(const float* enc, const float* o, const float* up, float* out, int64_t n, void* stream);
int bf_op_sigmoid_gate_bwd(const float* enc, const float* o, const float* dy, float* denc, float* dout_o, int64_t n, void* stream);
/* ChannelwiseMultiplier / Multiplier of the resnet builder (bfcnn/custom_layers.py:1028-1160; backbone_blocks.py:215-221): the factor
   m[c] = relu(w0[c or 0] + w1) for bf_op_scale_add (nw = C: per channel, nw = 1: one scalar), and d w0 from d m */
int bf_op_relu_shift(const float* w0, int nw, float w1, float* m, int channels, void* stream);
int bf_op_relu_shift_bwd(const float* w0, int nw, float w1, const float* dm, float* dw0, int channels, void* stream);
int bf_op_linear_shift(const float* w0, int nw, float w1, float* m, int channels, void* stream);   /* activation "linear": m = w0 + w1 */
/* the normalise / denormalise layers on their own (bfcnn/model.py:364-430; inside the hydras they are fused into the first
   convolution and the head): inverse 0: (clip(x, v_min, v_max) - v_min) / (v_max - v_min) - 0.5; 1: (clip(x, -.5, .5) + .5) * range + v_min */
int bf_op_normalize(const float* x, float* out, int64_t n, float v_min, float v_max, int inverse, void* stream);
/* layout helpers: out[r][c * m + j] = x[r][c] (a DepthwiseConv2D with depth_multiplier m is a plain depthwise convolution of the
   repeated tensor) and its adjoint out[r][c] = sum_j x[r][c * m + j]; keras Conv2D(groups) kernel [cin / groups][cout] to / from the
   block-diagonal dense [cin][cout] (extract = 1 writes w from dense) */
int bf_op_channel_repeat(const float* x, float* out, int64_t npix, int channels, int m, void* stream);
int bf_op_channel_group_sum(const float* x, float* out, int64_t npix, int channels, int m, void* stream);
int bf_op_group_kernel(float* w, float* dense, int cin, int cout, int groups, int extract, void* stream);
int bf_op_flip_hw(const float* w, float* out, int k, int inner, void* stream);
int bf_op_transpose2d(const float* w, float* out, int a, int b, void* stream);

/* ---- data-parallel exchange (the reference is single-device, bfcnn/train_loop.py:259-321) -----------------
 * ONE sum-all-reduce of the flat fp32 gradient buffer over RCCL per training step; every rank then runs the identical
 * bf_adam_step with grad_scale = 1 / world.  RCCL is bound at run time: BF_EUNSUPPORTED when librccl is not installed.
 *   rank 0: bf_comm_unique_id(id) -> id to every rank over any host channel -> each rank, with ITS GPU current:
 *   bf_comm_init_rank(&comm, world, rank, id) -> per step bf_allreduce_grads(h, grads, n, comm, stream) -> bf_comm_destroy.
 * `comm` is an ncclComm_t; one the host already owns (e.g. from its own ncclCommInitRank) is accepted as well. */
int bf_comm_unique_id(char id_out[128]);
int bf_comm_init_rank(void** comm_out, int world, int rank, const char id[128]);
int bf_comm_destroy(void* comm);
int bf_allreduce_grads(bf_handle h, float* grads, int64_t n, void* comm, void* stream);
const char* bf_comm_last_error(void);

/* y += a * x over n floats (overwrite != 0: y = x): gradient accumulation over micro-batches (bfcnn/train_loop.py:296-310). */
int bf_op_axpy(float* y, const float* x, float a, int overwrite, int64_t n, void* stream);

/* ---- weight pruning on the flat parameter vector (bfcnn/pruning.py:68-205; blind_image_denoising_amd/pruning.py is the host side) ----
 * w = device float[n], pruned IN PLACE; ranges = device int64[n_tensors][2], the [begin, end) element range of every tensor to
 * prune (the Conv2D / DepthwiseConv2D kernels); an element outside every range is never written, and a range is clipped to
 * [0, n).  Codes are the values of the reference's PruneStrategy; comparisons and products are fp32, i.e. what NumPy computes on a
 * float32 array with a Python scalar, so every strategy but BIFURCATE reproduces the NumPy result bit for bit.
 *   NONE                          nothing is launched
 *   MINIMUM_THRESHOLD             w = 0 where |w| < minimum_threshold (strict)
 *   MINIMUM_THRESHOLD_SHRINKAGE   w *= shrinkage where |w| < shrinkage_threshold, then w = 0 where |w| < minimum_threshold
 *   MINIMUM_THRESHOLD_BIFURCATE   where |w| < minimum_threshold, w = a draw from U(-2t, 2t); then w = 0 where |w| < minimum_threshold.
 *                                 The draw of element i is s * 2t with s = (2 m + 1) / 2^24 - 1, m = the top 24 bits of word 0 of
 *                                 Philox4x32-10(counter = (i lo, i hi, 0, 0), key = seed): it depends on the seed and on the
 *                                 element's position in w alone.
 *   DROP_BOTTOM                   per tensor, threshold = the element of rank kth[tensor] (0-based; the host passes
 *                                 int(np.round(size * percentage)) and refuses a rank outside the tensor) in ascending order of |w|,
 *                                 found exactly by a four-pass radix select over the bit patterns of |w|; it is written to
 *                                 thresholds[tensor]; then w = 0 where |w| < threshold (strict: ties at the threshold survive).  kth =
 *                                 device int64[n_tensors], thresholds = device float[n_tensors]; both are read / written by this
 *                                 strategy only (NULL otherwise).  A tensor holds fewer than 2^31 elements.
 * PCA_PROJECTION (4) returns BF_EUNSUPPORTED: it is a host eigen-decomposition.  BF_EINVAL for NULL or empty arguments. */
enum bf_prune_strategy {
    BF_PRUNE_NONE = 0, BF_PRUNE_MINIMUM_THRESHOLD = 1, BF_PRUNE_MINIMUM_THRESHOLD_BIFURCATE = 2,
    BF_PRUNE_MINIMUM_THRESHOLD_SHRINKAGE = 3, BF_PRUNE_PCA_PROJECTION = 4, BF_PRUNE_DROP_BOTTOM = 5
};
int bf_op_prune_tensors(float* w, int64_t n, const int64_t* ranges, int n_tensors, int strategy, float minimum_threshold,
                        float shrinkage, float shrinkage_threshold, uint64_t seed, const int64_t* kth, float* thresholds,
                        void* stream);
/* counts[tensor] = number of elements of the tensor's range with |w| <= threshold (threshold 0: exact zeros, -0.0 included);
 * counts = device int64[n_tensors]; one workgroup per tensor, reduced in a fixed order. */
int bf_op_count_below(const float* w, int64_t n, const int64_t* ranges, int n_tensors, float threshold, int64_t* counts,
                      void* stream);

/* ---- self-ensemble: the dihedral group D4 around a denoiser (blind_image_denoising_amd/self_ensemble.py is the host side) ----
 * Member k = 0..7 of x[B,H,W,C] is T_k(x) = flipW^(k >> 2)(rot90^(k & 3)(x)), rot90 = np.rot90(x, 1, axes=(1, 2)) (counter-
 * clockwise), flipW = x[:, :, ::-1]; T_k^-1(y) = rot90^(-(k & 3))(flipW^(k >> 2)(y)).  Even k keeps the shape, odd k swaps H and W.
 * `members` is a bit mask over k (1..255).  Layout of a set of members: the even ones in one batch [n_even*B, H, W, C], the odd
 * ones in another [n_odd*B, W, H, C], each member-major in ascending k (member j of a batch = its images j*B .. (j+1)*B-1).  A
 * NULL odd batch while odd members are selected means the JOINT layout, for H == W only (BF_EINVAL otherwise): all selected
 * members in the even batch, [n*B, H, W, C], member-major in ascending k.  C is 1 or 3 (BF_EUNSUPPORTED otherwise); any H, W,
 * B >= 1 (B and ceil(H / 32) at most 65535).  One launch each, no allocation, no synchronisation, graph-capturable.
 *
 * bf_op_dihedral_stack_u8: reads src once and writes every selected member.  src must not alias a destination.
 * bf_op_dihedral_merge: per output element s = f_k0[T_k0^-1 position]; s += f_k1[...]; ... over the selected members in ascending
 *   k (sequential fp32 adds), m = s / (float)n (correctly rounded), out = m as float32 (out_u8 == 0) or
 *   (uint8) rintf(fminf(fmaxf(m, 0), 255)) -- round half to even, what the head kernels do.  Every input is read once, out
 *   [B,H,W,C] is written once.  The order of the sum is part of the contract: the result is reproducible bit for bit. */
int bf_op_dihedral_stack_u8(const uint8_t* src, uint8_t* dst_even, uint8_t* dst_odd, int B, int H, int W, int C, int members,
                            void* stream);
int bf_op_dihedral_merge(const float* src_even, const float* src_odd, void* out, int B, int H, int W, int C, int members,
                         int out_u8, void* stream);

/* ---- tiled inference: overlapping tiles of one shape around a denoiser (blind_image_denoising_amd/tiling.py is the host side;
 * csrc/tiling.hip) ----
 * Plan per axis (length H, nominal tile T, overlap O, margin M; valid for T >= 1, 0 <= 2 M <= O <= T / 2):
 *   tile extent t = min(T, H); tile count n = 1 if H <= T, else ceil((H - O) / (T - O)); origins y_i = (i (H - t)) / (n - 1)
 *   (integer division; y_0 = 0 for n == 1).  The origins increase strictly, the first is 0, the last tile ends at H, neighbours
 *   overlap by at least O.  All tiles of a plan have the shape [t_h, t_w].
 * Integer weight of tile i at its local coordinate u in [0, t), with R = O - 2 M:
 *   lead(u) = R + 1 if y_i == 0, else clamp(u - M + 1, 0, R + 1);  trail(u) = R + 1 if y_i + t == H, else clamp(t - M - u, 0, R + 1);
 *   a_i(u) = min(lead, trail).  A tile's weight at a pixel is a_iy(y - y_iy) a_ix(x - x_ix): the outer M pixels of every interior
 *   tile edge weigh nothing, edges on the image border lose nothing, and every pixel has a positive weight from 1 to 3 tiles per axis.
 * Tile order: (b, iy, ix) row-major, N = B ny nx tiles.  `overlap` and `margin` hold for both axes.
 * Blend, per output sample, in fp64: num = sum w (double) f, den = sum w over the tiles with w > 0 in ascending tile order,
 *   q = num / den (correctly rounded); float32 result (float) q; uint8 result rintf(fminf(fmaxf((float) q, 0), 255)), half to even.
 *   The weights are small integers, each product is exact in fp64: the result is reproducible bit for bit.
 * C is 1 or 3 (BF_EUNSUPPORTED otherwise, and for frames beyond the kernels' 32-bit plan arithmetic: (n - 1) H >= 2^31 on an axis,
 * B H >= 2^31, a tile of 2^31 bytes, W > 65535 * 256).  BF_EINVAL for NULL or aliased pointers, sizes below 1, an invalid plan
 * or a tile range outside [0, N).  Scalars only: one launch each, no upload, no allocation, no synchronisation, graph-capturable.
 * Every element offset is 64-bit.
 *
 * bf_op_tile_split_u8: tiles [first, first + count) of the tile order of src[B,H,W,C] -> dst[count, t_h, t_w, C].
 * bf_op_tile_blend: tiles[N, t_h, t_w, C] float32 -> out[B,H,W,C], float32 (out_is_u8 == 0) or uint8; a gather, one thread per
 *   output pixel, no atomics. */
int bf_op_tile_split_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, int C, int tile_h, int tile_w, int overlap,
                        int64_t first, int64_t count, void* stream);
int bf_op_tile_blend(const float* tiles, void* out, int out_is_u8, int B, int H, int W, int C, int tile_h, int tile_w,
                     int overlap, int margin, void* stream);

/* ---- spatially correlated noise: its reach, pixel-shuffle down-sampling and random-replacing refinement around a denoiser
 * trained on white noise (blind_image_denoising_amd/pixel_shuffle.py is the host side; csrc/pixel_shuffle.hip) ----
 * Every entry takes scalars only: no upload, no allocation, no synchronisation, graph-capturable.  C in 1..4.
 *
 * bf_noise_correlation: the dilated Haar statistic of one uint8 NHWC batch in one pass.  For s = 1..max_stride (1..8), per image
 *   and channel, q_s(y,x) = |x(y,x) - x(y,x+s) - x(y+s,x) + x(y+s,x+s)| (0..510) at the (H - s)(W - s) positions with y + s < H and
 *   x + s < W.  `scratch` (bf_noise_correlation_scratch_bytes bytes, 8-byte aligned, zeroed by the call on `stream`) receives the
 *   exact histograms, int64 [B][C][max_stride][512] (bin 511 is padding and stays 0); out_sigma = double [B][C][max_stride], the
 *   grouped-data median of the histogram / 2 / 0.6745 by the rule of bf_noise_estimate.  H, W >= max_stride + 1.  The counts are
 *   64-bit integer sums, exact in any order: repeated calls return the same bits, an image inside a batch the bits of that image
 *   alone.  BF_EINVAL for NULL, a bad shape or stride, or short or misaligned scratch.
 *
 * bf_op_pd_split_u8 / bf_op_pd_merge: Hs = ceil(H / s), Ws = ceil(W / s), s = `stride` in 1..8 (BF_EUNSUPPORTED beyond), H, W >= 2 s
 *   unless s == 1 (BF_EINVAL).
 *   split: src uint8 [B,H,W,C] -> dst uint8 [B s^2, Hs, Ws, C]; member b s^2 + i s + j at (u, v) = src(b, y, x) with y = u s + i, lowered
 *     by s when that is >= H (the last row of the SAME phase is repeated), x = v s + j likewise.
 *   merge: src float32 [B s^2, Hs, Ws, C] -> out [B,H,W,C], out(b,y,x,c) = src(b s^2 + (y mod s) s + (x mod s), y div s, x div s, c);
 *     float32 (out_is_u8 == 0) or uint8 = rintf(fminf(fmaxf(v, 0), 255)), half to even.  s == 1 is a copy / a cast.
 *
 * bf_op_pd_replace_u8 / bf_op_pd_mean: `copies` = T in 1..16, H W C < 2^31 - 4096, B <= 65535.
 *   replace: base, noisy uint8 [B,H,W,C] -> dst uint8 [B T, H, W, C]; member b T + t is `base` with the pixels (all channels) replaced
 *     by `noisy` whose Philox word is below `threshold`: pixel p = y W + x (image-local: every image gets the same masks) takes word
 *     p & 3 of philox4x32_10(counter = (lo32 g, hi32 g, t, 5), key = (lo32 seed, hi32 seed)), g = p >> 2.  threshold 0 replaces nothing.
 *   mean: src float32 [B T, H, W, C] -> out [B,H,W,C] = (fp64 sum over t ascending) / T, one correctly rounded division, cast to
 *     float32, or clipped and rounded half to even to uint8. */
int64_t bf_noise_correlation_scratch_bytes(int B, int H, int W, int C, int max_stride);
int bf_noise_correlation(const uint8_t* img, int B, int H, int W, int C, int max_stride, void* scratch, int64_t scratch_bytes,
                         double* out_sigma, void* stream);
int bf_op_pd_split_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, int C, int stride, void* stream);
int bf_op_pd_merge(const float* src, void* out, int out_is_u8, int B, int H, int W, int C, int stride, void* stream);
int bf_op_pd_replace_u8(const uint8_t* base, const uint8_t* noisy, uint8_t* dst, int B, int H, int W, int C, int copies,
                        unsigned threshold, uint64_t seed, void* stream);
int bf_op_pd_mean(const float* src, void* out, int out_is_u8, int B, int H, int W, int C, int copies, void* stream);

/* ---- burst merge: block-matching alignment of T frames to one of them and the robust temporal merge along the alignment
 * (blind_image_denoising_amd/burst.py is the host side; csrc/burst.hip) ----
 * frames = uint8 [B,T,H,W,C], T in 1..16, C in 1..4, `ref` in 0..T-1 the reference frame; clamp(p) clips a coordinate to the frame.
 * Everything is integer arithmetic up to the one division of the merge.  Scalars only: no upload, no allocation, no
 * synchronisation, graph-capturable.  BF_EINVAL for NULL, a bad shape or setting, short or misaligned buffers, and frames beyond
 * the kernels' 32-bit arithmetic (H W C > 2^29 - 1, B T (H W / 16 + H + W + 1) > 2^29 - 1).
 *
 * Luma pyramid, `levels` = K in 1..4: L_0 = (2 sum_c x_c + C) / (2 C) (integer division), uint8; level k + 1 is ceil(H_k / 2) x
 *   ceil(W_k / 2), each value (the sum of the 2 x 2 cell at (2 y, 2 x), coordinates clamped, + 2) >> 2.
 * Alignment: tiles of 16 x 16 at every level, the grid of level k is gy_k x gx_k = ceil(H_k / 16) x ceil(W_k / 16), edge tiles are
 *   cut by the frame.  Coarsest level first; tile (i, j) of level k starts from d0 = 2 d_{k+1}[min(i >> 1, gy_{k+1} - 1),
 *   min(j >> 1, gx_{k+1} - 1)] (0 at the coarsest level) and takes, among d = d0 + (u, v), u, v in -R..R (`search` = R in 1..7),
 *   the one with the smallest key (cost, u u + v v, u, v), compared lexicographically,
 *   cost(d) = sum over the tile's pixels p of |L_ref(p) - L_alt(clamp(p + d))|.
 *   field_out = int32 [B,T,gy_0,gx_0,2] as (dy, dx), zero for t == ref.  The reach is R (2^K - 1) pixels.
 * Scratch (bf_burst_align_scratch_bytes bytes, 16-byte aligned), every part starting on a multiple of 16 bytes and padded to one:
 *   uint8 [B T, H_k, W_k] luma for k = 0..K-1, then int32 [B T, gy_k, gx_k, 2] fields for k = 1..K-1.  Both are left behind
 *   for the caller to read.
 *
 * Merge: pixel p lies in tile (p_y / 16, p_x / 16) whose displacement in frame t is d_t = field[b,t,.,.].
 *   D_t = sum over q in the 5 x 5 window around p (q clamped first), over the channels, of (alt_t(clamp(q + d_t)) - ref(q))^2;
 *   thresholds = int64 [B,2] = (lo, hi) per image, 0 <= lo < hi < 2^54;
 *   w_t = 256 if D_t <= lo, 0 if D_t >= hi, else ((hi - D_t) 256) / (hi - lo) (integer division); w_ref = 256;
 *   num_c = sum_t w_t alt_t,c(clamp(p + d_t)), den = sum_t w_t, sq = sum_t w_t^2;
 *   out [B,H,W,C] = (float) ((double) num_c / (double) den): one correctly rounded division, one cast (out_is_u8 == 0), or that
 *   float32 value rounded half to even to uint8.  counts_or_null = int32 [B,H,W,2] = (den, sq): the noise of the merged pixel is
 *   sigma sqrt(sq) / den.  A displacement is any int32 (clamp saturates).  `out` must not alias `frames`. */
int64_t bf_burst_align_scratch_bytes(int B, int T, int H, int W, int C, int levels);
int bf_burst_align(const uint8_t* frames, int B, int T, int H, int W, int C, int ref, int levels, int search, void* scratch,
                   int64_t scratch_bytes, int* field_out, void* stream);
int bf_op_burst_merge(const uint8_t* frames, const int* field, const int64_t* thresholds, int B, int T, int H, int W, int C, int ref,
                      void* out, int out_is_u8, int* counts_or_null, void* stream);

/* ---- video: one step of the recursive motion-compensated temporal filter (blind_image_denoising_amd/video.py is the host side;
 * csrc/video.hip) ----
 * The state of B parallel streams: acc = uint16 [B,H,W,C], the accumulated frame times 256, in 0..65280; cnt = uint16 [B,H,W], the
 * number of frames in a pixel times 256, 0 = empty.  The state's image is state8 = (acc + 128) >> 8 as uint8.
 * x = uint8 [B,H,W,C] the new frame, C in 1..4; field = int32 [B,gy,gx,2] as (dy, dx) on the 16 x 16 tiles of bf_burst_align (its
 * field of frame 1 of the pair (x, state8_in) with ref 0), any int32 (clamp saturates); thresholds = int64 [B,2] = (lo, hi) per
 * image, 0 <= lo < hi < 2^54; n_max in 1..64 the temporal support.  clamp(p) clips a coordinate to the frame.  All integers, for
 * pixel p in tile (p_y / 16, p_x / 16) with displacement d:
 *   D = sum over q in the 5 x 5 window around p (q clamped first), over the channels, of (state8_in(clamp(q + d)) - x(q))^2;
 *   w = 256 if D <= lo, 0 if D >= hi, else ((hi - D) 256) / (hi - lo)   (the ramp of bf_op_burst_merge);
 *   s = clamp(p + d);  n = min(cnt_in(s), 256 (n_max - 1));  m = (w n) >> 8;  den = 256 + m;
 *   acc_out(p, c) = (65536 x(p, c) + m acc_in(s, c) + (den >> 1)) / den;  cnt_out(p) = den;
 *   image_out(p, c) = uint8 (acc_out + 128) >> 8, the image of the new state (what the next step aligns against, and the uint8
 *   output);  out_f32_or_null(p, c) = float32 acc_out / 256 (exact).
 * An empty state passes the frame through (acc = 256 x, cnt = 256) whatever field and acc_in hold; so does n_max = 1.
 * state8_in is derived from acc_in, not read.  Scalars only: no upload, no allocation, no synchronisation, graph-capturable.
 * BF_EINVAL for NULL (but out_f32_or_null), a bad shape or setting, n_max outside 1..64, misaligned pointers (2 bytes for acc and
 * cnt, 4 for field and out_f32, 8 for thresholds), frames beyond the kernel's 32-bit arithmetic (H W C > 2^29 - 1,
 * B (H W / 16 + H + W + 1) > 2^29 - 1), and when an output overlaps an input or another output: a tile reads its neighbours'
 * frame and state, the step is not in place. */
int bf_op_video_update(const uint8_t* x, const uint16_t* acc_in, const uint16_t* cnt_in, const int* field, const int64_t* thresholds,
                       int B, int H, int W, int C, int n_max, uint16_t* acc_out, uint16_t* cnt_out, uint8_t* image_out,
                       float* out_f32_or_null, void* stream);

/* ---- non-local means: a denoiser without weights (Buades, Coll, Morel 2005; blind_image_denoising_amd/nlm.py is the host side;
 * csrc/nlm.hip) ----
 * images = uint8 [B,H,W,C], C in 1..4, B H W C < 2^31; `patch` = p in 1..3, `search` = r in 1..10; n = C (2 p + 1)^2.
 * table = int32 [1024], TABLE[i] = rint(4096 exp(-(i + 0.5) 9 / 1024)) for i < 1023, TABLE[1023] = 0 (nlm.nlm_table builds it; the
 * kernel evaluates no exponential).  params = int64 [B,2] = (offset, mult) per image, 0 <= offset, 0 <= mult <= 2^32 - 1 (values
 * outside are clamped to that range; nlm.nlm_params makes them from a noise level).  P = the image with edge replication.
 * Pixel x, every offset d != 0 with |dy|, |dx| <= r and q = x + d inside the frame (candidates outside are left out):
 *   D = sum over c and |u|, |v| <= p of (P[x + (u,v), c] - P[q + (u,v), c])^2  (< 2^24);  a = max(D - offset, 0);
 *   idx = min((a mult) >> 32, 1023) (a 64-bit product);  w = TABLE[idx] -- but every w is 0 when mult == 2^32 - 1: the filter is
 *   off, the image comes back unchanged;
 *   the centre gets w_c = max(1, max_q w);  num_c = sum_q w I[q,c] + w_c I[x,c],  den = sum_q w + w_c  (both < 2^31);
 *   out [B,H,W,C] = (float) ((double) num_c / (double) den): one correctly rounded division, one cast (cast_to_uint8 == 0), or
 *   uint8 (2 num_c + den) / (2 den) (integer division).  weights_or_null = int32 [B,H,W] = den.
 * Sums of integers: the result does not depend on the launch geometry.  One launch, no allocation, no synchronisation:
 * graph-capturable.  BF_EINVAL for NULL, a bad shape or setting, a misaligned pointer, or out == images. */
int bf_op_nlm(const uint8_t* images, const int64_t* params, const int32_t* table, int B, int H, int W, int C, int patch, int search,
              void* out, int cast_to_uint8, int32_t* weights_or_null, void* stream);

/* ---- BM3D: block matching and collaborative filtering (Dabov, Foi, Katkovnik, Egiazarian 2007; blind_image_denoising_amd/bm3d.py
 * is the host side; csrc/bm3d.hip) ----
 * noisy, guide = uint8 [B,H,W,C], C in 1..4, H, W >= 8, B H W C < 2^31; `search` = r in 1..12, `step` in 1..8.  Blocks are 8 x 8, a
 * group holds at most 16.  Hn = the Sylvester Hadamard matrix, H2n = [[Hn, Hn], [Hn, -Hn]].  Per C a forward matrix A with squared
 * row norms n2 and a back matrix Bk, Bk A = s I:  C = 1: [1], s = 1;  C = 2: A = Bk = H2, n2 = 2, s = 2;  C = 4: A = Bk = H4, n2 = 4,
 * s = 4;  C = 3: A = [1,1,1], [1,0,-1], [1,-2,1], n2 = 3, 2, 6, Bk = [2,3,1], [2,0,-2], [2,-3,1], s = 6.
 * params = int64 [B,4] = (tau1, thr1, tau2, v1) per image, each >= 0 (negative values are taken as 0; bm3d.bm3d_params makes them
 * from a noise level).  `wiener` == 0 reads tau = tau1 and thr1, else tau = tau2 and v1.
 * Reference blocks: top-left corners 0, step, 2 step, ... <= n - 8 and n - 8 along each axis.  For each, the candidates are the
 * blocks (cy, cx) with max(0, y - r) <= cy <= min(H - 8, y + r) and the same in x (no padding):
 *   D = the squared difference of the guide's blocks over 64 pixels and C channels (< 2^24); a candidate counts if D <= tau, the
 *   reference itself always; key = (D << 10) | ((dy + r)(2 r + 1) + dx + r), the reference's own -1; the group is the first K by
 *   ascending key, K = the largest power of two <= min(count, 16).
 *   t = H8 block H8 of the noisy blocks, then HK along the group, then A along the channels (|t| <= 255 * 64 * 16 * 4 < 2^20); with
 *   `wiener` tb = the same of the guide's blocks.
 *   wiener == 0:  t stays where t t > (thr1 K) n2[c], else 0; w = max(4096 / max(number kept, 1), 1).
 *   wiener != 0:  S = tb tb, g = (S << 12) / max(S + (v1 K) n2[c], 1) (<= 4096; S << 12 <= 2^52), t = (t g + 2048) >> 12
 *                 (arithmetic shift); w = min(max(2^36 / max(sum of g g, 1), 1), 2^14)  (sum of g g <= 2^36).
 *   back: Bk along the channels, HK along the group, H8 . H8 per block, times 16 / K: the scale is 1024 s.
 *   acc [B,H,W,C+1] int64: for every pixel of the K blocks num[pixel, c] += w value, den[pixel] += w (den is the last entry).
 * Bounds.  |t| never grows in the shrinkage, and a back transform of any subset of 2^m coefficients is at most 2^(m/2) times their
 * root sum of squares, so with rowabs(A) = (3, 2, 4) and a row of |Bk| = (2, 3, 1) (C = 3; 4 x 4 for C = 4) every back value is
 * below 2^15 * 255 * 16 < 2^27 and the kernel's transform is 32-bit.  One contribution w value is below 2^41.  A pixel lies in 64
 * blocks, each a member of at most (2 r + 1)^2 groups: at step 1 and r = 12 that is 40 000 < 2^16 contributions, |num| < 2^57,
 * den < 2^30, and d = den 1024 s < 2^43 below.
 * bf_op_bm3d_step zeroes acc on the stream (hipMemsetAsync) and launches; a tile of reference blocks is summed in LDS first.  Integer sums: the result
 * does not depend on the order of the atomic adds.  No allocation, no synchronisation: graph-capturable.
 * bf_op_bm3d_finish: d = den 1024 s; out [B,H,W,C] = uint8 min((2 max(num, 0) + d) / (2 d), 255) (integer division), or with
 * cast_to_uint8 == 0 (float) ((double) num / (double) d), one correctly rounded division and one cast, not clipped;
 * weights_or_null = int64 [B,H,W] = den (>= 1 after a step: every pixel lies in a reference block).
 * BF_EINVAL for NULL (but weights_or_null), a bad shape or setting, a misaligned pointer (8 bytes for params, acc and weights, 4
 * for a float out), or when acc is one of the other buffers. */
int bf_op_bm3d_step(const uint8_t* noisy, const uint8_t* guide, const int64_t* params, int B, int H, int W, int C, int search, int step,
                    int wiener, int64_t* acc, void* stream);
int bf_op_bm3d_finish(const int64_t* acc, int B, int H, int W, int C, void* out, int cast_to_uint8, int64_t* weights_or_null,
                      void* stream);

/* ---- restoration with the denoiser's implicit prior: the state update of Kadkhodaie & Simoncelli, "Stochastic solutions for linear
 * inverse problems using the prior implicit in a denoiser" (NeurIPS 2021), Algorithm 2, between two denoiser calls
 * (blind_image_denoising_amd/restore.py is the host side; csrc/restore.hip) ----
 * Images are float32 [B,H,W,C] on the 0..255 scale, C in 1..4, n = H W C < 2^31.  A constraint is an orthogonal projection P and an
 * anchor a = the measurement embedded in image space:
 *   kind 0 (mask):  mask = uint8 [B,H,W,mask_channels], mask_channels = 1 (all channels) or C; m = (mask != 0); P v = m v;
 *                   anchor = the measured image [B,H,W,C], uint8 or float32 (anchor_is_u8); its values where m = 0 are never read.
 *   kind 1 (block): factor = s in 2..8, H and W multiples of s; P v = every s x s block of every channel replaced by its mean;
 *                   anchor = the low-resolution image [B,H/s,W/s,C], uint8 or float32; a = it repeated s x s.  mask is not read.
 * Every output element is formed in fp64 from its float32 operands and rounded to float32 once.
 * z_t = standard normals: elements 4 g .. 4 g + 3 of an image (flat index inside the image) share philox4x32_10(counter = (g,
 *   sample_id, t, 6), key = (lo32 seed, hi32 seed)); words (0, 1) give elements 4 g and 4 g + 1 as the cosine and sine branch of
 *   Box-Muller with u1 = ((r0 >> 8) + 1) / 2^24, u2 = (r1 >> 8) / 2^24, words (2, 3) elements 4 g + 2 and 4 g + 3 in the same way.
 *   sample_id = uint32 [B] on the device, NULL: the image's index b.
 * No entry uploads, allocates or synchronises: graph-capturable.  BF_EINVAL for NULL, C outside 1..4, n >= 2^31, s outside 2..8, H
 * or W no multiple of s, mask_channels neither 1 nor C, a misaligned pointer, aliased outputs, short scratch; nothing is launched.
 *
 * bf_op_restore_init:      y = 127.5 (1 - P 1) + a + sigma_0 z_0   (mask: a where measured, 127.5 elsewhere; block: a).
 * bf_op_restore_direction: d = D - y + a - P D  (= (I - P)(D - y) + (a - P y); the mask form selects a - y or D - y) from y and
 *   D = `denoised`; sumsq = double [B] = sum over the image of d^2, of the fp64 values before their rounding to float32.  The sum
 *   is the fixed-order two-stage sum of csrc/block_reduce.h through `scratch` (bf_op_restore_scratch_bytes bytes, 8-byte aligned;
 *   no atomics): the same bits in two calls, and for an image alone or inside a batch.  d must not alias y or denoised.
 * bf_op_restore_step:      iteration t >= 1 with the step size h_t in (0, 1], beta in [0, 1], sigma_l > 0.  Per image, all on the
 *   device: sigma_t = sqrt(sumsq / n); trace_or_null = double [trace_rows, B] gets trace[t - 1][b] = sigma_t (t <= trace_rows);
 *   the image MOVES when steps[b] == t - 1 (it has moved in every iteration before) and sigma_t > sigma_l:
 *   gamma_t^2 = ((1 - beta h_t)^2 - (1 - h_t)^2) sigma_t^2,  y += h_t d + gamma_t z_t  in place,  steps[b] = t;
 *   else it is frozen: y and steps[b] (int32 [B], zero before t = 1) stay as they are, now and in every later iteration.
 *   No noise is drawn when gamma_t = 0 (beta = 1).  y must not alias d.
 * bf_op_restore_finish:    x = D - P D + a from D = the denoiser's output for the final y; with a mask the measured samples are
 *   the measurement itself (a select, not arithmetic).  out = float32 [B,H,W,C], or uint8 (out_is_u8): rounded half to even and
 *   clipped to 0..255, as the head kernel does.  out must not alias denoised. */
int64_t bf_op_restore_scratch_bytes(int B, int H, int W, int C);
int bf_op_restore_init(float* y, int B, int H, int W, int C, int kind, const uint8_t* mask, int mask_channels, int factor,
                       const void* anchor, int anchor_is_u8, double sigma_0, uint64_t seed, const uint32_t* sample_id_or_null,
                       void* stream);
int bf_op_restore_direction(const float* y, const float* denoised, int B, int H, int W, int C, int kind, const uint8_t* mask,
                            int mask_channels, int factor, const void* anchor, int anchor_is_u8, float* d, void* scratch,
                            int64_t scratch_bytes, double* sumsq, void* stream);
int bf_op_restore_step(float* y, const float* d, const double* sumsq, int B, int H, int W, int C, double h_t, double beta,
                       double sigma_l, int t, uint64_t seed, const uint32_t* sample_id_or_null, double* trace_or_null, int trace_rows,
                       int* steps, void* stream);
int bf_op_restore_finish(const float* denoised, int B, int H, int W, int C, int kind, const uint8_t* mask, int mask_channels,
                         int factor, const void* anchor, int anchor_is_u8, void* out, int out_is_u8, void* stream);

/* ---- risk estimation without a clean image: Stein's unbiased risk estimate around a denoiser (blind_image_denoising_amd/risk.py
 * is the host side; csrc/risk.hip).  For y = x + n, n ~ N(0, sigma^2): E |f(y) - x|^2 / N = E[ |f(y) - y|^2 / N - sigma^2 +
 * (2 sigma^2 / N) div f(y) ], div f(y) ~ s . (f(y + a s) - f(y)) / a for a random sign vector s (Ramani, Blu, Unser 2008).
 * Probe p = 1..probes (at most 8) of amplitude a = `amplitude` grey levels (1..16).  Sign of element e = (h W + w) C + c of an
 * image (the same for every image of a batch): j = e >> 2, i = e & 3, r = philox4x32_10(counter = (lo32 j, hi32 j, p, 2),
 * key = (lo32 seed, hi32 seed)), s = +1 when bit 31 of r[i] is set, else -1; s = -s when y + a s leaves 0..255.
 * channels in 1..4, any B, H, W >= 1 with H W C < 2^31 - 4096.  Neither entry allocates or synchronises: graph-capturable.
 * BF_EINVAL for NULL, a bad shape, `probes` or `amplitude`, or short or misaligned scratch.
 *
 * bf_op_risk_probe_u8: dst = uint8 [(1 + probes) B, H, W, C], member-major: member 0 = src, member p = src + a s_p.  src is read
 *   once; one Philox call serves four elements; one launch.  src must not alias dst.
 * bf_op_risk_sums: y = the uint8 batch, f = the float32 result for the stack above, [(1 + probes) B, H, W, C];
 *   out = device double[B][C][1 + probes]:  out[n][c][0] = sum over h, w of (f_0 - y)^2,  out[n][c][p] = sum of s_p (f_p - f_0),
 *   s_p regenerated from (seed, p, e, y), every term formed in fp64 from the fp32 and uint8 values.  Reduced in a fixed order
 *   (per-workgroup partials in `scratch`, bf_op_risk_sums_scratch_bytes bytes, 8-byte aligned; then one workgroup per image):
 *   repeated calls return the same bits, and an image inside a batch the bits of that image alone. */
int bf_op_risk_probe_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, int C, int probes, int amplitude, uint64_t seed,
                        void* stream);
int64_t bf_op_risk_sums_scratch_bytes(int B, int H, int W, int C, int probes);
int bf_op_risk_sums(const uint8_t* y, const float* f, int B, int H, int W, int C, int probes, int amplitude, uint64_t seed,
                    void* scratch, int64_t scratch_bytes, double* out, void* stream);

/* bf_op_risk_sums for noise whose variance is affine in the signal, var_i = a y_i + b (plugged in at the noisy value):
 * E |f(y) - x|^2 = E[ |f(y) - y|^2 - sum var_i + 2 sum var_i df_i/dy_i ] is linear in four kinds of sums per image and channel.
 *   out = device double[B][C][2 + 2 probes] = (R, Y, D_1..D_K, Dy_1..Dy_K):  R and D_p as bf_op_risk_sums and with its bits,
 *   Y = sum y (an exact integer),  Dy_p = sum of y s_p (f_p - f_0).
 * The same probe stack, signs, unit ownership and fixed-order reduction; scratch: bf_op_risk_sums_affine_scratch_bytes bytes. */
int64_t bf_op_risk_sums_affine_scratch_bytes(int B, int H, int W, int C, int probes);
int bf_op_risk_sums_affine(const uint8_t* y, const float* f, int B, int H, int W, int C, int probes, int amplitude, uint64_t seed,
                           void* scratch, int64_t scratch_bytes, double* out, void* stream);

/* ---- training on noisy images alone: Neighbor2Neighbor pairs (Huang et al., CVPR 2021; blind_image_denoising_amd/neighbor.py is
 * the host side; csrc/neighbor.hip).  From a noisy batch y [B,H,W,C] (uint8 when y_is_u8 != 0, else float32; H, W even and >= 2,
 * C in 1..4) the sampler picks, in every 2x2 cell, an ordered pair of adjacent pixels: input = g1(y), target = g2(y), both float32
 * [B,H/2,W/2,C].  With f = the denoiser's float32 output for y [B,H,W,C] (NULL: none) the paper's regulariser is folded into the
 * target, target = g2(y) + lambda (g1(f) - g2(f)), lambda = gamma / (1 + gamma) in [0, 1): for a squared loss
 * |p - g2|^2 + gamma |p - g2 - d|^2 = (1 + gamma) |p - (g2 + lambda d)|^2 + const.
 * Cell and group: W2 = W / 2; cell (i, j) of image b belongs to Philox group g = i ceil(W2 / 4) + (j >> 2) (never across a row).
 * Draw: r = philox4x32_10(counter = (lo32 g, hi32 g, b, 3), key = (lo32 seed, hi32 seed)), k = r[j & 3] >> 29.
 * Positions of a cell: 0 = (0,0), 1 = (0,1), 2 = (1,0), 3 = (1,1) (row, column); (p1, p2) = T[k],
 * T = [(0,1),(0,2),(1,3),(2,3),(1,0),(2,0),(3,1),(3,2)], the eight ordered 4-adjacent pairs.  One k for all channels of a cell;
 * the images of a batch draw differently (b is in the counter).
 * Outputs: input = (float) y[p1]; target = (float) y[p2] when f is NULL, else fmaf(lambda, f[p1] - f[p2], (float) y[p2]) with the
 * difference rounded to fp32 first.  y and f are read once, each output is written once.  A float y with f = NULL and lambda = 0
 * samples any tensor (f(y) itself, for instance) with the same pairs.
 * One launch, no allocation, no synchronisation: graph-capturable.  BF_EINVAL for NULL y / input / target, B < 1, odd or zero H or W,
 * C outside 1..4, a lambda that is not finite or outside [0, 1), or an output that overlaps y, f or the other output. */
int bf_op_neighbor_pairs(const void* y, int y_is_u8, const float* f, float lambda, float* input, float* target, int B, int H, int W,
                         int C, uint64_t seed, void* stream);

/* ---- blind degradations for training: JPEG, blur, quantisation, drop-out (blind_image_denoising_amd/degrade.py is the host side;
 * csrc/degrade.hip) ----
 * Common: src is [B,H,W,C], uint8 when src_is_u8 != 0, else float32; a sample's 8-bit code is p = clip(rint(x), 0, 255) (half to
 * even; the identity on the integer-valued samples bf_noise_augment writes).  Everything after that is integer arithmetic with
 * arithmetic (floor) shifts, every accumulator fits int32 (uint32 for the vertical blur sum), so the float32 outputs -- integers
 * in [0, 255] -- are the same bits for every launch geometry and base alignment.  Per-image parameters are DEVICE int32 arrays
 * of B entries; one launch covers the batch.  BF_EINVAL for NULL or aliased pointers, sizes below 1, C outside 1..4;
 * BF_EUNSUPPORTED for B > 65535 or an axis beyond the grid limits.  No allocation, no synchronisation: graph-capturable.
 *
 * bf_op_degrade_jpeg: encode / decode round trip without entropy coding.  C is 1 or 3 (else BF_EINVAL); quality[b] in 1..100, or 0
 * for an image of the batch that is not encoded (its codes come out: what lets one launch serve a batch of which some images fire);
 * subsampling 444 or 420 (C == 1: a Y plane with the luminance table, subsampling has no effect).
 *   padding by edge replication to a multiple of 8 (16 for 420); every step works on the padded planes, the crop comes last
 *   Y = (19595 R + 38470 G + 7471 B + 32768) >> 16;  Cb = (-11058 R - 21710 G + 32768 B + (128 << 16) + 32767) >> 16;
 *   Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16;  420 chroma: (a + b + c + d + 2) >> 2 over each 2 x 2 cell
 *   tables: Annex K base tables, s = 5000 / q for q < 50 else 200 - 2 q, tbl = clip((base s + 50) / 100, 1, 255)
 *   DCT of p - 128 with T[u][x] = rint(8192 c(u) / 2 cos((2 x + 1) u pi / 16)):  a[y][u] = (sum_x T[u][x] p[y][x] + 512) >> 10,
 *   c8[v][u] = (sum_y T[v][y] a[y][u] + 4096) >> 13 (8 x the coefficient);  k = sign(c8) ((|c8| + 4 tbl) / (8 tbl)), c = k tbl
 *   inverse: a[y][u] = (sum_v T[v][y] c[v][u] + 512) >> 10,  p[y][x] = clip(((sum_u T[u][x] a[y][u] + 32768) >> 16) + 128, 0, 255)
 *   420 upsampling, triangle filter on the padded half-size plane with replicated edges: rows v_even = 3 c[i] + c[i-1],
 *   v_odd = 3 c[i] + c[i+1];  columns o_even = (3 v[j] + v[j-1] + 8) >> 4, o_odd = (3 v[j] + v[j+1] + 7) >> 4
 *   cb = Cb - 128, cr = Cr - 128:  R = Y + ((91881 cr + 32768) >> 16),  G = Y + ((-22553 cb - 46802 cr + 32768) >> 16),
 *   B = Y + ((116130 cb + 32768) >> 16), clipped.
 *   420 makes two launches through planar uint8 scratch of bf_op_degrade_jpeg_scratch_bytes bytes (0 for 444 and C == 1);
 *   BF_EWORKSPACE when it is too small.
 * bf_op_degrade_blur: separable Gaussian with integer taps.  taps = int32 [B][25], the first 2 radius[b] + 1 of a row used,
 *   radius[b] in 0..12, a row's taps non-negative with sum 65536 (degrade.gaussian_taps builds them; radius 0 with the tap 65536 is
 *   the identity).  Borders clamp.  h = sum w p (< 2^24), h8 = (h + 128) >> 8; v = sum w h8 (< 2^32, unsigned);
 *   out = (v + 2^23) >> 24.  One launch, tiled through LDS with the halo.
 * bf_op_degrade_pointwise: out = min(255, ((p + step / 2) / step) step), step[b] in 1..255; then, with threshold[b] = t =
 *   floor(rate 2^24) > 0, pixel i = y W + x of image b is dropped (all channels 0) when word 0 of philox4x32_10(counter =
 *   (lo32 i, hi32 i, b, 4), key = (lo32 seed, hi32 seed)) >> 8 is below t.  mask: uint8 [B,H,W], 1 = dropped, or NULL. */
int64_t bf_op_degrade_jpeg_scratch_bytes(int B, int H, int W, int C, int subsampling);
int bf_op_degrade_jpeg(const void* src, int src_is_u8, float* dst, int B, int H, int W, int C, const int32_t* quality,
                       int subsampling, void* scratch, int64_t scratch_bytes, void* stream);
int bf_op_degrade_blur(const void* src, int src_is_u8, float* dst, int B, int H, int W, int C, const int32_t* taps,
                       const int32_t* radius, void* stream);
int bf_op_degrade_pointwise(const void* src, int src_is_u8, float* dst, uint8_t* mask, int B, int H, int W, int C,
                            const int32_t* step, const int32_t* threshold, uint64_t seed, void* stream);

/* ---- options and diagnostics (not part of the drop-in surface; used by tests/) ------------- */

/* Inference forwards keep a status word in the LAST 2048 bytes of the workspace they are given (ws + ws_bytes - 2048,
 * int32; the rest of that tail is kernel scratch): 0 after a clean forward; bit BF_STATUS_F16_RANGE is set when an activation left the f16 range inside the
 * split-f16 blocks (the output is then not trustworthy: re-run with option "arith" = 0).  Reading it needs a stream
 * synchronisation, which is the caller's decision (the Python host checks it whenever it hands back host arrays). */
#define BF_STATUS_F16_RANGE 1

/* "fused_blocks" = 1 (default): one kernel per residual block; 0: one kernel per convolution.
 * "arith" = 1 (default): fused inference blocks run split-f16 ("f16x3": x = hi + lo in f16, three products,
 *   fp32 accumulation) on the f16 matrix cores, ~fp32 accuracy, needs |activation| < 65504;
 *   0: exact fp32 on the f32 matrix cores.  Training and the unfused path are always exact fp32.
 * "train_arith" = 1 (default): the training convolutions (forward, data gradient, weight gradient) run split-f16 on the
 *   f16 matrix cores; 0: exact fp32.  With it (all default 1, A/B only): "train_fused_bwd" = weight gradient, data gradient
 *   and the BatchNorm-backward apply of a convolution in one kernel; "train_fused_fwd" = a block's BatchNorm apply + skip Add
 *   formed by the next block's first convolution while it stages its tile; "train_zigzag" = consecutive tile kernels walk the
 *   tensors in opposite directions (Infinity Cache reuse).  "train_fused_bwd2" and "train_bwd_dbuf" selected two backward kernels that
 *   measured slower than the ones they were to replace and have been removed: both names are accepted for every
 *   value and change nothing ("train_bwd_block" is the one-kernel-per-block backward).
 * "fused_head" = 1: with split-f16 blocks, a linear denoiser head and 3 output channels, the head (premultiplied 16 x 3
 *   matrix, tanh, denormalise, rounding) runs in the epilogue of the last block: no head kernel, the last block output is
 *   never written; 0 (default): separate head kernel (the two measure within 0.5 % of each other).
 * "h3_pair": 1 (default): wherever the full-row streaming kernel applies, consecutive residual blocks run TWO per launch
 *   (fused_block2_h3w_kernel: the activation between them stays in LDS; an odd block count runs its single block first); 0: one
 *   block per launch.  "h3_pair_head": 1: the last pair launch also runs a linear 3-channel head in its store step (no head
 *   kernel); 0 (default; the two measure the same).  "h3_pair_base": 1 (default): where the FIRST launch of a forward is such a pair
 *   (not reversed, not carrying the head) and the row-streaming base kernel is the one that would run (uint8 RGB, 3x3, [0, 255]; see
 *   "base_rows"), that launch computes the base convolution itself, bit for bit what the base kernel writes: no base kernel, its
 *   output is neither written nor read back; 0: the base kernel launches (A/B).  "h3_pair" = 2 and "base_rows" = 2 (A/B and tests only) run the two-block kernel /
 *   the row-streaming base convolution wherever they CAN run instead of where the selection prefers them ("base_rows" = 0: the
 *   tile kernel of the base convolution everywhere; process-wide).
 * "h3_variant": kernel of the split-f16 fused blocks (A/B only; negative = default): 4 full-row streaming where it applies,
 *   2 row-streaming 16x16 tiles, every other value (1; 0 and 3 named kernels that have been retired) row-streaming 16x32 tiles.
 * "fused_tile": accepted for compatibility; every value runs the one exact-fp32 fused block kernel (fused_block_v4_kernel).
 *   Both succeed for every integer. */
int bf_set_option(bf_handle h, const char* key, int value);

/* with option "timing" = 1 every forward brackets its residual-block launches with two HIP events on
 * the caller's stream (a ring of 256 pairs; setting the option again restarts the window); after the
 * caller has synchronised, this returns the SUM of the elapsed milliseconds of the brackets of all
 * forwards since the option was set (the last 256 at most) and the number of kernel launches inside
 * them (bench.py roofline: average launch duration over the timed region).
 * bf_train_step uses the same ring with another meaning: one pair around every launch of its one-kernel block
 * backward (bwd_block_h3t_kernel, where the step runs it).  A window holds pairs of ONE meaning: the first pair of the other
 * kind restarts it, as setting the option does, so after a forward the figures are those of the forwards since the last
 * training step, and after a training step those of the block-backward launches since the last forward. */
int bf_get_timing(bf_handle h, float* ms, int* launches);
/* name of the kernel that ran most of the residual-block launches of the handle's LAST forward ("" before the first one) and
 * the number of block launches that forward made: what a profile of the run must show, and the key bench.py looks counter
 * traffic up by.  The string is static storage. */
const char* bf_get_block_kernel(bf_handle h, int* launches_per_forward);
/* the kernels that ran the residual blocks of the handle's LAST bf_train_step, as "fwd: <kernels>; bwd: <kernels>" ("" before the
 * first step): what a profile of a training run must show (bench.py's train records carry it).  Valid until the next step. */
const char* bf_get_train_kernels(bf_handle h);

/* The single-kernel diagnostic entries (bf_debug_*: one kernel at a time on fp32 NHWC tensors, used by the parity tests, the
 * profiling tools and bench.py's live roofline of the training kernel) are declared in bfcnn_hip_debug.h; they are exported by
 * the same library and are not part of the drop-in ABI above. */

#ifdef __cplusplus
}
#endif
#endif /* BFCNN_HIP_H */
