// The optimiser of the C-ABI engine.
#include "engine.h"
#include "block_reduce.h"
#include <cmath>

// ------------------------------------------------------------------------------------------
// Adam (keras 2.13, bfcnn/optimizer.py:190-206) with global_clipnorm (tf.clip_by_global_norm)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void grad_norm_kernel(const float* __restrict__ g, int64_t n, float grad_scale, float* scratch,
                                                         float* losses)
{
    __shared__ double red[1024];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 1024) {
        const double v = (double)g[i] * grad_scale;
        acc += v * v;
    }
    const double sum = bf_block_reduce<1024, BfSum>(red, (int)threadIdx.x, acc);
    if (threadIdx.x == 0) {
        scratch[0] = (float)sqrt(sum);
        if (losses) losses[BF_LOSS_GRAD_NORM] = scratch[0];
    }
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, int64_t n, float alpha, float beta_1, float beta_2,
                                                   float epsilon, float clip, float grad_scale, const float* __restrict__ scratch)
{
    float factor = grad_scale;
    if (clip > 0.f) {
        const float norm = scratch[0];
        factor *= clip / fmaxf(norm, clip);
    }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float gi = g[i] * factor;
        const float mi = m[i] + (gi - m[i]) * (1.0f - beta_1);
        const float vi = v[i] + (gi * gi - v[i]) * (1.0f - beta_2);
        m[i] = mi;
        v[i] = vi;
        p[i] = p[i] - (mi * alpha) / (sqrtf(vi) + epsilon);
    }
}

// per-tensor clipping (keras clipnorm = tf.clip_by_norm on every gradient tensor, optimizer.py:165-169): one workgroup per
// tensor sums its squares in a fixed order; factor = c / max(norm, c)
__global__ __launch_bounds__(256) void tensor_clip_factor_kernel(const float* __restrict__ g, const int64_t* __restrict__ offs,
                                                                 float grad_scale, float clipnorm, float* __restrict__ factor)
{
    __shared__ double red[256];
    const int64_t a = offs[blockIdx.x], b = offs[blockIdx.x + 1];
    double acc = 0.0;
    for (int64_t i = a + threadIdx.x; i < b; i += 256) {
        const double x = (double)g[i] * grad_scale;
        acc += x * x;
    }
    const double sum = bf_block_reduce<256, BfSum>(red, (int)threadIdx.x, acc);
    if (threadIdx.x == 0) factor[blockIdx.x] = clipnorm / fmaxf((float)sqrt(sum), clipnorm);
}

__global__ __launch_bounds__(256) void adam_tensor_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, const int64_t* __restrict__ offs,
                                                          const float* __restrict__ factor, float clipvalue, float alpha, float beta_1,
                                                          float beta_2, float epsilon, float grad_scale)
{
    const int64_t a = offs[blockIdx.x], b = offs[blockIdx.x + 1];
    const float f = grad_scale * (factor ? factor[blockIdx.x] : 1.f);
    for (int64_t i = a + threadIdx.x; i < b; i += 256) {
        float gi = g[i] * f;
        if (clipvalue > 0.f) gi = fminf(fmaxf(gi, -clipvalue), clipvalue);
        const float mi = m[i] + (gi - m[i]) * (1.0f - beta_1);
        const float vi = v[i] + (gi * gi - v[i]) * (1.0f - beta_2);
        m[i] = mi;
        v[i] = vi;
        p[i] = p[i] - (mi * alpha) / (sqrtf(vi) + epsilon);
    }
}

// bf_adam_step with keras' other two clipping modes.  Precedence as keras 2.13 (_clip_gradients): clipnorm (per tensor), else
// global_clipnorm, else clipvalue.  tensor_offsets = device int64[n_tensors + 1] (offsets of the trainable tensors in the flat
// vector, last = n_params), tensor_scratch = device float[n_tensors]; both only read when clipnorm or clipvalue is on.
static int adam_core(bf_handle h, int64_t n, float* params, const float* grads, float* m, float* v, int64_t iterations, float lr,
                     float beta_1, float beta_2, float epsilon, float global_clipnorm, float grad_scale, float* losses, float* scratch,
                     void* stream)
{
    if (!params || !grads || !m || !v || !scratch || n <= 0) return fail(h, BF_EINVAL, "bf_adam_step: NULL argument");
    if (iterations < 0) return fail(h, BF_EINVAL, "iterations must be >= 0");
    hipStream_t s = (hipStream_t)stream;
    if (global_clipnorm > 0.f || losses) {
        hipLaunchKernelGGL(grad_norm_kernel, dim3(1), dim3(1024), 0, s, grads, n, grad_scale, scratch, losses);
        BF_HIP(hipGetLastError(), "grad_norm");
    }
    const double t = (double)iterations + 1.0;
    const double alpha = (double)lr * sqrt(1.0 - pow((double)beta_2, t)) / (1.0 - pow((double)beta_1, t));
    const int grid = (int)((n + 255) / 256 < 512 ? (n + 255) / 256 : 512);
    hipLaunchKernelGGL(adam_kernel, dim3(grid), dim3(256), 0, s, params, grads, m, v, n, (float)alpha, beta_1, beta_2, epsilon,
                       global_clipnorm, grad_scale, scratch);
    BF_HIP(hipGetLastError(), "adam");
    return BF_OK;
}

static int adam_ex_core(bf_handle h, int64_t n, float* params, const float* grads, float* m, float* v, int64_t iterations, float lr,
                        float beta_1, float beta_2, float epsilon, float global_clipnorm, float clipnorm, float clipvalue,
                        const int64_t* tensor_offsets, int n_tensors, float* tensor_scratch, float grad_scale, float* losses,
                        float* scratch, void* stream)
{
    const bool local = clipnorm > 0.f, by_value = !local && !(global_clipnorm > 0.f) && clipvalue > 0.f;
    if (!local && !by_value)
        return adam_core(h, n, params, grads, m, v, iterations, lr, beta_1, beta_2, epsilon, global_clipnorm, grad_scale, losses, scratch,
                         stream);
    if (!params || !grads || !m || !v || !scratch || !tensor_offsets || n_tensors <= 0 || (local && !tensor_scratch))
        return fail(h, BF_EINVAL, "bf_adam_step_ex: NULL argument");
    if (iterations < 0) return fail(h, BF_EINVAL, "iterations must be >= 0");
    hipStream_t s = (hipStream_t)stream;
    if (losses) {
        hipLaunchKernelGGL(grad_norm_kernel, dim3(1), dim3(1024), 0, s, grads, n, grad_scale, scratch, losses);
        BF_HIP(hipGetLastError(), "grad_norm");
    }
    if (local) {
        hipLaunchKernelGGL(tensor_clip_factor_kernel, dim3(n_tensors), dim3(256), 0, s, grads, tensor_offsets, grad_scale, clipnorm,
                           tensor_scratch);
        BF_HIP(hipGetLastError(), "tensor_clip_factor");
    }
    const double t = (double)iterations + 1.0;
    const double alpha = (double)lr * sqrt(1.0 - pow((double)beta_2, t)) / (1.0 - pow((double)beta_1, t));
    hipLaunchKernelGGL(adam_tensor_kernel, dim3(n_tensors), dim3(256), 0, s, params, grads, m, v, tensor_offsets,
                       local ? tensor_scratch : (const float*)nullptr, by_value ? clipvalue : 0.f, (float)alpha, beta_1, beta_2, epsilon,
                       grad_scale);
    BF_HIP(hipGetLastError(), "adam_tensor");
    return BF_OK;
}

extern "C" int bf_adam_step_ex(bf_handle h, float* params, const float* grads, float* m, float* v, int64_t iterations, float lr,
                               float beta_1, float beta_2, float epsilon, float global_clipnorm, float clipnorm, float clipvalue,
                               const int64_t* tensor_offsets, int n_tensors, float* tensor_scratch, float grad_scale, float* losses,
                               float* scratch, void* stream)
{
    if (!h) return BF_EINVAL;
    return adam_ex_core(h, h->n_params, params, grads, m, v, iterations, lr, beta_1, beta_2, epsilon, global_clipnorm, clipnorm, clipvalue,
                        tensor_offsets, n_tensors, tensor_scratch, grad_scale, losses, scratch, stream);
}

extern "C" int bf_adam_step(bf_handle h, float* params, const float* grads, float* m, float* v, int64_t iterations, float lr,
                            float beta_1, float beta_2, float epsilon, float global_clipnorm, float grad_scale, float* losses,
                            float* scratch, void* stream)
{
    if (!h) return BF_EINVAL;
    return adam_core(h, h->n_params, params, grads, m, v, iterations, lr, beta_1, beta_2, epsilon, global_clipnorm, grad_scale, losses,
                     scratch, stream);
}

// the same update for a flat parameter vector that no bf_handle describes (models assembled from the operator library:
// unet_laplacian); n = number of parameters, everything else as bf_adam_step_ex
extern "C" int bf_op_adam_step(float* params, const float* grads, float* m, float* v, int64_t n, int64_t iterations, float lr, float beta_1,
                               float beta_2, float epsilon, float global_clipnorm, float clipnorm, float clipvalue,
                               const int64_t* tensor_offsets, int n_tensors, float* tensor_scratch, float grad_scale, float* losses,
                               float* scratch, void* stream)
{
    return adam_ex_core(nullptr, n, params, grads, m, v, iterations, lr, beta_1, beta_2, epsilon, global_clipnorm, clipnorm, clipvalue,
                        tensor_offsets, n_tensors, tensor_scratch, grad_scale, losses, scratch, stream);
}
