// On-device data corruption for training: prepare_data_fn of bfcnn/dataset.py:126-239 without tf.data.
//   geometric_augmentation_fn (dataset.py:131-159): whole-batch flip left-right / up-down (the host draws the two
//     coin flips, as the reference draws them once per batch), then tf.round (dataset.py:234)
//   noise_augmentation_fn (dataset.py:161-230): x * truncated_normal(mean 1, std m) then + truncated_normal(mean 0,
//     std a), each applied or not per batch (host coin flips; m, a ~ U[min,max] drawn by the host), then tf.round.
//     No clipping after the noise (the reference has none).
// tf.random.truncated_normal: values more than 2 standard deviations from the mean are dropped and re-picked.
// Random numbers: Philox4x32-10, counter = (element index lo, hi, attempt, stream), key = seed -- counter based, so
// the result does not depend on the launch geometry and a numpy restatement (oracle/bfcnn_oracle.py) can follow it.
// HBM-bound: reads 4 B, writes 8 B per element.
// bf_op_camera_noise_u8 (below) is apart from that path: signal-dependent noise on uint8 images, not truncated.
#include "bf_common.h"
#include "philox.h"

// first standard normal with |z| <= 2 of the element's stream (Box-Muller on successive Philox outputs)
__device__ __forceinline__ float truncated_normal(uint32_t idx_lo, uint32_t idx_hi, uint32_t stream, uint32_t k0, uint32_t k1)
{
    for (uint32_t attempt = 0; attempt < 16; ++attempt) {
        uint32_t r[4];
        philox4x32_10(idx_lo, idx_hi, attempt, stream, k0, k1, r);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float u1 = ((float)(r[2 * h] >> 8) + 1.0f) * (1.0f / 16777216.0f);       // (0, 1]
            const float u2 = (float)(r[2 * h + 1] >> 8) * (1.0f / 16777216.0f);            // [0, 1)
            const float rad = sqrtf(-2.0f * logf(u1));
            const float z0 = rad * cosf(6.28318530717958647692f * u2), z1 = rad * sinf(6.28318530717958647692f * u2);
            if (fabsf(z0) <= 2.0f) return z0;
            if (fabsf(z1) <= 2.0f) return z1;
        }
    }
    return 0.0f;      // probability 0.0455^64
}

__global__ __launch_bounds__(256) void noise_augment_kernel(const float* __restrict__ in, float* __restrict__ out_clean,
                                                            float* __restrict__ out_noisy, int B, int H, int W, int C, int flip_mask,
                                                            float mult_std, float add_std, uint32_t k0, uint32_t k1)
{
    const int64_t n = (int64_t)B * H * W * C;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % C);
        int64_t t = i / C;
        const int x = (int)(t % W); t /= W;
        const int y = (int)(t % H);
        const int64_t b = t / H;
        const int sx = (flip_mask & 1) ? W - 1 - x : x, sy = (flip_mask & 2) ? H - 1 - y : y;
        const float clean = rintf(in[((b * H + sy) * W + sx) * C + c]);      // tf.round = half to even
        float v = clean;
        // the stream is indexed by the OUTPUT element, so the noise field does not move with the flips
        if (mult_std > 0.f) v *= 1.0f + mult_std * truncated_normal((uint32_t)i, (uint32_t)(i >> 32), 0u, k0, k1);
        if (add_std > 0.f) v += add_std * truncated_normal((uint32_t)i, (uint32_t)(i >> 32), 1u, k0, k1);
        if (out_clean) out_clean[i] = clean;
        out_noisy[i] = rintf(v);
    }
}

extern "C" int bf_noise_augment(const float* in, float* out_clean, float* out_noisy, int B, int H, int W, int C, int flip_mask,
                                float mult_std, float add_std, uint64_t seed, void* stream)
{
    if (!in || !out_noisy || B <= 0 || H <= 0 || W <= 0 || C <= 0) return BF_EINVAL;
    if (mult_std < 0.f || add_std < 0.f || (flip_mask & ~3)) return BF_EINVAL;
    if (in == out_clean || in == out_noisy) return BF_EINVAL;               // flips read other elements: not in place
    const int64_t n = (int64_t)B * H * W * C;
    int64_t g = (n + 255) / 256;
    hipLaunchKernelGGL(noise_augment_kernel, dim3((unsigned)(g < 16384 ? g : 16384)), dim3(256), 0, (hipStream_t)stream, in,
                       out_clean, out_noisy, B, H, W, C, flip_mask, mult_std, add_std, (uint32_t)seed, (uint32_t)(seed >> 32));
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}

// ---- signal-dependent (Poisson-Gaussian) camera noise on uint8 images ----
// y = clip(rint(x + sqrt(gain_c x + read_sigma_c^2) z), 0, 255), z an UNTRUNCATED standard normal: Box-Muller on words 0 and 1 of
// philox4x32_10(counter = (lo32 e, hi32 e, 0, 3), key = seed), e = (h W + w) C + c the element's index inside its image, so that
// an image gets the same bits alone or inside a batch.  The noise model the estimator of noise_level.hip fits: var(y | x) =
// gain x + read_sigma^2.  A thread owns four consecutive elements (one dword where the image stride and the bases allow it).
struct CameraNoiseParams { float gain[4], read_var[4]; };

__global__ __launch_bounds__(256) void camera_noise_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int64_t n,
                                                              int groups_x, int C, CameraNoiseParams prm, uint32_t k0, uint32_t k1,
                                                              int vec)
{
    const int b = blockIdx.x / groups_x;
    const int64_t e0 = 4 * ((int64_t)(blockIdx.x % groups_x) * 256 + threadIdx.x);
    if (e0 >= n) return;
    const uint8_t* __restrict__ s = src + (int64_t)b * n + e0;              // element e0 + i is read and written only for e0 + i < n
    uint8_t* __restrict__ d = dst + (int64_t)b * n + e0;
    unsigned x4 = 0u, y4 = 0u;
    if (vec) x4 = *reinterpret_cast<const unsigned*>(s);
    else
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (e0 + i < n) x4 |= (unsigned)s[i] << (8 * i);
    int c = (int)(e0 % C);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t e = e0 + i;
        uint32_t r[4];
        philox4x32_10((uint32_t)e, (uint32_t)((uint64_t)e >> 32), 0u, 3u, k0, k1, r);
        const float u1 = ((float)(r[0] >> 8) + 1.0f) * (1.0f / 16777216.0f);       // (0, 1]
        const float u2 = (float)(r[1] >> 8) * (1.0f / 16777216.0f);                // [0, 1)
        const float z = sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
        const float x = (float)(x4 >> (8 * i) & 255u);
        const float gain = c == 0 ? prm.gain[0] : c == 1 ? prm.gain[1] : c == 2 ? prm.gain[2] : prm.gain[3];
        const float rvar = c == 0 ? prm.read_var[0] : c == 1 ? prm.read_var[1] : c == 2 ? prm.read_var[2] : prm.read_var[3];
        const float v = rintf(x + sqrtf(gain * x + rvar) * z);
        y4 |= (unsigned)fminf(fmaxf(v, 0.0f), 255.0f) << (8 * i);
        c = c + 1 == C ? 0 : c + 1;
    }
    if (vec) *reinterpret_cast<unsigned*>(d) = y4;
    else
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (e0 + i < n) d[i] = (uint8_t)(y4 >> (8 * i));
}

extern "C" int bf_op_camera_noise_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, int C, const float* gain,
                                     const float* read_sigma, uint64_t seed, void* stream)
{
    if (!src || !dst || !gain || !read_sigma || B <= 0 || H <= 0 || W <= 0 || C < 1 || C > 4) return BF_EINVAL;
    CameraNoiseParams prm = {};
    for (int c = 0; c < C; ++c) {                                           // host arrays, passed on by value
        if (!(gain[c] >= 0.f) || !(read_sigma[c] >= 0.f) || !(gain[c] <= 3.0e38f) || !(read_sigma[c] <= 1.0e19f)) return BF_EINVAL;
        prm.gain[c] = gain[c];
        prm.read_var[c] = read_sigma[c] * read_sigma[c];
    }
    const int64_t n = (int64_t)H * W * C;
    const int64_t groups_x = ((n + 3) / 4 + 255) / 256;
    if (n > INT32_MAX - 4096 || groups_x * B > INT32_MAX) return BF_EINVAL;
    const int vec = n % 4 == 0 && ((uintptr_t)src | (uintptr_t)dst) % 4 == 0;
    hipLaunchKernelGGL(camera_noise_u8_kernel, dim3((unsigned)(groups_x * B)), dim3(256), 0, (hipStream_t)stream, src, dst, n,
                       (int)groups_x, C, prm, (uint32_t)seed, (uint32_t)(seed >> 32), vec);
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}
