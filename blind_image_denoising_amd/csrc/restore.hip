// Restoration with the denoiser's implicit prior (Kadkhodaie & Simoncelli, NeurIPS 2021, Algorithm 2): the state update between
// two denoiser calls.  The host side is blind_image_denoising_amd/restore.py; the contract is in include/bfcnn_hip.h, the choices
// and the measurements are DESIGN.md 7.19.  Nothing is uploaded, allocated or synchronised; sigma_t never comes to the host.
//
// Geometry, the same in every kernel: an image of n = H W C elements is cut into chunks of 1024 consecutive elements, a workgroup
// of 256 threads owns the chunks tile, tile + tiles, .. of ONE image (tiles = min(chunks, 256): a function of n alone), a thread
// the four consecutive elements 4 g .. 4 g + 3 of a chunk: one float4 per array where n % 4 == 0 and the bases are 16-byte aligned,
// scalar loads and stores otherwise (the tail of n % 4 != 0 and unaligned image strides).  The group index g is also the Philox
// counter, so the draws do not depend on the geometry.
//
// Arithmetic.  Every output element is formed in fp64 from its float32 operands and rounded to float32 ONCE:
//   direction  d  = fl(D - y + a - P D)                         |d - exact| <= 2^-24 |d| <= 4 * 2^-24 M
//   step       y' = fl(y + h d + gamma z)                       one rounding of a value <= (2 + gamma |z| / M) M
//   finish     x  = fl(D - P D + a)                             block constraint; the mask constraint selects
// with M the largest magnitude among the element's operands (for the block constraint the s x s values of D under P included);
// the fp64 operations themselves err by parts in 2^53.  That is one float32 rounding per formula, inside the eight the tests allow.
// The block mean is the fp64 sum of the s x s floats in row-major order times 1 / s^2.  sum d^2 adds the fp64 values BEFORE the
// rounding to float32: every thread in ascending order of its elements, then the fixed two-stage sum of block_reduce.h (one
// partial per workgroup, one workgroup per image adds them): the same bits in two calls, and for an image alone or in a batch.
//
// Noise.  z of the elements 4 g .. 4 g + 3 = Box-Muller on philox4x32_10(counter = (g, sample_id, t, 6), key = seed): words (0, 1)
// give the cosine and sine branch, words (2, 3) the next two, u1 = ((r >> 8) + 1) / 2^24, u2 = (r >> 8) / 2^24, radius =
// sqrtf(-2 logf(u1)), angle through sincospif(2 u2): the argument 2 u2 is exact, where 2 pi u2 would be rounded first.
//
// Freezing.  An image takes part in iteration t when its step count is t - 1 (it moved in every iteration so far) and sigma_t >
// sigma_l.  The update kernel only READS the counts; a second launch of B threads appends sigma_t to the trace and bumps the
// counts of the images that moved, so no workgroup can see a count another one has already bumped.
#include "bf_common.h"
#include "block_reduce.h"
#include "philox.h"

namespace {

constexpr int RS_THREADS = 256, RS_CHUNK = 4 * RS_THREADS, RS_MAX_TILES = 256;
constexpr unsigned RS_PHILOX_STREAM = 6u;                        // counter word 3: the list is in pixel_shuffle.hip (0..5 are taken)
enum { RS_MASK = 0, RS_BLOCK = 1 };

struct RsShape { int H, W, C, n, chunks, tiles; };
struct RsCon {
    int kind, mask_c, factor, anchor_u8;
    const uint8_t* mask;                                         // RS_MASK: uint8 [B,H,W,mask_c], mask_c = 1 or C
    const void* anchor;                                          // RS_MASK: [B,H,W,C]; RS_BLOCK: [B,H/s,W/s,C]; uint8 or float32
    double inv_ss;                                               // 1 / s^2
};

bool rs_shape(int B, int H, int W, int C, RsShape& g)
{
    if (B <= 0 || H <= 0 || W <= 0 || C < 1 || C > 4) return false;
    const int64_t n = (int64_t)H * W * C;
    if (n > INT32_MAX) return false;
    g.H = H; g.W = W; g.C = C; g.n = (int)n;
    g.chunks = (int)((n + RS_CHUNK - 1) / RS_CHUNK);
    g.tiles = g.chunks < RS_MAX_TILES ? g.chunks : RS_MAX_TILES;
    return (int64_t)B * g.tiles <= INT32_MAX;
}

bool rs_constraint(const RsShape& g, int kind, const uint8_t* mask, int mask_channels, int factor, const void* anchor, int anchor_is_u8,
                   RsCon& c)
{
    if (!anchor || (kind != RS_MASK && kind != RS_BLOCK)) return false;
    if (kind == RS_MASK && (!mask || (mask_channels != 1 && mask_channels != g.C))) return false;
    if (kind == RS_BLOCK && (factor < 2 || factor > 8 || g.H % factor || g.W % factor)) return false;
    if (!anchor_is_u8 && (uintptr_t)anchor % 4) return false;
    c.kind = kind; c.mask_c = mask_channels; c.factor = kind == RS_BLOCK ? factor : 1; c.anchor_u8 = anchor_is_u8 != 0;
    c.mask = mask; c.anchor = anchor; c.inv_ss = 1.0 / (double)(c.factor * c.factor);
    return true;
}

// what the constraint says about element e of image b: whether it is measured (mask; every element of a block constraint takes part
// in a measurement), the anchor a there (read only where measured), and P D there (block, with D's image given)
struct RsElem { bool measured; float a; double pd; };

__device__ __forceinline__ float rs_anchor_at(const RsCon& c, int64_t i)
{
    return c.anchor_u8 ? (float)static_cast<const uint8_t*>(c.anchor)[i] : static_cast<const float*>(c.anchor)[i];
}

__device__ __forceinline__ RsElem rs_elem(const RsCon& c, const RsShape& g, int64_t b, int e, const float* __restrict__ Dimg)
{
    RsElem r = {true, 0.f, 0.0};
    if (c.kind == RS_MASK) {
        const int64_t mi = c.mask_c == 1 ? b * (g.n / g.C) + e / g.C : b * g.n + e;
        r.measured = c.mask[mi] != 0;
        if (r.measured) r.a = rs_anchor_at(c, b * g.n + e);
        return r;
    }
    const int s = c.factor, px = e / g.C, ch = e - px * g.C, i = px / g.W, j = px - i * g.W, li = i / s, lj = j / s;
    r.a = rs_anchor_at(c, ((b * (g.H / s) + li) * (g.W / s) + lj) * g.C + ch);
    if (Dimg) {
        double sum = 0.0;
        for (int u = 0; u < s; ++u) {
            const float* __restrict__ row = Dimg + ((int64_t)(li * s + u) * g.W + lj * s) * g.C + ch;
            for (int v = 0; v < s; ++v) sum += (double)row[v * g.C];
        }
        r.pd = sum * c.inv_ss;
    }
    return r;
}

template <bool VEC>
__device__ __forceinline__ void rs_load4(const float* __restrict__ p, int cnt, float (&v)[4])
{
    if (VEC) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = i < cnt ? p[i] : 0.f;
    }
}

template <bool VEC>
__device__ __forceinline__ void rs_store4(float* __restrict__ p, int cnt, const float (&v)[4])
{
    if (VEC) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < cnt) p[i] = v[i];
}

__device__ __forceinline__ void rs_normals(uint32_t g, uint32_t sample, uint32_t t, uint32_t k0, uint32_t k1, float (&z)[4])
{
    uint32_t r[4];
    philox4x32_10(g, sample, t, RS_PHILOX_STREAM, k0, k1, r);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float u1 = ((float)(r[2 * h] >> 8) + 1.0f) * (1.0f / 16777216.0f);       // (0, 1]
        const float u2 = (float)(r[2 * h + 1] >> 8) * (1.0f / 16777216.0f);            // [0, 1)
        const float radius = sqrtf(-2.0f * logf(u1));
        float sn, cs;
        sincospif(2.0f * u2, &sn, &cs);
        z[2 * h] = radius * cs;
        z[2 * h + 1] = radius * sn;
    }
}

// the thread's group of four elements in `chunk` of its image: false past the end; cnt = how many of the four exist
__device__ __forceinline__ bool rs_group(const RsShape& g, int chunk, int64_t& e0, int& cnt)
{
    e0 = (int64_t)chunk * RS_CHUNK + 4 * threadIdx.x;
    cnt = g.n - e0 < 4 ? (int)(g.n - e0) : 4;
    return e0 < g.n;
}

// y0 = 127.5 (1 - P 1) + a + sigma_0 z_0
template <bool VEC>
__global__ __launch_bounds__(RS_THREADS) void restore_init_kernel(float* __restrict__ y, RsCon c, RsShape g, double sigma0,
                                                                  const uint32_t* __restrict__ sample_id, uint32_t k0, uint32_t k1)
{
    const int64_t b = blockIdx.x / g.tiles;
    const uint32_t sample = sample_id ? sample_id[b] : (uint32_t)b;
    float* __restrict__ yi = y + b * g.n;
    for (int chunk = blockIdx.x % g.tiles; chunk < g.chunks; chunk += g.tiles) {
        int64_t e0;
        int cnt;
        if (!rs_group(g, chunk, e0, cnt)) continue;
        float z[4], out[4];
        rs_normals((uint32_t)(e0 >> 2), sample, 0u, k0, k1, z);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            out[i] = 0.f;
            if (i < cnt) {
                const RsElem el = rs_elem(c, g, b, (int)e0 + i, nullptr);
                out[i] = (float)((el.measured ? (double)el.a : 127.5) + sigma0 * (double)z[i]);
            }
        }
        rs_store4<VEC>(yi + e0, cnt, out);
    }
}

template <bool VEC>
__global__ __launch_bounds__(RS_THREADS) void restore_direction_kernel(const float* __restrict__ y, const float* __restrict__ D,
                                                                       float* __restrict__ d, double* __restrict__ partial, RsCon c, RsShape g)
{
    __shared__ double red[RS_THREADS / 64][1];
    const int64_t b = blockIdx.x / g.tiles;
    const float* __restrict__ Di = D + b * g.n;
    double acc = 0.0;
    for (int chunk = blockIdx.x % g.tiles; chunk < g.chunks; chunk += g.tiles) {
        int64_t e0;
        int cnt;
        if (!rs_group(g, chunk, e0, cnt)) continue;
        float yv[4], Dv[4], out[4];
        rs_load4<VEC>(y + b * g.n + e0, cnt, yv);
        rs_load4<VEC>(Di + e0, cnt, Dv);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            out[i] = 0.f;
            if (i < cnt) {
                const RsElem el = rs_elem(c, g, b, (int)e0 + i, Di);
                double v;
                if (c.kind == RS_MASK) v = (el.measured ? (double)el.a : (double)Dv[i]) - (double)yv[i];
                else v = ((double)Dv[i] - (double)yv[i]) + ((double)el.a - el.pd);
                out[i] = (float)v;
                acc += v * v;
            }
        }
        rs_store4<VEC>(d + b * g.n + e0, cnt, out);
    }
    bf_tile_stage<1>(red, 0, acc);
    bf_tile_partials<1>(red, 1, partial + blockIdx.x);
}

// sumsq[b] = the sum of the image's partials; one workgroup per image
__global__ __launch_bounds__(256) void restore_sumsq_kernel(const double* __restrict__ partial, double* __restrict__ sumsq, int tiles)
{
    __shared__ double red[256];
    const double s = bf_finalize_partials(partial + (int64_t)blockIdx.x * tiles, (int64_t)tiles, (int64_t)1, red);
    if (threadIdx.x == 0) sumsq[blockIdx.x] = s;
}

struct RsStep { double h, gamma_factor, sigma_l; int t; };       // gamma_t^2 = gamma_factor sigma_t^2

__device__ __forceinline__ bool rs_moves(const double* __restrict__ sumsq, const int* __restrict__ steps, int64_t b, int n, const RsStep& p,
                                         double& sigma)
{
    sigma = sqrt(sumsq[b] / (double)n);
    return steps[b] == p.t - 1 && sigma > p.sigma_l;             // a NaN sigma freezes
}

template <bool VEC>
__global__ __launch_bounds__(RS_THREADS) void restore_step_kernel(float* __restrict__ y, const float* __restrict__ d,
                                                                  const double* __restrict__ sumsq, const int* __restrict__ steps,
                                                                  const uint32_t* __restrict__ sample_id, RsShape g, RsStep p, uint32_t k0,
                                                                  uint32_t k1)
{
    const int64_t b = blockIdx.x / g.tiles;
    double sigma;
    if (!rs_moves(sumsq, steps, b, g.n, p, sigma)) return;       // the whole workgroup
    const double gamma = sqrt(p.gamma_factor) * sigma;
    const uint32_t sample = sample_id ? sample_id[b] : (uint32_t)b;
    for (int chunk = blockIdx.x % g.tiles; chunk < g.chunks; chunk += g.tiles) {
        int64_t e0;
        int cnt;
        if (!rs_group(g, chunk, e0, cnt)) continue;
        float yv[4], dv[4], z[4] = {0.f, 0.f, 0.f, 0.f};
        rs_load4<VEC>(y + b * g.n + e0, cnt, yv);
        rs_load4<VEC>(d + b * g.n + e0, cnt, dv);
        if (gamma > 0.0) rs_normals((uint32_t)(e0 >> 2), sample, (uint32_t)p.t, k0, k1, z);
#pragma unroll
        for (int i = 0; i < 4; ++i) yv[i] = (float)((double)yv[i] + p.h * (double)dv[i] + gamma * (double)z[i]);
        rs_store4<VEC>(y + b * g.n + e0, cnt, yv);
    }
}

// behind the update: trace[t - 1][b] = sigma_t, steps[b] = t for the images that moved
__global__ __launch_bounds__(256) void restore_book_kernel(const double* __restrict__ sumsq, int* __restrict__ steps, double* __restrict__ trace,
                                                           int B, int n, RsStep p)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    double sigma;
    const bool moves = rs_moves(sumsq, steps, b, n, p, sigma);
    if (trace) trace[(int64_t)(p.t - 1) * B + b] = sigma;
    if (moves) steps[b] = p.t;
}

// x = D - P D + a; the measured samples of a mask constraint are the measurement itself
template <bool VEC>
__global__ __launch_bounds__(RS_THREADS) void restore_finish_kernel(const float* __restrict__ D, void* __restrict__ out, int out_u8, RsCon c,
                                                                    RsShape g)
{
    const int64_t b = blockIdx.x / g.tiles;
    const float* __restrict__ Di = D + b * g.n;
    for (int chunk = blockIdx.x % g.tiles; chunk < g.chunks; chunk += g.tiles) {
        int64_t e0;
        int cnt;
        if (!rs_group(g, chunk, e0, cnt)) continue;
        float Dv[4], v[4];
        rs_load4<VEC>(Di + e0, cnt, Dv);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[i] = 0.f;
            if (i < cnt) {
                const RsElem el = rs_elem(c, g, b, (int)e0 + i, Di);
                if (c.kind == RS_MASK) v[i] = el.measured ? el.a : Dv[i];
                else v[i] = (float)(((double)Dv[i] - el.pd) + (double)el.a);
            }
        }
        if (!out_u8) {
            rs_store4<VEC>((float*)out + b * g.n + e0, cnt, v);
            continue;
        }
        unsigned q = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) q |= (unsigned)fminf(fmaxf(rintf(v[i]), 0.f), 255.f) << (8 * i);       // rintf = round half to even
        uint8_t* __restrict__ o = (uint8_t*)out + b * g.n + e0;
        if (VEC) *reinterpret_cast<unsigned*>(o) = q;            // n % 4 == 0 and out 16-byte aligned: a dword boundary
        else
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < cnt) o[i] = (uint8_t)(q >> (8 * i));
    }
}

bool rs_vec(const RsShape& g, const void* a, const void* b = nullptr, const void* c = nullptr)
{
    return g.n % 4 == 0 && ((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) % 16 == 0;
}

int rs_done() { return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP; }

}  // namespace

extern "C" int64_t bf_op_restore_scratch_bytes(int B, int H, int W, int C)
{
    RsShape g;
    if (!rs_shape(B, H, W, C, g)) return BF_EINVAL;
    return (int64_t)B * g.tiles * (int64_t)sizeof(double);
}

extern "C" int bf_op_restore_init(float* y, int B, int H, int W, int C, int kind, const uint8_t* mask, int mask_channels, int factor,
                                  const void* anchor, int anchor_is_u8, double sigma_0, uint64_t seed, const uint32_t* sample_id_or_null,
                                  void* stream)
{
    RsShape g;
    RsCon c;
    if (!y || !rs_shape(B, H, W, C, g) || !rs_constraint(g, kind, mask, mask_channels, factor, anchor, anchor_is_u8, c)) return BF_EINVAL;
    if ((uintptr_t)y % 4 || (uintptr_t)sample_id_or_null % 4 || !(sigma_0 >= 0.0) || !(sigma_0 <= 1.0e30)) return BF_EINVAL;
    const dim3 grid((unsigned)((int64_t)B * g.tiles)), block(RS_THREADS);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    if (rs_vec(g, y)) hipLaunchKernelGGL(restore_init_kernel<true>, grid, block, 0, s, y, c, g, sigma_0, sample_id_or_null, k0, k1);
    else hipLaunchKernelGGL(restore_init_kernel<false>, grid, block, 0, s, y, c, g, sigma_0, sample_id_or_null, k0, k1);
    return rs_done();
}

extern "C" int bf_op_restore_direction(const float* y, const float* denoised, int B, int H, int W, int C, int kind, const uint8_t* mask,
                                       int mask_channels, int factor, const void* anchor, int anchor_is_u8, float* d, void* scratch,
                                       int64_t scratch_bytes, double* sumsq, void* stream)
{
    RsShape g;
    RsCon c;
    if (!y || !denoised || !d || !scratch || !sumsq || !rs_shape(B, H, W, C, g) ||
        !rs_constraint(g, kind, mask, mask_channels, factor, anchor, anchor_is_u8, c))
        return BF_EINVAL;
    if (((uintptr_t)y | (uintptr_t)denoised | (uintptr_t)d) % 4 || ((uintptr_t)scratch | (uintptr_t)sumsq) % 8) return BF_EINVAL;
    if (d == y || d == denoised || scratch_bytes < (int64_t)B * g.tiles * (int64_t)sizeof(double)) return BF_EINVAL;
    const dim3 grid((unsigned)((int64_t)B * g.tiles)), block(RS_THREADS);
    hipStream_t s = (hipStream_t)stream;
    double* partial = (double*)scratch;
    if (rs_vec(g, y, denoised, d)) hipLaunchKernelGGL(restore_direction_kernel<true>, grid, block, 0, s, y, denoised, d, partial, c, g);
    else hipLaunchKernelGGL(restore_direction_kernel<false>, grid, block, 0, s, y, denoised, d, partial, c, g);
    hipLaunchKernelGGL(restore_sumsq_kernel, dim3((unsigned)B), dim3(256), 0, s, partial, sumsq, g.tiles);
    return rs_done();
}

extern "C" int bf_op_restore_step(float* y, const float* d, const double* sumsq, int B, int H, int W, int C, double h_t, double beta,
                                  double sigma_l, int t, uint64_t seed, const uint32_t* sample_id_or_null, double* trace_or_null,
                                  int trace_rows, int* steps, void* stream)
{
    RsShape g;
    if (!y || !d || !sumsq || !steps || !rs_shape(B, H, W, C, g)) return BF_EINVAL;
    if (((uintptr_t)y | (uintptr_t)d | (uintptr_t)steps | (uintptr_t)sample_id_or_null) % 4 || ((uintptr_t)sumsq | (uintptr_t)trace_or_null) % 8)
        return BF_EINVAL;
    if (y == d || !(h_t > 0.0) || !(h_t <= 1.0) || !(beta >= 0.0) || !(beta <= 1.0) || !(sigma_l > 0.0) || t < 1) return BF_EINVAL;
    if (trace_or_null && t > trace_rows) return BF_EINVAL;
    const double keep = 1.0 - beta * h_t, drop = 1.0 - h_t, factor = keep * keep - drop * drop;          // >= 0 as beta <= 1
    const RsStep p = {h_t, factor > 0.0 ? factor : 0.0, sigma_l, t};
    const dim3 grid((unsigned)((int64_t)B * g.tiles)), block(RS_THREADS);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    if (rs_vec(g, y, d)) hipLaunchKernelGGL(restore_step_kernel<true>, grid, block, 0, s, y, d, sumsq, steps, sample_id_or_null, g, p, k0, k1);
    else hipLaunchKernelGGL(restore_step_kernel<false>, grid, block, 0, s, y, d, sumsq, steps, sample_id_or_null, g, p, k0, k1);
    hipLaunchKernelGGL(restore_book_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, sumsq, steps, trace_or_null, B, g.n, p);
    return rs_done();
}

extern "C" int bf_op_restore_finish(const float* denoised, int B, int H, int W, int C, int kind, const uint8_t* mask, int mask_channels,
                                    int factor, const void* anchor, int anchor_is_u8, void* out, int out_is_u8, void* stream)
{
    RsShape g;
    RsCon c;
    if (!denoised || !out || !rs_shape(B, H, W, C, g) || !rs_constraint(g, kind, mask, mask_channels, factor, anchor, anchor_is_u8, c))
        return BF_EINVAL;
    if ((uintptr_t)denoised % 4 || (!out_is_u8 && (uintptr_t)out % 4) || out == (const void*)denoised) return BF_EINVAL;
    const dim3 grid((unsigned)((int64_t)B * g.tiles)), block(RS_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (rs_vec(g, denoised, out)) hipLaunchKernelGGL(restore_finish_kernel<true>, grid, block, 0, s, denoised, out, out_is_u8, c, g);
    else hipLaunchKernelGGL(restore_finish_kernel<false>, grid, block, 0, s, denoised, out, out_is_u8, c, g);
    return rs_done();
}
