// Weight pruning on the flat parameter vector, in place (the strategies of bfcnn/pruning.py:130-205 without the host round trip).
// A device table of [begin, end) element ranges names the convolution kernels; nothing outside a range is ever written, and a
// range is clipped to the vector before it is used.  Comparisons and products are fp32 -- what NumPy computes on a float32 array
// with a Python scalar -- so the deterministic strategies reproduce the NumPy result bit for bit.
//
//   prune_elementwise_kernel   MINIMUM_THRESHOLD / _SHRINKAGE / _BIFURCATE: grid (tensor, PR_SPLIT), a tensor's elements dealt
//                              over PR_SPLIT workgroups.  The bifurcate draw is Philox4x32-10 keyed by the seed and indexed by
//                              the element's position in the flat vector: independent of the launch geometry.
//   prune_drop_bottom_kernel   one workgroup of 16 waves per tensor.  The k-th smallest |w| is found EXACTLY by a radix select over
//                              the bit patterns of |w| (non-negative floats order as their uint32 bits; NaNs sort last, as in
//                              np.sort): four passes, most significant byte first, each a 256-bin histogram of the elements that
//                              still match the prefix found so far, then a scan that picks the bin holding rank k.  No sort.
//                              The threshold is written out and every |w| < threshold set to 0 (strict: ties at the threshold stay).
//   count_below_kernel         one workgroup per tensor: number of |w| <= threshold, shuffle + LDS reduction.
//
// Histogram contention.  Trained weights share their high byte (a handful of exponents), so 64 lanes adding 1 to one LDS word
// would serialise.  Every wave owns a sub-histogram, and within a wave up to PR_PEEL rounds take the digit of the first pending
// lane, ballot the lanes that hold the same digit and add their popcount once; lanes still pending after that (the low bytes,
// where digits are spread and collisions are rare) add 1 each.  Counts are integers: the result does not depend on any order.
#include "bf_common.h"
#include "philox.h"

namespace {

constexpr int PR_SPLIT = 8;            // workgroups per tensor of the elementwise strategies
constexpr int PR_SEL_THREADS = 1024;   // the select: 16 waves, one sub-histogram each
constexpr int PR_SEL_WAVES = PR_SEL_THREADS / 64;
constexpr int PR_PEEL = 4;

// [begin, end) of tensor t clipped to [0, n)
__device__ __forceinline__ void pr_range(const int64_t* __restrict__ ranges, int t, int64_t n, int64_t& a, int64_t& e)
{
    a = ranges[2 * t];
    e = ranges[2 * t + 1];
    a = a < 0 ? 0 : (a > n ? n : a);
    e = e < a ? a : (e > n ? n : e);
}

__global__ __launch_bounds__(256) void prune_elementwise_kernel(float* __restrict__ w, int64_t n, const int64_t* __restrict__ ranges,
                                                                int strategy, float t, float shrinkage, float shrinkage_threshold,
                                                                uint32_t k0, uint32_t k1)
{
    int64_t a, e;
    pr_range(ranges, blockIdx.x, n, a, e);
    for (int64_t i = a + (int64_t)blockIdx.y * 256 + threadIdx.x; i < e; i += (int64_t)gridDim.y * 256) {
        float x = w[i];
        const float x0 = x;
        if (strategy == BF_PRUNE_MINIMUM_THRESHOLD_SHRINKAGE) {
            if (fabsf(x) < shrinkage_threshold) x = x * shrinkage;
        } else if (strategy == BF_PRUNE_MINIMUM_THRESHOLD_BIFURCATE) {
            if (fabsf(x) < t) {
                uint32_t r[4];
                philox4x32_10((uint32_t)i, (uint32_t)((uint64_t)i >> 32), 0u, 0u, k0, k1, r);
                // s = (2 m + 1) / 2^24 - 1 with m the draw's top 24 bits: 2^24 equally likely values in (-1, 1), symmetric, never
                // 0 or +-1, each exact in fp32; x = s * 2t is U(-2t, 2t) with one rounding and |x| < 2t
                const float s = (float)((int)(2u * (r[0] >> 8) + 1u) - (1 << 24)) * (1.0f / 16777216.0f);
                x = s * (2.0f * t);
            }
        }
        if (fabsf(x) < t) x = 0.0f;
        // only elements that change are stored (bitwise: -0.0 below t becomes +0.0, as NumPy's assignment makes it)
        if (__float_as_uint(x) != __float_as_uint(x0)) w[i] = x;
    }
}

// adds the digits of the wave's valid lanes to its sub-histogram h[256]; called by all 64 lanes together
__device__ __forceinline__ void pr_hist_add(unsigned* h, bool valid, unsigned digit, int lane)
{
    bool pending = valid;
#pragma unroll 1
    for (int r = 0; r < PR_PEEL; ++r) {
        const unsigned long long todo = __ballot(pending);
        if (!todo) return;                                                  // wave-uniform
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned d = (unsigned)__shfl((int)digit, leader);
        const bool mine = pending && digit == d;
        const unsigned long long same = __ballot(mine);
        if (lane == leader) atomicAdd(&h[d], (unsigned)__popcll(same));
        pending = pending && !mine;
    }
    if (pending) atomicAdd(&h[digit], 1u);
}

__global__ __launch_bounds__(PR_SEL_THREADS) void prune_drop_bottom_kernel(float* __restrict__ w, int64_t n,
                                                                           const int64_t* __restrict__ ranges,
                                                                           const int64_t* __restrict__ kth,
                                                                           float* __restrict__ thresholds)
{
    __shared__ unsigned hist[PR_SEL_WAVES][256];
    __shared__ unsigned total[256];
    __shared__ unsigned sel[2];                     // digit of the bin that holds rank k, rank inside that bin
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t a, e;
    pr_range(ranges, blockIdx.x, n, a, e);
    const int64_t len = e - a;
    if (len <= 0 || len > 0x7fffffffLL) {           // nothing to do / counts would not fit 32 bits: the tensor is left as it is
        if (tid == 0) thresholds[blockIdx.x] = len <= 0 ? 0.0f : __uint_as_float(0x7fc00000u);
        return;
    }
    int64_t k64 = kth[blockIdx.x];
    k64 = k64 < 0 ? 0 : (k64 > len - 1 ? len - 1 : k64);                    // the host refuses k outside [0, len) before it launches
    unsigned k = (unsigned)k64, prefix = 0;

#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = tid; i < PR_SEL_WAVES * 256; i += PR_SEL_THREADS) (&hist[0][0])[i] = 0;
        __syncthreads();
        // every lane of the workgroup makes the same number of trips: the ballots inside pr_hist_add see whole waves
        for (int64_t base = a; base < e; base += PR_SEL_THREADS) {
            const int64_t i = base + tid;
            bool valid = i < e;
            unsigned bits = 0;
            if (valid) {
                bits = __float_as_uint(w[i]) & 0x7fffffffu;
                if (shift < 24) valid = (bits >> (shift + 8)) == (prefix >> (shift + 8));
            }
            pr_hist_add(hist[wave], valid, (bits >> shift) & 255u, lane);
        }
        __syncthreads();
        if (tid < 256) {
            unsigned s = 0;
#pragma unroll
            for (int v = 0; v < PR_SEL_WAVES; ++v) s += hist[v][tid];
            total[tid] = s;
        }
        __syncthreads();
        if (wave == 0) {                            // lane l holds bins 4l .. 4l+3; inclusive scan of the lane sums over the wave
            unsigned c[4], s = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) { c[j] = total[4 * lane + j]; s += c[j]; }
            unsigned incl = s;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned v = (unsigned)__shfl_up((int)incl, off);
                if (lane >= off) incl += v;
            }
            const unsigned excl = incl - s;
            if (k >= excl && k < incl) {            // exactly one lane: the counts sum to the number of candidates, and k is below it
                unsigned r = k - excl;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (r < c[j]) { sel[0] = 4u * lane + j; sel[1] = r; break; }
                    r -= c[j];
                }
            }
        }
        __syncthreads();
        prefix |= sel[0] << shift;
        k = sel[1];
        // (the next pass starts by clearing hist and a barrier; sel is rewritten only after two more barriers)
    }

    const float thr = __uint_as_float(prefix);
    if (tid == 0) thresholds[blockIdx.x] = thr;
    for (int64_t i = a + tid; i < e; i += PR_SEL_THREADS) {
        const float x = w[i];
        if (fabsf(x) < thr) w[i] = 0.0f;
    }
}

__global__ __launch_bounds__(256) void count_below_kernel(const float* __restrict__ w, int64_t n, const int64_t* __restrict__ ranges,
                                                          float threshold, int64_t* __restrict__ counts)
{
    __shared__ unsigned long long part[4];
    int64_t a, e;
    pr_range(ranges, blockIdx.x, n, a, e);
    unsigned long long c = 0;
    for (int64_t i = a + threadIdx.x; i < e; i += 256) c += fabsf(w[i]) <= threshold ? 1u : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += (unsigned long long)__shfl_down((long long)c, off);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = (int64_t)(part[0] + part[1] + part[2] + part[3]);
}

}  // namespace

extern "C" int bf_op_prune_tensors(float* w, int64_t n, const int64_t* ranges, int n_tensors, int strategy, float minimum_threshold,
                                   float shrinkage, float shrinkage_threshold, uint64_t seed, const int64_t* kth, float* thresholds,
                                   void* stream)
{
    if (!w || !ranges || n <= 0 || n_tensors <= 0) return BF_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    switch (strategy) {
    case BF_PRUNE_NONE:
        return BF_OK;
    case BF_PRUNE_MINIMUM_THRESHOLD:
    case BF_PRUNE_MINIMUM_THRESHOLD_BIFURCATE:
    case BF_PRUNE_MINIMUM_THRESHOLD_SHRINKAGE:
        hipLaunchKernelGGL(prune_elementwise_kernel, dim3(n_tensors, PR_SPLIT), dim3(256), 0, s, w, n, ranges, strategy,
                           minimum_threshold, shrinkage, shrinkage_threshold, (uint32_t)seed, (uint32_t)(seed >> 32));
        break;
    case BF_PRUNE_DROP_BOTTOM:
        if (!kth || !thresholds) return BF_EINVAL;
        hipLaunchKernelGGL(prune_drop_bottom_kernel, dim3(n_tensors), dim3(PR_SEL_THREADS), 0, s, w, n, ranges, kth, thresholds);
        break;
    default:
        return BF_EUNSUPPORTED;                                             // PCA_PROJECTION: a host eigen-decomposition
    }
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}

extern "C" int bf_op_count_below(const float* w, int64_t n, const int64_t* ranges, int n_tensors, float threshold, int64_t* counts,
                                 void* stream)
{
    if (!w || !ranges || !counts || n <= 0 || n_tensors <= 0) return BF_EINVAL;
    hipLaunchKernelGGL(count_below_kernel, dim3(n_tensors), dim3(256), 0, (hipStream_t)stream, w, n, ranges, threshold, counts);
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}
