// Workgroup reductions with a FIXED order of operations.  The order is part of the contract of every function
// here: fp32 and fp64 addition do not associate, and "two calls return the same bits" / "an image inside a batch returns the bits
// of that image alone" (metrics.hip, noise_estimate.hip, risk.hip) hold because the additions below happen in this order and
// in no other.  Changing a pairing changes result bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct BfSum { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
struct BfMax { __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); } };

// Sum over the 64 lanes of a wave, every lane gets it: the xor butterfly 32, 16, 8, 4, 2, 1 (float, double, 32- and 64-bit integers).
// All 64 lanes must be active.
template <typename T>
__device__ __forceinline__ T bf_wave_sum(T v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// op over the NT values of a workgroup of NT threads (a power of two), every thread gets it.  red = NT elements of LDS.
// Pairing: step st = NT/2, NT/4, .. 1 forms red[t] = op(red[t], red[t + st]) for t < st.  The barrier behind the read of red[0]
// lets the caller reuse red at once.
template <int NT, typename Op, typename T>
__device__ __forceinline__ T bf_block_reduce(T* red, const int tid, const T v)
{
    static_assert(NT >= 2 && (NT & (NT - 1)) == 0, "the tree halves a power of two");
    red[tid] = v;
    __syncthreads();
    for (int st = NT / 2; st > 0; st >>= 1) {
        if (tid < st) red[tid] = Op()(red[tid], red[tid + st]);
        __syncthreads();
    }
    const T r = red[0];
    __syncthreads();
    return r;
}

// ---- the two-stage sum of the evaluation kernels: no atomics, one partial per workgroup and quantity, one workgroup adds them ----
// Stage one, in a workgroup of 256 threads (4 waves) that reduces up to QMAX quantities, each independently of the others:
//   every thread has added its own terms in ascending order;
//   bf_tile_stage     the wave butterfly of quantity q, lane 0 parks the wave's sum in red[wave][q]   (all threads call it);
//   bf_tile_partials  behind a barrier, thread q < nq writes (r0 + r1) + (r2 + r3) to partial[q].
template <int QMAX, typename T>
__device__ __forceinline__ void bf_tile_stage(T (*red)[QMAX], const int q, const T v)
{
    const T w = bf_wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = w;
}

template <int QMAX, typename T>
__device__ __forceinline__ void bf_tile_partials(T (*red)[QMAX], const int nq, T* __restrict__ partial)
{
    __syncthreads();
    const int q = threadIdx.x;
    if (q < nq) partial[q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
}

// Stage two, in a workgroup of 256 threads: the sum of p[i * stride], i < tiles -- thread t adds i = t, t + 256, .. in ascending
// order, then the tree of bf_block_reduce.  Every thread gets the sum; red (256 elements) is free again on return.
template <typename T>
__device__ __forceinline__ T bf_finalize_partials(const T* __restrict__ p, const int64_t tiles, const int64_t stride, T* red)
{
    T acc = (T)0;
    for (int64_t i = threadIdx.x; i < tiles; i += 256) acc += p[i * stride];
    return bf_block_reduce<256, BfSum>(red, (int)threadIdx.x, acc);
}
