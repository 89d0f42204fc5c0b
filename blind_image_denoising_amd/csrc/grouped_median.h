// Grouped-data median of a 512-bin (padded) histogram of 64-bit counts, in a workgroup of 256 threads: the scan shared by the
// finalize kernels of noise_estimate.hip and noise_level.hip (Donoho's MAD rule on q = twice the modulus of the Haar HH
// coefficient: sigma = median / 2 / 0.6745).  Bin 0 covers [0, 1/2), bin k >= 1 covers [k - 1/2, k + 1/2); the one bin k with
// cum(k-1) < n/2 <= cum(k) is interpolated linearly.  A histogram that is empty or has all its mass in bin 0 gives 0: no cell
// differs from zero, there is nothing to interpolate.
#pragma once
#include <hip/hip_runtime.h>

constexpr int BF_MEDIAN_BINS_PAD = 512;

// hk = the bins tid and tid + 256 of the histogram as this thread holds them, cum = 512 elements of LDS.  Exactly one thread
// writes *sigma.  Every thread gets n, the number of cells; cum is free again on return.
__device__ __forceinline__ unsigned long long bf_grouped_median_sigma(const unsigned long long (&hk)[2], unsigned long long* cum,
                                                                      double* sigma)
{
    const int tid = threadIdx.x;
    cum[tid] = hk[0];
    cum[tid + 256] = hk[1];
    __syncthreads();
    const unsigned long long bin0 = cum[0];
    __syncthreads();
    // inclusive scan of the 512 bins, two per thread
    for (int off = 1; off < BF_MEDIAN_BINS_PAD; off <<= 1) {
        unsigned long long v[2];
        for (int j = 0; j < 2; ++j) {
            const int i = tid + j * 256;
            v[j] = cum[i] + (i >= off ? cum[i - off] : 0ull);
        }
        __syncthreads();
        cum[tid] = v[0];
        cum[tid + 256] = v[1];
        __syncthreads();
    }
    const unsigned long long n = cum[BF_MEDIAN_BINS_PAD - 1];
    const double half = (double)n / 2.0;
    if (tid == 0 && (n == 0ull || bin0 == n)) *sigma = 0.0;
    if (n != 0ull && bin0 != n)
        for (int j = 0; j < 2; ++j) {
            const int k = tid + j * 256;
            const double before = (double)(cum[k] - hk[j]);
            if (hk[j] != 0ull && (double)cum[k] >= half && before < half) {
                const double lo = k == 0 ? 0.0 : (double)k - 0.5, width = k == 0 ? 0.5 : 1.0;
                const double med = lo + width * (half - before) / (double)hk[j];
                *sigma = med / 2.0 / 0.6745;
            }
        }
    __syncthreads();
    return n;
}
