// Self-ensemble ("x8" test-time augmentation) around the denoiser: the eight flips and rotations of an image batch written in
// one pass over the uint8 input (bf_op_dihedral_stack_u8), and inverse transform + mean + round-half-even + cast of the float
// results in one pass over them (bf_op_dihedral_merge).
//
// Numbering, for k = 0..7 on x[B,H,W,C]:  T_k(x) = flipW^(k >> 2)(rot90^(k & 3)(x)), rot90 = np.rot90(x, 1, axes=(1, 2)),
// flipW = x[:, :, ::-1].  Source pixel (y, x) of an [H, W] image lands in member k at
//     even k (shape kept, [H, W]):     row = fy ? H-1-y : y,  column = fx ? W-1-x : x
//     odd k (shape swapped, [W, H]):   row = fx ? W-1-x : x,  column = fy ? H-1-y : y
// with (fx, fy) per k from the tables below; the merge reads member k at the same position, which IS T_k^-1.
//
// Both kernels work on DH_T x DH_T pixel tiles of the untransformed image, one workgroup per tile, and index global memory by
// BYTE (stack) or FLOAT (merge) of a tile row, so that the lanes of a wave touch consecutive addresses of one row in the read and
// in every write whatever the transform does to the pixels (a reversed row is walked forwards through its destination).  A
// shape-swapping member turns tile rows into tile columns: that goes through an LDS tile which is filled along rows and read along
// columns.  LDS rows are padded to an odd number of dwords (u8: DH_T*C + 4 bytes = 25 / 9 dwords) or to DH_T*C + C floats
// (99 / 33), so that the column walk of a 32-lane group (ds_read_u8 / ds_read_b32 bank = (address / 4) mod 32) lands on 32
// different banks.
#include "bf_common.h"

namespace {

constexpr int DH_T = 32;                 // tile edge in pixels
constexpr int DH_THREADS = 256;

__constant__ const unsigned char DH_FX[8] = {0, 1, 1, 0, 1, 1, 0, 0};
__constant__ const unsigned char DH_FY[8] = {0, 0, 1, 1, 0, 1, 1, 0};

struct DihedralMembers {
    void* ptr[8];        // first image of member j in its batch (j-th selected k in ascending order)
    int k[8];
    int n;
};

template <int C>
__global__ __launch_bounds__(DH_THREADS) void dihedral_stack_u8_kernel(const uint8_t* __restrict__ src, DihedralMembers mem,
                                                                       int H, int W)
{
    constexpr int ROWB = DH_T * C + 4;                   // LDS row pitch in bytes
    constexpr int TILE_B = DH_T * DH_T * C;
    __shared__ uint8_t tile[DH_T * ROWB];
    const int x0 = blockIdx.x * DH_T, y0 = blockIdx.y * DH_T;
    const int64_t b = blockIdx.z;
    const int tw = min(DH_T, W - x0), th = min(DH_T, H - y0);

    for (int t = threadIdx.x; t < TILE_B; t += DH_THREADS) {
        const int r = t / (DH_T * C), cb = t % (DH_T * C);
        if (r < th && cb < tw * C) tile[r * ROWB + cb] = src[((b * H + y0 + r) * W + x0) * C + cb];
    }
    __syncthreads();

    for (int m = 0; m < mem.n; ++m) {
        const int k = mem.k[m];
        const bool fx = DH_FX[k], fy = DH_FY[k];
        uint8_t* __restrict__ dst = (uint8_t*)mem.ptr[m] + b * H * W * C;
        if (!(k & 1)) {
            // tile row r -> destination row y0 + r (or its mirror); destination bytes of that row run forwards from column x0
            // (or from the mirror of the tile's last column): pixel p of the run is source pixel p (or tw-1-p)
            const int j0 = fx ? W - x0 - tw : x0;
            for (int t = threadIdx.x; t < TILE_B; t += DH_THREADS) {
                const int r = t / (DH_T * C), cb = t % (DH_T * C), p = cb / C, ch = cb % C;
                if (r < th && p < tw) {
                    const int i = fy ? H - 1 - (y0 + r) : y0 + r;
                    dst[((int64_t)i * W + j0 + p) * C + ch] = tile[r * ROWB + (fx ? tw - 1 - p : p) * C + ch];
                }
            }
        } else {
            // tile COLUMN r -> destination row x0 + r (or its mirror) of the [W, H] image; pixel p of the run is source row p
            // (or th-1-p) of that column
            const int j0 = fy ? H - y0 - th : y0;
            for (int t = threadIdx.x; t < TILE_B; t += DH_THREADS) {
                const int r = t / (DH_T * C), cb = t % (DH_T * C), p = cb / C, ch = cb % C;
                if (r < tw && p < th) {
                    const int i = fx ? W - 1 - (x0 + r) : x0 + r;
                    dst[((int64_t)i * H + j0 + p) * C + ch] = tile[(fy ? th - 1 - p : p) * ROWB + r * C + ch];
                }
            }
        }
    }
}

template <int C>
__global__ __launch_bounds__(DH_THREADS) void dihedral_merge_kernel(DihedralMembers mem, void* __restrict__ out, int out_u8,
                                                                    int H, int W)
{
    constexpr int ROWF = DH_T * C + C;                   // LDS row pitch in floats
    constexpr int TILE_F = DH_T * DH_T * C;
    constexpr int PER = TILE_F / DH_THREADS;             // accumulators per thread: 12 (C = 3) or 4
    __shared__ float tile[DH_T * ROWF];
    const int x0 = blockIdx.x * DH_T, y0 = blockIdx.y * DH_T;
    const int64_t b = blockIdx.z;
    const int tw = min(DH_T, W - x0), th = min(DH_T, H - y0);

    float s[PER];
    for (int m = 0; m < mem.n; ++m) {                    // ascending k: the order of the sum is part of the contract
        const int k = mem.k[m];
        const bool fx = DH_FX[k], fy = DH_FY[k];
        const float* __restrict__ f = (const float*)mem.ptr[m] + b * H * W * C;
        if (!(k & 1)) {
            const int j0 = fx ? W - x0 - tw : x0;
#pragma unroll
            for (int q = 0; q < PER; ++q) {
                const int t = threadIdx.x + q * DH_THREADS;
                const int r = t / (DH_T * C), cb = t % (DH_T * C), p = cb / C, ch = cb % C;
                float v = 0.f;
                if (r < th && p < tw) {
                    const int i = fy ? H - 1 - (y0 + r) : y0 + r;
                    v = f[((int64_t)i * W + j0 + (fx ? tw - 1 - p : p)) * C + ch];
                }
                s[q] = m == 0 ? v : s[q] + v;
            }
        } else {
            // the member's [tw rows x th columns] tile: filled along its rows, read along its columns
            const int j0 = fy ? H - y0 - th : y0;
            __syncthreads();                             // the reads of the previous odd member are done
            for (int t = threadIdx.x; t < TILE_F; t += DH_THREADS) {
                const int r = t / (DH_T * C), cb = t % (DH_T * C);
                if (r < tw && cb < th * C) {
                    const int i = fx ? W - 1 - (x0 + r) : x0 + r;
                    tile[r * ROWF + cb] = f[((int64_t)i * H + j0) * C + cb];
                }
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < PER; ++q) {
                const int t = threadIdx.x + q * DH_THREADS;
                const int r = t / (DH_T * C), cb = t % (DH_T * C), p = cb / C, ch = cb % C;
                float v = 0.f;
                if (r < th && p < tw) v = tile[p * ROWF + (fy ? th - 1 - r : r) * C + ch];
                s[q] = m == 0 ? v : s[q] + v;
            }
        }
    }

    const float n = (float)mem.n;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int t = threadIdx.x + q * DH_THREADS;
        const int r = t / (DH_T * C), cb = t % (DH_T * C);
        if (r < th && cb < tw * C) {
            const float mean = __fdiv_rn(s[q], n);
            const int64_t o = ((b * H + y0 + r) * W + x0) * C + cb;
            if (out_u8) ((uint8_t*)out)[o] = (uint8_t)rintf(fminf(fmaxf(mean, 0.f), 255.f));   // half to even, as the head kernel
            else ((float*)out)[o] = mean;
        }
    }
}

// the selected members in ascending k with the address of each one's first image: even k in `even`, odd k in `odd`, member-major
// within each; odd == NULL with odd members selected = the joint layout (H == W only): every member in `even`, ascending k
int dihedral_members(DihedralMembers& mem, const void* even, const void* odd, int B, int H, int W, int C, int members,
                     size_t elem)
{
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || members <= 0 || members > 255) return BF_EINVAL;
    const bool any_even = members & 0x55, any_odd = members & 0xAA;
    const bool joint = any_odd && !odd;
    if (joint && H != W) return BF_EINVAL;
    if ((any_even || joint) && !even) return BF_EINVAL;
    if (C != 1 && C != 3) return BF_EUNSUPPORTED;
    if (B > 65535 || (H + DH_T - 1) / DH_T > 65535) return BF_EUNSUPPORTED;
    const size_t member_bytes = (size_t)B * H * W * C * elem;
    int n_even = 0, n_odd = 0;
    mem.n = 0;
    for (int k = 0; k < 8; ++k) {
        if (!(members >> k & 1)) continue;
        const bool to_odd = (k & 1) && !joint;
        const size_t slot = joint ? (size_t)mem.n : (size_t)(to_odd ? n_odd++ : n_even++);
        mem.ptr[mem.n] = (char*)(to_odd ? odd : even) + slot * member_bytes;
        mem.k[mem.n++] = k;
    }
    return BF_OK;
}

}  // namespace

extern "C" int bf_op_dihedral_stack_u8(const uint8_t* src, uint8_t* dst_even, uint8_t* dst_odd, int B, int H, int W, int C,
                                       int members, void* stream)
{
    if (!src || src == dst_even || src == dst_odd) return BF_EINVAL;
    DihedralMembers mem;
    const int rc = dihedral_members(mem, dst_even, dst_odd, B, H, W, C, members, 1);
    if (rc != BF_OK) return rc;
    const dim3 grid((W + DH_T - 1) / DH_T, (H + DH_T - 1) / DH_T, B);
    if (C == 3) hipLaunchKernelGGL(dihedral_stack_u8_kernel<3>, grid, dim3(DH_THREADS), 0, (hipStream_t)stream, src, mem, H, W);
    else hipLaunchKernelGGL(dihedral_stack_u8_kernel<1>, grid, dim3(DH_THREADS), 0, (hipStream_t)stream, src, mem, H, W);
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}

extern "C" int bf_op_dihedral_merge(const float* src_even, const float* src_odd, void* out, int B, int H, int W, int C,
                                    int members, int out_u8, void* stream)
{
    if (!out || out == (const void*)src_even || out == (const void*)src_odd) return BF_EINVAL;
    DihedralMembers mem;
    const int rc = dihedral_members(mem, src_even, src_odd, B, H, W, C, members, sizeof(float));
    if (rc != BF_OK) return rc;
    const dim3 grid((W + DH_T - 1) / DH_T, (H + DH_T - 1) / DH_T, B);
    if (C == 3) hipLaunchKernelGGL(dihedral_merge_kernel<3>, grid, dim3(DH_THREADS), 0, (hipStream_t)stream, mem, out, out_u8, H, W);
    else hipLaunchKernelGGL(dihedral_merge_kernel<1>, grid, dim3(DH_THREADS), 0, (hipStream_t)stream, mem, out, out_u8, H, W);
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}
