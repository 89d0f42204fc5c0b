// BM3D (bf_op_bm3d_step, bf_op_bm3d_finish): block matching and collaborative filtering (Dabov, Foi, Katkovnik, Egiazarian, IEEE
// TIP 2007) in integer arithmetic.  The host side is blind_image_denoising_amd/bm3d.py; the definition is in include/bfcnn_hip.h,
// the choices and the measurements are DESIGN.md 7.21.  Scalars only: nothing is uploaded, allocated or synchronised.
//
// A workgroup of eight waves owns a tile of reference blocks whose corners span fewer than 24 pixels each way, and a wave one
// reference block at a time.  The wave's search region (at most 32 x 32 pixels of the guide, one dword per pixel with the channels
// in its bytes) goes to LDS, rows 33 dwords apart.  Matching: a lane owns up to ten of the (2 r + 1)^2 candidates; with
// D = S(ref) + S(q) - 2 X every pixel pair costs two v_dot4_u32_u8, and the reference's pixel is one LDS broadcast shared by the
// lane's candidates.  Selection: the keys (D << 10) | index are unique, so K - 1 rounds of a wave minimum pick the group in order.
// Transform: a lane is one of the 64 pixels of a block and holds its 16 x C values along the group.  The 8 x 8 Hadamard is six
// xor butterflies across the lanes, H16 along the group is lane-local and always runs at 16 on a group padded with zeros:
// H16 = H(16 / K) (x) HK, so the first K outputs of the forward pass are HK of the group, and the first K outputs of the back pass
// over (u, 0, ..., 0) are HK u -- the definition's 16 / K brings every group to one scale.  The Wiener gain's 64-bit division is
// one fp64 division and an exact correction (both operands < 2^53).  Aggregation: every block of a tile's groups lies within
// r + 7 pixels of the tile's corners, at most 55 x 55 pixels; the workgroup sums them in LDS (ds_add_u64, (C + 1) K wave
// instructions per reference block) and adds the pixels that were reached to global memory once, with 64-bit integer atomics,
// because the reach of neighbouring tiles overlaps.  Integer sums: any order gives the same bits.  Adding every group straight to
// global memory instead made the aggregation 86 % of a step.
#include "bf_common.h"

#ifndef BM3D_ABLATE
#define BM3D_ABLATE 0       // timing only (tools/ablate_unit.sh bm3d BM3D_ABLATE 1): 1 = a step without its aggregation
#endif

namespace {

constexpr int BM_BLOCK = 8, BM_GROUP = 16, BM_MAXR = 12, BM_MAXSTEP = 8, BM_WAVE = 64, BM_WAVES = 8, BM_THREADS = BM_WAVE * BM_WAVES;
constexpr int BM_SPAN = 24;                                          // a tile's reference corners: fewer than 24 pixels from first to last
constexpr int BM_REACH = BM_SPAN + 2 * BM_MAXR + BM_BLOCK - 1;       // 55: the pixels a tile's groups can reach along an axis
constexpr int BM_SIDE = 2 * BM_MAXR + BM_BLOCK;                      // 32
constexpr int BM_PITCH = BM_SIDE + 1;                                // 33 = 1 mod 4
constexpr int BM_SLOTS = ((2 * BM_MAXR + 1) * (2 * BM_MAXR + 1) + BM_WAVE - 1) / BM_WAVE;      // 10 candidates per lane
constexpr long long BM_MAX_TAU = 1ll << 24;                          // D <= 255^2 * 64 * 4 < 2^24
constexpr long long BM_MAX_THR = 1ll << 40;                          // t t <= 2^40
constexpr long long BM_MAX_V = 1ll << 52;                            // S << 12 <= 2^52: above it every gain is 0
constexpr unsigned long long BM_NO_KEY = ~0ull;

template <int C> __device__ __forceinline__ constexpr int bm_n2(int c) { return C == 3 ? (c == 0 ? 3 : (c == 1 ? 2 : 6)) : C; }

// A along the channels
template <int C> __device__ __forceinline__ void bm_channels_forward(int* v)
{
    if constexpr (C == 2) {
        const int a = v[0], b = v[1];
        v[0] = a + b; v[1] = a - b;
    } else if constexpr (C == 3) {
        const int a = v[0], b = v[1], c = v[2];
        v[0] = a + b + c; v[1] = a - c; v[2] = a - 2 * b + c;
    } else if constexpr (C == 4) {
        const int a = v[0], b = v[1], c = v[2], d = v[3];
        v[0] = a + b + c + d; v[1] = a - b + c - d; v[2] = a + b - c - d; v[3] = a - b - c + d;
    }
}

// Bk along the channels: Bk A = s I
template <int C> __device__ __forceinline__ void bm_channels_back(int* v)
{
    if constexpr (C == 3) {
        const int a = v[0], b = v[1], c = v[2];
        v[0] = 2 * a + 3 * b + c; v[1] = 2 * a - 2 * c; v[2] = 2 * a - 3 * b + c;
    } else {
        bm_channels_forward<C>(v);                                   // Hadamard matrices are their own back matrix
    }
}

// H16 along the group, lane-local
template <int C> __device__ __forceinline__ void bm_group_hadamard(int (&v)[BM_GROUP][C])
{
#pragma unroll
    for (int m = 1; m < BM_GROUP; m <<= 1)
#pragma unroll
        for (int k = 0; k < BM_GROUP; ++k)
            if (!(k & m))
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int a = v[k][c], b = v[k | m][c];
                    v[k][c] = a + b;
                    v[k | m][c] = a - b;
                }
}

// H8 . H8 of the first K blocks: the lane is the pixel, six xor butterflies
template <int C> __device__ __forceinline__ void bm_block_hadamard(int (&v)[BM_GROUP][C], int K, int lane)
{
#pragma unroll
    for (int k = 0; k < BM_GROUP; ++k) {
        if (k < K) {                                                 // uniform
#pragma unroll
            for (int m = 1; m < BM_WAVE; m <<= 1) {
                const bool hi = lane & m;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int other = __shfl_xor(v[k][c], m);
                    v[k][c] = hi ? other - v[k][c] : other + v[k][c];
                }
            }
        }
    }
}

// floor(a / dn) for a <= 2^52, dn >= 1: above a the quotient is 0, else both convert to fp64 exactly, the quotient of the correctly
// rounded division is within one of the integer quotient, and the products below say which way
__device__ __forceinline__ unsigned bm_gain(unsigned long long a, unsigned long long dn)
{
    if (dn > a) return 0u;
    unsigned long long q = (unsigned long long)((double)a / (double)dn);
    if (q * dn > a) --q;
    else if ((q + 1) * dn <= a) ++q;
    return (unsigned)q;
}

// what a wave wrote to LDS is visible to its other lanes: the LDS serves a wave's accesses in order, this keeps the compiler from
// moving them across
__device__ __forceinline__ void bm_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// blockIdx.x = (b ty + i) tx + j: the reference blocks (iy, ix), i rb <= iy < min((i + 1) rb, ny) and the same in x, of image b; the
// reference block (iy, ix) is at (min(iy step, H - 8), min(ix step, W - 8)); (rb - 1) step < BM_SPAN
template <int C, bool WIENER>
__global__ __launch_bounds__(BM_THREADS) void bm3d_step_kernel(const uint8_t* __restrict__ noisy, const uint8_t* __restrict__ guide,
                                                               const long long* __restrict__ params, int H, int W, int R, int step,
                                                               int ny, int nx, int rb, int ty, int tx, unsigned long long* __restrict__ acc)
{
    __shared__ unsigned long long lacc[BM_REACH * BM_REACH * (C + 1)];
    __shared__ unsigned regs[BM_WAVES][BM_SIDE * BM_PITCH];
    __shared__ int gposs[BM_WAVES][BM_GROUP];                        // (row << 8) | column of a block of the group inside the region
    const int lane = threadIdx.x & (BM_WAVE - 1), wave = threadIdx.x / BM_WAVE;
    unsigned* reg = regs[wave];
    int* gpos = gposs[wave];
    int g = blockIdx.x;
    const int iy0 = ((g / tx) % ty) * rb, ix0 = (g % tx) * rb;
    const int64_t b = g / tx / ty;
    const int iy1 = min(iy0 + rb, ny), ix1 = min(ix0 + rb, nx), nrefs = (iy1 - iy0) * (ix1 - ix0);
    // the pixels the tile's groups reach: rows ay0 .. ay0 + ah - 1, ah <= (rb - 1) step + 2 R + 8 <= BM_REACH
    const int ay0 = max(0, min(iy0 * step, H - BM_BLOCK) - R), ax0 = max(0, min(ix0 * step, W - BM_BLOCK) - R);
    const int ah = min(H, min((iy1 - 1) * step, H - BM_BLOCK) + R + BM_BLOCK) - ay0;
    const int aw = min(W, min((ix1 - 1) * step, W - BM_BLOCK) + R + BM_BLOCK) - ax0;
    for (int e = threadIdx.x; e < ah * aw * (C + 1); e += BM_THREADS) lacc[e] = 0ull;
    __syncthreads();
    const uint8_t* __restrict__ gi = guide + b * H * W * C;
    const uint8_t* __restrict__ ni = noisy + b * H * W * C;
    const long long* __restrict__ prm = params + 4 * b;
    const int tau = (int)min(max(prm[WIENER ? 2 : 0], 0ll), BM_MAX_TAU);

    for (int ref_i = wave; ref_i < nrefs; ref_i += BM_WAVES) {      // uniform in the wave; no workgroup barrier inside
        const int iy = iy0 + ref_i / (ix1 - ix0), ix = ix0 + ref_i % (ix1 - ix0);
        const int y = min(iy * step, H - BM_BLOCK), x = min(ix * step, W - BM_BLOCK);
        const int ya = max(0, y - R), yb = min(H - BM_BLOCK, y + R), xa = max(0, x - R), xb = min(W - BM_BLOCK, x + R);
        const int rh = yb - ya + BM_BLOCK, rw = xb - xa + BM_BLOCK;      // <= 32: the region lies wholly inside the frame
        bm_wave_sync();                                                  // the reads of the reference block before are done

        for (int e = lane; e < rh * rw; e += BM_WAVE) {
            const int ly = e / rw, lx = e - ly * rw;
            const uint8_t* __restrict__ s = gi + ((int64_t)(ya + ly) * W + xa + lx) * C;
            unsigned v = 0u;
#pragma unroll
            for (int c = 0; c < C; ++c) v |= (unsigned)s[c] << (8 * c);
            reg[ly * BM_PITCH + lx] = v;
        }
        bm_wave_sync();

        // ---- matching: candidate i = lane + 64 j of the (2 R + 1)^2 window, i = (dy + R)(2 R + 1) + dx + R
        const int side = 2 * R + 1, ncand = side * side, nslots = (ncand + BM_WAVE - 1) / BM_WAVE;
        const int ry = y - ya, rx = x - xa;
        int caddr[BM_SLOTS];
        bool valid[BM_SLOTS];
#pragma unroll
        for (int j = 0; j < BM_SLOTS; ++j) {
            const int i = lane + BM_WAVE * j;
            const int dy = i / side - R, dx = i % side - R, cy = y + dy, cx = x + dx;
            valid[j] = i < ncand && cy >= ya && cy <= yb && cx >= xa && cx <= xb && !(dy == 0 && dx == 0);
            caddr[j] = valid[j] ? (cy - ya) * BM_PITCH + cx - xa : 0;   // a candidate that does not exist reads the region's corner
        }
        unsigned X[BM_SLOTS], Sq[BM_SLOTS], Sr = 0u;
#pragma unroll
        for (int j = 0; j < BM_SLOTS; ++j) X[j] = Sq[j] = 0u;
        const unsigned* __restrict__ ref = reg + ry * BM_PITCH + rx;
#pragma unroll 1
        for (int u = 0; u < BM_BLOCK; ++u)
#pragma unroll
            for (int v = 0; v < BM_BLOCK; ++v) {
                const unsigned p = ref[u * BM_PITCH + v];
                Sr = __builtin_amdgcn_udot4(p, p, Sr, false);
#pragma unroll
                for (int j = 0; j < BM_SLOTS; ++j)
                    if (j < nslots) {                                    // uniform
                        const unsigned q = reg[caddr[j] + u * BM_PITCH + v];
                        X[j] = __builtin_amdgcn_udot4(p, q, X[j], false);
                        Sq[j] = __builtin_amdgcn_udot4(q, q, Sq[j], false);
                    }
            }
        unsigned long long key[BM_SLOTS];
        int n = 1;                                                       // the reference block itself always counts
#pragma unroll
        for (int j = 0; j < BM_SLOTS; ++j) {
            const unsigned D = Sr + Sq[j] - 2u * X[j];                   // >= 0: a sum of squares
            const bool counts = valid[j] && D <= (unsigned)tau;
            key[j] = counts ? ((unsigned long long)D << 10) | (unsigned)(lane + BM_WAVE * j) : BM_NO_KEY;
            n += __popcll(__ballot(counts));
        }
        const int K = n >= BM_GROUP ? BM_GROUP : 1 << (31 - __clz(n));

        // ---- selection: the reference first (its key is -1), then K - 1 wave minima of unique keys
        if (lane == 0) gpos[0] = (ry << 8) | rx;
        for (int k = 1; k < K; ++k) {
            unsigned long long m = key[0];
#pragma unroll
            for (int j = 1; j < BM_SLOTS; ++j) m = min(m, key[j]);
#pragma unroll
            for (int off = BM_WAVE / 2; off > 0; off >>= 1) m = min(m, (unsigned long long)__shfl_xor(m, off));
#pragma unroll
            for (int j = 0; j < BM_SLOTS; ++j) key[j] = key[j] == m ? BM_NO_KEY : key[j];
            if (lane == 0) {
                const int i = (int)(m & 1023u);
                gpos[k] = ((ry + i / side - R) << 8) | (rx + i % side - R);
            }
        }
        bm_wave_sync();

        // ---- the group: the lane's pixel of every block
        const int py = lane >> 3, px = lane & 7;
        int t[BM_GROUP][C], tb[WIENER ? BM_GROUP : 1][C];
#pragma unroll
        for (int k = 0; k < BM_GROUP; ++k) {
            if (k < K) {
                const int pos = gpos[k], ly = (pos >> 8) + py, lx = (pos & 255) + px;
                const uint8_t* __restrict__ s = ni + ((int64_t)(ya + ly) * W + xa + lx) * C;
#pragma unroll
                for (int c = 0; c < C; ++c) t[k][c] = s[c];
                if constexpr (WIENER) {
                    const unsigned q = reg[ly * BM_PITCH + lx];
#pragma unroll
                    for (int c = 0; c < C; ++c) tb[k][c] = (q >> (8 * c)) & 0xFFu;
                }
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    t[k][c] = 0;
                    if constexpr (WIENER) tb[k][c] = 0;
                }
            }
        }

        // ---- forward: H8 . H8 per block, H16 along the padded group (its first K outputs are HK), A along the channels
        bm_block_hadamard<C>(t, K, lane);
        bm_group_hadamard<C>(t);
#pragma unroll
        for (int k = 0; k < BM_GROUP; ++k) bm_channels_forward<C>(t[k]);
        if constexpr (WIENER) {
            bm_block_hadamard<C>(tb, K, lane);
            bm_group_hadamard<C>(tb);
#pragma unroll
            for (int k = 0; k < BM_GROUP; ++k) bm_channels_forward<C>(tb[k]);
        }

        // ---- shrink the first K coefficients, zero the copies
        unsigned long long w;
        if constexpr (WIENER) {
            const unsigned long long vK = (unsigned long long)min(max(prm[3], 0ll), BM_MAX_V) * (unsigned)K;      // <= 2^56
            unsigned gg = 0u;                                            // <= 64 coefficients of g g <= 2^24 per lane
#pragma unroll
            for (int k = 0; k < BM_GROUP; ++k)
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    if (k < K) {
                        const unsigned long long S = (unsigned long long)((long long)tb[k][c] * tb[k][c]);
                        const unsigned gain = bm_gain(S << 12, max(S + vK * (unsigned)bm_n2<C>(c), 1ull));
                        t[k][c] = (int)(((long long)t[k][c] * (long long)gain + 2048) >> 12);
                        gg += gain * gain;
                    } else {
                        t[k][c] = 0;
                    }
                }
            unsigned long long tt = gg;
#pragma unroll
            for (int off = BM_WAVE / 2; off > 0; off >>= 1) tt += (unsigned long long)__shfl_xor(tt, off);
            w = min(max((1ull << 36) / max(tt, 1ull), 1ull), 1ull << 14);
        } else {
            const long long thrK = min(max(prm[1], 0ll), BM_MAX_THR) * K;       // <= 2^44
            int nnz = 0;
#pragma unroll
            for (int k = 0; k < BM_GROUP; ++k)
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const bool keep = k < K && (long long)t[k][c] * t[k][c] > thrK * bm_n2<C>(c);
                    if (k < K) nnz += __popcll(__ballot(keep));
                    t[k][c] = keep ? t[k][c] : 0;
                }
            w = (unsigned long long)max(4096 / max(nnz, 1), 1);
        }

        // ---- back: Bk along the channels, H16 along the group, H8 . H8 per block, times 16 / K (|value| < 2^27, bfcnn_hip.h)
#pragma unroll
        for (int k = 0; k < BM_GROUP; ++k) bm_channels_back<C>(t[k]);
        bm_group_hadamard<C>(t);
        bm_block_hadamard<C>(t, K, lane);
        const int up = BM_GROUP / K;

        // ---- aggregate
        if (BM3D_ABLATE == 1 && prm[0] != INT64_MIN) continue;           // a condition no caller meets keeps the work above alive
#pragma unroll
        for (int k = 0; k < BM_GROUP; ++k) {
            if (k < K) {
                const int pos = gpos[k], ly = (pos >> 8) + py, lx = (pos & 255) + px;
                unsigned long long* a = lacc + ((ya + ly - ay0) * aw + xa + lx - ax0) * (C + 1);
#pragma unroll
                for (int c = 0; c < C; ++c) atomicAdd(a + c, (unsigned long long)((long long)w * (long long)(t[k][c] * up)));
                atomicAdd(a + C, w);
            }
        }
    }

    // ---- the pixels the tile reached, to global memory: neighbouring tiles reach the same pixels
    __syncthreads();
    for (int e = threadIdx.x; e < ah * aw; e += BM_THREADS) {
        const unsigned long long* l = lacc + e * (C + 1);
        if (l[C] == 0ull) continue;                                  // den: no group reached the pixel
        const int ly = e / aw, lx = e - ly * aw;
        unsigned long long* __restrict__ a = acc + ((b * H + ay0 + ly) * W + ax0 + lx) * (C + 1);
#pragma unroll
        for (int c = 0; c <= C; ++c) atomicAdd(a + c, l[c]);
    }
}

// one thread per pixel
__global__ __launch_bounds__(256) void bm3d_finish_kernel(const long long* __restrict__ acc, int64_t npix, int C, int scale,
                                                          void* __restrict__ out, int out_u8, long long* __restrict__ weights)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const long long* __restrict__ a = acc + p * (C + 1);
    const long long den = a[C], d = den * 1024 * scale;              // < 2^43 (bfcnn_hip.h)
    for (int c = 0; c < C; ++c) {
        const long long num = a[c];
        if (out_u8) {
            const unsigned long long q = d > 0 ? (2ull * (unsigned long long)max(num, 0ll) + (unsigned long long)d) / (2ull * (unsigned long long)d) : 0ull;
            ((uint8_t*)out)[p * C + c] = (uint8_t)min(q, 255ull);
        } else {
            ((float*)out)[p * C + c] = (float)__ddiv_rn((double)num, (double)d);
        }
    }
    if (weights) weights[p] = den;
}

template <int C>
void bm3d_launch(bool wiener, int B, hipStream_t s, const uint8_t* noisy, const uint8_t* guide, const long long* prm, int H, int W,
                 int R, int step, int ny, int nx, unsigned long long* acc)
{
    const int rb = (BM_SPAN - 1) / step + 1;                         // (rb - 1) step < BM_SPAN
    const int ty = (ny + rb - 1) / rb, tx = (nx + rb - 1) / rb;
    const dim3 grid((unsigned)((int64_t)B * ty * tx));               // <= B ny nx
    if (wiener) hipLaunchKernelGGL((bm3d_step_kernel<C, true>), grid, dim3(BM_THREADS), 0, s, noisy, guide, prm, H, W, R, step, ny, nx, rb, ty, tx, acc);
    else hipLaunchKernelGGL((bm3d_step_kernel<C, false>), grid, dim3(BM_THREADS), 0, s, noisy, guide, prm, H, W, R, step, ny, nx, rb, ty, tx, acc);
}

int bm3d_scale(int C) { return C == 3 ? 6 : C; }                    // Bk A = s I

bool bm3d_bad_shape(int B, int H, int W, int C)
{
    return B <= 0 || H < BM_BLOCK || W < BM_BLOCK || C < 1 || C > 4 || (int64_t)B * H * W * C > INT32_MAX;
}

}  // namespace

extern "C" int bf_op_bm3d_step(const uint8_t* noisy, const uint8_t* guide, const int64_t* params, int B, int H, int W, int C, int search,
                               int step, int wiener, int64_t* acc, void* stream)
{
    if (!noisy || !guide || !params || !acc || bm3d_bad_shape(B, H, W, C)) return BF_EINVAL;
    if (search < 1 || search > BM_MAXR || step < 1 || step > BM_MAXSTEP) return BF_EINVAL;
    if ((uintptr_t)params % 8 || (uintptr_t)acc % 8 || (const void*)acc == (const void*)noisy || (const void*)acc == (const void*)guide)
        return BF_EINVAL;
    const int ny = (H - BM_BLOCK) / step + 1 + ((H - BM_BLOCK) % step ? 1 : 0), nx = (W - BM_BLOCK) / step + 1 + ((W - BM_BLOCK) % step ? 1 : 0);
    if ((int64_t)B * ny * nx > INT32_MAX) return BF_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(acc, 0, (size_t)B * H * W * (C + 1) * sizeof(int64_t), s) != hipSuccess) return BF_EHIP;
    const long long* prm = (const long long*)params;
    unsigned long long* a = (unsigned long long*)acc;
    switch (C) {
    case 1: bm3d_launch<1>(wiener != 0, B, s, noisy, guide, prm, H, W, search, step, ny, nx, a); break;
    case 2: bm3d_launch<2>(wiener != 0, B, s, noisy, guide, prm, H, W, search, step, ny, nx, a); break;
    case 3: bm3d_launch<3>(wiener != 0, B, s, noisy, guide, prm, H, W, search, step, ny, nx, a); break;
    default: bm3d_launch<4>(wiener != 0, B, s, noisy, guide, prm, H, W, search, step, ny, nx, a); break;
    }
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}

extern "C" int bf_op_bm3d_finish(const int64_t* acc, int B, int H, int W, int C, void* out, int cast_to_uint8, int64_t* weights_or_null,
                                 void* stream)
{
    if (!acc || !out || bm3d_bad_shape(B, H, W, C)) return BF_EINVAL;
    if ((uintptr_t)acc % 8 || (uintptr_t)weights_or_null % 8 || (!cast_to_uint8 && (uintptr_t)out % 4) || out == (const void*)acc ||
        (const void*)weights_or_null == (const void*)acc)
        return BF_EINVAL;
    const int64_t npix = (int64_t)B * H * W;
    hipLaunchKernelGGL(bm3d_finish_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const long long*)acc,
                       npix, C, bm3d_scale(C), out, cast_to_uint8, (long long*)weights_or_null);
    return hipGetLastError() == hipSuccess ? BF_OK : BF_EHIP;
}
