// Fused residual block on the f16 matrix cores with split-f16 ("f16x3") operands: the row-streaming tile kernel
// (fused_block_h3r_kernel), the one rule that selects between it and the full-row streaming kernel (fused_h3v.hip), the
// launch, and the fp32 <-> split-planar converters of the debug entries.  The weight packer is pack_h3.hip, the training
// convolutions on the same inner loop are train_conv_h3.hip, two blocks per launch is fused_h3w.hip.
//
// Same reference semantics as fused_block_v4_kernel in conv3x3_c16.hip (bfcnn/backbone_blocks.py:174-242 with
// the inference BatchNormalization folded to scale/shift): out = x + scale * conv2(act(conv1 x)) + shift.
//
// Arithmetic.  An fp32 value v is carried as two f16 numbers hi = f16(v), lo = f16(v - hi) (22 mantissa
// bits together).  A 3x3 16->16 convolution is evaluated as
//     conv(x_hi, w_hi) + conv(x_lo, w_hi) + conv(x_hi, w_lo)          (the lo*lo term is < 2^-22 relative)
// on v_mfma_f32_16x16x32_f16 with fp32 accumulation: 15 MFMAs of 16 cycles per 16-pixel group instead of
// 36 MFMAs of 32 cycles on the f32 matrix path (4.8x fewer matrix cycles).  The weights of one kernel are
// pre-scaled by a power of two (max |w| * s in [2^13, 2^14)) so that w_lo stays a normal f16 number; 1/s is
// folded into the epilogues (exact).  tools/exp/emulate_f16x3.py sizes the error of this arithmetic against
// the fp64 oracle: 2.2e-7 normalised MAE through 1x18 (exact-fp32 arithmetic: 1.9e-7; the bar is 1e-4).
// Precondition: |activation| < 65504 (f16 range); the exact-fp32 kernel stays selectable.
//
// K packing.  One MFMA contracts K = 32 = 2 x 16 input channels; lanes q = 0,1 carry k-slots 0..15, lanes q = 2,3
// k-slots 16..31, each lane 8 consecutive channels of one pixel = ONE ds_read_b128.  Taps are paired HORIZONTALLY:
// (dy,0)|(dy,1) share an MFMA (w_hi x x_hi, w_lo x x_hi, w_hi x x_lo), and tap (dy,2) runs as [w_hi | w_hi] x [x_hi | x_lo]
// and [w_lo | 0] x [x_hi | x_lo]: 3 * (3 + 2) = 15 MFMAs per group.  A B fragment therefore depends on the INPUT ROW
// only: the four fragments of input row i (pair hi, pair lo, single, single = 4 ds_read_b128) serve the three output
// rows i, i-1, i-2 of a wave that walks down a run of R consecutive rows of one 16-column strip (h3_rows.h) --
// 4 * (R + 2) / R reads per output row, the next row's fragments in flight while the current row's MFMAs run (16 VGPRs
// of prefetch), three live accumulators.  The group-per-pass kernel this one replaced paired taps vertically, read 10
// fragments per group and parked its waves in s_waitcnt 40 % of their cycles (matrix pipe 36 % busy, LDS 34 %: latency, not
// throughput); DESIGN.md 4.1b keeps the history and the numbers of the retired kernels.
//
// Layout ("split-planar", HBM and LDS alike): per image 4 planes [rows][cols][8 x f16] = hi(c0..7),
// hi(c8..15), lo(c0..7), lo(c8..15); 64 B per pixel in total, the same as fp32 NHWC.  A b128 operand read
// is bank-conflict free (16 consecutive pixels x 16 B per lane group, both channel halves one plane apart
// = a multiple of 256 B), a lane's result goes back as ONE 16-byte record of eight channels (h3_split_record),
// and tiles move HBM -> LDS by DMA without a conversion pass.
//
// Schedule.  Persistent workgroups (8 waves on 16x32 tiles, one per CU; 4 waves on 16x16 tiles, two per CU),
// XCD-contiguous tile chunks.  The input tile is DOUBLE buffered: tile t+1 is requested while conv1 of tile t runs (one
// DMA instruction per input row) and has the rest of the tile to land; the residual comes from the LDS input tile (its
// centre), so the loop holds no vector-memory operation except the DMA and the result stores, and the one explicit
// vmcnt per tile is exact.  Barriers are bare s_barrier with lgkmcnt(0) only (hipcc puts vmcnt(0) in front of every
// __syncthreads it can see, which would drain the DMA).
#include "bf_common.h"
#include "h3_core.h"
#include "h3_rows.h"

template <int TH_, int TW_, int NW_>
struct H3Cfg {
    static constexpr int TH = TH_, TW = TW_, NW = NW_, NT = NW_ * 64;
    static constexpr int MH = TH + 2, MW = TW + 2;             // intermediate region
    static constexpr int IH = TH + 4, IW = TW + 4;             // input region
    static constexpr int GPR = TW / 16;                        // 16-pixel groups per row
    static constexpr int RSTEP = NW / GPR;                     // rows between a wave's consecutive groups
    static constexpr int SG = (MH + 7) / 8;                    // strip groups (columns TW, TW+1 of the intermediate region)
    static constexpr int IN_PLANE = IH * IW * 16;              // bytes per input-tile plane
    static constexpr int MID_PLANE = (MH * MW * 16 + 255) / 256 * 256;
    static constexpr int IN_ELEMS = 4 * IH * IW;               // 16-byte elements per input tile
    static constexpr int PF = (IN_ELEMS + NT - 1) / NT;        // DMA wave-instructions per wave (max)
    static constexpr int TIN_BYTES = PF * NT * 16;             // 4 planes + pad to PF whole workgroup-instructions
    static constexpr int LDS_BYTES = 4 * MID_PLANE + 2 * TIN_BYTES;
    static_assert(TW % 16 == 0 && NW % GPR == 0, "rows must be whole MFMA groups, waves whole rows");
    static constexpr int WG_PER_CU = (160 * 1024) / LDS_BYTES >= 2 && NW <= 4 ? 2 : 1;
    static_assert(TH % RSTEP == 0, "conv2 groups must divide evenly over the waves");
    static_assert(IN_PLANE % 256 == 0, "input planes must keep the two channel halves 256-B congruent");
    static_assert(IN_ELEMS % 64 == 0, "DMA moves whole wave-instructions");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS");
};

struct H3Tile {
    int y0, x0;
    size_t img;      // byte offset of the image in the split-planar tensor
};

template <class Cfg>
__device__ __forceinline__ H3Tile h3_tile(const FusedH3Args& a, int t)
{
    H3Tile r;
    const int tx = t % a.tiles_x;
    t /= a.tiles_x;
    const int ty = t % a.tiles_y;
    const int b = t / a.tiles_y;
    r.y0 = ty * Cfg::TH;
    r.x0 = tx * Cfg::TW;
    r.img = (size_t)b * a.H * a.W * 64;
    return r;
}

template <class Cfg>
__device__ __forceinline__ bool h3_interior(const FusedH3Args& a, const H3Tile& t)
{
    return t.y0 >= 2 && t.y0 + Cfg::TH + 2 <= a.H && t.x0 >= 2 && t.x0 + Cfg::TW + 2 <= a.W;
}

// DMA of one input tile (2-pixel halo) into an LDS buffer.  Element e = tid + i*NT of the tile (plane-major,
// then row, then column) comes from tile origin + pfoff[i]; out-of-image elements come from a zero line.
// EVERY wave issues exactly PF wave-instructions per call, whatever the tile (elements past the tile's end
// and the whole tile when !live are zero-line reads into the buffer's pad), so that the number of operations
// younger than a tile's DMA is a compile-time constant for the vmcnt at the end of the tile.
template <class Cfg, bool INTERIOR>
__device__ __forceinline__ void h3_dma(const FusedH3Args& a, const H3Tile& t, char* __restrict__ tin, const int tid,
                                       const int wave, const unsigned (&pfoff)[Cfg::PF], const bool live)
{
    const char* origin = reinterpret_cast<const char*>(a.in) + t.img + ((ptrdiff_t)(t.y0 - 2) * a.W + (t.x0 - 2)) * 16;
    const char* zeros = reinterpret_cast<const char*>(a.zeros);
#pragma unroll
    for (int i = 0; i < Cfg::PF; ++i) {
        const char* src = origin + pfoff[i];
        bool use = live;
        if ((i + 1) * Cfg::NT > Cfg::IN_ELEMS) use = use && (i * Cfg::NT + wave * 64) < Cfg::IN_ELEMS;     // wave-uniform
        if (!INTERIOR) {
            const int e = tid + i * Cfg::NT;
            const int r = e % (Cfg::IH * Cfg::IW);
            const int row = r / Cfg::IW, col = r - row * Cfg::IW;
            const int gy = t.y0 - 2 + row, gx = t.x0 - 2 + col;
            use = use && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
        }
        if (!use) src = zeros;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(tin + (i * Cfg::NT + wave * 64) * 16),
                                         16, 0, 0);
    }
}

// one of the PF wave-instructions of h3_dma (I compile-time): lets the row-streaming kernel spread the DMA issue
// over conv1's rows.  Measured with s_memtime stamps (tools/stamp_h3.py): issuing the 6 instructions back to back
// at the top of the tile costs a wave 1000-2100 cycles -- the 48 KB of the 8 waves queue up in the vector-memory
// issue path (~32 cycles per 1-KiB wave-instruction per CU) and every wave stalls in-order behind its own.
template <class Cfg, bool INTERIOR, int I>
__device__ __forceinline__ void h3_dma_one(const FusedH3Args& a, const H3Tile& t, const char* origin, char* __restrict__ tin,
                                           const int tid, const int wave, const unsigned (&pfoff)[Cfg::PF], const bool live)
{
    const char* src = origin + pfoff[I];
    bool use = live;
    if ((I + 1) * Cfg::NT > Cfg::IN_ELEMS) use = use && (I * Cfg::NT + wave * 64) < Cfg::IN_ELEMS;     // wave-uniform
    if (!INTERIOR) {
        const int e = tid + I * Cfg::NT;
        const int r = e % (Cfg::IH * Cfg::IW);
        const int row = r / Cfg::IW, col = r - row * Cfg::IW;
        const int gy = t.y0 - 2 + row, gx = t.x0 - 2 + col;
        use = use && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
    }
    if (!use) src = reinterpret_cast<const char*>(a.zeros);
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)(tin + (I * Cfg::NT + wave * 64) * 16), 16, 0, 0);
}

template <class Cfg>
struct H3RPlan {
    static constexpr int NRUN = Cfg::RSTEP;                            // row runs per strip = waves per strip
    static constexpr int R1_SMALL = Cfg::MH / NRUN, R1_BIG = R1_SMALL + 1, N_BIG = Cfg::MH % NRUN;   // conv1: 18 = 5+5+4+4
    static constexpr int R2 = Cfg::TH / NRUN;                          // conv2: 16 = 4x4
    static constexpr int N_SHORT = (NRUN - N_BIG) * Cfg::GPR;          // waves with the short run: they take the strip groups,
    static constexpr int SG_PER_WAVE = (Cfg::SG + N_SHORT - 1) / N_SHORT;  // strip group sg + k * N_SHORT on short wave sg
    static constexpr int NROWS_MIN = R1_SMALL + 2;                      // conv1 input rows of the shortest run (DMA issue slots)
    static_assert(Cfg::TH % NRUN == 0, "conv2 rows must divide over the runs");
    static_assert(N_BIG > 0 && N_BIG < NRUN, "plan assumes both run lengths occur");
};

template <class Cfg, bool INTERIOR>
__device__ __forceinline__ void h3r_conv1_store(const FusedH3Args& a, char* __restrict__ tmid, const int wr, f32x4 v,
                                                const float inv_s, const float relu_floor, const int gy, const int gx)
{
    if (!(H3_ABLATE & 64)) {
        // activation without a branch and without the canonicalising v_max x,x hipcc puts in front of fmaxf:
        // max(v, floor) with floor = 0 (relu) or -inf (linear) as median(v, floor, +inf)
        v = v * inv_s;
        v.x = __builtin_amdgcn_fmed3f(v.x, relu_floor, __builtin_inff()); v.y = __builtin_amdgcn_fmed3f(v.y, relu_floor, __builtin_inff());
        v.z = __builtin_amdgcn_fmed3f(v.z, relu_floor, __builtin_inff()); v.w = __builtin_amdgcn_fmed3f(v.w, relu_floor, __builtin_inff());
    }
    if (!INTERIOR) {
        // conv2 must see ZERO padding outside the image, not conv1 evaluated there
        if (gy < 0 || gy >= a.H || gx < 0 || gx >= a.W) v = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    *reinterpret_cast<h8*>(tmid + wr) = h3_split_record(v);      // wr: plane (q>>1) + 2*(q&1), pixel * 16
}

struct H3RLane {
    int p1, s1;      // conv1 pair / single fragment address of the run's first input row (input tile)
    int w1;          // conv1 result write of the run's first row (intermediate tile)
    int p2, s2;      // conv2 pair / single fragment address (intermediate tile)
    int rr;          // residual read of the run's first output row (input tile centre)
    unsigned g;      // global byte offset of the lane's 8-byte record of the run's first output row from the tile origin
    int px;
};

// issues the next tile's DMA wave-instructions I, I + NROWS, ... after conv1's input row I
template <class Cfg, bool NX_INTERIOR, int NROWS>
struct H3DmaHook {
    const FusedH3Args& a;
    const H3Tile& nx;
    const char* origin;
    char* tnx;
    int tid, wave;
    const unsigned (&pfoff)[Cfg::PF];
    bool live;
    template <int I> __device__ __forceinline__ void row() const
    {
        if constexpr (I < NROWS && I < Cfg::PF) {
            if (!(H3_ABLATE & 1)) h3_dma_one<Cfg, NX_INTERIOR, I>(a, nx, origin, tnx, tid, wave, pfoff, live);
            if constexpr (I + NROWS < Cfg::PF) {
                static_assert(I + 2 * NROWS >= Cfg::PF, "at most two DMA instructions per row");
                if (!(H3_ABLATE & 1)) h3_dma_one<Cfg, NX_INTERIOR, I + NROWS>(a, nx, origin, tnx, tid, wave, pfoff, live);
            }
        }
    }
};

template <class Cfg, int R, bool INTERIOR, class Hook>
__device__ __forceinline__ void h3r_conv1_run(const FusedH3Args& a, const char* __restrict__ tin, char* __restrict__ tmid,
                                              const h8 (&w)[13], const float inv_s, const float relu_floor, const H3RLane& L,
                                              const H3Tile& t, const int o0, const Hook& hook)
{
    // (plain values, no references to the lane-constant struct: a reference member kept the whole struct in scratch memory)
    struct Epi {
        struct Pre {};
        enum { EXTRA_MFMA = 0 };
        const FusedH3Args& a; char* __restrict__ tmid; float inv_s, relu_floor; int w1, gy0, gx;
        __device__ __forceinline__ Pre pre(const int) const { return Pre{}; }
        __device__ __forceinline__ f32x4 finish(const int, const f32x4 acc, const Pre&) const { return acc; }
        __device__ __forceinline__ void operator()(const int o, const f32x4 v) const
        {
            h3r_conv1_store<Cfg, INTERIOR>(a, tmid, w1 + o * Cfg::MW * 16, v, inv_s, relu_floor, gy0 + o, gx);
        }
    } const epi{a, tmid, inv_s, relu_floor, L.w1, t.y0 - 1 + o0, t.x0 - 1 + L.px};
    h3r_rows<R, Cfg::IW * 16, 2 * Cfg::IN_PLANE>(tin, L.p1, L.s1, w, epi, hook);
}

// HEAD = 1: the last block of a network with a linear denoiser head: y . wh (16 x 3, premultiplied), tanh, denormalise,
// [round, uint8] happen in the conv2 epilogue; the block output is never written and the head kernel (one more pass over
// the 64 B / pixel activation) disappears.
template <class Cfg, int HEAD = 0>
__global__ __launch_bounds__(Cfg::NT, 2) void fused_block_h3r_kernel(FusedH3Args a)
{
    using Plan = H3RPlan<Cfg>;
    extern __shared__ __attribute__((aligned(16))) char h3_lds[];
    char* tmid = h3_lds;                                        // [4][MH][MW][8 f16] (+ pad per plane)
    char* tin0 = h3_lds + 4 * Cfg::MID_PLANE;                   // [4][IH][IW][8 f16] (+ pad), two buffers
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, q = lane >> 4;
    const int run = wave / Cfg::GPR, wcol = (wave % Cfg::GPR) * 16;
#if H3_ABLATE & 256
    if (wave >= Cfg::NW / 2) __builtin_amdgcn_s_setprio(1);    // experiment: favour the younger wave of each SIMD
#endif
    const unsigned plane_g = (unsigned)a.H * (unsigned)a.W * 16u;       // bytes per global plane
    const bool big = run < Plan::N_BIG;
    const int o1 = big ? run * Plan::R1_BIG : Plan::N_BIG * Plan::R1_BIG + (run - Plan::N_BIG) * Plan::R1_SMALL;   // conv1 first row
    const int o2 = run * Plan::R2;                                                                               // conv2 first row
    const int sg = wave - Plan::N_BIG * Cfg::GPR;               // first strip group of this wave (short-run waves: sg >= 0)

    H3RLane L0;
    L0.px = wcol + n;
    {
        const int b1 = (q & 1) * Cfg::IN_PLANE + (o1 * Cfg::IW + L0.px) * 16;
        L0.p1 = b1 + (q >> 1) * 16;
        L0.s1 = b1 + 32 + (q >> 1) * 2 * Cfg::IN_PLANE;
        L0.w1 = ((q >> 1) + 2 * (q & 1)) * Cfg::MID_PLANE + (o1 * Cfg::MW + L0.px) * 16;
        const int b2 = (q & 1) * Cfg::MID_PLANE + (o2 * Cfg::MW + L0.px) * 16;
        L0.p2 = b2 + (q >> 1) * 16;
        L0.s2 = b2 + 32 + (q >> 1) * 2 * Cfg::MID_PLANE;
        // residual operand [x_hi | x_lo] of the centre pixel: lanes q < 2 read the hi planes, q >= 2 the lo planes
        L0.rr = ((q & 1) + 2 * (q >> 1)) * Cfg::IN_PLANE + ((o2 + 2) * Cfg::IW + L0.px + 2) * 16;
        L0.g = (unsigned)((q >> 1) + 2 * (q & 1)) * plane_g + (unsigned)(o2 * a.W + L0.px) * 16u;
    }

    unsigned pfoff[Cfg::PF];
#pragma unroll
    for (int i = 0; i < Cfg::PF; ++i) {
        const int e = tid + i * Cfg::NT;
        const int pl = e / (Cfg::IH * Cfg::IW), r = e - pl * (Cfg::IH * Cfg::IW);
        const int row = r / Cfg::IW, col = r - row * Cfg::IW;
        pfoff[i] = (unsigned)pl * plane_g + (unsigned)(row * a.W + col) * 16u;
    }

    h8 w1[13], w2[13];                                          // [12]: s2 * identity (conv2 only: adds the residual)
#pragma unroll
    for (int i = 0; i < 13; ++i) {
        w1[i] = reinterpret_cast<const h8*>(a.w1r)[i * 64 + lane];
        w2[i] = reinterpret_cast<const h8*>(a.w2r)[i * 64 + lane];
    }
    const float inv_s1 = a.aux[0];
    const float inv_s2 = a.aux[48];                             // BN scale is folded into the row-layout w2
    const float relu_floor = a.act1_relu ? 0.f : -__builtin_inff();
    const f32x4 sh = *reinterpret_cast<const f32x4*>(a.aux + 32 + q * 4);
    f32x4 whr[4];                                               // HEAD: rows 4q .. 4q+3 of the 16 x 4 head matrix
#pragma unroll
    for (int j = 0; j < 4; ++j) whr[j] = HEAD ? *reinterpret_cast<const f32x4*>(a.head_wh + (4 * q + j) * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};

    const int nxcd = gridDim.x >= 8 ? 8 : 1;
    const int label = blockIdx.x % nxcd, slot = blockIdx.x / nxcd;
    const int per_label = gridDim.x / nxcd;
    const int chunk = (a.ntiles + nxcd - 1) / nxcd;
    const int t_begin = label * chunk;
    const int t_end = min(a.ntiles, t_begin + chunk);
    int t = t_begin + slot;
    if (t >= t_end) return;

    {
        const H3Tile c0 = h3_tile<Cfg>(a, t);
        h3_dma<Cfg, false>(a, c0, tin0, tid, wave, pfoff, true);
        __builtin_amdgcn_s_waitcnt(h3_vmcnt(0));               // also retires the weight / scale loads above
        h3_barrier();
    }

#if H3_ABLATE & 32
    unsigned long long stamp_sum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, stamp_prev;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamp_prev)::"memory");
#endif
    int buf = 0;
    H3Tile carry = h3_tile<Cfg>(a, t);
    // tile coordinates advance incrementally: per_label = (sb * tiles_y + sy) * tiles_x + sx, two carries per step
    // (the three integer divisions of h3_tile cost ~350 scalar-dependent cycles per tile on every wave)
    int c_tx = carry.x0 / Cfg::TW, c_ty = carry.y0 / Cfg::TH;
    const int sx = per_label % a.tiles_x, sy = (per_label / a.tiles_x) % a.tiles_y;
    const size_t img_bytes = (size_t)a.H * a.W * 64;
    const size_t sb_bytes = (size_t)(per_label / a.tiles_x / a.tiles_y) * img_bytes;
    for (; t < t_end; t += per_label, buf ^= 1) {
        const H3Tile cur = carry;                                // (a fresh const per iteration: the epilogue structs hold references)
        const int t1 = t + per_label;
        const bool has1 = t1 < t_end;
        char* tin = tin0 + buf * Cfg::TIN_BYTES;
        const bool interior = h3_interior<Cfg>(a, cur);
        H3RLane L = L0;
        asm volatile("" : "+v"(L.p1), "+v"(L.w1), "+v"(L.p2), "+v"(L.rr), "+v"(L.g));
        H3_STAMP(6);                                             // tile index math

        // next tile: global -> the other LDS buffer (last read by the previous tile's conv2 residual, one barrier
        // ago); its PF DMA instructions are issued one per input row inside conv1 and land during conv2
        H3Tile nx = cur;
        if (has1) {
            c_tx += sx;
            const int cx = c_tx >= a.tiles_x;
            c_tx -= cx ? a.tiles_x : 0;
            c_ty += sy + cx;
            const int cy = c_ty >= a.tiles_y;
            c_ty -= cy ? a.tiles_y : 0;
            nx.x0 = c_tx * Cfg::TW;
            nx.y0 = c_ty * Cfg::TH;
            nx.img = cur.img + sb_bytes + (cy ? img_bytes : 0);
        }
        const char* nx_origin = reinterpret_cast<const char*>(a.in) + nx.img + ((ptrdiff_t)(nx.y0 - 2) * a.W + (nx.x0 - 2)) * 16;
        char* tnx = tin0 + (buf ^ 1) * Cfg::TIN_BYTES;
        const bool nx_interior = h3_interior<Cfg>(a, nx);
        H3_STAMP(0);                                             // next-tile index math
        // ---- conv1: input tile -> intermediate tile ------------------------------------------------------
#define H3R_CONV1(RV)                                                                                                       \
        do {                                                                                                               \
            if (nx_interior) {                                                                                             \
                const H3DmaHook<Cfg, true, Plan::NROWS_MIN> hook{a, nx, nx_origin, tnx, tid, wave, pfoff, has1};           \
                if (interior) h3r_conv1_run<Cfg, RV, true>(a, tin, tmid, w1, inv_s1, relu_floor, L, cur, o1, hook);                    \
                else h3r_conv1_run<Cfg, RV, false>(a, tin, tmid, w1, inv_s1, relu_floor, L, cur, o1, hook);                            \
            } else {                                                                                                       \
                const H3DmaHook<Cfg, false, Plan::NROWS_MIN> hook{a, nx, nx_origin, tnx, tid, wave, pfoff, has1};          \
                if (interior) h3r_conv1_run<Cfg, RV, true>(a, tin, tmid, w1, inv_s1, relu_floor, L, cur, o1, hook);                    \
                else h3r_conv1_run<Cfg, RV, false>(a, tin, tmid, w1, inv_s1, relu_floor, L, cur, o1, hook);                            \
            }                                                                                                              \
        } while (0)
        if (big) {
            H3R_CONV1(Plan::R1_BIG);
        } else {
            // strip group FIRST: at the end of conv1 its read -> MFMA -> write chain ran alone (the partner wave on the
            // SIMD was already parked at the barrier) and cost ~1100 cycles, all of it barrier time for the other waves
            // (8 rows x 2 columns per group; its lane addresses are rebuilt here, ~10 VALU, instead of living in VGPRs)
#pragma unroll
            for (int k = 0; k < Plan::SG_PER_WAVE; ++k) {
                const int g = sg + k * Plan::N_SHORT;
                if (g < Cfg::SG) {
                    const int srow = min(8 * g + (n >> 1), Cfg::MH - 1);      // partial last group: clamp (same values twice)
                    const int scol = Cfg::TW + (n & 1);
                    const int bg = (q & 1) * Cfg::IN_PLANE + (srow * Cfg::IW + scol) * 16;
                    const int gw = ((q >> 1) + 2 * (q & 1)) * Cfg::MID_PLANE + (srow * Cfg::MW + scol) * 16;
                    const f32x4 v = bf_acc_ready(h3r_group<Cfg::IW * 16, 2 * Cfg::IN_PLANE>(tin, bg + (q >> 1) * 16, bg + 32 + (q >> 1) * 2 * Cfg::IN_PLANE, w1));
                    if (interior) h3r_conv1_store<Cfg, true>(a, tmid, gw, v, inv_s1, relu_floor, 0, 0);
                    else h3r_conv1_store<Cfg, false>(a, tmid, gw, v, inv_s1, relu_floor, cur.y0 - 1 + srow, cur.x0 - 1 + scol);
                }
            }
            H3R_CONV1(Plan::R1_SMALL);
        }
#undef H3R_CONV1
        H3_STAMP(1);                                             // conv1 (+ DMA issue)
        h3_barrier();                                            // tmid complete
        H3_STAMP(2);                                             // barrier A

        // ---- conv2 + folded BN + residual (from the LDS input tile) -> global ---------------------------
        {
            char* out_row0 = reinterpret_cast<char*>(a.out) + cur.img + ((size_t)cur.y0 * a.W + cur.x0) * 16;
            const size_t rowbytes = (size_t)a.W * 16;
            const size_t lo_g = 2 * (size_t)plane_g;
            struct Epi2 {
                typedef h8 Pre;
                enum { EXTRA_MFMA = 1 };
                const FusedH3Args& a; const char* __restrict__ tin; h8 wres; char* out_row0; size_t rowbytes, lo_g;
                float inv_s2; f32x4 sh; bool interior; int rr, y_base, x_px, lane; unsigned g;
                f32x4 wh0, wh1, wh2, wh3; char* head_row0; int q;
                // residual operand [x_hi | x_lo] of the centre pixel of output row o: requested one row step early
                __device__ __forceinline__ Pre pre(const int o) const { return *reinterpret_cast<const h8*>(tin + rr + o * Cfg::IW * 16); }
                // residual on the matrix pipe: acc += (s2 * I) x [x_hi | x_lo] -- exact (power-of-two times f16 in
                // fp32) and one MFMA + one ds_read_b128 instead of two ds_read_b64 and 12 conversions / additions
                __device__ __forceinline__ f32x4 finish(const int, const f32x4 acc, const Pre& xr) const { return MFMA_H(wres, xr, acc); }
                __device__ __forceinline__ void operator()(const int o, const f32x4 acc) const
                {
                    const f32x4 v = (H3_ABLATE & 64) ? acc : acc * inv_s2 + sh;
                    if constexpr (HEAD) {
                        // the lane's 4 channels times their rows of the head matrix, summed over the 4 lanes of the pixel
                        f32x4 hsum = wh0 * v.x + wh1 * v.y + wh2 * v.z + wh3 * v.w;
                        const bool finite = fabsf(v.x) <= 3.0e38f && fabsf(v.y) <= 3.0e38f && fabsf(v.z) <= 3.0e38f && fabsf(v.w) <= 3.0e38f;
                        if (!finite && a.status) atomicOr(a.status, BF_STATUS_F16_RANGE);      // never on valid activations
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            hsum[k] += __shfl_xor(hsum[k], 16, 64);
                            hsum[k] += __shfl_xor(hsum[k], 32, 64);
                        }
                        // after the reduction the 4 lanes of a pixel hold the same three sums: lane group q writes output
                        // channel q (q = 3: dump line), ONE store per row and wave, every lane with its own tanh
                        const float hk = q == 0 ? hsum[0] : (q == 1 ? hsum[1] : hsum[2]);
                        const bool live = q < 3 && y_base + o < a.Ho && x_px < a.Wo;
                        // tanh(2h) = 1 - 2 / (exp(4h) + 1): a handful of instructions inside the matrix loop (libm tanhf: ~30)
                        float r = (1.0f - 2.0f / (__expf(4.0f * hk) + 1.0f)) * 0.51f;
                        if (a.denormalize) r = (fminf(fmaxf(r, -0.5f), 0.5f) + 0.5f) * (a.v_max - a.v_min) + a.v_min;
                        if (a.head_u8) {
                            unsigned char* p = live ? reinterpret_cast<unsigned char*>(head_row0) + (size_t)o * a.Wo * 3 + q
                                                    : reinterpret_cast<unsigned char*>(a.dump) + lane * 16;
                            *p = (unsigned char)fminf(fmaxf(rintf(r), 0.f), 255.f);              // rintf = round-half-even
                        } else {
                            float* p = live ? reinterpret_cast<float*>(head_row0) + (size_t)o * a.Wo * 3 + q
                                            : reinterpret_cast<float*>(a.dump) + lane * 4;
                            *p = r;
                        }
                        return;
                    }
                    const h8 rec = h3_split_record(v);
                    // out-of-image lanes store to a dump line: every wave issues exactly R2 stores per tile
                    char* p = out_row0 + o * rowbytes + g;
                    if (!(y_base + o < a.H && x_px < a.W))   /* branch-free on purpose: see h3_split_record's neighbour comment */ p = reinterpret_cast<char*>(a.dump) + lane * 16;
                    if (H3_ABLATE & 2) { if (v.x == 12345.678f) *reinterpret_cast<h8*>(p) = rec; }   // keeps the work live
                    else *reinterpret_cast<h8*>(p) = rec;
                }
            };
            char* head_row0 = nullptr;
            if constexpr (HEAD) {
                const size_t bimg = cur.img / img_bytes;             // image index (once per tile)
                head_row0 = reinterpret_cast<char*>(a.head_out) +
                            ((bimg * a.Ho + (size_t)(cur.y0 + o2)) * a.Wo + (size_t)(cur.x0 + L.px)) * 3 * (a.head_u8 ? 1 : 4);
            }
            const Epi2 epi2{a, tin, w2[12], out_row0, rowbytes, lo_g, inv_s2, sh, interior, L.rr, cur.y0 + o2, cur.x0 + L.px, lane, L.g,
                            whr[0], whr[1], whr[2], whr[3], head_row0, q};
            h3r_rows<Plan::R2, Cfg::MW * 16, 2 * Cfg::MID_PLANE>(tmid, L.p2, L.s2, w2, epi2, H3NoHook{});
        }
        // next tile's DMA landed <=> at most the R2 stores above are outstanding: they are the only vector-memory operations
        // younger than it on this wave.  The loop holds no ordinary global LOAD on purpose: hipcc waits vmcnt(0) for any load
        // that is pending together with LDS-DMA (measured: tools/exp/dma_waitcnt.hip), which would drain the DMA here
        H3_STAMP(3);                                             // conv2 + stores
        __builtin_amdgcn_s_waitcnt(h3_vmcnt((H3_ABLATE & 2) ? 0 : Plan::R2));      // HEAD: also one store per row
        H3_STAMP(4);                                             // wait for the next tile's DMA
        h3_barrier();
        H3_STAMP(5);                                             // barrier B
        carry = nx;                                              // tile coordinates are computed once per tile
    }
#if H3_ABLATE & 32
    if (a.dbg && lane == 0) {
        for (int k = 0; k < 8; ++k) a.dbg[((size_t)blockIdx.x * Cfg::NW + wave) * 8 + k] = stamp_sum[k];
    }
#endif
}

using H3Default = H3Cfg<16, 32, 8>;
using H3Small = H3Cfg<16, 16, 4>;

// Default kernel (variant < 0 everywhere): the full-row streaming kernel (4, fused_h3v.hip) for images up to 256 columns when
// the batch holds enough rows to amortise a band's ~10-step fill (B * H >= 3072: from ~12 rows per workgroup on; measured at
// 256 x 256: batch 8 0.46 ms (tiles) vs 0.49, batch 16 0.78 vs 0.75, batch 128 5.5 vs 4.5), the row-streaming tile kernel (1, or
// 2 for very small inputs) otherwise -- a single 256 x 256 image takes 162 us through the 18 blocks on tiles, 367 us on one-row bands.
static int g_h3_variant = -1;                         // override of the default for debug entries without a handle (tests, A/B)
void bf_set_h3_variant(int v) { g_h3_variant = v < 0 ? -1 : v; }
// Below one 16 x 32 tile per CU (or between one and two) the 16 x 16 tiles of variant 2 -- two 4-wave workgroups per CU -- put more of
// the chip to work: resnet 1x18 on one 256 x 256 image 149 us for 177, one 128 x 128 image 138 for 166, three 256 x 256 images 241 for
// 267; from 512 tiles on the larger tile is 3-5 % faster (tools/exp/small_batch_variants.py).
static int h3_default_variant(const H3Request& a)
{
    // (short AND narrow images -- under 24 rows, up to 128 columns -- stay on tiles: 2 000 x 4 x 64 1 186 us on tiles, 1 559 streaming)
    if (!a.head && bf_fused_block_h3v_supports(a.H, a.W) && (int64_t)a.B * a.H >= 3072 && (a.H >= 24 || a.W > 128)) return 4;
    const int64_t tiles32 = (int64_t)a.B * ((a.H + 15) / 16) * ((a.W + 31) / 32);
    return (!a.head && !a.compact && tiles32 < 512 && tiles32 != 256) ? 2 : 1;
}

// The one selection rule.  The value asked for is the call's own (a.variant), else the process-wide override, else the default
// for the shape; bit 8 of it (tests: the bottom-up walk of the full-row streaming kernel) is not part of the choice.  4 is the
// full-row streaming kernel where it applies (images up to 256 columns, no head epilogue), 2 the tile kernel on 16 x 16 tiles, and
// EVERY other value -- 1, the numbers of retired kernels (0, 3), anything unknown -- the tile kernel on 16 x 32 tiles.
H3Choice bf_select_fused_block_h3(const H3Request& a)
{
    const int requested = a.variant >= 0 ? a.variant : (g_h3_variant >= 0 ? g_h3_variant : h3_default_variant(a));
    const int variant = requested & 255;
    H3Choice c;
    c.bottom_up = (requested & 256) != 0;
    if (variant == 4 && !a.head && bf_fused_block_h3v_supports(a.H, a.W)) c.kernel = H3Kernel::FullRow;
    else c.kernel = variant == 2 ? H3Kernel::Tiles16 : H3Kernel::Tiles32;
    return c;
}

template <class Cfg>
static hipError_t launch_h3(void (*kernel)(FusedH3Args), FusedH3Args a, hipStream_t s)
{
    a.tiles_x = (a.W + Cfg::TW - 1) / Cfg::TW;
    a.tiles_y = (a.H + Cfg::TH - 1) / Cfg::TH;
    a.ntiles = a.B * a.tiles_x * a.tiles_y;
    {
        const hipError_t ea = bf_set_max_lds(reinterpret_cast<const void*>(kernel), Cfg::LDS_BYTES);      // once per device
        if (ea != hipSuccess) return ea;
    }
    const int resident = 256 * Cfg::WG_PER_CU;                  // persistent: every workgroup resident at once
    int grid = a.ntiles < resident ? a.ntiles : resident;
    if (grid >= 8) grid -= grid % 8;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(Cfg::NT), Cfg::LDS_BYTES, s, a);
    return hipGetLastError();
}

// Two blocks per launch (fused_h3w.hip) beyond the shapes of the one-block streaming kernel: its 128-column strips take any image width,
// and at two blocks per launch a band's fill is amortised earlier -- with the library's default selection, from 4 096 rows of strips per
// forward on (B * H * ceil(W / 128)) consecutive blocks run two per launch; an odd block count runs its single block on whatever
// bf_select_fused_block_h3 picks.  Measured (tools/exp/regime_sweep.py, resnet 1x18, us per forward, pairs / 16 x 32 tiles):
// 8 x 256^2 403 / 429, 6 x 256^2 357 / 355, 2 x 512^2 404 / 424, 1 x 512^2 295 / 282, 32 x 128^2 397 / 420, 16 x 128^2 291 / 281,
// 32 x 512^2 4 300 / 5 570, 1 x 1080 x 1920 2 207 / 2 747.
// Images of fewer than 24 rows are the exception (a band's 12-step fill per handful of rows): 512 x 8 x 256 runs 830 us on the one-block
// streaming kernel, 899 in pairs; 300 x 20 x 100 867 on tiles, 969 in pairs -- they keep the one-block selection of h3_default_variant.
// A variant forced through set_option / bf_debug_set_h3_variant pairs exactly where it selects the streaming kernel (tests, A/B).
bool bf_fused_block_h3_use_pairs(const H3Request& a)
{
    if (a.head || a.compact) return false;
    if (a.variant >= 0 || g_h3_variant >= 0) return bf_select_fused_block_h3(a).kernel == H3Kernel::FullRow;
    const int64_t nstrips = (a.W + 127) / 128;
    return a.W >= 1 && a.H >= 24 && (int64_t)a.B * a.H * nstrips >= 4096;
}

const char* bf_fused_block_h3_kernel_name(H3Kernel k)
{
    return k == H3Kernel::FullRow ? "fused_block_h3v_kernel" : "fused_block_h3r_kernel";
}

// launches the kernel the caller chose (bf_select_fused_block_h3 with the arguments of THIS launch): nothing is chosen here
hipError_t bf_launch_fused_block_h3_as(const FusedH3Args& args, H3Kernel k, hipStream_t s)
{
    FusedH3Args a = args;
    if (!a.zeros || !a.dump) return hipErrorInvalidValue;
    if ((int64_t)a.H * a.W * 64 >= ((int64_t)1 << 32)) return hipErrorInvalidValue;      // 32-bit in-image offsets
    if (k == H3Kernel::FullRow) return bf_launch_fused_block_h3v(a, s);
    if (a.compact) return hipErrorInvalidValue;                 // only the streaming kernel reads the compact layout
    if (k == H3Kernel::Tiles16) return launch_h3<H3Small>(fused_block_h3r_kernel<H3Small>, a, s);   // two 4-wave workgroups per CU
    if (a.head_wh) return launch_h3<H3Default>(fused_block_h3r_kernel<H3Default, 1>, a, s);
    return launch_h3<H3Default>(fused_block_h3r_kernel<H3Default>, a, s);
}

// handle-less callers (debug entries): select, then launch that
hipError_t bf_launch_fused_block_h3(const FusedH3Args& args, hipStream_t s)
{
    FusedH3Args a = args;
    const H3Choice c = bf_select_fused_block_h3({a.B, a.H, a.W, a.variant, a.head_wh != nullptr, a.compact != 0});
    if (c.bottom_up) a.reverse_tiles = 1;                       // tests: the bottom-up walk of the full-row streaming kernel
    return bf_launch_fused_block_h3_as(a, c.kernel, s);
}

// ------------------------------------------------------------------------------------------
// fp32 NHWC [B,H,W,16]  <->  split-planar [B][4][H][W][8 x f16]   (tests, debug entry points)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void h3_from_f32_kernel(const float* __restrict__ x, char* __restrict__ y, int64_t npix, int64_t hw)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix * 2; i += (int64_t)gridDim.x * 256) {
        const int64_t pix = i >> 1;
        const int half = (int)(i & 1);
        const int64_t b = pix / hw, p = pix - b * hw;
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(x + pix * 16 + half * 8);
        const f32x4 v1 = *reinterpret_cast<const f32x4*>(x + pix * 16 + half * 8 + 4);
        h4 h0, l0, h1, l1;
        h3_split(v0, h0, l0);
        h3_split(v1, h1, l1);
        char* base = y + b * hw * 64 + p * 16;
        h8 hi = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
        h8 lo = {l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
        *reinterpret_cast<h8*>(base + (int64_t)half * hw * 16) = hi;
        *reinterpret_cast<h8*>(base + (int64_t)(2 + half) * hw * 16) = lo;
    }
}

__global__ __launch_bounds__(256) void h3_to_f32_kernel(const char* __restrict__ y, float* __restrict__ x, int64_t npix, int64_t hw)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix * 2; i += (int64_t)gridDim.x * 256) {
        const int64_t pix = i >> 1;
        const int half = (int)(i & 1);
        const int64_t b = pix / hw, p = pix - b * hw;
        const char* base = y + b * hw * 64 + p * 16;
        const h8 hi = *reinterpret_cast<const h8*>(base + (int64_t)half * hw * 16);
        const h8 lo = *reinterpret_cast<const h8*>(base + (int64_t)(2 + half) * hw * 16);
        float* o = x + pix * 16 + half * 8;
#pragma unroll
        for (int c = 0; c < 8; ++c) o[c] = (float)hi[c] + (float)lo[c];
    }
}

hipError_t bf_launch_h3_from_f32(const float* x, void* y, int B, int H, int W, hipStream_t s)
{
    const int64_t npix = (int64_t)B * H * W;
    const int64_t g = (npix * 2 + 255) / 256;
    hipLaunchKernelGGL(h3_from_f32_kernel, dim3((unsigned)(g < 16384 ? g : 16384)), dim3(256), 0, s, x, (char*)y, npix, (int64_t)H * W);
    return hipGetLastError();
}

hipError_t bf_launch_h3_to_f32(const void* y, float* x, int B, int H, int W, hipStream_t s)
{
    const int64_t npix = (int64_t)B * H * W;
    const int64_t g = (npix * 2 + 255) / 256;
    hipLaunchKernelGGL(h3_to_f32_kernel, dim3((unsigned)(g < 16384 ? g : 16384)), dim3(256), 0, s, (const char*)y, x, npix, (int64_t)H * W);
    return hipGetLastError();
}
