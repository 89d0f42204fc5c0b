// TWO fused residual blocks per launch, split-f16 arithmetic, row streaming on 128-column STRIPS (fused_block2_h3w_kernel).
//
// Reference semantics (bfcnn/backbone_blocks.py:167-246, the loop over the blocks of a resnet level, with the inference
// BatchNormalization folded), two iterations of it per launch:
//     x1 = x0 + scale_a * conv2a(act(conv1a x0)) + shift_a ;   x2 = x1 + scale_b * conv2b(act(conv1b x1)) + shift_b
// Same arithmetic, weight images (pack_h3_kernel's row-streaming images) and split-planar activation layout as
// fused_block_h3v_kernel (fused_h3v.hip); x1 and both intermediate activations only ever exist in LDS, so a pair of blocks
// moves 128 B per pixel through HBM where two launches of the one-block kernel move 256.
//
// The one-block kernel keeps whole 256-column rows in its rings (16.5 KB per ring row) and has no room for a second block.
// Here a workgroup owns a STRIP of 128 output columns and walks down a band of rows, one image row per step, through a
// chain of four convolutions.  Every convolution works on the same GRID of 144 columns = nine 16-pixel MFMA groups that
// contains the strip plus its halo (x0 needs 4 columns beyond the strip on an interior side, the first intermediate 3, x1 2,
// the second intermediate 1); at an image edge the grid starts / ends ON the edge, so a 256-column image is two strips with
// grids [0, 144) and [112, 256): 9 groups per row and convolution where 8 are output (12.5 % more matrix work, 6 % more
// input bytes).  Columns of the grid that no output depends on hold finite garbage.
//
//   * 12 waves = 4 roles x 3 waves, three matrix waves per SIMD; wave k of a role owns grid columns [48k, 48k+48) = three MFMA
//     groups and holds ONE kernel's weights (52 VGPRs).  A1 = conv1a, B1 = conv2a (+ residual x0, folded BN) -> x1 ring,
//     A2 = conv1b, B2 = conv2b (+ residual x1) -> global memory (H3W_DIRECT_STORE; a launch with the head, or a build with the
//     constant 0: -> staging rows);
//   * the memory instructions ride on matrix waves: the A2 waves request x0 row s+3 by LDS-DMA (four 1-KiB pieces each),
//     the B2 waves store their own records of the output row, 8 bytes per lane, six wave-instructions per wave and step (loads
//     and stores on DIFFERENT waves: `s_waitcnt vmcnt(N)` counts both and stores retire early, see fused_h3v.hip; with the
//     staging rows the A1 waves store, 16 bytes per lane);
//   * LDS rings (ring column = grid column + 1; ring columns 0 and 145 are never written: the zero padding at an image
//     edge): x0 5 rows, first intermediate 2, x1 3, second intermediate 2 -> 112 KiB; + 2 staging rows where they exist -> 130 KiB;
//   * step s, band-relative rows (x0 row k is consumed at step k+4): A1 turns x0 row s-4 into its three vertical-tap
//     contributions and completes intermediate row s-5; B1 consumes intermediate row s-6 and completes x1 row s-7 (its
//     accumulator starts as the residual (s2 I) x [x_hi | x_lo] on top of the folded shift); A2 consumes x1 row s-8 ->
//     second intermediate row s-9; B2 consumes it in step s+1 and completes AND stores output row s-11 in step s (staged: the
//     storer stores it in s+1).  ONE barrier per step, nrows + 12 steps per band;
//   * inside a step (H3W_EPI_ORDER 2) a wave takes its three groups one after the other, and each group accumulator by accumulator: the
//     five MFMAs of the row it COMPLETES first (a2), then the five of the row above (a1), then [the residual and] the five of the row it
//     starts (c0).  The completed row's epilogue -- 10 or 14 one-instruction micro-ops, the last two its LDS writes or global stores -- rides
//     two by two behind MFMA 7, 8, ... of the SAME group, so the last MFMA of a step is followed by the barrier alone and the group-0
//     shadows are used.  Every accumulator still receives its own five (six) MFMAs in the order it always did: same bits;
//   * rows and columns outside the image are forced to zero in every ring (they are the NEXT convolution's zero padding,
//     not values computed from padded input);
//   * the FIRST launch of a forward on uint8 images (FusedH3WArgs::base_u8, template parameter BASE) has no loader: it computes
//     its x0 rows itself, the base convolution of base_rows.hip bit for bit, from uint8 rows (H3WProducer below) -- no base
//     kernel, and x0 is neither written to nor read from global memory.
#include "h3v_core.h"
#include "h3_bands.h"
#include "base_rows.h"

// wave priorities (s_setprio) per role; H3W_PRIO_SET picks a preset for A/B builds: 1 = younger roles higher (0,1,2,3),
// 2 = older roles higher (3,2,1,0), 3 = second convolutions high (0,2,0,2), 4 = first convolutions high (2,0,2,0)
#ifndef H3W_PRIO_SET
#define H3W_PRIO_SET 0
#endif
#if H3W_PRIO_SET == 1
#define H3W_PRIO_A1 0
#define H3W_PRIO_B1 1
#define H3W_PRIO_A2 2
#define H3W_PRIO_B2 3
#elif H3W_PRIO_SET == 2
#define H3W_PRIO_A1 3
#define H3W_PRIO_B1 2
#define H3W_PRIO_A2 1
#define H3W_PRIO_B2 0
#elif H3W_PRIO_SET == 3
#define H3W_PRIO_A1 0
#define H3W_PRIO_B1 2
#define H3W_PRIO_A2 0
#define H3W_PRIO_B2 2
#elif H3W_PRIO_SET == 4
#define H3W_PRIO_A1 2
#define H3W_PRIO_B1 0
#define H3W_PRIO_A2 2
#define H3W_PRIO_B2 0
#endif
#ifndef H3W_PRIO_A1
#define H3W_PRIO_A1 1
#endif
#ifndef H3W_PRIO_B1
#define H3W_PRIO_B1 1
#endif
#ifndef H3W_PRIO_A2
#define H3W_PRIO_A2 1
#endif
#ifndef H3W_PRIO_B2
#define H3W_PRIO_B2 1
#endif

// unit order: 1 = XCD-contiguous (h3_bands.h): the two strips of an image run on ONE XCD and the 16 columns both read come out of
// its L2 (FETCH per launch 571 -> 538 MB for 537 MB algorithmic; the same-box A/B within its noise); 0 = launch order (A/B)
#ifndef H3W_XCD_ORDER
#define H3W_XCD_ORDER 1
#endif

// where a finished output row leaves the workgroup (a launch with the head, H3WMem<3>, always stages: its storer reads whole pixels):
// 0 = B2 writes it to the staging rows and the A1 waves read it back one step later and store it (16-byte records);
// 1 = B2 stores its own 8-byte half-records from registers, in the MFMA shadows where the two ds_write_b64 of a group sat: no staging
//     rows, no storer hook, 17 KB less LDS traffic per row step (same-box A/B: DESIGN 4.1c, profiles/r07_direct_store_ab.txt)
#ifndef H3W_DIRECT_STORE
#define H3W_DIRECT_STORE 1
#endif

// order of a group's MFMAs and place of the epilogues inside a role's step (every accumulator receives its own MFMAs in the same order under
// every value, so the results are the same bits):
// 0 = taps interleaved (a2, a1, c0 per tap); a group's epilogue rides behind MFMA 2, 3, ... of the NEXT group, the last group's runs behind the
//     step's last MFMA, in front of the barrier, in nobody's shadow;
// 1 = the LAST group of a step multiplies accumulator by accumulator (a2 x 5, a1 x 5, [residual,] c0 x 5): the row it completes is final after
//     its fifth MFMA and its own epilogue rides behind MFMA 7, 8, ... of the same group, the previous group's behind MFMA 0 .. 6;
// 2 = every group in that order with its own epilogue behind its own MFMA 7, 8, ...: no hand-over between groups, group 0's shadows are used
// Same-box A/B (profiles/r08_pair_schedule_ab.txt): 2 +4.2 % images/s, 1 +2.1 %.
#ifndef H3W_EPI_ORDER
#define H3W_EPI_ORDER 2
#endif
// operands of step s+1 that are final a step earlier are read in step s, in front of the barrier:
// 0 = every operand is read behind the barrier that starts its step;
// 1 = the B roles read the residual operand of group 0 of step s+1 during the last group of step s (B1: x0 ring row s, which A1 consumes in
//     step s; B2: the x1 row B1 completed in step s-1) and carry it across the barrier, so their first MFMA waits for no LDS read;
// 2 = 1 + every role reads its group-1 fragment behind its first MFMA instead of in front of it: the twelve waves' group-0 reads are served first
// Neither paid: alone inside the parent's spread, with H3W_EPI_ORDER 2 (where the residual is the eleventh MFMA of a group) -0.4 / -0.6 %.
// A1's own fragment cannot be read early: its x0 row is final only at the barrier in front of its step, in the loader launch too (H3WMem<1>::end).
#ifndef H3W_PREFETCH
#define H3W_PREFETCH 0
#endif
static_assert(H3W_EPI_ORDER >= 0 && H3W_EPI_ORDER <= 2 && H3W_PREFETCH >= 0 && H3W_PREFETCH <= 2, "schedule constants");

struct H3WGeom {
    static constexpr int NG = 9, GW = 16 * NG;         // grid: nine 16-column groups
    static constexpr int G = 3;                        // groups per matrix wave
    static constexpr int NR = 3, NW = 12, NT = 768;    // waves per role, per workgroup, threads
    static constexpr int SW = 128;                     // output columns of a strip
    static constexpr int PITCH = (GW + 2) * 16;        // bytes per plane-row of a ring; ring column = grid column + 1
    static constexpr int NRX0 = 5, NRM = 2, NRX1 = 3, NRO = 2;      // ring depths (rows)
    static constexpr int PD = 3;                       // DMA distance: x0 row s+3 is requested in step s, awaited at the end of step s+1
    static constexpr int UNROLL = 6;                   // steps per loop iteration: slots mod 2 / mod 3 and the accumulator rotation static
    static constexpr int X0_PLANE = (NRX0 * PITCH + 255) / 256 * 256, M_PLANE = (NRM * PITCH + 255) / 256 * 256;
    static constexpr int X1_PLANE = (NRX1 * PITCH + 255) / 256 * 256;
    static constexpr int OUT_PLANE = GW * 16, OUT_SLOT = 4 * OUT_PLANE;       // staging rows are indexed by GRID column too
    static constexpr int X0_OFF = 0, M1_OFF = X0_OFF + 4 * X0_PLANE, X1_OFF = M1_OFF + 4 * M_PLANE, M2_OFF = X1_OFF + 4 * X1_PLANE;
    // the staging rows exist where a storer reads them back: in every launch of an H3W_DIRECT_STORE 0 build, else in the head launch
    // alone (LDS_BYTES_STAGED); the other launches end at the rings (112 KiB) and the producer's tables follow there
    static constexpr int OUT_OFF = M2_OFF + 4 * M_PLANE, LDS_BYTES_STAGED = OUT_OFF + NRO * OUT_SLOT;
    static constexpr int LDS_BYTES = H3W_DIRECT_STORE ? OUT_OFF : LDS_BYTES_STAGED;
    // producer launch only (H3WProducer, behind the rings): the [r, g, b, 1_inside] records of four input rows, each row twice
    // (the second copy shifted by one pixel, as in base_rows.hip), the base convolution's A operands + 1 / s, reduction scratch
    static constexpr int BIN_RING = 4, BIN_ROWPX = GW + 4;       // ring pixel j = image column G0 - 1 + j; j <= GW + 1 are written
    static constexpr int BIN_SLOT = 2 * BIN_ROWPX * 8;
    static constexpr int BIN_OFF = LDS_BYTES, BWA_OFF = BIN_OFF + BIN_RING * BIN_SLOT, BINVS_OFF = BWA_OFF + 3 * 64 * 16;
    static constexpr int BRED_OFF = BINVS_OFF + 16, LDS_BYTES_BASE = BRED_OFF + NT * 4;
    static_assert(LDS_BYTES_BASE <= 160 * 1024 && BIN_OFF % 16 == 0 && BIN_SLOT % 16 == 0 && LDS_BYTES_BASE % 16 == 0, "LDS (producer)");
    static constexpr int LEAD = 12;                    // steps from the first x0 row of a band to the store of its first output row
    static constexpr int NSTAMP = 4;
    static_assert(UNROLL % NRM == 0 && UNROLL % NRO == 0 && UNROLL % NRX1 == 0 && UNROLL % 3 == 0, "static slots");
    static_assert(NRX0 == PD + 2, "x0 ring: rows s-1 (residual), s (conv1a), s+1 (landed), s+2, s+3 (in flight)");
    static_assert(LDS_BYTES_STAGED <= 160 * 1024 && LDS_BYTES <= LDS_BYTES_STAGED && LDS_BYTES % 16 == 0 && LDS_BYTES_STAGED % 16 == 0, "LDS");
    static_assert(3 * X0_PLANE + NRX0 * PITCH < 65536, "fragment offsets fit the 16-bit ds offset");
};

// H3W_EPI_ORDER: the groups of a wave that multiply accumulator by accumulator, and the MFMA of such a group behind which the first micro-ops
// of its own epilogue ride.  The accumulator they read was finished by MFMA 4: three MFMAs lie in between, one more than the rule above H3VEpi asks for
constexpr bool h3w_grouped(const int g) { return H3W_EPI_ORDER == 2 || (H3W_EPI_ORDER == 1 && g == H3WGeom::G - 1); }
constexpr int H3W_OWN_SLOT = 7;

struct H3WTile : BandUnit {    // a band of one strip (h3_bands.h) + the strip's columns
    int X0, X1;                  // output columns [X0, X1)
    int G0;                      // image column of grid column 0
    int D0, D1;                  // x0 columns fetched: [D0, D1), inside the grid and the image
};

__device__ __forceinline__ H3WTile h3w_tile(const FusedH3WArgs& a, const int t)
{
    H3WTile r{bf_band_unit<H3W_XCD_ORDER != 0>(a, t)};
    r.X0 = r.sx * H3WGeom::SW;
    r.X1 = min(a.W, r.X0 + H3WGeom::SW);
    r.G0 = min(max(r.X0 - 8, 0), max(a.W - H3WGeom::GW, 0));
    r.D0 = max(0, (r.X0 - 4) & ~7);
    r.D1 = min(a.W, (r.X1 + 4 + 7) & ~7);
    return r;
}

// ---------------------------------------------------------------------------------------------------------------------
// role A: a block's first convolution (+ activation): ring row -> three vertical-tap contributions -> intermediate ring.
// State across steps: acc[g][3] (intermediate rows of steps s, s-1, s-2 modulo 3).
// ---------------------------------------------------------------------------------------------------------------------
template <int INP>                 // plane stride of the input ring
struct H3WRoleA {
    using Gm = H3WGeom;
    const char* tin;
    char* tmid;
    h8 w[13];
    f32x4 acc[Gm::G][3];
    int rp, rs;                  // lane's LDS byte offset in ring slot 0, group 0: pair fragment (hi planes), single fragment
    int wr;                      // lane's LDS byte offset of its 8-byte hi record in mid ring slot 0, group 0 (lo: + 2 planes)
    float inv_s, relu_floor;
    float lane_scale[Gm::G];     // inv_s where the lane's column is inside the image, else 0
    bool skip_last = false;      // timing experiment (H3V_ABLATE & 256): the role's third wave multiplies two groups only

    __device__ __forceinline__ void init(const void* wimg, const FusedH3WArgs& a, const float* aux, const int lane, const int gc0)
    {
        const int q = lane >> 4;
#pragma unroll
        for (int i = 0; i < 13; ++i) w[i] = reinterpret_cast<const h8*>(wimg)[bf_band_wimage(a, i) * 64 + lane];
        inv_s = aux[0];
        relu_floor = a.act1_relu ? 0.f : -__builtin_inff();
        // taps dx = 0, 1 of grid column c are ring columns c, c + 1 (ring column = grid column + 1, centre tap dx = 1)
        rp = (q & 1) * INP + (gc0 + (q >> 1)) * 16;
        rs = ((q & 1) + 2 * (q >> 1)) * INP + (gc0 + 2) * 16;
        wr = (q >> 1) * Gm::M_PLANE + (gc0 + 1) * 16 + (q & 1) * 8;          // channels 4q .. 4q+3: plane q>>1, half-record q&1
#pragma unroll
        for (int g = 0; g < Gm::G; ++g)
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[g][k] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    __device__ __forceinline__ void set_tile(const H3WTile& t, const int W, const int gc0)
    {
#pragma unroll
        for (int g = 0; g < Gm::G; ++g) lane_scale[g] = (t.G0 + gc0 + 16 * g < W) ? inv_s : 0.f;
    }

    __device__ __forceinline__ H3VFrag load(const int islot_bytes, const int g) const
    {
        H3VFrag f;
        const char* p = tin + rp + islot_bytes;
        f.ph = *reinterpret_cast<const h8*>(p + g * 256);
        f.pl = *reinterpret_cast<const h8*>(p + g * 256 + 2 * INP);
        f.s = *reinterpret_cast<const h8*>(tin + rs + islot_bytes + g * 256);
        return f;
    }

    __device__ __forceinline__ H3VEpi<true> epilogue(const int g, const int mslot, const f32x4 v, const bool rowok) const
    {
        H3VEpi<true> e;
        e.v = v;
        e.sc = rowok ? lane_scale[g] : 0.f;              // rows / columns outside the image are the next convolution's zero padding
        e.floor_ = relu_floor;
        e.p = tmid + wr + mslot * Gm::PITCH + g * 256;
        e.lo_off = 2 * Gm::M_PLANE;
        return e;
    }

    // MFMAs [J, JEND) of the 15 of group g.  !GROUPED: the taps interleaved, micro-ops of the previous group's epilogue (prev) after MFMA 2,
    // 3, ...  GROUPED: a2 x 5, a1 x 5, c0 x 5; prev's micro-ops after MFMA 0 .. 6, and after MFMA H3W_OWN_SLOT (three MFMAs behind the one
    // that finished acc[g][a2]), ... those of the group's own epilogue, which is built there into *own
    template <int J, int JEND, bool GROUPED, class Epi>
    __device__ __forceinline__ void mfmas(const int g, const int a1, const int a2, const H3VFrag& cur, f32x4& c0, Epi* prev, Epi* own,
                                          const int mslot, const bool rowok)
    {
        if constexpr (J < JEND) {
            constexpr int k = GROUPED ? J % 5 : J / 3, which = GROUPED ? J / 5 : J % 3;
            if (!(H3V_ABLATE & 8) && !(skip_last && g == Gm::G - 1)) {
                if constexpr (which == 0) acc[g][a2] = h3v_mfma(cur, w, 2, k, acc[g][a2]);
                else if constexpr (which == 1) acc[g][a1] = h3v_mfma(cur, w, 1, k, acc[g][a1]);
                else c0 = h3v_mfma(cur, w, 0, k, c0);
            } else if (J == 0) {
                acc[g][a2][0] += (float)cur.ph[0] + (float)cur.pl[1] + (float)cur.s[2];
            }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (!GROUPED) {
                if constexpr (J >= 2) {
                    if (prev) prev->template pair<J - 2>();
                }
            } else if constexpr (J < H3W_OWN_SLOT) {
                if (prev) prev->template pair<J>();
            } else {
                if constexpr (J == H3W_OWN_SLOT) *own = epilogue(g, mslot, acc[g][a2], rowok);
                own->template pair<J - H3W_OWN_SLOT>();
            }
            mfmas<J + 1, JEND, GROUPED>(g, a1, a2, cur, c0, prev, own, mslot, rowok);
        }
    }

    // group g of step s: the loop body of step() as a template, so that the order of a group is a constant of its instantiation
    template <int PH, int g, class Hook>
    __device__ __forceinline__ void group(H3VFrag& cur, const int islot_bytes, const bool rowok, Hook& hook)
    {
        constexpr int a0 = PH % 3, a1 = (PH + 2) % 3, a2 = (PH + 1) % 3;      // accumulators of intermediate rows s, s-1, s-2
        constexpr int mslot = PH % Gm::NRM;
        constexpr bool grouped = h3w_grouped(g);
        constexpr bool late_nx = H3W_PREFETCH == 2 && g == 0;        // the group-1 fragment is read behind the step's first MFMA
        using Epi = H3VEpi<true>;
        H3VFrag nx;
        Epi own;
        if constexpr (g + 1 < Gm::G && !late_nx) nx = load(islot_bytes, g + 1);
        __builtin_amdgcn_sched_barrier(0);
        f32x4 c0 = {0.f, 0.f, 0.f, 0.f};
        if constexpr (g > 0 && H3W_EPI_ORDER != 2) {
            Epi e = epilogue(g - 1, mslot, acc[g - 1][a2], rowok);
            mfmas<0, 15, grouped>(g, a1, a2, cur, c0, &e, &own, mslot, rowok);
        } else {
            mfmas<0, 1, grouped>(g, a1, a2, cur, c0, (Epi*)nullptr, &own, mslot, rowok);
            if constexpr (late_nx) {
                nx = load(islot_bytes, 1);
                __builtin_amdgcn_sched_barrier(0);
            }
            mfmas<1, 15, grouped>(g, a1, a2, cur, c0, (Epi*)nullptr, &own, mslot, rowok);
        }
        if constexpr (g == 0) {
            hook.after_first_group();
            __builtin_amdgcn_sched_barrier(0);
        }
        acc[g][a0] = c0;
        if constexpr (g + 1 < Gm::G) cur = nx;
    }

    // step s (s % UNROLL == PH): consumes the ring row at byte offset islot_bytes, completes the intermediate row of slot PH % 2
    template <int PH, class Hook>
    __device__ __forceinline__ void step(const int islot_bytes, const bool rowok, Hook& hook)
    {
        static_assert(Gm::G == 3, "three groups per wave");
        H3VFrag cur = load(islot_bytes, 0);
        group<PH, 0>(cur, islot_bytes, rowok, hook);
        group<PH, 1>(cur, islot_bytes, rowok, hook);
        group<PH, 2>(cur, islot_bytes, rowok, hook);
        if constexpr (!h3w_grouped(Gm::G - 1)) {
            H3VEpi<true> e = epilogue(Gm::G - 1, PH % Gm::NRM, bf_acc_ready(acc[Gm::G - 1][(PH + 1) % 3]), rowok);
            e.all();
        }
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// role B: a block's second convolution + folded BN + residual.  B1 writes the x1 ring, B2 the staging rows.
// ---------------------------------------------------------------------------------------------------------------------
// The epilogue of a role that stores its output row itself (B2 under H3W_DIRECT_STORE): micro-ops 0 .. 7 of H3VEpi<false>, then the lane's
// two 8-byte records (hi, lo) go to global memory where micro-ops 8 and 9 wrote them to LDS -- as the fifth pair of the epilogue, wherever
// H3W_EPI_ORDER places it (2: behind MFMA 11 of the group's own sixteen; 0: behind the sixth MFMA of the next group, the last group's at
// the end of the step).  mask: the lanes that store -- the row is one of the band's (else 0) and the lane's column one
// of the strip's; a wave-uniform lane mask, so the guard is one scalar instruction on the execution mask and no vector one.
struct H3WEpiStore : H3VEpi<false> {
    char* image;
    unsigned image_bytes, off;   // off: the lane's byte offset inside the image's first row (plane, column, half-record)
    size_t row_hi, row_lo;       // wave-uniform byte offsets of the row in the lane's hi plane pair and in its lo pair (+ 2 planes)
    unsigned long long mask;
    __device__ __forceinline__ void store()
    {
        if (__builtin_amdgcn_inverse_ballot_w64(mask)) {
            h3_stream_store8(image, image_bytes, row_hi, off, (H3V_ABLATE & 64) ? (h3v_u2){__builtin_bit_cast(unsigned, v.x), __builtin_bit_cast(unsigned, v.y)} : (h3v_u2){h0, h1});
            h3_stream_store8(image, image_bytes, row_lo, off, (H3V_ABLATE & 64) ? (h3v_u2){__builtin_bit_cast(unsigned, v.z), __builtin_bit_cast(unsigned, v.w)} : (h3v_u2){l0, l1});
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    template <int SLOT> __device__ __forceinline__ void pair()
    {
        if constexpr (SLOT < 4) H3VEpi<false>::template pair<SLOT>();
        else if constexpr (SLOT == 4) store();
    }
    __device__ __forceinline__ void all()
    {
        pair<0>(); pair<1>(); pair<2>(); pair<3>(); pair<4>();
    }
};
template <bool DIRECT> struct H3WEpiOf { using type = H3VEpi<false>; };
template <> struct H3WEpiOf<true> { using type = H3WEpiStore; };

template <int RESP, int OUTP, bool DIRECT = false>      // plane strides of the ring the residual comes from and of the ring / staging row written;
struct H3WRoleB {                                       // DIRECT: no LDS output, the role stores its rows to global memory
    using Gm = H3WGeom;
    using Epi = typename H3WEpiOf<DIRECT>::type;
    const char* tmid;
    const char* tres;
    char* tout;
    h8 w[13];
    f32x4 acc[Gm::G][3];
    int rp, rs;                  // lane's LDS byte offset in mid ring slot 0, group 0: pair / single fragments
    int rr;                      // lane's LDS byte offset of the residual operand [x_hi | x_lo] in its ring's slot 0, group 0
    int wo;                      // lane's LDS byte offset of its 8-byte hi record in output slot 0, group 0 (lo: + 2 planes)
    float inv_s2;
    f32x4 shs;                   // folded BN shift of the lane's four channels times s2 (the accumulators' scale)
    float lane_scale[Gm::G];
    bool skip_last = false;      // timing experiment (H3V_ABLATE & 256)
    h8 xr_pre;                   // H3W_PREFETCH: the residual operand of group 0 of the next step, carried across the barrier
    // DIRECT only
    char* gout;                  // FusedH3WArgs::out
    char* image;                 // the unit's image in it
    unsigned plane_g;            // bytes per global plane
    unsigned go;                 // lane's byte offset of its hi record inside the image's first row, group 0 (group g: + 256 g; lo: + 2 planes)
    unsigned long long okm[Gm::G];      // the lanes whose column of group g is an output column of the strip, inside [X0, X1) (wave-uniform)
    bool have;                   // the row this step completes is one of the band's (wave-uniform)
    size_t row_hi, row_lo;       // its byte offset inside a plane / + 2 planes (wave-uniform, < 2^32)

    __device__ __forceinline__ void init(const void* wimg, const FusedH3WArgs& a, const float* aux, const int lane, const int gc0,
                                         const bool out_is_ring)
    {
        const int q = lane >> 4;
        gout = reinterpret_cast<char*>(a.out);
        plane_g = (unsigned)a.H * (unsigned)a.W * 16u;
        image = nullptr;
        go = 0;
        have = false;
        row_hi = row_lo = 0;
        xr_pre = (h8){0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int g = 0; g < Gm::G; ++g) okm[g] = 0;
#pragma unroll
        for (int i = 0; i < 13; ++i) w[i] = reinterpret_cast<const h8*>(wimg)[bf_band_wimage(a, i) * 64 + lane];
        inv_s2 = aux[48];
        shs = *reinterpret_cast<const f32x4*>(aux + 32 + q * 4) * (1.0f / inv_s2);     // inv_s2 is a power of two: exact
        rp = (q & 1) * Gm::M_PLANE + (gc0 + (q >> 1)) * 16;
        rs = ((q & 1) + 2 * (q >> 1)) * Gm::M_PLANE + (gc0 + 2) * 16;
        rr = ((q & 1) + 2 * (q >> 1)) * RESP + (gc0 + 1) * 16;
        wo = (q >> 1) * OUTP + (gc0 + (out_is_ring ? 1 : 0)) * 16 + (q & 1) * 8;
#pragma unroll
        for (int g = 0; g < Gm::G; ++g)
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[g][k] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    __device__ __forceinline__ void set_tile(const H3WTile& t, const int W, const int gc0)
    {
#pragma unroll
        for (int g = 0; g < Gm::G; ++g) lane_scale[g] = (t.G0 + gc0 + 16 * g < W) ? inv_s2 : 0.f;
        if constexpr (DIRECT) {
            // the halo groups of the strip's grid, the columns right of a ragged strip and of the image: not stored
            const int q = (threadIdx.x & 63) >> 4, c0 = t.G0 + gc0;
#pragma unroll
            for (int g = 0; g < Gm::G; ++g) okm[g] = __builtin_amdgcn_ballot_w64((c0 + 16 * g >= t.X0) & (c0 + 16 * g < t.X1));
            go = (unsigned)(q >> 1) * plane_g + (unsigned)c0 * 16u + (unsigned)(q & 1) * 8u;
            image = gout + t.img;
        }
    }
    // DIRECT: band-relative row k is the output row this step completes
    __device__ __forceinline__ void set_row(const H3WTile& t, const int W, const int k)
    {
        if constexpr (DIRECT) {
            have = (k >= 0) & (k < t.nrows) & !(H3V_ABLATE & 2);                      // wave-uniform
            row_hi = (size_t)t.y(have ? k : 0) * W * 16;
            row_lo = row_hi + 2 * (size_t)plane_g;
        }
    }

    __device__ __forceinline__ H3VFrag load(const int mslot, const int g) const
    {
        H3VFrag f;
        const int o = mslot * Gm::PITCH + g * 256;
        f.ph = *reinterpret_cast<const h8*>(tmid + rp + o);
        f.pl = *reinterpret_cast<const h8*>(tmid + rp + o + 2 * Gm::M_PLANE);
        f.s = *reinterpret_cast<const h8*>(tmid + rs + o);
        return f;
    }
    __device__ __forceinline__ h8 load_res(const int xslot_bytes, const int g) const
    {
        return *reinterpret_cast<const h8*>(tres + rr + xslot_bytes + g * 256);
    }

    // the accumulator already holds s2 * (scale * conv2 + x + shift) (the shift is the C operand of the row's first MFMA)
    __device__ __forceinline__ Epi epilogue(const int g, const int oslot_bytes, const f32x4 accv, const bool rowok) const
    {
        Epi e;
        e.v = accv;
        e.sc = rowok ? lane_scale[g] : 0.f;
        e.floor_ = 0.f;
        if constexpr (DIRECT) {
            e.p = nullptr;
            e.lo_off = 0;
            e.image = image;
            e.image_bytes = 4u * plane_g;
            e.off = go + 256u * g;
            e.row_hi = row_hi;
            e.row_lo = row_lo;
            e.mask = have ? okm[g] : 0ull;
        } else {
            e.p = tout + wo + oslot_bytes + g * 256;
            e.lo_off = 2 * OUTP;
        }
        return e;
    }

    // MFMAs [J, JEND) of the 1 + 15 of group g.  !GROUPED: the residual, then the taps interleaved; micro-ops of the previous group's epilogue
    // (prev) after MFMA 2, 3, ...  GROUPED: a2 x 5, a1 x 5, the residual, c0 x 5; prev's micro-ops after MFMA 0 .. 6, those of the group's own
    // epilogue, built there into *own, after MFMA H3W_OWN_SLOT, ... (as H3WRoleA::mfmas)
    template <int J, int JEND, bool GROUPED, class Epi>
    __device__ __forceinline__ void mfmas(const int g, const int a1, const int a2, const H3VFrag& cur, const h8 xr, f32x4& c0, Epi* prev, Epi* own,
                                          const int oslot_bytes, const bool rowok)
    {
        if constexpr (J < JEND) {
            constexpr int RES = GROUPED ? 10 : 0, T = J - (J > RES ? 1 : 0);      // the residual's place; the tap MFMA's index among the 15
            if (!(H3V_ABLATE & 4) && !(skip_last && g == Gm::G - 1)) {
                if constexpr (J == RES) {
                    // residual: (s2 * I) x [x_hi | x_lo], exact, on top of the folded BN shift (times s2) as the C operand
                    c0 = MFMA_H(w[12], xr, shs);
                } else {
                    constexpr int k = GROUPED ? T % 5 : T / 3, which = GROUPED ? T / 5 : T % 3;
                    if constexpr (which == 0) acc[g][a2] = h3v_mfma(cur, w, 2, k, acc[g][a2]);
                    else if constexpr (which == 1) acc[g][a1] = h3v_mfma(cur, w, 1, k, acc[g][a1]);
                    else c0 = h3v_mfma(cur, w, 0, k, c0);
                }
            } else if (J == 0) {
                acc[g][a2][0] += (float)cur.ph[0] + (float)cur.pl[1] + (float)cur.s[2] + (float)xr[3];
            }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (!GROUPED) {
                if constexpr (J >= 2) {
                    if (prev) prev->template pair<J - 2>();
                }
            } else if constexpr (J < H3W_OWN_SLOT) {
                if (prev) prev->template pair<J>();
            } else {
                if constexpr (J == H3W_OWN_SLOT) *own = epilogue(g, oslot_bytes, acc[g][a2], rowok);
                own->template pair<J - H3W_OWN_SLOT>();
            }
            mfmas<J + 1, JEND, GROUPED>(g, a1, a2, cur, xr, c0, prev, own, oslot_bytes, rowok);
        }
    }

    // H3W_PREFETCH: the residual operand of group 0 of the NEXT step (byte offset next_xslot_bytes of its ring: a row that is final in this
    // step) -- read in the last group of a step, and in every step the role has no row in, so that each of its steps finds it in registers
    __device__ __forceinline__ void prefetch(const int next_xslot_bytes)
    {
        if (H3W_PREFETCH) xr_pre = load_res(next_xslot_bytes, 0);
    }

    // group g of step s (as H3WRoleA::group)
    template <int PH, int g, class Hook>
    __device__ __forceinline__ void group(H3VFrag& cur, h8& xr, const int xslot_bytes, const int next_xslot_bytes, const int oslot_bytes,
                                          const bool rowok, Hook& hook)
    {
        constexpr int mslot = (PH + 1) % Gm::NRM;                              // (s - 1) mod 2
        constexpr int a0 = PH % 3, a1 = (PH + 2) % 3, a2 = (PH + 1) % 3;
        constexpr bool grouped = h3w_grouped(g);
        constexpr bool late_nx = H3W_PREFETCH == 2 && g == 0;        // the group-1 operands are read behind the step's first MFMA
        H3VFrag nx;
        h8 xn;
        Epi own;
        if constexpr (g + 1 < Gm::G && !late_nx) {
            nx = load(mslot, g + 1);
            xn = load_res(xslot_bytes, g + 1);
        }
        if constexpr (g + 1 == Gm::G) prefetch(next_xslot_bytes);
        __builtin_amdgcn_sched_barrier(0);
        f32x4 c0;
        if constexpr (g > 0 && H3W_EPI_ORDER != 2) {
            Epi e = epilogue(g - 1, oslot_bytes, acc[g - 1][a2], rowok);
            mfmas<0, 16, grouped>(g, a1, a2, cur, xr, c0, &e, &own, oslot_bytes, rowok);
        } else {
            mfmas<0, 1, grouped>(g, a1, a2, cur, xr, c0, (Epi*)nullptr, &own, oslot_bytes, rowok);
            if constexpr (late_nx) {
                nx = load(mslot, 1);
                xn = load_res(xslot_bytes, 1);
                __builtin_amdgcn_sched_barrier(0);
            }
            mfmas<1, 16, grouped>(g, a1, a2, cur, xr, c0, (Epi*)nullptr, &own, oslot_bytes, rowok);
        }
        if constexpr (g == 0) {
            hook.after_first_group();
            __builtin_amdgcn_sched_barrier(0);
        }
        acc[g][a0] = c0;
        if constexpr (g + 1 < Gm::G) {
            cur = nx;
            xr = xn;
        }
    }

    // step s (s % UNROLL == PH): consumes the intermediate row completed in step s-1, starts an output row with the residual at
    // byte offset xslot_bytes of its ring (next_xslot_bytes: the one of step s+1), completes the output row of byte offset oslot_bytes
    template <int PH, class Hook>
    __device__ __forceinline__ void step(const int xslot_bytes, const int next_xslot_bytes, const int oslot_bytes, const bool rowok, Hook& hook)
    {
        static_assert(Gm::G == 3, "three groups per wave");
        H3VFrag cur = load((PH + 1) % Gm::NRM, 0);
        h8 xr = H3W_PREFETCH ? xr_pre : load_res(xslot_bytes, 0);
        group<PH, 0>(cur, xr, xslot_bytes, next_xslot_bytes, oslot_bytes, rowok, hook);
        group<PH, 1>(cur, xr, xslot_bytes, next_xslot_bytes, oslot_bytes, rowok, hook);
        group<PH, 2>(cur, xr, xslot_bytes, next_xslot_bytes, oslot_bytes, rowok, hook);
        if constexpr (!h3w_grouped(Gm::G - 1)) {
            Epi e = epilogue(Gm::G - 1, oslot_bytes, bf_acc_ready(acc[Gm::G - 1][(PH + 1) % 3]), rowok);
            e.all();
        }
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// Memory work rides on matrix waves (H3WMem<KIND> is the hook of a role's steps; KIND 0 = none).
// KIND 1, the loader: LDS-DMA of the x0 rows.  Wave j of its role moves piece j (grid columns [64j, 64j+64), the third piece 16
// columns) of all four planes: four wave-instructions per step, EVERY step (rows outside the band / the image read the zero
// line), so that the vmcnt of the wait is a constant.
// KIND 2, the storer (only where the staging rows exist and no head: H3W_DIRECT_STORE 0): the staged output row -> global memory.
// Eight 1-KiB pieces (plane, half) per row; wave j moves pieces 3j .. 3j+2.  The staging reads are issued at the start of the
// step, the stores behind the first group's MFMAs.
// Loads and stores sit on DIFFERENT waves: `s_waitcnt vmcnt(N)` counts both and stores retire early (fused_h3v.hip).  Under
// H3W_DIRECT_STORE the stores are B2's own (H3WEpiStore), so H3W_MEM_ROLES only places the loader; its value 3 would put the loads on B2
// as well and is refused.
// ---------------------------------------------------------------------------------------------------------------------
#ifndef H3W_MEM_ROLES
#define H3W_MEM_ROLES 0          // which roles carry {loader, storer}: 0 = {A2, A1}, 1 = {A1, B1}, 2 = {B1, A1}, 3 = {B2, A1}
#endif
static_assert(!(H3W_DIRECT_STORE && H3W_MEM_ROLES == 3), "loads and stores on different waves");
constexpr int h3w_mem_kind(const int role)
{
    constexpr int loader[4] = {2, 0, 1, 3}, storer[4] = {0, 1, 0, 0};
    return role == loader[H3W_MEM_ROLES] ? 1 : (role == storer[H3W_MEM_ROLES] ? 2 : 0);
}

template <int KIND>
struct H3WMem {
    __device__ __forceinline__ H3WMem(const FusedH3WArgs&, char*, const char*, int, unsigned) {}
    __device__ __forceinline__ void set_tile(const H3WTile&, int) {}
    __device__ __forceinline__ void prologue(const H3WTile&) {}
    __device__ __forceinline__ void begin(const H3WTile&, int, int) {}
    __device__ __forceinline__ void after_first_group() {}
    __device__ __forceinline__ void end() {}
    __device__ __forceinline__ void finish() {}
};

template <>
struct H3WMem<1> {
    using Gm = H3WGeom;
    const FusedH3WArgs& a;
    char* tin;
    int piece;
    unsigned plane_g;
    unsigned col_off;            // lane's byte offset inside a plane-row of the image
    bool active;                 // lane's column is fetched: inside [D0, D1) and the piece
    int dslot;                   // (s + PD) mod 5

    __device__ __forceinline__ H3WMem(const FusedH3WArgs& a_, char* tx0, const char*, const int rw, const unsigned pg)
        : a(a_), tin(tx0), piece(rw), plane_g(pg), col_off(0), active(false), dslot(0) {}
    __device__ __forceinline__ void set_tile(const H3WTile& t, const int lane)
    {
        const int c = t.G0 + 64 * piece + lane;
        active = (c >= t.D0) & (c < t.D1) & (64 * piece + lane < Gm::GW);
        col_off = (unsigned)c * 16u;
    }
    // x0 ring row r (band-relative row r - 4) into ring slot `slot`
    __device__ __forceinline__ void dma_row(const H3WTile& t, const int r, const int slot) const
    {
        if (H3V_ABLATE & 1) return;
        const int y = t.y(r - 4);
        const bool ok = (y >= 0) & (y < a.H) & (r < t.nrows + 8);                   // wave-uniform
#pragma unroll
        for (int plane = 0; plane < 4; ++plane) {
            const char* src = ok ? reinterpret_cast<const char*>(a.in) + t.img + (size_t)plane * plane_g + (size_t)y * a.W * 16 + col_off
                                 : reinterpret_cast<const char*>(a.zeros);
            char* dst = tin + plane * Gm::X0_PLANE + slot * Gm::PITCH + (1 + 64 * piece) * 16;
            if (active) h3_dma16(src, dst);
        }
    }
    static constexpr int INFLIGHT = 2 * 4;             // pieces of the two rows younger than the one awaited
    __device__ __forceinline__ void wait_landed() const { __builtin_amdgcn_s_waitcnt(h3_vmcnt((H3V_ABLATE & 1) ? 0 : INFLIGHT)); }
    // rows 0 .. PD-1 requested, row 0 landed
    __device__ __forceinline__ void prologue(const H3WTile& t)
    {
#pragma unroll
        for (int r = 0; r < Gm::PD; ++r) dma_row(t, r, r);
        wait_landed();
        dslot = Gm::PD;
    }
    __device__ __forceinline__ void begin(const H3WTile& t, const int s, int)
    {
        dma_row(t, s + Gm::PD, dslot);
        dslot = h3v_wrap(dslot + 1, Gm::NRX0);
    }
    __device__ __forceinline__ void after_first_group() {}
    __device__ __forceinline__ void end() { wait_landed(); }      // row s+1 (requested two steps ago) has landed
    // the rows requested past the band's end (zero-line reads into dead slots) must not land in the next band's rows
    __device__ __forceinline__ void finish() { __builtin_amdgcn_s_waitcnt(h3_vmcnt(0)); }
};

template <>
struct H3WMem<2> {
    using Gm = H3WGeom;
    const FusedH3WArgs& a;
    const char* tout;
    int first, np;               // pieces [first, first + np)
    unsigned plane_g;
    int st_off[3];               // lane's byte offset inside a staging slot
    unsigned g_off[3];           // lane's byte offset inside the image (plane + column)
    bool okc[3];
    h8 rec[3];
    bool have;
    char* image;                 // the unit's image in a.out
    size_t row_off;              // byte offset of the output row inside a plane (< 2^32)

    __device__ __forceinline__ H3WMem(const FusedH3WArgs& a_, char*, const char* tout_, const int rw, const unsigned pg)
        : a(a_), tout(tout_), first(3 * rw), np(rw < 2 ? 3 : 2), plane_g(pg), have(false), image(nullptr), row_off(0) {}
    __device__ __forceinline__ void set_tile(const H3WTile& t, const int lane)
    {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int p = first + i, plane = p >> 1, c = t.X0 + 64 * (p & 1) + lane;
            okc[i] = (i < np) & (c < t.X1);
            st_off[i] = plane * Gm::OUT_PLANE + (c - t.G0) * 16;
            g_off[i] = (unsigned)plane * plane_g + (unsigned)c * 16u;
        }
    }
    __device__ __forceinline__ void prologue(const H3WTile&) {}
    // step s (phase PH = s mod 6): output row s - 12, staged by B2 in step s-1
    __device__ __forceinline__ void begin(const H3WTile& t, const int s, const int PH)
    {
        const int k = s - Gm::LEAD, oslot = (PH + 1) % Gm::NRO;
        have = (k >= 0) & (k < t.nrows) & !(H3V_ABLATE & 2);                          // wave-uniform
        if (!have) return;
        image = reinterpret_cast<char*>(a.out) + t.img;
        row_off = (size_t)t.y(k) * a.W * 16;
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (i < np) rec[i] = *reinterpret_cast<const h8*>(tout + oslot * Gm::OUT_SLOT + st_off[i]);
    }
    __device__ __forceinline__ void after_first_group()
    {
        if (!have) return;
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (okc[i]) h3_stream_store16(image, 4u * plane_g, row_off, g_off[i], rec[i]);
    }
    __device__ __forceinline__ void end() {}
    __device__ __forceinline__ void finish() {}
};

// KIND 3, the head storer (last pair of a network, FusedH3WArgs::head_wh): instead of storing the staged row, waves 0 and 1 of the
// role take one pixel per lane (64 columns each), read its 16 channels (hi + lo: four 16-byte records), multiply by the
// premultiplied 16 x 3 head matrix and store tanh(2 h) * 0.51 denormalised, cropped, [rounded to uint8]: 3 bytes instead of 64
// per pixel leave the chip and the head kernel's pass over the activation disappears.
template <>
struct H3WMem<3> {
    using Gm = H3WGeom;
    const FusedH3WArgs& a;
    const char* tout;
    int half;                    // columns [64 half, 64 half + 64) of the strip; >= 2: nothing to do
    int st_off;                  // lane's byte offset inside plane 0 of a staging slot
    int col;                     // lane's image column
    bool okc;

    __device__ __forceinline__ H3WMem(const FusedH3WArgs& a_, char*, const char* tout_, const int rw, const unsigned)
        : a(a_), tout(tout_), half(rw), st_off(0), col(0), okc(false) {}
    __device__ __forceinline__ void set_tile(const H3WTile& t, const int lane)
    {
        col = t.X0 + 64 * half + lane;
        okc = (half < 2) & (col < t.X1) & (col < a.Wo);
        st_off = (col - t.G0) * 16;
    }
    __device__ __forceinline__ void prologue(const H3WTile&) {}
    __device__ __forceinline__ void begin(const H3WTile& t, const int s, const int PH)
    {
        const int k = s - Gm::LEAD, oslot = (PH + 1) % Gm::NRO;
        bool have = (half < 2) & (k >= 0) & (k < t.nrows) & !(H3V_ABLATE & 2);        // wave-uniform
        if (have) have = t.y(k) < a.Ho;
        if (!have) return;
        char* orow = reinterpret_cast<char*>(a.head_out) + ((size_t)t.b * a.Ho + (size_t)t.y(k)) * a.Wo * 3 * (a.head_u8 ? 1 : 4);
        const char* src = tout + oslot * Gm::OUT_SLOT + st_off;
        // the whole head sits HERE, in front of the role's step (not behind its first group's MFMAs): no fragment is live yet
        float h0 = 0.f, h1 = 0.f, h2 = 0.f;
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const h8 hi = *reinterpret_cast<const h8*>(src + hf * Gm::OUT_PLANE), lo = *reinterpret_cast<const h8*>(src + (2 + hf) * Gm::OUT_PLANE);
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float v = (float)hi[c] + (float)lo[c];
                const f32x4 w = *reinterpret_cast<const f32x4*>(a.head_wh + (hf * 8 + c) * 4);
                h0 = fmaf(v, w.x, h0);
                h1 = fmaf(v, w.y, h1);
                h2 = fmaf(v, w.z, h2);
            }
        }
        // an activation left the f16 range somewhere in the split-f16 blocks: inf / NaN propagate to here (0 * inf = NaN: a zero
        // head weight does not hide one)
        const bool finite = fabsf(h0) <= 3.0e38f && fabsf(h1) <= 3.0e38f && fabsf(h2) <= 3.0e38f;
        if (!finite && a.status) atomicOr(a.status, BF_STATUS_F16_RANGE);
        float r[3] = {h0, h1, h2};
#pragma unroll
        for (int o = 0; o < 3; ++o) {
            // tanh(2h) = 1 - 2 / (exp(4h) + 1): a handful of instructions (libm tanhf: ~30)
            float v = (1.0f - 2.0f / (__expf(4.0f * r[o]) + 1.0f)) * 0.51f;
            if (a.denormalize) v = (fminf(fmaxf(v, -0.5f), 0.5f) + 0.5f) * (a.v_max - a.v_min) + a.v_min;
            r[o] = v;
        }
        if (!okc) return;
        if (a.head_u8) {
            unsigned char* p = reinterpret_cast<unsigned char*>(orow) + (size_t)col * 3;
#pragma unroll
            for (int o = 0; o < 3; ++o) p[o] = (unsigned char)fminf(fmaxf(rintf(r[o]), 0.f), 255.f);      // rintf = round-half-even
        } else {
            float* p = reinterpret_cast<float*>(orow) + (size_t)col * 3;
#pragma unroll
            for (int o = 0; o < 3; ++o) p[o] = r[o];
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    __device__ __forceinline__ void after_first_group() {}
    __device__ __forceinline__ void end() {}
    __device__ __forceinline__ void finish() {}
};

// ---------------------------------------------------------------------------------------------------------------------
// The producer (first launch of a forward, FusedH3WArgs::base_u8; such a launch has no loader and issues no DMA at all): the x0
// ring rows are computed in the launch from uint8 image rows, with base_conv_rows_kernel's arithmetic (base_rows.h: the same A
// operands, three dependent MFMAs per 16 pixels in the order dy = 0, 1, 2, the same scale and split), so the ring holds bit for
// bit what the loader would have fetched.  H3WProducer<NGW, FETCH> is the share of one wave: NGW of the nine 16-pixel groups of a
// row, and (FETCH) one pixel per lane of the next input row; which roles carry what: H3W_BASE_SPREAD.
//   * input ring: input row u of a band is image row ybase + u - 5, kept in slot u mod 4.  x0 ring row r (image row ybase + r - 4)
//     multiplies input rows r, r + 1, r + 2;
//   * step s: the pixel requested in step s-1 (ring pixel 64 k + lane of fetching wave k, three byte loads) goes to input row
//     s + 4, the pixel of input row s + 5 is requested, x0 ring row s + 1 is produced from input rows s + 1 .. s + 3: complete at the
//     barrier that ends step s, one step before A1 reads it (the loader's rows land one step earlier still);
//   * per band: fill() writes input rows 0 .. 3 and requests row 4, and behind a barrier of its own prologue() produces x0 row 0;
//   * everything sits in front of the role's step, where no fragment is live; rows / columns outside the image are forced to zero
//     through the epilogue scale, rows no role reads (r >= nrows + 8) are not produced.
// Only the top-down walk exists (the first launch of a forward is never reversed).
// ---------------------------------------------------------------------------------------------------------------------
#ifndef H3W_BASE_SPREAD
#define H3W_BASE_SPREAD 1        // 0 = the A2 waves produce three groups each; 1 = one group per wave of B1, A2, B2; 2 = of A1, B1, A2
#endif
// groups per wave of a role / the first group of its wave rw / the role whose waves fetch the pixels (never a role that stores: A1 with the staging rows, B2 without)
constexpr int h3w_base_groups(const int role)
{
    return H3W_BASE_SPREAD == 0 ? (role == 2 ? 3 : 0) : (H3W_BASE_SPREAD == 1 ? (role >= 1 ? 1 : 0) : (role <= 2 ? 1 : 0));
}
constexpr int h3w_base_first_group(const int role, const int rw)
{
    return H3W_BASE_SPREAD == 0 ? 3 * rw : (H3W_BASE_SPREAD == 1 ? 3 * (role - 1) + rw : 3 * role + rw);
}
constexpr bool h3w_base_fetches(const int role) { return role == 2; }

template <int NGW, bool FETCH>
struct H3WProducer {
    using Gm = H3WGeom;
    const FusedH3WArgs& a;
    char* tx0;
    char* tring;
    const char* twa;
    int g0, fw;                  // first group of the wave; index of the wave among the fetching ones
    float inv_s, floor_;
    int wr;                      // lane's LDS byte offset of its 8-byte hi record in x0 ring slot 0, group g0 (as H3WRoleA::wr)
    int fo;                      // lane's byte offset of its group-g0 B fragment inside an input ring slot
    int col0;                    // image column of the lane's x0 column in group g0
    int px, xcol;                // ring pixel this lane fetches (>= GW + 2: none) and its image column
    const uint8_t* img;
    unsigned raw[3];             // the pixel requested in the previous step
    BrPixel rawp;
    int dslot;                   // (s + 1) mod 5

    __device__ __forceinline__ H3WProducer(const FusedH3WArgs& a_, char* lds, const int g0_, const int fw_)
        : a(a_), tx0(lds + Gm::X0_OFF), tring(lds + Gm::BIN_OFF), twa(lds + Gm::BWA_OFF), g0(g0_), fw(fw_), wr(0), fo(0), col0(0),
          px(0), xcol(0), img(nullptr), raw{0u, 0u, 0u}, rawp{false, false}, dslot(0)
    {
        inv_s = *reinterpret_cast<const float*>(lds + Gm::BINVS_OFF);
        floor_ = a.base_relu ? 0.f : -__builtin_inff();
    }
    __device__ __forceinline__ void set_tile(const H3WTile& t, const int lane)
    {
        const int n = lane & 15, q = lane >> 4, gc0 = 16 * g0 + n;
        wr = (q >> 1) * Gm::X0_PLANE + (gc0 + 1) * 16 + (q & 1) * 8;
        // B fragment of lane (n, q): the pixel pair starting at ring pixel p = grid column + 2 (q & 1) (q even: taps dx 0, 1; q odd:
        // tap dx 2 and a pixel that meets zero weights), from copy p & 1 at its aligned position; group g: + 128 g bytes
        const int p = gc0 + 2 * (q & 1);
        fo = ((p & 1) * Gm::BIN_ROWPX + (p & ~1)) * 8;
        twa = tx0 - Gm::X0_OFF + Gm::BWA_OFF + lane * 16;
        col0 = t.G0 + gc0;
        px = 64 * fw + lane;
        xcol = t.G0 - 1 + px;
        img = reinterpret_cast<const uint8_t*>(a.base_u8) + (size_t)t.b * a.Hs * a.Ws * 3;
    }
    // input row u: this lane's pixel -> raw (plain loads: the compiler waits for them where commit() reads them)
    __device__ __forceinline__ void request(const H3WTile& t, const int u)
    {
        const int yy = t.ybase + u - 5;
        const bool need = (px < Gm::GW + 2) & (u <= t.nrows + 9);          // rows past x0 row nrows + 7 feed nothing
        rawp = br_pixel(yy, xcol, a.H, a.W, a.Hs, a.Ws);
        rawp.inside &= need;
        rawp.colour &= need;
        if (rawp.colour) {
            const uint8_t* p = img + ((size_t)yy * a.Ws + xcol) * 3;
            raw[0] = p[0];
            raw[1] = p[1];
            raw[2] = p[2];
        }
    }
    // raw -> input ring row u: ring pixel j goes to copy 0 at j and to copy 1 at j - 1
    __device__ __forceinline__ void commit(const int u)
    {
        if (px >= Gm::GW + 2) return;
        const h4 v = br_record(rawp, raw[0], raw[1], raw[2]);
        h4* row = reinterpret_cast<h4*>(tring + (u & (Gm::BIN_RING - 1)) * Gm::BIN_SLOT);
        row[px] = v;
        if (px > 0) row[Gm::BIN_ROWPX + px - 1] = v;
    }
    // the wave's groups of x0 ring row r into ring slot `slot`
    __device__ __forceinline__ void produce(const H3WTile& t, const int r, const int slot)
    {
        if (r >= t.nrows + 8) return;                                        // wave-uniform
        const int y = t.y(r - 4);
        const bool rowok = (y >= 0) & (y < a.H);
        f32x4 acc[NGW];
#pragma unroll
        for (int g = 0; g < NGW; ++g) acc[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const h8 wa = *reinterpret_cast<const h8*>(twa + dy * 64 * 16);           // re-read every step: not held across the role's step
            const char* row = tring + ((r + dy) & (Gm::BIN_RING - 1)) * Gm::BIN_SLOT + fo;
#pragma unroll
            for (int g = 0; g < NGW; ++g) acc[g] = MFMA_H(wa, *reinterpret_cast<const h8*>(row + g * 128), acc[g]);
        }
#pragma unroll
        for (int g = 0; g < NGW; ++g) {
            H3VEpi<true> e;
            e.v = bf_acc_ready(acc[g]);
            e.sc = (rowok & (col0 + 16 * g < a.W)) ? inv_s : 0.f;            // outside the image: conv1a's zero padding
            e.floor_ = floor_;
            e.p = tx0 + wr + slot * Gm::PITCH + g * 256;
            e.lo_off = 2 * Gm::X0_PLANE;
            e.all();
        }
    }
    __device__ __forceinline__ void fill(const H3WTile& t)
    {
        if constexpr (FETCH) {
#pragma unroll
            for (int u = 0; u < Gm::BIN_RING; ++u) {
                request(t, u);
                commit(u);
            }
            request(t, Gm::BIN_RING);
        }
    }
    __device__ __forceinline__ void prologue(const H3WTile& t)
    {
        produce(t, 0, 0);
        dslot = 1;
    }
    __device__ __forceinline__ void begin(const H3WTile& t, const int s)
    {
        if constexpr (FETCH) {
            commit(s + 4);
            request(t, s + 5);
        }
        produce(t, s + 1, dslot);
        dslot = h3v_wrap(dslot + 1, Gm::NRX0);
        __builtin_amdgcn_sched_barrier(0);
    }
};

template <>
struct H3WProducer<0, false> {     // a wave without a share, and every wave of a launch that fetches its x0 rows
    __device__ __forceinline__ H3WProducer(const FusedH3WArgs&, char*, int, int) {}
    __device__ __forceinline__ void set_tile(const H3WTile&, int) {}
    __device__ __forceinline__ void fill(const H3WTile&) {}
    __device__ __forceinline__ void prologue(const H3WTile&) {}
    __device__ __forceinline__ void begin(const H3WTile&, int) {}
};

// the hook of a role: the head storer replaces the storer in a HEAD launch; a BASE launch has no loader; where B2 stores its rows itself
// (h3w_direct) there is no storer
template <bool HEAD>
constexpr bool h3w_direct() { return H3W_DIRECT_STORE != 0 && !HEAD; }
template <bool HEAD, bool BASE>
constexpr int h3w_hook_kind(const int role)
{
    const int k = h3w_mem_kind(role);
    return k == 2 ? (HEAD ? 3 : (h3w_direct<HEAD>() ? 0 : 2)) : ((BASE && k == 1) ? 0 : k);
}

template <bool HEAD, bool BASE>
__global__ __launch_bounds__(H3WGeom::NT, 3) void fused_block2_h3w_kernel(FusedH3WArgs a)
{
    using Gm = H3WGeom;
    extern __shared__ __attribute__((aligned(16))) char h3w_lds[];
    char* tx0 = h3w_lds + Gm::X0_OFF;                           // [4 planes][5 rows][146 columns][8 f16]
    char* tm1 = h3w_lds + Gm::M1_OFF;                           // [4 planes][2 rows][146][8]
    char* tx1 = h3w_lds + Gm::X1_OFF;                           // [4 planes][3 rows][146][8]
    char* tm2 = h3w_lds + Gm::M2_OFF;                           // [4 planes][2 rows][146][8]
    constexpr bool DIRECT = h3w_direct<HEAD>();                 // B2 stores its rows itself: no staging rows
    constexpr int LDS_RINGS = DIRECT ? Gm::LDS_BYTES : Gm::LDS_BYTES_STAGED;
    char* tout = DIRECT ? nullptr : h3w_lds + Gm::OUT_OFF;      // [2 rows][4 planes][144 columns][8 f16]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15;
    const int role = wave / Gm::NR, rw = wave - role * Gm::NR;
    const unsigned plane_g = (unsigned)a.H * (unsigned)a.W * 16u;      // bytes per global plane
    const int gc0 = 16 * Gm::G * rw + n;                        // lane's grid column in its wave's group 0

    // ring columns 0 and 145 are the zero padding at an image edge: cleared once, never written
    // (a BASE launch: so is everything of the input ring that is never written, the pixel past the last pair among it)
    if (BASE && a.status && blockIdx.x == 0 && tid == 0) *a.status = 0;       // first kernel of a forward
    for (int i = tid * 16; i < (BASE ? Gm::LDS_BYTES_BASE : LDS_RINGS); i += Gm::NT * 16)
        *reinterpret_cast<f32x4*>(h3w_lds + i) = (f32x4){0.f, 0.f, 0.f, 0.f};
    __syncthreads();
    if constexpr (BASE) {
        // the base convolution's A operands, as base_conv_rows_kernel computes them in its prologue
        const float bs = br_weight_scale(a.base_w, reinterpret_cast<float*>(h3w_lds + Gm::BRED_OFF));
        if (wave == 0) {
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
                *reinterpret_cast<h8*>(h3w_lds + Gm::BWA_OFF + (dy * 64 + lane) * 16) = br_operand(a.base_w, bs, dy, lane);
            if (lane == 0) *reinterpret_cast<float*>(h3w_lds + Gm::BINVS_OFF) = 1.0f / bs;
        }
        __syncthreads();
    }

#if H3V_ABLATE & 32
    unsigned long long stamp_sum[Gm::NSTAMP] = {0, 0, 0, 0}, stamp_prev, real0;
    asm volatile("s_memrealtime %0\n\ts_memtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(real0), "=s"(stamp_prev)::"memory");
#endif

#define H3W_ROW_IN_IMAGE(k) ((t.y(k) >= 0) & (t.y(k) < a.H))
// one band of one strip: R = the matrix role object, M = its memory hook, P = its share of the producer, ACTIVE(s) = the role has a row in step s,
// STEP(PH) = the role's step call, IDLE(PH) = what it does in a step it has no row in.  Every role runs the same number of barriers.
#define H3W_BAND(R, M, P, ACTIVE, STEP, IDLE)                                                                        \
    for (int ti = blockIdx.x; ti < a.ntiles; ti += gridDim.x) {                                               \
        const H3WTile t = h3w_tile(a, ti);                                                                    \
        R.set_tile(t, a.W, gc0);                                                                              \
        M.set_tile(t, lane);                                                                                  \
        P.set_tile(t, lane);                                                                                  \
        if constexpr (BASE) {                                /* producer launch: the first input rows */      \
            P.fill(t);                                                                                        \
            h3v_barrier();                                                                                    \
        }                                                                                                     \
        P.prologue(t);                                                                                        \
        M.prologue(t);                                                                                        \
        h3v_barrier();                                       /* x0 row 0 has landed / is complete */          \
        const int nsteps = t.nrows + Gm::LEAD;                                                                \
        int slot5 = 0;                                       /* s mod 5 */                                    \
        for (int s0 = 0; s0 < nsteps; s0 += Gm::UNROLL) {                                                     \
            H3W_ONE(0, M, P, ACTIVE, STEP, IDLE); H3W_ONE(1, M, P, ACTIVE, STEP, IDLE); H3W_ONE(2, M, P, ACTIVE, STEP, IDLE); \
            H3W_ONE(3, M, P, ACTIVE, STEP, IDLE); H3W_ONE(4, M, P, ACTIVE, STEP, IDLE); H3W_ONE(5, M, P, ACTIVE, STEP, IDLE); \
        }                                                                                                     \
        M.finish();                                                                                           \
        h3v_barrier();                                                                                        \
    }
#define H3W_ONE(PH, M, P, ACTIVE, STEP, IDLE)                                                                       \
    do {                                                                                                      \
        const int s = s0 + PH;                                                                                \
        P.begin(t, s);                                                                                        \
        M.begin(t, s, PH);                                                                                    \
        if (ACTIVE(s)) { STEP(PH); }                                                                          \
        else { M.after_first_group(); IDLE(PH); }                                                             \
        slot5 = h3v_wrap(slot5 + 1, Gm::NRX0);                                                                \
        H3V_STAMP(0);                                                                                         \
        M.end();                                                                                              \
        H3V_STAMP(1);                                                                                         \
        h3v_barrier();                                                                                        \
        H3V_STAMP(2);                                                                                         \
    } while (0)

    if (role == 0) {
        // ---- A1: conv1a on the x0 ring (dynamic slot s mod 5) -> first intermediate ring
        __builtin_amdgcn_s_setprio(H3W_PRIO_A1);
        H3WRoleA<Gm::X0_PLANE> R;
        R.tin = tx0; R.tmid = tm1;
        R.init(a.w1r[0], a, a.aux[0], lane, gc0);
        R.skip_last = (H3V_ABLATE & 256) && rw == Gm::NR - 1;
        H3WMem<h3w_hook_kind<HEAD, BASE>(0)> M(a, tx0, tout, rw, plane_g);
        H3WProducer<BASE ? h3w_base_groups(0) : 0, BASE && h3w_base_groups(0) && h3w_base_fetches(0)> P(a, h3w_lds, h3w_base_first_group(0, rw), rw);
        __builtin_amdgcn_s_waitcnt(h3_vmcnt(0));               // weight / scale loads
#define H3W_ACTIVE(s) ((s) < t.nrows + 8)
#define H3W_STEP(PH) R.template step<PH>(slot5 * Gm::PITCH, (s >= 2) & H3W_ROW_IN_IMAGE(s - 5), M)
#define H3W_IDLE(PH) do { } while (0)
        H3W_BAND(R, M, P, H3W_ACTIVE, H3W_STEP, H3W_IDLE)
#undef H3W_ACTIVE
#undef H3W_STEP
#undef H3W_IDLE
    } else if (role == 1) {
        // ---- B1: conv2a + residual x0 (ring row s-1) -> x1 ring
        __builtin_amdgcn_s_setprio(H3W_PRIO_B1);
        H3WRoleB<Gm::X0_PLANE, Gm::X1_PLANE> R;
        R.tmid = tm1; R.tres = tx0; R.tout = tx1;
        R.init(a.w2r[0], a, a.aux[0], lane, gc0, true);
        R.skip_last = (H3V_ABLATE & 256) && rw == Gm::NR - 1;
        H3WMem<h3w_hook_kind<HEAD, BASE>(1)> M(a, tx0, tout, rw, plane_g);
        H3WProducer<BASE ? h3w_base_groups(1) : 0, BASE && h3w_base_groups(1) && h3w_base_fetches(1)> P(a, h3w_lds, h3w_base_first_group(1, rw), rw);
        __builtin_amdgcn_s_waitcnt(h3_vmcnt(0));
#define H3W_ACTIVE(s) (((s) >= 3) & ((s) < t.nrows + 9))
        // the residual of step s is x0 ring row s-1; the one of step s+1, row s (slot5: the row A1 consumes in this step), is final already
#define H3W_STEP(PH) R.template step<PH>(h3v_wrap(slot5 + Gm::NRX0 - 1, Gm::NRX0) * Gm::PITCH, slot5 * Gm::PITCH, (PH % Gm::NRX1) * Gm::PITCH, H3W_ROW_IN_IMAGE(s - 7), M)
#define H3W_IDLE(PH) R.prefetch(slot5 * Gm::PITCH)
        H3W_BAND(R, M, P, H3W_ACTIVE, H3W_STEP, H3W_IDLE)
#undef H3W_ACTIVE
#undef H3W_STEP
#undef H3W_IDLE
    } else if (role == 2) {
        // ---- A2: conv1b on the x1 ring -> second intermediate ring
        __builtin_amdgcn_s_setprio(H3W_PRIO_A2);
        H3WRoleA<Gm::X1_PLANE> R;
        R.tin = tx1; R.tmid = tm2;
        R.init(a.w1r[1], a, a.aux[1], lane, gc0);
        R.skip_last = (H3V_ABLATE & 256) && rw == Gm::NR - 1;
        H3WMem<h3w_hook_kind<HEAD, BASE>(2)> M(a, tx0, tout, rw, plane_g);
        H3WProducer<BASE ? h3w_base_groups(2) : 0, BASE && h3w_base_groups(2) && h3w_base_fetches(2)> P(a, h3w_lds, h3w_base_first_group(2, rw), rw);
        __builtin_amdgcn_s_waitcnt(h3_vmcnt(0));
#define H3W_ACTIVE(s) (((s) >= 6) & ((s) < t.nrows + 10))
#define H3W_STEP(PH) R.template step<PH>(((PH + 2) % Gm::NRX1) * Gm::PITCH, H3W_ROW_IN_IMAGE(s - 9), M)
#define H3W_IDLE(PH) do { } while (0)
        H3W_BAND(R, M, P, H3W_ACTIVE, H3W_STEP, H3W_IDLE)
#undef H3W_ACTIVE
#undef H3W_STEP
#undef H3W_IDLE
    } else {
        // ---- B2: conv2b + residual x1 -> staging rows, or (DIRECT) global memory: output row s - 11 is complete in step s
        __builtin_amdgcn_s_setprio(H3W_PRIO_B2);
        H3WRoleB<Gm::X1_PLANE, Gm::OUT_PLANE, DIRECT> R;
        R.tmid = tm2; R.tres = tx1; R.tout = tout;
        R.init(a.w2r[1], a, a.aux[1], lane, gc0, false);
        R.skip_last = (H3V_ABLATE & 256) && rw == Gm::NR - 1;
        H3WMem<h3w_hook_kind<HEAD, BASE>(3)> M(a, tx0, tout, rw, plane_g);
        H3WProducer<BASE ? h3w_base_groups(3) : 0, BASE && h3w_base_groups(3) && h3w_base_fetches(3)> P(a, h3w_lds, h3w_base_first_group(3, rw), rw);
        __builtin_amdgcn_s_waitcnt(h3_vmcnt(0));
#define H3W_ACTIVE(s) (((s) >= 9) & ((s) < t.nrows + 11))
        // the residual of step s is the x1 row B1 completed in step s-2; the one of step s+1 was completed in step s-1 (the row A2 consumes now)
#define H3W_STEP(PH) R.set_row(t, a.W, s - (Gm::LEAD - 1)); R.template step<PH>(((PH + 1) % Gm::NRX1) * Gm::PITCH, ((PH + 2) % Gm::NRX1) * Gm::PITCH, (PH % Gm::NRO) * Gm::OUT_SLOT, true, M)
#define H3W_IDLE(PH) R.prefetch(((PH + 2) % Gm::NRX1) * Gm::PITCH)
        H3W_BAND(R, M, P, H3W_ACTIVE, H3W_STEP, H3W_IDLE)
#undef H3W_ACTIVE
#undef H3W_STEP
#undef H3W_IDLE
    }
#undef H3W_BAND
#undef H3W_ONE
#undef H3W_ROW_IN_IMAGE
#if H3V_ABLATE & 32
    {
        unsigned long long real1;
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(real1)::"memory");
        stamp_sum[3] = real1 - real0;                               // 100 MHz ticks: clock = cycles / ticks * 100 MHz
    }
    if (a.dbg && lane == 0) {
        for (int k = 0; k < Gm::NSTAMP; ++k) a.dbg[((size_t)blockIdx.x * Gm::NW + wave) * 8 + k] = stamp_sum[k];
    }
#endif
}

bool bf_fused_block2_h3w_supports(int H, int W) { return W >= 1 && H >= 1; }

hipError_t bf_launch_fused_block2_h3w(const FusedH3WArgs& args, hipStream_t s)
{
    using Gm = H3WGeom;
    FusedH3WArgs a = args;
    if (!a.zeros || (!a.in && !a.base_u8) || (!a.out && !a.head_wh) || !bf_fused_block2_h3w_supports(a.H, a.W)) return hipErrorInvalidValue;
    // the producer launch: the top-down walk only, never with the head, the image inside the frame
    if (a.base_u8 && (!a.base_w || a.head_wh || a.reverse_tiles || a.Hs < 1 || a.Ws < 1 || a.Hs > a.H || a.Ws > a.W)) return hipErrorInvalidValue;
    if ((int64_t)a.H * a.W * 64 >= ((int64_t)1 << 32)) return hipErrorInvalidValue;      // 32-bit in-image offsets
    const BandPlan p = bf_band_plan(a.B, a.H, (a.W + Gm::SW - 1) / Gm::SW, Gm::LEAD + 2);
    a.nstrips = p.nstrips;
    a.rows_per_tile = p.rows_per_tile;
    a.tiles_y = p.tiles_y;
    a.ntiles = p.ntiles;
    if (a.head_wh && (!a.head_out || a.Ho < 1 || a.Wo < 1 || a.Ho > a.H || a.Wo > a.W)) return hipErrorInvalidValue;
    void (*kernel)(FusedH3WArgs) = a.base_u8 ? fused_block2_h3w_kernel<false, true>
                                   : a.head_wh ? fused_block2_h3w_kernel<true, false> : fused_block2_h3w_kernel<false, false>;
    const int lds = a.base_u8 ? Gm::LDS_BYTES_BASE : (a.head_wh ? Gm::LDS_BYTES_STAGED : Gm::LDS_BYTES);
    const hipError_t e = bf_set_max_lds(reinterpret_cast<const void*>(kernel), lds);      // once per device
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(Gm::NT), lds, s, a);
    return hipGetLastError();
}
