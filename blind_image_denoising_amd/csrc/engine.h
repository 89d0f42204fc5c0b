// What the units of the C-ABI engine share: the handle, error reporting, the timing ring and the few host functions one unit
// calls in another.  engine.hip = handle, tensor inventory, options, reports and size queries ; engine_infer.hip = inference pack,
// forward plan, forward ; engine_train.hip = bf_train_step ; engine_adam.hip = the optimiser.  Device code never crosses a unit.
#pragma once
#include "bf_common.h"
#include <string>
#include <utility>
#include <vector>

constexpr int BF_TIMING_RING = 256;

// Option "timing": a ring of HIP-event pairs, one pair per begin() / end().  Every pair of a measurement window has ONE meaning:
// Forward = the residual-block launches of a forward, TrainBlock = one bwd_block_h3t launch of a training step.  A pair of the
// other kind restarts the window, so bf_get_timing never adds up pairs of both (it reports launches = launches_in_pair * n).
struct TimingRing {
    enum Kind { None, Forward, TrainBlock };
    std::vector<hipEvent_t> ev;     // 2 * BF_TIMING_RING events once the option has been set, none before
    int64_t n = 0;                  // pairs recorded since the window (re)started
    int launches_in_pair = 0;       // of the last pair
    Kind kind = None;

    void restart() { n = 0; kind = None; }
    hipError_t begin(hipStream_t s) { return hipEventRecord(ev[2 * (n % BF_TIMING_RING)], s); }
    hipError_t end(hipStream_t s, int launches, Kind k)
    {
        int64_t slot = n % BF_TIMING_RING;
        if (k != kind) {            // the other caller's pairs are in the ring: this pair (its first event is recorded) becomes pair 0
            std::swap(ev[0], ev[2 * slot]);
            n = 0; slot = 0; kind = k;
        }
        launches_in_pair = launches;
        ++n;
        return hipEventRecord(ev[2 * slot + 1], s);
    }
};

struct bf_engine {
    bf_resnet_desc d;
    std::string err;
    std::vector<bf_tensor_info> tensors, states;
    int64_t n_params = 0, n_state = 0;
    // parameter offsets (floats)
    int64_t p_base = 0, p_blocks = 0, p_block_stride = 0, p_head0 = 0, p_head1 = 0;
    int64_t n_base = 0;
    // packed-inference layout (floats)
    int64_t k_base = 0, k_blocks = 0, k_block_stride = 0, k_w0 = 0, k_w1 = 0, k_wh = 0, k_zero = 0, k_h3 = 0, k_total = 0;
    int fused_blocks = 1;
    int fused_head = 0;      // 1: split-f16 path, linear head, 3 output channels: head folded into the last block's epilogue
                             // (measured 5.49 vs 5.51 ms per batch of 128: the longer epilogue of the last block costs what the
                             // head kernel saves, so it stays an option)
    int h3_zigzag = 1;              // alternate the band order of consecutive split-f16 blocks (Infinity Cache reuse)
    int h3_variant = -1;            // split-f16 block kernel: < 0 = library default (bf_set_h3_variant), else that variant
    int h3_compact = 0;             // 1: full-row streaming kernel keeps the activations between the launches in the compact layout
    int h3_pair = 1;                // 1: where the streaming kernel applies, consecutive blocks run two per launch (fused_h3w.hip)
    int h3_pair_head = 0;           // 1: the last pair launch also runs a linear 3-channel head (no head kernel, the last activation is
                                    // never written).  Off by default: measured equal (4.437 vs 4.435 ms per batch of 128): the ~250
                                    // vector instructions per 64 pixels cost the issue-bound launch what the head kernel's pass costs
    int h3_pair_base = 1;           // 1: where the first launch of a forward is a pair and base_conv_rows_kernel could run, that launch
                                    // computes the base convolution itself (fused_h3w.hip H3WMem<4>): no base kernel, x0 is never
                                    // written or read back; the same bits.  0: the base kernel launches (A/B)
    int block_launches = 0;         // launches of the last forward's residual blocks (bf_get_timing)
    const char* block_kernel = "";  // name of the kernel that ran most of them
    std::string train_kernels;      // the block kernels of the last bf_train_step (bf_get_train_kernels)
                                    // (fp8 lo planes, 48 B per pixel; bf_common.h): +5 % images/s for 6e-6 instead of 2e-7 normalised MAE
    // arithmetic of the fused inference blocks: 1 = split-f16 on the f16 matrix cores (fused_h3.hip, needs
    // |activation| < 65504), 0 = exact fp32 on the f32 matrix cores (conv3x3_c16.hip)
    int arith = 1;
    // arithmetic of the training convolutions (forward + data gradient): 1 = split-f16 on the f16 matrix cores (default),
    // 0 = exact fp32 on the f32 matrix cores; the weight gradients follow the same switch
    int train_arith = 1;
    int train_zigzag = 1;           // split-f16 training: consecutive kernels walk their tiles in opposite directions
    int train_fused_fwd = 1;        // split-f16 training: BatchNorm apply + skip Add of block i formed while block i+1's first convolution stages its tile
    int train_fwd_block = 1;        // [3,3] blocks with BatchNorm + ReLU, W <= 256: the whole training forward of a block in ONE row-streaming
                                    // kernel (train_fwd_h3t.hip; T kept in LDS unless the backward pass reads it).  1 = where a forward holds
                                    // enough rows (bf_train_step), 2 = wherever it can run (tests), 0 = the two convolution kernels
    int train_bwd_block = 1;        // [3,3] blocks with BatchNorm + ReLU: the whole backward of a block in ONE row-streaming kernel that recomputes
                                    // T from the block input (train_bwd_h3t.hip: 5 tensor passes for 9, and the forward pass need not write T).
                                    // 1 = where a step holds enough strip rows, 2 = wherever it can run (tests), 0 = one kernel per convolution
    int train_fold_finalize = 1;    // block kernels: the BatchNorm finalisation kernels between the blocks (bn_finalize / bn_bwd_finalize, ~6 us +
                                    // two kernel boundaries each, 34 per step of 1x18) run in the prologue of the next block kernel instead
    int train_fused_bwd = 1;        // split-f16 training: weight + data gradient (+ BatchNorm backward) of a convolution in one kernel
    // optional HIP-event brackets: around the residual-block launches of a forward, or around every bwd_block_h3t launch of a
    // training step (bench.py rooflines)
    int timing = 0;
    TimingRing timed;
};

int fail(bf_handle h, int code, const char* fmt, ...);
int hip_fail(bf_handle h, hipError_t e, const char* what);

#define BF_HIP(call, what) do { hipError_t e__ = (call); if (e__ != hipSuccess) return hip_fail(h, e__, what); } while (0)

static inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// ------------------------------------------------------------------------------------------
// pow2 target of pad_to_power_of_2 (bfcnn/utilities.py:736-751): the reference evaluates
// 2^ceil(log(n)/log(2)) in float32; for every n <= 4096 that equals the exact next power of two
// (checked in tests/test_oracle_properties.py), which is what is computed here.
// ------------------------------------------------------------------------------------------
static inline int pow2_target(int n)
{
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

// engine_infer.hip: pack_all_convs_kernel (the exact-fp32 weight images; bf_pack_inference, and bf_train_step with train_arith 0)
hipError_t bf_launch_pack_all_convs(const float* params, int64_t p_blocks, int64_t p_stride, float* dst, int64_t d_stride, int layers,
                                    int with_dgrad, int nconv, int unit, hipStream_t s);
// engine_train.hip: floats of the training workspace (bf_workspace_bytes)
int64_t bf_train_workspace_floats(bf_handle h, int B, int H, int W);
