"""Timing of bf_image_metrics (csrc/metrics.hip): uint8 batch 128 of 256 x 256 x 3 and one 375 x 1242 x 3 frame, 11 x 11 window, next
to the resnet 1 x 18 forward (DenoiserModule u8 -> u8) on the same batch.  The call is timed at the C ABI with its buffers allocated
once (what `evaluate` pays per batch besides two small allocations).  Device events around repetitions that add up to >= 1 s of
work per sample; several samples, median and spread printed; time per SSIM window next to the bytes the call has to read.
Run on the GPU box:  python tools/exp/metrics_bench.py [--samples 5]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
import blind_image_denoising_amd as bf                     # noqa: E402
from blind_image_denoising_amd import _native as N          # noqa: E402
from oracle import bfcnn_oracle as O                        # noqa: E402


def timed(fn, min_seconds=1.0):
    """ms per call: repetitions sized from a first estimate so that one sample covers >= min_seconds"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        fn()
    e1.record()
    torch.cuda.synchronize()
    reps = max(10, int(min_seconds * 1e4 / max(e0.elapsed_time(e1), 1e-3)) + 1)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def metrics_call(a, b, filter_size=11):
    B, H, W, C = a.shape
    lib = N.lib()
    nbytes = lib.bf_image_metrics_scratch_bytes(B, H, W, C, filter_size)
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=a.device)
    out = torch.empty((B, 4), dtype=torch.float64, device=a.device)
    dtype = N.BF_DTYPE_U8 if a.dtype == torch.uint8 else N.BF_DTYPE_F32

    def call():
        N.check(lib.bf_image_metrics(N.ptr(a), N.ptr(b), dtype, B, H, W, C, 255.0, filter_size, 1.5, 0.01, 0.03, N.ptr(out),
                                     N.ptr(scratch), nbytes, N.stream_ptr(a)), None, "bf_image_metrics")
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    rng = np.random.default_rng(0)
    for name, shape, dtype in (("batch 128 of 256x256x3 uint8", (128, 256, 256, 3), torch.uint8),
                               ("one 375x1242x3 uint8 frame", (1, 375, 1242, 3), torch.uint8),
                               ("batch 128 of 256x256x3 float32", (128, 256, 256, 3), torch.float32)):
        clean = rng.integers(0, 256, shape).astype(np.float64)
        noisy = np.clip(np.round(clean + rng.normal(0, 20, shape)), 0, 255)
        a, b = torch.from_numpy(clean).to(dtype).cuda(), torch.from_numpy(noisy).to(dtype).cuda()
        call = metrics_call(a, b)
        for _ in range(5):
            call()
        r = np.array([timed(call) for _ in range(args.samples)])
        windows = shape[0] * (shape[1] - 10) * (shape[2] - 10) * shape[3]
        nbytes = 2 * a.numel() * a.element_size()
        med = float(np.median(r))
        print(f"bf_image_metrics {name}, 11x11: median {med * 1e3:.1f} us (min {r.min() * 1e3:.1f}, max {r.max() * 1e3:.1f}, {len(r)} samples); "
              f"{windows} windows = {med * 1e6 / windows:.4f} ns per window; reads {nbytes / 1e6:.1f} MB = {nbytes / med / 1e9:.2f} TB/s", flush=True)

    cfg = O.canonical_config(no_layers=18)
    spec = O.ResnetSpec.from_config(cfg["model"])
    params, state = O.init_params(spec, seed=42)
    model = bf.model_builder(cfg["model"], device="cuda:0").hydra
    model.set_weights(params, state)
    module = bf.DenoiserModule(model)
    x = torch.from_numpy(rng.integers(0, 256, (128, 256, 256, 3)).astype(np.uint8)).cuda()
    for _ in range(3):
        module(x)
    f = np.array([timed(lambda: module(x)) for _ in range(args.samples)])
    print(f"resnet 1x18 forward, batch 128 of 256x256x3 u8 -> u8: median {np.median(f):.3f} ms (min {f.min():.3f}, max {f.max():.3f})", flush=True)
    module.check_status()


if __name__ == "__main__":
    main()
