"""Timing of bf_noise_estimate (csrc/noise_estimate.hip) next to bf_image_metrics (11 x 11 window) at the same shapes: uint8 batch 128
of 256 x 256 x 3, one 375 x 1242 x 3 frame, and the float32 batch.  Both calls are timed at the C ABI with their buffers allocated once.
The images are flat grey plus Gaussian noise of sigma 20, and random bytes: the first fills few histogram bins (many lanes of a wave
on one LDS bin), the second spreads them.  Device events around repetitions that add up to >= --seconds of work per sample; median
and spread printed, with the rate at which the batch is read.
Run on the GPU box:  python tools/exp/noise_estimate_bench.py [--samples 5] [--seconds 1.0]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
from blind_image_denoising_amd import _native as N          # noqa: E402
from metrics_bench import metrics_call, timed               # noqa: E402


def noise_call(a):
    B, H, W, C = a.shape
    lib = N.lib()
    nbytes = lib.bf_noise_estimate_scratch_bytes(B, H, W, C)
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=a.device)
    out = torch.empty((B, C, 4), dtype=torch.float64, device=a.device)
    dtype = N.BF_DTYPE_U8 if a.dtype == torch.uint8 else N.BF_DTYPE_F32

    def call():
        N.check(lib.bf_noise_estimate(N.ptr(a), dtype, B, H, W, C, N.ptr(scratch), nbytes, N.ptr(out), N.stream_ptr(a)), None,
                "bf_noise_estimate")
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    rng = np.random.default_rng(0)

    def report(what, call, nbytes):
        for _ in range(5):
            call()
        r = np.array([timed(call, args.seconds) for _ in range(args.samples)])
        med = float(np.median(r))
        print(f"{what}: median {med * 1e3:.1f} us (min {r.min() * 1e3:.1f}, max {r.max() * 1e3:.1f}, {len(r)} samples); "
              f"reads {nbytes / 1e6:.1f} MB = {nbytes / med / 1e9:.3f} TB/s", flush=True)

    for name, shape, dtype in (("batch 128 of 256x256x3 uint8", (128, 256, 256, 3), torch.uint8),
                               ("one 375x1242x3 uint8 frame", (1, 375, 1242, 3), torch.uint8),
                               ("batch 128 of 256x256x3 float32", (128, 256, 256, 3), torch.float32)):
        grey = np.clip(np.round(128.0 + rng.normal(0, 20, shape)), 0, 255)
        noise = rng.integers(0, 256, shape).astype(np.float64)
        a, b = torch.from_numpy(grey).to(dtype).cuda(), torch.from_numpy(noise).to(dtype).cuda()
        nbytes = a.numel() * a.element_size()
        report(f"bf_noise_estimate {name}, grey + sigma 20", noise_call(a), nbytes)
        report(f"bf_noise_estimate {name}, random bytes", noise_call(b), nbytes)
        report(f"bf_image_metrics {name}, 11x11", metrics_call(a, b), 2 * nbytes)


if __name__ == "__main__":
    main()
