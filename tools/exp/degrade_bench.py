"""Timing of the three degradation kernels at a training shape, by device events over rotating buffer sets (more
than the 256 MiB Infinity Cache holds), next to the bytes each has to move.

    python tools/exp/degrade_bench.py [--batch 32] [--size 256]"""
import argparse
import pathlib
import sys

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[2]))
import blind_image_denoising_amd as bf              # noqa: E402
from blind_image_denoising_amd import degrade as D  # noqa: E402


def timed(launch, sets, iters=200, warmup=20):
    for i in range(warmup):
        launch(i % sets)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        launch(i % sets)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    from blind_image_denoising_amd import _native as N
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    args = ap.parse_args()
    B, S, C, sets = args.batch, args.size, 3, 16
    dev = torch.device("cuda")
    n = B * S * S * C
    xs = [torch.randint(0, 256, (B, S, S, C), device=dev, dtype=torch.uint8).float() for _ in range(sets)]
    outs = [torch.empty_like(x) for x in xs]
    lib, stream = N.lib(), N.stream_ptr(xs[0])

    def i32(values):
        return torch.from_numpy(np.ascontiguousarray(values, dtype=np.int32)).to(dev)
    rows = []
    for name, sigma in (("blur sigma 1.0 (radius 3)", 1.0), ("blur sigma 4.0 (radius 12)", 4.0)):
        taps, radius = D._tap_table(np.full(B, sigma))
        d_taps, d_radius = i32(taps.reshape(-1)), i32(radius)
        rows.append((name, 8 * n, lambda k, d_taps=d_taps, d_radius=d_radius: N.call(
            "bf_op_degrade_blur", N.ptr(xs[k]), 0, N.ptr(outs[k]), B, S, S, C, N.ptr(d_taps), N.ptr(d_radius), stream)))
    quality = i32(np.full(B, 30))
    for name, sub in (("jpeg 4:4:4", 444), ("jpeg 4:2:0 (two launches)", 420)):
        nbytes = lib.bf_op_degrade_jpeg_scratch_bytes(B, S, S, C, sub)
        scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        rows.append((name, 8 * n + 2 * nbytes, lambda k, sub=sub, nbytes=nbytes, scratch=scratch: N.call(
            "bf_op_degrade_jpeg", N.ptr(xs[k]), 0, N.ptr(outs[k]), B, S, S, C, N.ptr(quality), sub, N.ptr(scratch), nbytes, stream)))
    step, thr, zero = i32(np.full(B, 4)), i32(np.full(B, int(0.2 * 2 ** 24))), i32(np.zeros(B))
    masks = [torch.empty((B, S, S), dtype=torch.uint8, device=dev) for _ in range(sets)]
    rows.append(("pointwise quantise", 8 * n, lambda k: N.call("bf_op_degrade_pointwise", N.ptr(xs[k]), 0, N.ptr(outs[k]), None, B, S, S, C,
                                                                N.ptr(step), N.ptr(zero), 7, stream)))
    rows.append(("pointwise quantise + drop + mask", 8 * n + n // C, lambda k: N.call(
        "bf_op_degrade_pointwise", N.ptr(xs[k]), 0, N.ptr(outs[k]), N.ptr(masks[k]), B, S, S, C, N.ptr(step), N.ptr(thr), 7, stream)))
    for name, moved, launch in rows:
        for rep in range(2):
            ms = timed(launch, sets)
            print(f"{name:<36} {B}x{S}x{S}x{C} f32: {ms * 1e3:8.1f} us, {moved / 1e6:6.1f} MB moved, {moved / ms / 1e9:5.2f} TB/s", flush=True)


if __name__ == "__main__":
    main()
