"""What the five entry points of csrc/pixel_shuffle.hip cost on one 2048 x 2048 x 3 frame: HIP-event times after
a warm-up, the median over windows of back-to-back calls, each against the bytes it must move (split, merge, replace and mean:
one read and one write per sample; the correlation kernel: one read) at the 6.29 TB/s a float4 copy reaches on the MI355X, and as
a share of the denoiser call it wraps (the shipped unet_laplacian v5.6 in float form: on the [s^2, H / s, W / s, 3] sub-images for
noise_correlation, split and merge, on the [T, H, W, 3] copies for replace and mean).  One JSON document on stdout and, with
--out, in that file (rewritten after every measurement, so that a run that stops early leaves what it measured).

    python tools/exp/pixel_shuffle_time.py --out pixel_shuffle_time.json"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
import torch

import blind_image_denoising_amd as bf

STREAM_BYTES_PER_S = 6.29e12          # measured float4 copy rate of the MI355X's HBM3E


def event_time_us(fn, warmup: int, reps: int, rounds: int = 5):
    """median and spread over `rounds` windows of `reps` back-to-back calls each, in microseconds per call"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        per_call.append(e0.elapsed_time(e1) / reps * 1e3)
    return {"median_us": float(np.median(per_call)), "min_us": float(min(per_call)), "max_us": float(max(per_call)),
            "calls_per_window": reps, "windows": rounds}


def graphed(fn, reps: int):
    """`reps` back-to-back calls of fn captured into one graph: its replay"""
    current = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(current)
    with torch.cuda.stream(side):                                # warm-up off the capture: code objects, allocator
        fn()
    current.wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(reps):
            fn()
    return graph.replay


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--stride", type=int, default=2)
    ap.add_argument("--max-stride", type=int, default=6)
    ap.add_argument("--copies", type=int, default=8)
    ap.add_argument("--model", default="unet_laplacian_v5.6")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pixel_shuffle_time.py measures on the GPU: none is visible")
    torch.cuda.set_device(0)
    B, H, W, C, s, T, S = 1, args.size, args.size, 3, args.stride, args.copies, args.max_stride
    n = B * H * W * C
    rng = np.random.default_rng(0)
    # a flat frame under white noise of sigma 20: the histogram kernel's time depends on how many bins the counts fall into, and
    # uniform random bytes would spread them over all 511
    image = torch.from_numpy(np.clip(np.rint(128.0 + 20.0 * rng.standard_normal((B, H, W, C))), 0, 255).astype(np.uint8)).cuda()
    base = torch.from_numpy(rng.integers(0, 256, (B, H, W, C), dtype=np.uint8)).cuda()
    members = bf.pd_split_u8(image, s)
    member_floats = members.float()
    copies = bf.pd_replace_u8(base, image, T)
    copy_floats = copies.float()
    out = {"device": torch.cuda.get_device_name(0), "shape": [B, H, W, C], "stride": s, "max_stride": S, "copies": T,
           "stream_bytes_per_s": STREAM_BYTES_PER_S, "kernels": {}, "denoiser": {}}

    def emit():
        text = json.dumps(bf.metrics.json_safe(out), indent=1)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return text

    padded = members.numel()                                     # the sub-images repeat a row / column where s does not divide H / W
    kernels = {
        "bf_noise_correlation": (lambda: bf.noise_correlation_statistics(image, S), n, "sub_images"),
        "bf_op_pd_split_u8": (lambda: bf.pd_split_u8(image, s), n + padded, "sub_images"),
        "bf_op_pd_merge_u8": (lambda: bf.pd_merge(member_floats, B, H, W, s, True), 4 * n + n, "sub_images"),
        "bf_op_pd_merge_f32": (lambda: bf.pd_merge(member_floats, B, H, W, s, False), 4 * n + 4 * n, "sub_images"),
        "bf_op_pd_replace_u8": (lambda: bf.pd_replace_u8(base, image, T), 2 * n + T * n, "copies"),
        "bf_op_pd_mean_u8": (lambda: bf.pd_mean(copy_floats, T, True), 4 * T * n + n, "copies"),
        "bf_op_pd_mean_f32": (lambda: bf.pd_mean(copy_floats, T, False), 4 * T * n + 4 * n, "copies"),
    }
    for name, (fn, nbytes, wrapped) in kernels.items():
        # the kernels take microseconds, less than a launch from Python: `reps` calls are captured into one graph (every entry
        # point is graph-capturable) and a window is one replay
        replay = graphed(fn, args.reps)
        t = event_time_us(replay, args.warmup, 1)
        for key in ("median_us", "min_us", "max_us"):
            t[key] /= args.reps
        t["calls_per_window"] = args.reps
        t.update(bytes=int(nbytes), floor_us=nbytes / STREAM_BYTES_PER_S * 1e6, wrapped_call=wrapped)
        t["share_of_stream_rate"] = t["floor_us"] / t["median_us"]
        t["bytes_per_s"] = nbytes / (t["median_us"] * 1e-6)
        out["kernels"][name] = t
        emit()

    module = bf.load_model(args.model, device="cuda:0").float_form()
    for name, batch in (("sub_images", members), ("copies", copies)):
        try:
            out["denoiser"][name] = dict(event_time_us(lambda: module(batch), 2, 3), shape=list(batch.shape))
        except (RuntimeError, MemoryError) as e:                 # a batch the model's workspace cannot hold: recorded, not hidden
            out["denoiser"][name] = {"error": str(e), "shape": list(batch.shape)}
            emit()
            continue
        for t in out["kernels"].values():
            if t["wrapped_call"] == name:
                t["share_of_wrapped_call"] = t["median_us"] / out["denoiser"][name]["median_us"]
        emit()
    out["f16_range_status_ok"] = bool(module.check_status())
    print(emit())


if __name__ == "__main__":
    main()
