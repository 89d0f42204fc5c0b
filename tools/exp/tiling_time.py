"""What tiled inference costs beyond its denoiser calls, and how a tiled frame compares with the whole frame in one call.

Per model (canonical resnet 1x18; shipped unet_laplacian v5.6) on one 2048 x 2048 x 3 frame, HIP-event times after a warm-up,
device tensors in and out:
  (a) TiledDenoiserModule(tile=256, the default overlap / margin / tile_batch) on the frame
  (b) the float module on the already split chunks of (a) -- the denoiser calls alone
  (c) bf_op_tile_split_u8 for every chunk of (a) and bf_op_tile_blend alone, against their byte floors (split: one read and one
      write per tile byte; blend: 4 bytes read per tile float, one write per output sample) at the 6.29 TB/s a float4 copy
      reaches on the MI355X
  (d) DenoiserModule on the whole frame
and from them (a) - (b), the share of split + blend in (a), and (a) / (d).  The whole-frame calls run last.  One JSON document on
stdout and, with --out, in that file (rewritten after every model, so that a run that stops early leaves what it measured).

    python tools/exp/tiling_time.py --out tiling_time.json"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import tiling as TL

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


def kernel_record(t, nbytes):
    t = dict(t)
    t["bytes"] = int(nbytes)
    t["floor_us"] = nbytes / STREAM_BYTES_PER_S * 1e6
    t["share_of_stream_rate"] = t["floor_us"] / t["median_us"]
    return t


def measure_tiled(name, module, shape, tile, warmup, reps):
    B, H, W, C = shape
    image = torch.from_numpy(np.random.default_rng(0).integers(0, 256, shape, dtype=np.uint8)).to(module.model_hydra.device)
    tiled = bf.TiledDenoiserModule(module, tile=tile)
    plain = bf.DenoiserModule(module.model_hydra, cast_to_uint8=False)
    tiled(image)
    plan = tiled.last_plan
    n = B * plan.tiles
    K, starts = tiled.chunk_starts(n, tiled.tile_batch)
    split = lambda: [TL.tile_split_u8(image, tiled.tile, tiled.overlap, s, K) for s in starts]
    chunks = split()
    results = torch.empty((n, plan.t_h, plan.t_w, C), dtype=torch.float32, device=image.device)
    for s, chunk in zip(starts, chunks):
        results[s:s + K].copy_(plain(chunk))
    tile_samples = len(starts) * K * plan.t_h * plan.t_w * C
    rec = {"model": name, "shape": list(shape), "tile": tiled.tile, "overlap": tiled.overlap, "margin": tiled.margin,
           "tile_batch": K, "tiles": n, "denoiser_calls": len(starts), "tile_shape": [plan.t_h, plan.t_w],
           "pixels_computed_over_pixels_of_the_frame": len(starts) * K * plan.t_h * plan.t_w / (B * H * W),
           "tiled": event_time_us(lambda: tiled(image), warmup, reps),
           "denoiser_calls_on_split_chunks": event_time_us(lambda: [plain(c) for c in chunks], warmup, reps),
           "split_kernels": kernel_record(event_time_us(split, warmup, 10 * reps), 2 * tile_samples),
           "blend_kernel": kernel_record(event_time_us(lambda: TL.tile_blend(results, B, H, W, tiled.tile, tiled.overlap, tiled.margin),
                                                       warmup, 10 * reps), 4 * n * plan.t_h * plan.t_w * C + B * H * W * C)}
    rec["tiled_minus_denoiser_calls_us"] = rec["tiled"]["median_us"] - rec["denoiser_calls_on_split_chunks"]["median_us"]
    rec["split_plus_blend_share_of_tiled"] = (rec["split_kernels"]["median_us"] + rec["blend_kernel"]["median_us"]) / rec["tiled"]["median_us"]
    rec["f16_range_status_ok"] = bool(tiled.check_status())
    return rec, image


def measure_whole(rec, module, image, warmup, reps):
    rec["whole_frame"] = event_time_us(lambda: module(image), warmup, reps)
    rec["tiled_over_whole_frame"] = rec["tiled"]["median_us"] / rec["whole_frame"]["median_us"]
    module.check_status()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tiling_time.py measures on the GPU: none is visible")
    torch.cuda.set_device(0)
    shape = (1, args.size, args.size, 3)

    resnet = bf.model_builder(bf.CONFIGS_DICT["resnet_color_1x18_bn_16x3x3_256x256_l1_relu"]["model"], device="cuda:0", seed=0).hydra
    modules = [("resnet_color_1x18", bf.DenoiserModule(resnet)), ("unet_laplacian_v5.6", bf.load_model("unet_laplacian_v5.6", device="cuda:0"))]
    out = {"device": torch.cuda.get_device_name(0), "stream_bytes_per_s": STREAM_BYTES_PER_S, "timings": []}

    def emit():
        text = json.dumps(bf.metrics.json_safe(out), indent=1)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return text

    images = []
    for name, module in modules:
        rec, image = measure_tiled(name, module, shape, args.tile, args.warmup, args.reps)
        out["timings"].append(rec)
        images.append(image)
        emit()
    for rec, (_, module), image in zip(out["timings"], modules, images):
        measure_whole(rec, module, image, args.warmup, args.reps)
        emit()
    print(emit())


if __name__ == "__main__":
    main()
