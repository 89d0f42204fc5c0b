"""What the two entry points of csrc/burst.hip cost on one 8 x 2048 x 2048 x 3 burst: HIP-event times after a
warm-up, the median over windows of back-to-back calls.  The merge is held against the bytes it must move (T frames read, one
frame and the counts written) at the 6.29 TB/s a float4 copy reaches on the MI355X; the alignment against its SAD issue count
(levels x tiles x alternate frames x candidates x 64 v_sad_u8 per candidate, 64 lanes per issue, two cycles per issue on each of
1024 SIMDs at 2.4 GHz).  Then both as a share of the BurstDenoiserModule call around a denoiser, each run tile by tile
(TiledDenoiserModule at --tile): resnet 1x18 with random weights and the shipped unet_laplacian_v5.6.  A library built with
-DBF_BURST_PLAIN_SAD (BFCNN_HIP_LIB) times the byte-by-byte form of the alignment with the same command.  One JSON document on
stdout and, with --out, in that file (rewritten after every measurement).

    python tools/exp/burst_time.py --out burst_time.json"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import _native as N

STREAM_BYTES_PER_S = 6.29e12          # measured float4 copy rate of the MI355X's HBM3E
SIMDS, CLOCK_HZ, CYCLES_PER_ISSUE = 1024, 2.4e9, 2


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


def synthetic_burst(T: int, size: int, C: int, sigma: float, seed: int = 0) -> np.ndarray:
    """[1,T,size,size,C]: crops of a blocky texture at random shifts within +-24 pixels under white noise"""
    rng = np.random.default_rng(seed)
    big = np.kron(rng.integers(0, 200, (size // 8 + 8, size // 8 + 8, C)), np.ones((8, 8, 1), np.int64)).astype(np.float32)
    frames = np.empty((1, T, size, size, C), np.uint8)
    for t in range(T):
        dy, dx = (24, 24) if t == 0 else rng.integers(0, 49, 2)
        crop = big[dy:dy + size, dx:dx + size]
        frames[0, t] = np.clip(np.rint(crop + sigma * rng.standard_normal(crop.shape, dtype=np.float32)), 0, 255)
    return frames


def sad_issues(T: int, H: int, W: int, levels: int, search: int) -> int:
    """wave-wide v_sad_u8 issues the alignment needs at the least: every lane busy, no tile cut"""
    total = 0
    for h, w in bf.burst.level_shapes(H, W, levels):
        gy, gx = bf.burst.grid_shape(h, w)
        total += gy * gx * (T - 1) * (2 * search + 1) ** 2 * 64 // 64
    return total


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--search", type=int, default=4)
    ap.add_argument("--sigma", type=float, default=20.0)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--kernels-only", action="store_true", help="skip the denoiser calls")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("burst_time.py measures on the GPU: none is visible")
    torch.cuda.set_device(0)
    T, H, W, C, K, R = args.frames, args.size, args.size, 3, args.levels, args.search
    frames = torch.from_numpy(synthetic_burst(T, H, C, args.sigma)).cuda()
    thresholds = bf.burst_thresholds(torch.full((1,), args.sigma, dtype=torch.float64, device="cuda"), C)
    field = bf.burst_align(frames, 0, K, R)
    _, counts = bf.burst_merge(frames, field, thresholds, return_counts=True)
    out = {"device": torch.cuda.get_device_name(0), "library": str(N.LIB_PATH), "shape": [1, T, H, W, C], "levels": K, "search": R,
           "sigma": args.sigma, "stream_bytes_per_s": STREAM_BYTES_PER_S,
           "mean_frames_merged": float(counts[..., 0].double().mean()) / 256.0,
           "share_of_nonzero_displacements": float((field[0, 1:] != 0).any(dim=-1).double().mean()), "kernels": {}, "modules": {}}

    def emit():
        text = json.dumps(bf.metrics.json_safe(out), indent=1)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return text

    n = H * W * C
    t = event_time_us(lambda: bf.burst_align(frames, 0, K, R), args.warmup, args.reps)
    issues = sad_issues(T, H, W, K, R)
    t.update(sad_issues=issues, floor_us=issues * CYCLES_PER_ISSUE / (SIMDS * CLOCK_HZ) * 1e6, floor="v_sad_u8 issue",
             luma_bytes=T * n + T * H * W, luma_floor_us=(T * n + T * H * W) / STREAM_BYTES_PER_S * 1e6)
    t["share_of_floor"] = t["floor_us"] / t["median_us"]
    out["kernels"]["bf_burst_align"] = t
    emit()
    for name, cast, with_counts in (("bf_op_burst_merge_u8_counts", True, True), ("bf_op_burst_merge_u8", True, False),
                                    ("bf_op_burst_merge_f32", False, False)):
        nbytes = T * n + (n if cast else 4 * n) + (8 * H * W if with_counts else 0)
        t = event_time_us(lambda: bf.burst_merge(frames, field, thresholds, 0, cast, with_counts), args.warmup, args.reps)
        t.update(bytes=nbytes, floor_us=nbytes / STREAM_BYTES_PER_S * 1e6, floor="HBM at the algorithmic bytes",
                 bytes_per_s=nbytes / (t["median_us"] * 1e-6))
        t["share_of_floor"] = t["floor_us"] / t["median_us"]
        out["kernels"][name] = t
        emit()
    if not args.kernels_only:
        def resnet_1x18():
            from oracle import bfcnn_oracle as O
            cfg = bf.CONFIGS_DICT["resnet_color_1x18_bn_16x3x3_256x256_l1_relu"]
            model = bf.model_builder(cfg["model"], device="cuda:0").hydra
            model.set_weights(*O.init_params(O.ResnetSpec.from_config(cfg["model"]), seed=42))
            return bf.DenoiserModule(model)

        denoisers = {"resnet_1x18_random_weights": resnet_1x18,
                     "unet_laplacian_v5.6": lambda: bf.load_model("unet_laplacian_v5.6", device="cuda:0")}
        align_us = out["kernels"]["bf_burst_align"]["median_us"]
        merge_us = out["kernels"]["bf_op_burst_merge_u8_counts"]["median_us"]
        for name, make in denoisers.items():
            try:
                module = bf.BurstDenoiserModule(bf.TiledDenoiserModule(make(), tile=args.tile), sigma=args.sigma, levels=K, search=R)
                row = event_time_us(lambda: module(frames), 2, 3)
                row.update(tile=args.tile, align_share=align_us / row["median_us"], merge_share=merge_us / row["median_us"],
                           f16_range_status_ok=bool(module.check_status()))
            except (RuntimeError, MemoryError, NotImplementedError) as e:       # recorded, not hidden
                row = {"error": f"{type(e).__name__}: {e}"}
            out["modules"][name] = row
            emit()
    print(emit())


if __name__ == "__main__":
    main()
