"""What one frame of the recursive temporal filter costs, at 32 x 256 x 256 x 3 (parallel streams) and at
1 x 2048 x 2048 x 3: HIP-event times after a warm-up, the median over windows of back-to-back calls.  The state is filled first by
a few frames of a wandering synthetic scene; the timed step then runs on fixed inputs (it is not in place, so every call does
the same work).  Timed: bf_burst_align on the pair (frame, image of the state), bf_op_video_update in both output forms, and
bf_op_burst_merge at T = 2 on the same shape as the yardstick (the same staging without the state traffic).  The update is held
against the bytes it must move per pixel at C = 3 -- frame 3, acc 6 and cnt 2 read; acc 6, cnt 2 and image 3 written: 22, and 12
more for the float32 output -- at the 6.29 TB/s a float4 copy reaches on the MI355X.  Then align + update as a share of a
VideoDenoiserModule call around resnet 1x18 with random weights and the shipped unet_laplacian_v5.6 (tile by tile at 2048 x 2048).
One JSON document on stdout and, with --out, in that file (rewritten after every measurement).

    python tools/exp/video_bench.py --out video_bench.json"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import _native as N
from blind_image_denoising_amd import burst as BU
from blind_image_denoising_amd import video as VI

STREAM_BYTES_PER_S = 6.29e12          # measured float4 copy rate of the MI355X's HBM3E
SHAPES = ((32, 256, 256, 3), (1, 2048, 2048, 3))


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


def synthetic_sequence(B: int, T: int, size: int, C: int, sigma: float, seed: int = 0) -> torch.Tensor:
    """uint8 [B,T,size,size,C] on the device: crops of a blocky texture that wander by up to 6 pixels per frame, under white noise"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    rng = np.random.default_rng(seed)
    cells = torch.randint(0, 200, (B, size // 8 + 8, size // 8 + 8, C), generator=gen, device="cuda", dtype=torch.int32)
    big = cells.repeat_interleave(8, dim=1).repeat_interleave(8, dim=2).float()
    frames, pos = [], np.array([24, 24])
    for _ in range(T):
        pos = np.clip(pos + rng.integers(-6, 7, 2), 0, 48)
        crop = big[:, pos[0]:pos[0] + size, pos[1]:pos[1] + size]
        noise = torch.randn(crop.shape, generator=gen, device="cuda") * sigma
        frames.append(torch.clamp(torch.round(crop + noise), 0, 255).to(torch.uint8))
    return torch.stack(frames, dim=1)


def measure_shape(shape, args, out, emit):
    B, H, W, C = shape
    K, R = args.levels, args.search
    frames = synthetic_sequence(B, args.fill + 1, H, C, args.sigma)
    filt = bf.VideoDenoiserModule(None, n_max=args.n_max, levels=K, search=R, sigma=args.sigma)
    for t in range(args.fill):
        filt(frames[:, t].contiguous())
    state, x = filt.state, frames[:, args.fill].contiguous()
    thresholds = bf.burst_thresholds(torch.full((B,), args.sigma, dtype=torch.float64, device="cuda"), C)
    pair = torch.stack([x, state.image], dim=1)
    field2 = bf.burst_align(pair, 0, K, R)
    field = field2[:, 1].contiguous()
    _, after = bf.video_update(x, state, field, thresholds, args.n_max)
    row = {"shape": list(shape), "mean_frames_in_state": float(state.cnt.cpu().numpy().mean()) / 256.0,
           "mean_frames_after_step": float(after.cnt.cpu().numpy().mean()) / 256.0,
           "share_of_nonzero_displacements": float((field != 0).any(dim=-1).double().mean()), "kernels": {}, "modules": {}}
    out["shapes"]["x".join(map(str, shape))] = row
    px = B * H * W
    # bytes per pixel: frame C, acc 2 C and cnt 2 read, acc 2 C, cnt 2 and image C written (+ 4 C float32); merge: 2 C read, C + 8 written
    timed = (("stack_pair", lambda: torch.stack([x, state.image], dim=1), 4 * C),
             ("bf_burst_align_pair", lambda: BU._align(pair, 0, K, R), None),
             ("bf_op_video_update_u8", lambda: VI._update(x, state, field, thresholds, args.n_max, True), 6 * C + 4),
             ("bf_op_video_update_f32", lambda: VI._update(x, state, field, thresholds, args.n_max, False), 10 * C + 4),
             ("bf_op_burst_merge_T2_u8_counts", lambda: BU._merge(pair, field2, thresholds, 0, True, True), 3 * C + 8))
    for name, fn, per_px in timed:
        t = event_time_us(fn, args.warmup, args.reps)
        if per_px is not None:
            nbytes = per_px * px
            t.update(bytes_per_pixel=per_px, bytes=nbytes, floor_us=nbytes / STREAM_BYTES_PER_S * 1e6, floor="HBM at the algorithmic bytes",
                     bytes_per_s=nbytes / (t["median_us"] * 1e-6))
            t["share_of_floor"] = t["floor_us"] / t["median_us"]
        row["kernels"][name] = t
        emit()
    k = row["kernels"]
    row["update_over_merge_T2"] = k["bf_op_video_update_u8"]["median_us"] / k["bf_op_burst_merge_T2_u8_counts"]["median_us"]
    step = event_time_us(lambda: (filt._record.update(state=state), filt(x)), args.warmup, args.reps)       # the module's temporal step, state put back
    row["modules"]["temporal_filter_alone"] = step
    emit()
    if args.kernels_only:
        return

    def resnet_1x18():
        from oracle import bfcnn_oracle as O
        cfg = bf.CONFIGS_DICT["resnet_color_1x18_bn_16x3x3_256x256_l1_relu"]
        model = bf.model_builder(cfg["model"], device="cuda:0").hydra
        model.set_weights(*O.init_params(O.ResnetSpec.from_config(cfg["model"]), seed=42))
        return bf.DenoiserModule(model)

    denoisers = {"resnet_1x18_random_weights": resnet_1x18,
                 "unet_laplacian_v5.6": lambda: bf.load_model("unet_laplacian_v5.6", device="cuda:0")}
    temporal_us = k["bf_burst_align_pair"]["median_us"] + k["bf_op_video_update_u8"]["median_us"]
    for name, make in denoisers.items():
        try:
            inner = make()
            if H > args.tile:
                inner = bf.TiledDenoiserModule(inner, tile=args.tile)
            module = bf.VideoDenoiserModule(inner, n_max=args.n_max, levels=K, search=R, sigma=args.sigma)
            module._record = filt._record                          # the filled state

            def call():
                filt._record.update(state=state)
                return module(x)

            r = event_time_us(call, 2, 3 if H > args.tile else args.reps)
            r.update(tiled=H > args.tile, align_plus_update_us=temporal_us, align_plus_update_share=temporal_us / r["median_us"],
                     temporal_step_share=step["median_us"] / r["median_us"], f16_range_status_ok=bool(module.check_status()))
        except (RuntimeError, MemoryError, NotImplementedError) as e:       # recorded, not hidden
            r = {"error": f"{type(e).__name__}: {e}"}
        row["modules"][name] = r
        emit()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--fill", type=int, default=6, help="frames that fill the state before the timed step")
    ap.add_argument("--n-max", type=int, default=8)
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--search", type=int, default=4)
    ap.add_argument("--sigma", type=float, default=20.0)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--kernels-only", action="store_true", help="skip the denoiser calls")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("video_bench.py measures on the GPU: none is visible")
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0), "library": str(N.LIB_PATH), "n_max": args.n_max, "levels": args.levels,
           "search": args.search, "sigma": args.sigma, "stream_bytes_per_s": STREAM_BYTES_PER_S, "shapes": {}}

    def emit():
        text = json.dumps(bf.metrics.json_safe(out), indent=1)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return text

    for shape in SHAPES:
        measure_shape(shape, args, out, emit)
    print(emit())


if __name__ == "__main__":
    main()
