"""What a burst merge is worth, alone and in front of the shipped network.

Six 256 x 256 crops of tests/golden/lena.jpg at (100, 100) + the global shifts (0,0), (3,-5), (-11,7), (19,14), (-23,-20), (6,26)
get white noise of sigma 10, 20 and 40 (default_rng(0), rounded and clipped) or camera noise (bf.camera_noise: variance = gain x
+ read_sigma^2).  For each burst: the PSNR against the clean reference crop of the noisy reference frame, of the denoiser on
that frame alone, of BurstDenoiserModule(None) (the merge alone, sigma estimated from the reference frame), of the merge without
alignment (zero field), of BurstDenoiserModule around the denoiser, and for camera noise of both denoiser arms inside a
StabilisedDenoiserModule; the mean number of frames that went into a pixel; the merge alone for other k = (k_lo, k_hi); and,
with a 40 x 40 inverted square pasted at another place in every alternate frame, the PSNR inside the square's track of the robust
merge and of the plain mean of the aligned frames (all weights 256).  Nothing is asserted.  One JSON document on stdout and,
with --out, in that file.

    python tools/exp/burst_quality.py --out burst_quality.json"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch

import blind_image_denoising_amd as bf

SHIFTS = ((0, 0), (3, -5), (-11, 7), (19, 14), (-23, -20), (6, 26))
TRACK = (slice(100, 140), slice(100, 190))
K_CHOICES = ((1.5, 3.0), (1.0, 2.0), (1.25, 2.0), (2.0, 4.0), (3.0, 6.0))


def psnr(a, b) -> float:
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return float(10.0 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def with_intruder(frames: np.ndarray) -> np.ndarray:
    out = frames.copy()
    for t in range(1, out.shape[1]):
        out[0, t, 100:140, 100 + 8 * t:140 + 8 * t] = 255 - out[0, t, 100:140, 100 + 8 * t:140 + 8 * t]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--image", default=os.path.join(ROOT, "tests", "golden", "lena.jpg"))
    ap.add_argument("--model", default="unet_laplacian_v5.6")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("burst_quality.py measures on the GPU: none is visible")
    denoiser = bf.load_denoiser_model(args.model)
    image = np.asarray(bf.load_image(path=args.image, image_size=None, num_channels=3, expand_dims=True, normalize=False), np.uint8)[0]
    S = args.size
    clean = np.stack([image[100 + dy:100 + dy + S, 100 + dx:100 + dx + S] for dy, dx in SHIFTS])          # [T,S,S,3]
    cases = [("white", 10.0), ("white", 20.0), ("white", 40.0), ("camera", (0.6, 3.0)), ("camera", (1.5, 5.0))]
    rows = []
    for kind, level in cases:
        if kind == "white":
            rng = np.random.default_rng(0)
            frames = np.stack([np.clip(np.rint(c + rng.normal(0.0, level, c.shape)), 0, 255).astype(np.uint8) for c in clean])[None]
        else:
            device_clean = torch.from_numpy(clean).cuda()         # the noise depends on (seed, position): another seed per frame
            frames = torch.cat([bf.camera_noise(device_clean[t:t + 1], level[0], level[1], seed=t)
                                for t in range(len(SHIFTS))]).cpu().numpy()[None]
        ref, target = frames[:, 0], clean[0]
        merge_alone, merged_denoised = bf.BurstDenoiserModule(None), bf.BurstDenoiserModule(denoiser)
        sigma = bf.estimate_noise(ref)
        row = {"noise": kind, "level": level, "estimated_sigma": float(sigma[0]), "psnr_reference_frame": psnr(ref[0], target),
               "psnr_single_denoised": psnr(denoiser(ref)[0], target),
               "psnr_merged": psnr(merge_alone(frames)[0], target),
               "mean_frames_merged": float(merge_alone.last_counts[..., 0].double().mean()) / 256.0,
               "mean_noise_gain": float((merge_alone.last_counts[..., 1].double().sqrt() / merge_alone.last_counts[..., 0].double()).mean()),
               "psnr_merged_denoised": psnr(merged_denoised(frames)[0], target)}
        device_frames = torch.from_numpy(frames).cuda()
        thresholds = bf.burst_thresholds(torch.from_numpy(sigma).cuda(), 3)
        field = bf.burst_align(device_frames)
        row["psnr_merged_zero_field"] = psnr(bf.burst_merge(device_frames, torch.zeros_like(field), thresholds)[0], target)
        row["share_of_exact_tile_shifts"] = float(np.mean([
            ((field[0, t, :, :, 0] == -SHIFTS[t][0]) & (field[0, t, :, :, 1] == -SHIFTS[t][1])).double().mean().item()
            for t in range(1, len(SHIFTS))]))
        if kind == "camera":
            stabilised = bf.StabilisedDenoiserModule(denoiser)
            row["psnr_single_stabilised_denoised"] = psnr(stabilised(ref)[0], target)
            row["psnr_merged_stabilised_denoised"] = psnr(bf.BurstDenoiserModule(stabilised)(frames)[0], target)
        moving = torch.from_numpy(with_intruder(frames)).cuda()
        moving_field = bf.burst_align(moving)
        everything = torch.tensor([[10 ** 12, 10 ** 12 + 1]], dtype=torch.int64, device="cuda")
        row["track_psnr_plain_mean"] = psnr(bf.burst_merge(moving, moving_field, everything, cast_to_uint8=False)[0][TRACK], target[TRACK])
        row["by_k"] = {}
        for k in K_CHOICES:
            thr = bf.burst_thresholds(torch.from_numpy(sigma).cuda(), 3, *k)
            row["by_k"][f"{k[0]},{k[1]}"] = {
                "psnr_merged": psnr(bf.burst_merge(device_frames, field, thr, cast_to_uint8=False)[0], target),
                "track_psnr_robust": psnr(bf.burst_merge(moving, moving_field, thr, cast_to_uint8=False)[0][TRACK], target[TRACK])}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    denoiser.check_status()
    out = {"device": torch.cuda.get_device_name(0), "model": args.model, "image": os.path.basename(args.image),
           "burst": [1, len(SHIFTS), S, S, 3], "rows": rows}
    text = json.dumps(bf.metrics.json_safe(out), indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
