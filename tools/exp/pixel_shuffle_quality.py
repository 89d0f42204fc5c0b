"""What pixel-shuffle down-sampling is worth for the shipped network on correlated noise.

tests/golden/lena.jpg gets Gaussian noise that is white, filtered by [1,1] and filtered by [1,2,1] (separably, circularly, rescaled
to sigma), sigma 15 and 25, rounded and clipped.  For each of the six frames: the PSNR against the clean image of the noisy
frame, of bf.load_denoiser_model("unet_laplacian_v5.6") called directly, and of PixelShuffleDenoiserModule around it at stride
2, at stride 3, at "auto" and at "auto" with refine=8; the stride "auto" picked; and what estimate_noise (the MAD of the finest
band) and noise_correlation's sigma_white read on the noisy frame.  Nothing is asserted.  One JSON document on stdout and, with
--out, in that file.

    python tools/exp/pixel_shuffle_quality.py --out pixel_shuffle_quality.json"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch

import blind_image_denoising_amd as bf

KERNELS = {"white": [1.0], "[1,1]": [1.0, 1.0], "[1,2,1]": [1.0, 2.0, 1.0]}


def correlated_noise(shape, taps, sigma: float, seed: int) -> np.ndarray:
    n = np.random.default_rng(seed).standard_normal(shape)
    for axis in (0, 1):
        n = sum(w * np.roll(n, k, axis=axis) for k, w in enumerate(taps))
    return n * (sigma / n.std())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--image", default=os.path.join(ROOT, "tests", "golden", "lena.jpg"))
    ap.add_argument("--model", default="unet_laplacian_v5.6")
    ap.add_argument("--refine", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pixel_shuffle_quality.py measures on the GPU: none is visible")
    module = bf.load_denoiser_model(args.model)
    clean = np.asarray(bf.load_image(path=args.image, image_size=None, num_channels=3, expand_dims=True, normalize=False), np.uint8)
    arms = {"direct": module,
            "stride_2": bf.PixelShuffleDenoiserModule(module, 2),
            "stride_3": bf.PixelShuffleDenoiserModule(module, 3),
            "auto": bf.PixelShuffleDenoiserModule(module, "auto"),
            "auto_refined": bf.PixelShuffleDenoiserModule(module, "auto", refine=args.refine)}
    rows = []
    for name, taps in KERNELS.items():
        for sigma in (15.0, 25.0):
            noise = correlated_noise(clean.shape[1:], taps, sigma, seed=len(rows))
            noisy = np.clip(np.rint(clean[0].astype(np.float64) + noise), 0, 255).astype(np.uint8)[None]
            found = bf.noise_correlation(noisy)
            row = {"noise": name, "sigma": sigma, "psnr_noisy": float(bf.psnr(noisy, clean)[0]),
                   "estimate_noise": float(bf.estimate_noise(noisy)[0]), "sigma_white": float(found.sigma_white[0]),
                   "sigma_curve": [float(v) for v in found.sigma[0]], "stride_of_max_stride_6": int(found.stride[0])}
            for arm, call in arms.items():
                row["psnr_" + arm] = float(bf.psnr(call(noisy), clean)[0])
                if arm.startswith("auto"):
                    row["stride_" + arm] = call.last_stride
            rows.append(row)
            print(json.dumps(row), file=sys.stderr)
    module.check_status()
    out = {"device": torch.cuda.get_device_name(0), "model": args.model, "image": os.path.basename(args.image), "shape": list(clean.shape),
           "refine": args.refine, "rows": rows}
    text = json.dumps(bf.metrics.json_safe(out), indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
