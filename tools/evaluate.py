"""Evaluate a denoiser on image files: the acceptance protocol of the reference's tests/bfcnn/test_pretrained.py (truncated-normal
noise of each standard deviation, round, clip; PSNR, SSIM and MAE of the noisy and of the denoised frame against the clean one) as a
table, measured on the GPU by blind_image_denoising_amd.evaluate.  It reads only the files it is given.

    python tools/evaluate.py unet_laplacian_v5.6 frames/*.png --noise-std 10 15 20 25 30 --json report.json

MODEL is a registry name (blind_image_denoising_amd.models), a model directory, `nlm` or `bm3d` (non-local means, BM3D: the
classical baselines to put next to a network's numbers); IMAGES are files or directories.  Every image is its own batch,
so frames of different sizes can be mixed; --size H W resizes them first."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import blind_image_denoising_amd as bf                     # noqa: E402
from blind_image_denoising_amd import metrics as M          # noqa: E402
from blind_image_denoising_amd.file_operations import image_filenames_generator      # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("model")
    ap.add_argument("images", nargs="+")
    ap.add_argument("--noise-std", type=float, nargs="+", default=list(M.DEFAULT_NOISE_STD))
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--filter-size", type=int, default=11)
    ap.add_argument("--size", type=int, nargs=2, metavar=("H", "W"), default=None)
    ap.add_argument("--json", dest="json_path", default=None, help="write the report here as strict JSON")
    args = ap.parse_args(argv)
    module = bf.load_model(args.model)
    files = []
    for p in args.images:
        files += sorted(image_filenames_generator(directory=[p], verbose=False)()) if os.path.isdir(p) else [p]
    if not files:
        ap.error("no image files")
    channels = 3 if module.model_hydra is None else int(module.model_hydra.desc.in_channels)      # "nlm" has no model: colour
    size = None if args.size is None else tuple(args.size)
    batches = [np.asarray(bf.load_image(path=f, image_size=size, num_channels=channels, expand_dims=True, normalize=False), np.uint8)
               for f in files]
    report = bf.evaluate(module, batches, noise_std=args.noise_std, seed=args.seed, filter_size=args.filter_size)
    print(f"{args.model}: {len(files)} images")
    print(M.format_report(report))
    if args.json_path:
        with open(args.json_path, "w") as f:
            json.dump(M.json_safe({"model": args.model, "images": files, "seed": args.seed, "levels": report}), f, indent=1, allow_nan=False)
    return report


if __name__ == "__main__":
    main()
