"""Write degraded copies of a folder of images, on the GPU (blind_image_denoising_amd.degrade): Gaussian blur, quantisation, a JPEG
round trip and dropped pixels, in the order the training pipeline applies them.  Every output is a PNG, so the JPEG artefacts in
it are exactly the ones the kernel made.

    python tools/degrade.py photos/ degraded/ --jpeg 20
    python tools/degrade.py photos/ degraded/ --blur 1.5 --step 8 --drop 0.1 --seed 3

IN_DIR is a directory (or a single file).  Every image is its own batch, so frames of different sizes can be mixed."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import blind_image_denoising_amd as bf                     # noqa: E402
from blind_image_denoising_amd.file_operations import image_filenames_generator      # noqa: E402


def degrade(image: np.ndarray, jpeg=None, blur=None, step=None, drop=None, subsampling="420", seed=0) -> np.ndarray:
    """uint8 [1,H,W,C] -> uint8 [1,H,W,C]: the stages that are not None"""
    import torch
    x = torch.from_numpy(np.ascontiguousarray(image)).cuda()
    if blur is not None:
        x = bf.degrade_blur(x, blur)
    if step is not None:
        x = bf.degrade_pointwise(x, step)
    if jpeg is not None:
        x = bf.degrade_jpeg(x, jpeg, subsampling)
    if drop is not None:
        x = bf.degrade_pointwise(x, 1, drop, seed)
    return x.to(torch.uint8).cpu().numpy()                 # the kernels' outputs are integers in 0..255


def main(argv=None):
    from PIL import Image
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("in_dir", metavar="IN_DIR")
    ap.add_argument("out_dir", metavar="OUT_DIR")
    ap.add_argument("--jpeg", type=int, metavar="Q", help="JPEG quality 1..100")
    ap.add_argument("--subsampling", choices=("420", "444"), default="420")
    ap.add_argument("--blur", type=float, metavar="S", help="Gaussian sigma 0..4")
    ap.add_argument("--step", type=int, metavar="N", help="quantisation step 1..255")
    ap.add_argument("--drop", type=float, metavar="R", help="share of dropped pixels 0..0.9")
    ap.add_argument("--channels", type=int, choices=(1, 3), default=3)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    if args.jpeg is None and args.blur is None and args.step is None and args.drop is None:
        ap.error("nothing to do: give at least one of --jpeg, --blur, --step, --drop")
    files = sorted(image_filenames_generator(directory=[args.in_dir], verbose=False)()) if os.path.isdir(args.in_dir) else [args.in_dir]
    if not files:
        ap.error("no image files")
    os.makedirs(args.out_dir, exist_ok=True)
    written = []
    for k, f in enumerate(files):
        image = np.asarray(bf.load_image(path=f, image_size=None, num_channels=args.channels, expand_dims=True, normalize=False), np.uint8)
        out = degrade(image, args.jpeg, args.blur, args.step, args.drop, args.subsampling, args.seed + k)[0]
        path = os.path.join(args.out_dir, os.path.splitext(os.path.basename(f))[0] + ".png")
        Image.fromarray(out[..., 0] if out.shape[-1] == 1 else out).save(path)
        mse = np.mean((out.astype(np.float64) - image[0]) ** 2)
        print(f"{os.path.basename(f):<40.40} -> {path}  PSNR to the input {10 * np.log10(255.0 ** 2 / mse) if mse else float('inf'):.2f} dB")
        written.append(path)
    return written


if __name__ == "__main__":
    main()
