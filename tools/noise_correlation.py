"""How far the noise of every frame in a folder is correlated, on the GPU (blind_image_denoising_amd.noise_correlation; DESIGN.md
7.15): per image the curve sigma_s of the dilated Haar statistic for s = 1..--max-stride (root mean square over the channels),
the stride the rule picks (the smallest s with sigma_s >= threshold sigma_(s+1)) and sigma_white, the noise level a white-noise
estimator should have read; next to it what estimate_noise reads.  A flat curve is white noise; a curve that rises with s is noise
correlated over that many pixels (demosaiced, resized or filtered frames).  It reads only the files it is given and adds no noise.

    python tools/noise_correlation.py photos/ --channels 3 --max-stride 6

DIR is a directory (or a single file).  Every image is its own batch, so frames of different sizes can be mixed."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import blind_image_denoising_amd as bf                     # noqa: E402
from blind_image_denoising_amd.file_operations import image_filenames_generator      # noqa: E402


def format_row(name: str, found, mad: float) -> str:
    """one line of ONE image's NoiseCorrelation (NumPy fields, B = 1)"""
    return (f"{name:<40.40} " + " ".join(f"{v:7.3f}" for v in found.sigma[0]) + f"  {int(found.stride[0]):6d}  {found.sigma_white[0]:11.3f}"
            f"  {mad:9.3f}")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("dir", metavar="DIR")
    ap.add_argument("--channels", type=int, choices=(1, 3), default=3)
    ap.add_argument("--max-stride", type=int, default=6)
    ap.add_argument("--threshold", type=float, default=0.8)
    args = ap.parse_args(argv)
    files = sorted(image_filenames_generator(directory=[args.dir], verbose=False)()) if os.path.isdir(args.dir) else [args.dir]
    if not files:
        ap.error("no image files")
    print(f"{'image':<40} " + " ".join(f"  s = {s}" for s in range(1, args.max_stride + 1)) + "  stride  sigma_white  sigma_mad")
    found = []
    for f in files:
        image = np.asarray(bf.load_image(path=f, image_size=None, num_channels=args.channels, expand_dims=True, normalize=False), np.uint8)
        found.append(bf.noise_correlation(image, args.max_stride, args.threshold))
        print(format_row(os.path.basename(f), found[-1], float(bf.estimate_noise(image)[0])))
    return found


if __name__ == "__main__":
    main()
