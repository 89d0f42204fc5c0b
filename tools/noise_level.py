"""Fit the noise level function var(y | x) = gain * x + offset of every frame in a folder, on the GPU
(blind_image_denoising_amd.noise_level_function): per image and channel the fitted gain and offset, the noise standard deviation
they give at the grey levels 64, 128 and 192, and the share of the 2x2 cells excluded because they hold a 0 or a 255.  It reads
only the files it is given and adds no noise.

    python tools/noise_level.py photos/ --channels 3 --min-cells 64

DIR is a directory (or a single file).  Every image is its own batch, so frames of different sizes can be mixed."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import blind_image_denoising_amd as bf                     # noqa: E402
from blind_image_denoising_amd.file_operations import image_filenames_generator      # noqa: E402

AT = (64.0, 128.0, 192.0)


def format_rows(name: str, nlf) -> list:
    """one line per channel of ONE image's NoiseLevelFunction (NumPy fields, B = 1)"""
    sigmas = [nlf.sigma_at(x)[0] for x in AT]
    return [f"{name if c == 0 else '':<40.40} {c:2d}  {nlf.gain[0, c]:8.4f}  {nlf.offset[0, c]:9.3f}  "
            + "  ".join(f"{s[c]:7.3f}" for s in sigmas) + f"  {100.0 * nlf.excluded_fraction[0, c]:7.2f}%"
            for c in range(nlf.gain.shape[1])]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("dir", metavar="DIR")
    ap.add_argument("--channels", type=int, choices=(1, 3), default=3)
    ap.add_argument("--min-cells", type=int, default=64, help="a level enters the fit with at least this many 2x2 cells")
    args = ap.parse_args(argv)
    files = sorted(image_filenames_generator(directory=[args.dir], verbose=False)()) if os.path.isdir(args.dir) else [args.dir]
    if not files:
        ap.error("no image files")
    print(f"{'image':<40} ch      gain     offset  " + "  ".join(f"s({x:3.0f})" + " " for x in AT) + " excluded")
    fits = []
    for f in files:
        image = np.asarray(bf.load_image(path=f, image_size=None, num_channels=args.channels, expand_dims=True, normalize=False), np.uint8)
        nlf = bf.noise_level_function(image, min_cells=args.min_cells)
        fits.append(nlf)
        print("\n".join(format_rows(os.path.basename(f), nlf)))
    return fits


if __name__ == "__main__":
    main()
