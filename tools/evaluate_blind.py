"""Evaluate a blind denoiser on image files that are ALREADY noisy and have no clean counterpart: the noise standard deviation
estimated in each frame and in what the network returns for it, the root mean square of what the network removed, and the ratio of
that to the estimated noise (near 1 when the network removed what the estimator saw), measured on the GPU by
blind_image_denoising_amd.evaluate_blind.  It reads only the files it is given and adds no noise.

    python tools/evaluate_blind.py unet_laplacian_v5.6 photos/ --method mad --json report.json

MODEL is a registry name (blind_image_denoising_amd.models) or a model directory; IMAGES are files or directories.  Every image is
its own batch, so frames of different sizes can be mixed; --size H W resizes them all and evaluates them as one batch.  With --json
and no path (or "-") the report is printed as strict JSON instead of the table."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import blind_image_denoising_amd as bf                     # noqa: E402
from blind_image_denoising_amd import metrics as M          # noqa: E402
from blind_image_denoising_amd import noise_estimate as NE  # noqa: E402
from blind_image_denoising_amd.file_operations import image_filenames_generator      # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("model")
    ap.add_argument("images", nargs="+")
    ap.add_argument("--method", choices=NE.METHODS, default="mad")
    ap.add_argument("--size", type=int, nargs=2, metavar=("H", "W"), default=None)
    ap.add_argument("--json", dest="json_path", nargs="?", const="-", default=None,
                    help="write the report as strict JSON to this file; without a file name, print it instead of the table")
    args = ap.parse_args(argv)
    module = bf.load_model(args.model)
    channels = 3 if module.model_hydra is None else int(module.model_hydra.desc.in_channels)      # "nlm" has no model: colour
    files = []
    for p in args.images:
        files += sorted(image_filenames_generator(directory=[p], verbose=False)()) if os.path.isdir(p) else [p]
    if not files:
        ap.error("no image files")
    size = None if args.size is None else tuple(args.size)
    batches = [np.asarray(bf.load_image(path=f, image_size=size, num_channels=channels, expand_dims=True, normalize=False), np.uint8)
               for f in files]
    if size is not None:
        batches = [np.concatenate(batches)]
    report = bf.evaluate_blind(module, batches, method=args.method)
    document = M.json_safe({"model": args.model, "files": files, **report})
    if args.json_path == "-":
        print(json.dumps(document, indent=1, allow_nan=False))
        return report
    print(f"{args.model}: {len(files)} images")
    print(NE.format_blind_report(report))
    if args.json_path:
        with open(args.json_path, "w") as f:
            json.dump(document, f, indent=1, allow_nan=False)
    return report


if __name__ == "__main__":
    main()
