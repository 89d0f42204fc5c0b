"""Estimate the mean squared error and PSNR of a blind denoiser on image files that are ALREADY noisy and have no clean counterpart,
with Stein's unbiased risk estimate (blind_image_denoising_amd.evaluate_blind_risk): per frame the noise standard
deviation that entered the estimate, the estimated MSE and PSNR of what the network returns against the clean frame nobody has,
the divergence per sample, and the share of saturated samples (those violate the assumptions of the estimate).  It reads only the
files it is given and adds no noise.

    python tools/evaluate_risk.py unet_laplacian_v5.6 photos/ --probes 2 --json report.json

MODEL is a registry name (blind_image_denoising_amd.models) or a model directory; IMAGES are files or directories.  Every image is
its own batch, so frames of different sizes can be mixed; --size H W resizes them all and evaluates them as one batch.  --sigma
gives the noise standard deviation in grey levels instead of estimating it (--method).  --self-ensemble d4 | flips scores the
self-ensemble of the model.  With --json and no path (or "-") the report is printed as strict JSON instead of the table."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import blind_image_denoising_amd as bf                     # noqa: E402
from blind_image_denoising_amd import metrics as M          # noqa: E402
from blind_image_denoising_amd import risk as RK            # noqa: E402
from blind_image_denoising_amd.file_operations import image_filenames_generator      # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("model")
    ap.add_argument("images", nargs="+")
    ap.add_argument("--method", choices=RK.METHODS, default="mad")
    ap.add_argument("--sigma", type=float, default=None, help="noise standard deviation in grey levels (default: estimated per frame)")
    ap.add_argument("--probes", type=int, default=1, help=f"Monte-Carlo probes per frame, 1..{RK.MAX_PROBES}")
    ap.add_argument("--amplitude", type=int, default=1, help=f"probe amplitude in grey levels, 1..{RK.MAX_AMPLITUDE}")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--self-ensemble", choices=("d4", "flips"), default=None)
    ap.add_argument("--size", type=int, nargs=2, metavar=("H", "W"), default=None)
    ap.add_argument("--json", dest="json_path", nargs="?", const="-", default=None,
                    help="write the report as strict JSON to this file; without a file name, print it instead of the table")
    args = ap.parse_args(argv)
    module = bf.load_model(args.model, self_ensemble=args.self_ensemble)
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
    report = bf.evaluate_blind_risk(module, batches, sigma=args.sigma, method=args.method, probes=args.probes,
                                    amplitude=args.amplitude, seed=args.seed)
    document = M.json_safe({"model": args.model, "self_ensemble": args.self_ensemble, "files": files, **report})
    if args.json_path == "-":
        print(json.dumps(document, indent=1, allow_nan=False))
        return report
    print(f"{args.model}{'' if args.self_ensemble is None else ' x ' + args.self_ensemble}: {len(files)} images")
    print(RK.format_risk_report(report))
    if args.json_path:
        with open(args.json_path, "w") as f:
            json.dump(document, f, indent=1, allow_nan=False)
    return report


if __name__ == "__main__":
    main()
