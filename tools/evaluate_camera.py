"""What variance stabilisation is worth for a denoiser on camera noise (blind_image_denoising_amd.evaluate_camera):
every CLEAN frame of a folder gets synthetic camera noise of a known gain and read sigma (var = gain x + read_sigma^2), and PSNR,
SSIM and MAE against the clean frame are reported for the noisy frame, the model applied directly, the model between the
variance-stabilising transform and its exact unbiased inverse with the known parameters, and the same with the frame's own fit
(which is also printed).

    python tools/evaluate_camera.py photos/ --model unet_laplacian_v5.6 --gain 2 --read-sigma 2 --json report.json

DIR is a directory (or a single file) of clean frames; MODEL is a registry name (blind_image_denoising_amd.models) or a model
directory.  Every image is its own batch, so frames of different sizes can be mixed; --size H W resizes them all and evaluates them
as one batch.  --self-ensemble d4 | flips evaluates the self-ensemble of the model.  With --json and no path (or "-") the report is
printed as strict JSON instead of the table."""
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
    ap.add_argument("dir", metavar="DIR")
    ap.add_argument("--model", default="unet_laplacian_v5.6")
    ap.add_argument("--gain", type=float, default=2.0, help="grey levels per electron, 0..64")
    ap.add_argument("--read-sigma", type=float, default=2.0, help="read noise standard deviation in grey levels")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--self-ensemble", choices=("d4", "flips"), default=None)
    ap.add_argument("--size", type=int, nargs=2, metavar=("H", "W"), default=None)
    ap.add_argument("--json", dest="json_path", nargs="?", const="-", default=None,
                    help="write the report as strict JSON to this file; without a file name, print it instead of the table")
    args = ap.parse_args(argv)
    module = bf.load_model(args.model, self_ensemble=args.self_ensemble)
    channels = 3 if module.model_hydra is None else int(module.model_hydra.desc.in_channels)      # "nlm" has no model: colour
    files = sorted(image_filenames_generator(directory=[args.dir], verbose=False)()) if os.path.isdir(args.dir) else [args.dir]
    if not files:
        ap.error("no image files")
    size = None if args.size is None else tuple(args.size)
    batches = [np.asarray(bf.load_image(path=f, image_size=size, num_channels=channels, expand_dims=True, normalize=False), np.uint8)
               for f in files]
    if size is not None:
        batches = [np.concatenate(batches)]
    report = bf.evaluate_camera(module, batches, args.gain, args.read_sigma, seed=args.seed)
    document = M.json_safe({"model": args.model, "self_ensemble": args.self_ensemble, "files": files, **report})
    if args.json_path == "-":
        print(json.dumps(document, indent=1, allow_nan=False))
        return report
    print(f"{args.model}{'' if args.self_ensemble is None else ' x ' + args.self_ensemble}: {len(files)} images")
    print(bf.format_camera_report(report))
    if args.json_path:
        with open(args.json_path, "w") as f:
            json.dump(document, f, indent=1, allow_nan=False)
    return report


if __name__ == "__main__":
    main()
