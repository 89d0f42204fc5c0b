"""Merge and denoise bursts, each at its own size (blind_image_denoising_amd.BurstDenoiserModule).

    python tools/denoise_burst.py unet_laplacian_v5.6 bursts/ merged/ --tile 256

MODEL is a registry name (blind_image_denoising_amd.models) or a model directory.  A burst is a sub-folder of IN_DIR (its image
files in name order), or the image files directly in IN_DIR that share a name stem (the name without its trailing digits and
separators: shot_01.png, shot_02.png -> shot); 1 to 16 frames of one size.  The frames are aligned to frame --reference
("middle" by default), merged along the alignment and the merged frame is denoised, tile by tile with --tile; every result is
written to OUT_DIR/<burst>.png.  --sigma fixes the noise level the merge thresholds are made from (default: estimated from the
reference frame); --merge-only skips the denoiser.  One line per burst: frames, size, the mean number of frames merged into a
pixel, milliseconds (the call on the GPU with the upload and the download, without the file I/O)."""
import argparse
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import blind_image_denoising_amd as bf                     # noqa: E402
from blind_image_denoising_amd.file_operations import image_filenames_generator      # noqa: E402


def find_bursts(in_dir: str) -> dict:
    """{burst name: its files in name order}"""
    bursts = {}
    for entry in sorted(os.listdir(in_dir)):
        path = os.path.join(in_dir, entry)
        if os.path.isdir(path):
            files = sorted(image_filenames_generator(directory=[path], verbose=False)())
            if files:
                bursts[entry] = files
    for path in sorted(image_filenames_generator(directory=[in_dir], verbose=False)()):
        if os.path.dirname(os.path.abspath(path)) != os.path.abspath(in_dir):
            continue                                          # inside a sub-folder: taken above
        stem = os.path.splitext(os.path.basename(path))[0]
        bursts.setdefault(re.sub(r"[\s._-]*\d+$", "", stem) or stem, []).append(path)
    return bursts


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("model", metavar="MODEL")
    ap.add_argument("in_dir", metavar="IN_DIR")
    ap.add_argument("out_dir", metavar="OUT_DIR")
    ap.add_argument("--tile", type=int, default=None, help="denoise the merged frame as overlapping tiles of this size")
    ap.add_argument("--tile-batch", type=int, default=16)
    ap.add_argument("--reference", default="middle", help='index of the frame the others are aligned to, or "middle"')
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--search", type=int, default=4)
    ap.add_argument("--sigma", type=float, default=None)
    ap.add_argument("--merge-only", action="store_true")
    args = ap.parse_args(argv)
    from PIL import Image                                    # the library load_image decodes with
    if not os.path.isdir(args.in_dir):
        ap.error(f"{args.in_dir} is not a directory")
    bursts = find_bursts(args.in_dir)
    if not bursts:
        ap.error("no image files")
    if args.reference != "middle" and not args.reference.isdigit():
        ap.error('--reference is an index or "middle"')
    inner, channels = None, 3
    if not args.merge_only:
        tiled = None if args.tile is None else {"tile": args.tile, "tile_batch": args.tile_batch}
        inner = bf.load_model(args.model, tiled=tiled)
        channels = 3 if inner.model_hydra is None else int(inner.model_hydra.desc.in_channels)      # "nlm" has no model: colour
    os.makedirs(args.out_dir, exist_ok=True)
    written = []
    for name, files in bursts.items():
        frames = [np.asarray(bf.load_image(path=p, num_channels=channels, expand_dims=False, normalize=False), np.uint8) for p in files]
        if len({f.shape for f in frames}) != 1 or not 1 <= len(frames) <= bf.burst.MAX_FRAMES:
            print(f"{name}: skipped, {len(frames)} frames of sizes {sorted({f.shape for f in frames})} "
                  f"(1..{bf.burst.MAX_FRAMES} frames of one size make a burst)")
            continue
        reference = len(frames) // 2 if args.reference == "middle" else int(args.reference)
        module = bf.BurstDenoiserModule(inner, reference=min(reference, len(frames) - 1), levels=args.levels, search=args.search,
                                        sigma=args.sigma)
        batch = np.stack(frames)[None]
        start = time.perf_counter()
        out = module(batch)                                  # NumPy in, NumPy out: the call ends with the download
        ms = (time.perf_counter() - start) * 1e3
        target = os.path.join(args.out_dir, name + ".png")
        Image.fromarray(out[0, :, :, 0] if out.shape[-1] == 1 else out[0]).save(target)
        written.append(target)
        merged = "" if module.last_counts is None else f", {float(module.last_counts[..., 0].double().mean()) / 256.0:.2f} frames per pixel"
        print(f"{name}: {len(frames)} frames of {batch.shape[2]} x {batch.shape[3]} x {batch.shape[4]}, reference {module.reference}"
              f"{merged}, {ms:.1f} ms")
    return written


if __name__ == "__main__":
    main()
