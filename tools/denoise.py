"""Denoise a folder of images, each at its own size, tile by tile (blind_image_denoising_amd.TiledDenoiserModule).

    python tools/denoise.py unet_laplacian_v5.6 photos/ denoised/ --tile 256 --stabilise

MODEL is a registry name (blind_image_denoising_amd.models), a model directory, `nlm` or `bm3d` (non-local means, BM3D: no
network); IN_DIR is walked for image files, and every result is written to the same relative path below OUT_DIR (as PNG where the source format is lossy or has no writer).  Every frame
is cut into overlapping tiles of --tile pixels, the model runs on batches of --tile-batch tiles of one shape, and the results are
blended: --overlap and --margin default to what the model needs (its receptive radius where it has one).  --self-ensemble d4 |
flips averages the model over flips and rotations of every tile; --stabilise fits camera noise (variance = gain x + offset) on
the whole frame and runs the tiles between the variance-stabilising transform and its inverse; --pixel-shuffle [auto|N] runs the
sub-images of every N-th pixel of the frame (for noise that is correlated over a few pixels; auto measures N on the frame) and
--refine T adds the random-replacing second stage.  One line per file: size, tiles of the last denoiser call,
milliseconds (the call on the GPU with the upload and the download, without the file I/O)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import blind_image_denoising_amd as bf                     # noqa: E402
from blind_image_denoising_amd.file_operations import image_filenames_generator      # noqa: E402

_KEEP_FORMAT = (".png", ".bmp")                            # lossless and written by Pillow as they are; everything else -> .png


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("model", metavar="MODEL")
    ap.add_argument("in_dir", metavar="IN_DIR")
    ap.add_argument("out_dir", metavar="OUT_DIR")
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--overlap", type=int, default=None)
    ap.add_argument("--margin", type=int, default=None)
    ap.add_argument("--tile-batch", type=int, default=16)
    ap.add_argument("--self-ensemble", choices=("d4", "flips"), default=None)
    ap.add_argument("--stabilise", action="store_true")
    ap.add_argument("--pixel-shuffle", nargs="?", const="auto", default=None, metavar="auto|N",
                    help="for noise correlated over a few pixels: run the sub-images of every N-th pixel (auto: N from the frame)")
    ap.add_argument("--refine", type=int, default=0, metavar="T", help="with --pixel-shuffle: T random-replacing copies refine the result")
    args = ap.parse_args(argv)
    if args.refine and args.pixel_shuffle is None:
        ap.error("--refine needs --pixel-shuffle")
    shuffle = None
    if args.pixel_shuffle is not None:
        shuffle = {"stride": "auto" if args.pixel_shuffle == "auto" else int(args.pixel_shuffle), "refine": args.refine}
    from PIL import Image                                    # the library load_image decodes with
    if not os.path.isdir(args.in_dir):
        ap.error(f"{args.in_dir} is not a directory")
    files = sorted(image_filenames_generator(directory=[args.in_dir], verbose=False)())
    if not files:
        ap.error("no image files")
    module = bf.load_model(args.model, self_ensemble=args.self_ensemble, stabilise=True if args.stabilise else None,
                           tiled={"tile": args.tile, "overlap": args.overlap, "margin": args.margin, "tile_batch": args.tile_batch},
                           pixel_shuffle=shuffle)
    shuffled = (module._module if args.stabilise else module) if shuffle is not None else None
    tiled = shuffled._module if shuffled is not None else module._module if args.stabilise else module
    channels = 3 if module.model_hydra is None else int(module.model_hydra.desc.in_channels)      # "nlm" has no model: colour
    print(f"{args.model}: tile {tiled.tile}, overlap {tiled.overlap}, margin {tiled.margin}, {tiled.tile_batch} tiles per call"
          f"{'' if args.self_ensemble is None else ', self-ensemble ' + args.self_ensemble}{', stabilised' if args.stabilise else ''}"
          f"{'' if shuffled is None else f', pixel-shuffle {shuffled.stride}, refine {shuffled.refine}'}")
    written = []
    for path in files:
        frame = np.asarray(bf.load_image(path=path, num_channels=channels, expand_dims=True, normalize=False), np.uint8)
        start = time.perf_counter()
        out = module(frame)                                  # NumPy in, NumPy out: the call ends with the download
        ms = (time.perf_counter() - start) * 1e3
        relative = os.path.relpath(path, args.in_dir)
        stem, ext = os.path.splitext(relative)
        target = os.path.join(args.out_dir, relative if ext.lower() in _KEEP_FORMAT else stem + ".png")
        os.makedirs(os.path.dirname(target) or ".", exist_ok=True)
        Image.fromarray(out[0, :, :, 0] if out.shape[-1] == 1 else out[0]).save(target)
        written.append(target)
        print(f"{relative}: {frame.shape[1]} x {frame.shape[2]} x {frame.shape[3]}, {tiled.last_plan.tiles} tiles, "
              f"{'' if shuffled is None else f'stride {shuffled.last_stride}, '}{ms:.1f} ms")
    return written


if __name__ == "__main__":
    main()
