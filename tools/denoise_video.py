"""Denoise the frames of a folder as one video stream (blind_image_denoising_amd.VideoDenoiserModule).

    python tools/denoise_video.py unet_laplacian_v5.6 frames/ denoised/ --n-max 8 --tile 256

MODEL is a registry name (blind_image_denoising_amd.models), a model directory, "nlm" or "bm3d" (non-local means, BM3D: no weights) or "none" (the
temporal filter alone).  The image files directly in IN_DIR are the frames, in name order; all of them must have the same size.
Every frame is filtered recursively along the motion against what the stream has accumulated (up to --n-max frames per pixel),
then denoised, tile by tile with --tile; the result is written to OUT_DIR under the frame's name as PNG.  --sigma fixes the noise
level the thresholds are made from (default: estimated from every frame).  One line per frame: the mean number of frames in a
pixel, milliseconds (the call on the GPU with the upload and the download, without the file I/O)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import blind_image_denoising_amd as bf                     # noqa: E402
from blind_image_denoising_amd.file_operations import image_filenames_generator      # noqa: E402


def find_frames(in_dir: str) -> list:
    """the image files directly in `in_dir`, in name order"""
    files = [p for p in image_filenames_generator(directory=[in_dir], verbose=False)()
             if os.path.dirname(os.path.abspath(p)) == os.path.abspath(in_dir)]
    return sorted(files, key=os.path.basename)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("model", metavar="MODEL")
    ap.add_argument("in_dir", metavar="IN_DIR")
    ap.add_argument("out_dir", metavar="OUT_DIR")
    ap.add_argument("--n-max", type=int, default=8, help="frames a pixel accumulates at the most (1..64)")
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--search", type=int, default=4)
    ap.add_argument("--sigma", type=float, default=None)
    ap.add_argument("--tile", type=int, default=None, help="denoise the filtered frame as overlapping tiles of this size")
    ap.add_argument("--tile-batch", type=int, default=16)
    args = ap.parse_args(argv)
    from PIL import Image                                    # the library load_image decodes with
    if not os.path.isdir(args.in_dir):
        ap.error(f"{args.in_dir} is not a directory")
    files = find_frames(args.in_dir)
    if not files:
        ap.error("no image files")
    try:
        settings = bf.video_settings({"n_max": args.n_max, "levels": args.levels, "search": args.search, "sigma": args.sigma})
    except ValueError as e:
        ap.error(str(e))
    inner, channels = None, 3
    if args.model != "none":
        tiled = None if args.tile is None else {"tile": args.tile, "tile_batch": args.tile_batch}
        inner = bf.load_model(args.model, tiled=tiled)
        channels = 3 if inner.model_hydra is None else int(inner.model_hydra.desc.in_channels)      # "nlm" has no model: colour
    module = bf.VideoDenoiserModule(inner, **settings)
    os.makedirs(args.out_dir, exist_ok=True)
    written, shape = [], None
    for path in files:
        frame = np.asarray(bf.load_image(path=path, num_channels=channels, expand_dims=False, normalize=False), np.uint8)
        if shape is not None and frame.shape != shape:
            ap.error(f"{path} is {frame.shape[0]} x {frame.shape[1]}, the stream's frames are {shape[0]} x {shape[1]}: "
                     f"all frames of a stream have one size")
        shape = frame.shape
        start = time.perf_counter()
        out = module(frame[None])                            # NumPy in, NumPy out: the call ends with the download
        ms = (time.perf_counter() - start) * 1e3
        target = os.path.join(args.out_dir, os.path.splitext(os.path.basename(path))[0] + ".png")
        Image.fromarray(out[0, :, :, 0] if out.shape[-1] == 1 else out[0]).save(target)
        written.append(target)
        print(f"{os.path.basename(path)}: {shape[0]} x {shape[1]} x {shape[2]}, "
              f"{float(module.last_counts.cpu().numpy().mean()) / 256.0:.2f} frames per pixel, {ms:.1f} ms")
    return written


if __name__ == "__main__":
    main()
