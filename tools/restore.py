"""Inpaint, demosaic or up-sample a folder of images with a denoiser as the prior (blind_image_denoising_amd.restore).

    python tools/restore.py unet_laplacian_v5.6 photos/ restored/ --drop 0.3 --beta 1
    python tools/restore.py MODEL_DIR small/ large/ --upscale 2 --samples 3

MODEL is a registry name (blind_image_denoising_amd.models) or a model directory; IN_DIR is walked for image files, and every
result is written as PNG to the same relative path below OUT_DIR (`name_k.png` for sample k with --samples K > 1).  One of:
  --mask MASK.png   a grey image of the frames' size, non-zero = measured; the frames' pixels under its zeros are ignored
  --drop RATE       for demonstration: a random share RATE of the pixels of every (complete) frame is dropped, then restored
  --bayer           for demonstration: every (complete) frame is reduced to its RGGB mosaic, then demosaicked
  --upscale S       the frames are the low-resolution images: the result is S times as large, its S x S block means are the frame
--beta 1 is the deterministic variant (several times fewer iterations); the default 0.01 draws samples.  The model's float call
runs at the frame's own size, which it must accept (restore.py's header lists what the shipped models take).  One line per file:
size, iterations per sample, sigma at the end, whether every sample converged, milliseconds (uploads and downloads included)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import blind_image_denoising_amd as bf                     # noqa: E402
from blind_image_denoising_amd.file_operations import image_filenames_generator      # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("model", metavar="MODEL")
    ap.add_argument("in_dir", metavar="IN_DIR")
    ap.add_argument("out_dir", metavar="OUT_DIR")
    how = ap.add_mutually_exclusive_group(required=True)
    how.add_argument("--mask", metavar="MASK.png")
    how.add_argument("--drop", type=float, metavar="RATE")
    how.add_argument("--bayer", action="store_true")
    how.add_argument("--upscale", type=int, metavar="S")
    ap.add_argument("--beta", type=float, default=0.01)
    ap.add_argument("--samples", type=int, default=1, metavar="K")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sigma-0", type=float, default=255.0)
    ap.add_argument("--sigma-l", type=float, default=2.55)
    ap.add_argument("--h0", type=float, default=0.01)
    ap.add_argument("--max-iterations", type=int, default=2000)
    args = ap.parse_args(argv)
    if args.drop is not None and not 0.0 <= args.drop < 1.0:
        ap.error("--drop takes a rate in [0, 1)")
    from PIL import Image                                    # the library load_image decodes with
    if not os.path.isdir(args.in_dir):
        ap.error(f"{args.in_dir} is not a directory")
    files = sorted(image_filenames_generator(directory=[args.in_dir], verbose=False)())
    if not files:
        ap.error("no image files")
    module = bf.load_model(args.model)
    channels = int(getattr(module.model_hydra, "desc", module.model_hydra).in_channels)
    if args.bayer and channels != 3:
        ap.error("--bayer needs a model of three channels")
    fixed = None if args.mask is None else (np.asarray(Image.open(args.mask).convert("L")) != 0).astype(np.uint8)[None, :, :, None]
    settings = dict(beta=args.beta, samples=args.samples, seed=args.seed, sigma_0=args.sigma_0, sigma_l=args.sigma_l, h0=args.h0,
                    max_iterations=args.max_iterations)
    written = []
    for index, path in enumerate(files):
        frame = np.asarray(bf.load_image(path=path, num_channels=channels, expand_dims=True, normalize=False), np.uint8)
        _, H, W, _ = frame.shape
        start = time.perf_counter()
        if args.upscale is not None:
            result = bf.super_resolve(module, frame, args.upscale, **settings)
        else:
            if fixed is not None:
                if fixed.shape[1:3] != (H, W):
                    ap.error(f"{args.mask} is {fixed.shape[1]} x {fixed.shape[2]}, {path} is {H} x {W}")
                mask = fixed
            elif args.bayer:
                mask = bf.bayer_mask(1, H, W)
            else:
                keep = np.random.default_rng([args.seed, index]).random((1, H, W, 1)) >= args.drop
                mask = keep.astype(np.uint8)
            result = bf.inpaint(module, frame, mask, **settings)
        ms = (time.perf_counter() - start) * 1e3
        relative = os.path.relpath(path, args.in_dir)
        stem = os.path.splitext(relative)[0]
        for k, image in enumerate(result.image):
            target = os.path.join(args.out_dir, stem + (f"_{k}" if args.samples > 1 else "") + ".png")
            os.makedirs(os.path.dirname(target) or ".", exist_ok=True)
            Image.fromarray(image[:, :, 0] if image.shape[-1] == 1 else image).save(target)
            written.append(target)
        print(f"{relative}: {H} x {W} x {channels} -> {result.image.shape[1]} x {result.image.shape[2]}, iterations "
              f"{result.iterations.tolist()}, sigma {np.round(result.sigma, 2).tolist()}, "
              f"{'converged' if result.converged.all() else 'NOT converged'}, {ms:.1f} ms")
    return written


if __name__ == "__main__":
    main()
