"""What BM3D costs on the GPU: HIP-event times after a warm-up, the median over windows of back-to-back calls.
  step_one / step_two   bf_op_bm3d_step alone (csrc/bm3d.hip; the hard threshold, and the Wiener step on the first's result)
  finish                bf_op_bm3d_finish alone, uint8 out
  bm3d                  the whole call: two steps and two finishes
  nlm                   bf_op_nlm (patch 1, search 10) on the same batch
  unet_laplacian_v5_6   one call of the network on the same batch
all timed in alternating windows of one process, so that a drift of the machine hits all of them.  Sizes: 32 x 256 x 256 x 3 and
1 x 2048 x 2048 x 3 at search 12, step 4; sigma 20 on noise over a smooth ramp.  `flat` is the same on a constant frame, where
every group holds 16 blocks at distance 0: the bytes of its 64-bit atomic adds are known exactly (reference blocks x 16 x 64 x
(C + 1) x 8).  Run once with the library as built and once with the timing variant that skips the aggregation

    tools/ablate_unit.sh bm3d BM3D_ABLATE 1
    BFCNN_HIP_LIB=blind_image_denoising_amd/lib/variants/libbfcnn_hip_BM3D_ABLATE1.so python tools/exp/bm3d_bench.py --no-quality

the difference of the step times is what the aggregation costs, and the flat frame's bytes over that difference the rate of the
atomics.  With tests/golden/lena.jpg in place the PSNR table of the crops of tests/test_bm3d.py is recorded too.  One JSON document
on stdout and, with --out, in that file.

    python tools/exp/bm3d_bench.py --out bm3d_bench.json"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import _native as N
from nlm_bench import alternate

SIZES = ((32, 256, 256, 3), (1, 2048, 2048, 3))                     # B, H, W, C
SEARCH, STEP, SIGMA = 12, 4, 20.0


def reference_blocks(n: int, step: int) -> int:
    return (n - 8) // step + 1 + (1 if (n - 8) % step else 0)


def size(B, H, W, C, flat, unet, args):
    rng = np.random.default_rng(B + H)
    if flat:
        x = torch.full((B, H, W, C), 128, dtype=torch.uint8, device="cuda")
    else:
        ramp = 40.0 + 160.0 * (np.add.outer(np.arange(H), np.arange(W)) / float(H + W))[None, :, :, None]
        x = torch.from_numpy(np.clip(np.rint(ramp + rng.normal(0.0, SIGMA, (B, H, W, C))), 0, 255).astype(np.uint8)).cuda()
    sigma = torch.full((B,), SIGMA, dtype=torch.float64, device="cuda")
    params, nlm_params = bf.bm3d_params(sigma, C), bf.nlm_params(sigma, C, 1, 0.55)
    basic = bf.bm3d(x, params, SEARCH, STEP, wiener=False)
    acc = torch.empty((B, H, W, C + 1), dtype=torch.int64, device="cuda")
    out = torch.empty_like(x)
    stream = N.stream_ptr(x)

    def step(guide, wiener):
        return lambda: N.call("bf_op_bm3d_step", N.ptr(x), N.ptr(guide), N.ptr(params), B, H, W, C, SEARCH, STEP, wiener, N.ptr(acc), stream)
    fns = {"step_one": step(x, 0), "step_two": step(basic, 1),
           "finish": lambda: N.call("bf_op_bm3d_finish", N.ptr(acc), B, H, W, C, N.ptr(out), 1, N.ptr(None), stream),
           "bm3d": lambda: bf.bm3d(x, params, SEARCH, STEP)}
    if not flat:
        fns["nlm"] = lambda: bf.nlm(x, nlm_params, 1, 10)
        if unet is not None:
            fns["unet_laplacian_v5_6"] = lambda: unet(x)
    fns["step_one"]()                                                # the finish needs a filled accumulator: den >= 1
    t = alternate(fns, args.warmup, {name: args.reps for name in fns}, args.rounds)
    groups = B * reference_blocks(H, STEP) * reference_blocks(W, STEP)
    return {"shape": [B, H, W, C], "search": SEARCH, "step": STEP, "flat": flat, **t, "reference_blocks": groups,
            "atomic_bytes_at_16_blocks_per_group": groups * 16 * 64 * (C + 1) * 8}


def psnr(a, b) -> float:
    return float(10.0 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def quality(path: str):
    """the crops and the noise of tests/test_bm3d.py (default_rng(0), rounded and clipped): PSNR in dB"""
    from PIL import Image
    lena = np.asarray(Image.open(path).convert("RGB"), np.uint8)
    rows = []
    for lo, hi, sigma, channels in ((192, 320, 10.0, slice(0, 3)), (192, 320, 20.0, slice(0, 3)), (192, 320, 30.0, slice(0, 3)),
                                    (128, 384, 20.0, slice(0, 3)), (192, 320, 20.0, slice(1, 2))):
        clean = lena[lo:hi, lo:hi][None]
        noisy = np.clip(np.rint(clean + np.random.default_rng(0).normal(0.0, sigma, clean.shape)), 0, 255).astype(np.uint8)
        clean, noisy = clean[..., channels], noisy[..., channels]
        C = clean.shape[-1]
        level = torch.tensor([sigma], dtype=torch.float64, device="cuda")
        params = bf.bm3d_params(level, C)
        rows.append({"crop": [lo, hi], "sigma": sigma, "channels": C, "noisy": psnr(noisy, clean),
                     "nlm": psnr(bf.nlm(noisy, bf.nlm_params(level, C, 1, 0.55), 1, 10), clean),
                     "first_step": psnr(bf.bm3d(noisy, params, wiener=False), clean), "both_steps": psnr(bf.bm3d(noisy, params), clean)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bm3d_bench needs the GPU: nothing here can be measured without one")
    torch.cuda.set_device(0)
    unet = bf.load_model("unet_laplacian_v5.6", device="cuda:0") if "unet_laplacian_v5.6" in bf.models else None
    doc = {"device": torch.cuda.get_device_name(0), "library": str(N.LIB_PATH),
           "sizes": [size(*s, flat, unet, args) for s in SIZES for flat in (False, True)]}
    lena = os.path.join(ROOT, "tests", "golden", "lena.jpg")
    if not args.no_quality and os.path.isfile(lena):
        doc["psnr_db"] = quality(lena)
    text = json.dumps(doc, indent=2)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
