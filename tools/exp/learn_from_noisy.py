"""Does the engine learn from noisy images alone?  ONE noisy copy of the top three quarters of tests/golden/lena.jpg (sigma 20, rounded)
is written as a PNG; the canonical resnet 1x6 is trained from scratch on Neighbor2Neighbor pairs of its crops through the public API
(the directory pipeline without any noise option -> train_loop with `train.self_supervised`), and the result is judged on the held-out
bottom quarter + sigma 20 noise against its clean pixels, which the training never sees.  tests/test_gpu_neighbor.py runs the same
set-up; tools/exp/learn_to_denoise.py is its supervised counterpart.

    python tools/exp/learn_from_noisy.py [--seeds 7 8 9] [--gamma 0] [--epochs 16]"""
import argparse
import pathlib
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[2]))
import blind_image_denoising_amd as bf              # noqa: E402
from oracle import bfcnn_oracle as O                # noqa: E402
from PIL import Image                               # noqa: E402


def psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def mae(a, b):
    return np.abs(a.astype(np.float64) - b.astype(np.float64)).mean()


def config(directory, seed=7, gamma=0.0, ramp=True, epochs=16, layers=6, batch=16, crop=64, steps_per_epoch=64, validation=None):
    cfg = O.canonical_config(no_layers=layers)
    cfg["train"].update({"epochs": epochs, "gpu_batches_per_step": 1, "seed": seed,
                         "self_supervised": {"type": "neighbor2neighbor", "gamma": gamma, "ramp": ramp}})
    if validation is not None:
        cfg["train"]["self_supervised"]["validation"] = validation
    cfg["train"]["optimizer"]["schedule"]["config"]["learning_rate"] = 2e-3
    cfg["loss"] = {"hinge": 0.0, "cutoff": 255.0, "mae_multiplier": 1.0, "ssim_multiplier": 0.0, "regularization": 0.01}
    cfg["dataset"] = {"batch_size": batch, "color_mode": "rgb", "no_crops_per_image": steps_per_epoch * batch, "value_range": [0, 255],
                      "clip_value": True, "round_values": True, "random_up_down": True, "random_left_right": True, "input_shape": [crop, crop, 3], "inputs": [{"directory": str(directory)}]}
    return cfg


def noisy_u8(clean, sigma, seed):
    return np.clip(np.round(clean + np.random.default_rng(seed).normal(0, sigma, clean.shape)), 0, 255).astype(np.uint8)


def main(seed=7, gamma=0.0, epochs=16, sigma=20.0):
    lena = np.asarray(Image.open(pathlib.Path(__file__).resolve().parents[2] / "tests" / "golden" / "lena.jpg").convert("RGB"))
    tmp = pathlib.Path(tempfile.mkdtemp())
    (tmp / "img").mkdir()
    Image.fromarray(noisy_u8(lena[0:384], sigma, 1)).save(tmp / "img" / "noisy.png")     # the only image the loop is given
    held = lena[384:512][None]
    t0 = time.time()
    model, hist = bf.train_loop(config(tmp / "img", seed, gamma, epochs=epochs), str(tmp / "run"))
    dt = time.time() - t0
    noisy = noisy_u8(held, sigma, 0)
    den = bf.load_model(str(tmp / "run" / "final"))(noisy)
    print(f"seed {seed} gamma {gamma:g}: steps {len(hist)}  {dt:.1f} s  loss {hist[0]:.2f} -> {np.mean(hist[-20:]):.2f}   "
          f"PSNR noisy {psnr(held, noisy):.2f} dB -> denoised {psnr(held, den):.2f} dB (gain {psnr(held, den) - psnr(held, noisy):.2f})   "
          f"MAE {mae(held, noisy):.2f} -> {mae(held, den):.2f}", flush=True)
    return psnr(held, noisy), psnr(held, den)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seeds", type=int, nargs="+", default=[7, 8, 9])
    ap.add_argument("--gamma", type=float, default=0.0)
    ap.add_argument("--epochs", type=int, default=16)
    args = ap.parse_args()
    for s in args.seeds:
        main(s, args.gamma, args.epochs)
