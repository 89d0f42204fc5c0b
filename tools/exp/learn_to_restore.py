"""Does the engine learn to undo JPEG?  Trains the canonical resnet 1x6 from scratch on crops of tests/golden/lena.jpg whose only
corruption is the JPEG round trip of the `dataset.degradations` section (quality 10..40, every image, no noise), through the public
API as tools/exp/learn_to_denoise.py does, and prints the PSNR of the held-out quarter degraded and restored."""
import pathlib, sys, tempfile, time
import numpy as np
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[2]))
import blind_image_denoising_amd as bf
from oracle import bfcnn_oracle as O
from PIL import Image


def psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def main(layers=6, epochs=30, batch=16, crop=64, qualities=(10, 20, 40)):
    import torch
    lena = Image.open(pathlib.Path(__file__).resolve().parents[2] / "tests" / "golden" / "lena.jpg")
    tmp = pathlib.Path(tempfile.mkdtemp())
    (tmp / "img").mkdir()
    lena.crop((0, 0, 512, 384)).save(tmp / "img" / "train.png")                    # the top three quarters train, the rest is held out
    held = np.asarray(lena.convert("RGB"))[384:512, 0:512][None]
    cfg = O.canonical_config(no_layers=layers)
    cfg["train"].update({"epochs": epochs, "gpu_batches_per_step": 1})
    cfg["train"]["optimizer"]["schedule"]["config"]["learning_rate"] = 2e-3
    cfg["loss"] = {"hinge": 0.0, "cutoff": 255.0, "mae_multiplier": 1.0, "ssim_multiplier": 0.0, "regularization": 0.01}
    cfg["dataset"] = {"batch_size": batch, "color_mode": "rgb", "no_crops_per_image": 64 * batch, "value_range": [0, 255], "clip_value": True,
                      "round_values": True, "random_up_down": True, "random_left_right": True, "input_shape": [crop, crop, 3],
                      "inputs": [{"directory": str(tmp / "img")}],
                      "degradations": {"jpeg": {"quality": [10, 40], "subsampling": "420", "probability": 1.0}}}
    t0 = time.time()
    model, hist = bf.train_loop(cfg, str(tmp / "run"))
    dt = time.time() - t0
    print(f"steps {len(hist)}  {dt:.1f} s  loss {hist[0]:.2f} -> {np.mean(hist[-20:]):.2f}")
    restore = bf.load_model(str(tmp / "run" / "final"))
    results = []
    for q in qualities:
        degraded = bf.degrade_jpeg(torch.from_numpy(held).cuda(), q, "420").to(torch.uint8).cpu().numpy()
        restored = restore(degraded)
        results.append((q, psnr(held, degraded), psnr(held, restored)))
        print(f"quality {q}: PSNR degraded {results[-1][1]:.2f} dB -> restored {results[-1][2]:.2f} dB")
    return results


if __name__ == "__main__":
    main()
