"""What restoration with the denoiser's prior gives and costs on the GPU, on lena[128:384, 128:384].

Cases: 30 % of the pixels dropped, a 32 x 32 hole, the RGGB mosaic, x2 and x4 super-resolution.  Priors: the shipped
unet_laplacian_v5.6, and a resnet 1x6 trained here by the recipe of tools/exp/learn_to_denoise.py with `additional_noise` widened to
1 .. 255 (it trains on the top three quarters of the picture, which hold half of the crop).  Per (prior, beta in {0.01, 1}, case):
iterations, HIP-event time of the whole bf.restore call (the host reads every 16 iterations, as the algorithm does), PSNR on the
unmeasured samples against the mid-grey fill (against nearest up-sampling for super-resolution); `--repeats` runs, median and range.
Then, per prior: the PSNR at beta = 1 over a sweep of sigma_0 (is the prior usable from sigma_0 = 255, and if not, from where);
the share of an iteration spent in the update entries (bf_op_restore_direction + bf_op_restore_step) next to the denoiser call; and
the same update written with torch operators, in alternating windows.  One JSON document on stdout and, with --out, in that file.

    python tools/exp/restore_bench.py --out restore_bench.json"""
import argparse
import json
import os
import pathlib
import sys
import tempfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch

import blind_image_denoising_amd as bf
from oracle import bfcnn_oracle as O

RS = bf._restore


def psnr(a, b, where):
    e = (np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2
    return float(10 * np.log10(255.0 ** 2 / e[where].mean()))


def crop():
    from PIL import Image
    lena = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "lena.jpg")).convert("RGB"))
    return lena[128:384, 128:384][None]


def train_resnet(epochs: int):
    """learn_to_denoise.py's recipe, additional_noise 1 .. 255"""
    from PIL import Image
    lena = Image.open(os.path.join(ROOT, "tests", "golden", "lena.jpg"))
    tmp = pathlib.Path(tempfile.mkdtemp())
    (tmp / "img").mkdir()
    lena.crop((0, 0, 512, 384)).save(tmp / "img" / "train.png")
    cfg = O.canonical_config(no_layers=6)
    cfg["train"].update({"epochs": epochs, "gpu_batches_per_step": 1})
    cfg["train"]["optimizer"]["schedule"]["config"]["learning_rate"] = 2e-3
    cfg["loss"] = {"hinge": 0.0, "cutoff": 255.0, "mae_multiplier": 1.0, "ssim_multiplier": 0.0, "regularization": 0.01}
    cfg["dataset"] = {"batch_size": 16, "color_mode": "rgb", "no_crops_per_image": 64 * 16, "value_range": [0, 255], "clip_value": True,
                      "round_values": True, "random_up_down": True, "random_left_right": True, "input_shape": [64, 64, 3],
                      "additional_noise": [1.0, 255.0], "inputs": [{"directory": str(tmp / "img")}]}
    bf.train_loop(cfg, str(tmp / "run"))
    return bf.load_model(str(tmp / "run" / "final"))


def cases(clean):
    """{name: (constraint on the device, where quality is scored, the baseline image)}"""
    _, H, W, C = clean.shape
    rng = np.random.default_rng(0)
    out = {}
    masks = {"drop30": (rng.random((1, H, W, 1)) >= 0.3).astype(np.uint8), "hole32": np.ones((1, H, W, 1), np.uint8),
             "bayer": bf.bayer_mask(1, H, W)}
    masks["hole32"][:, 112:144, 112:144] = 0
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for name, m in masks.items():
        measured = np.broadcast_to(m != 0, clean.shape)
        out[name] = (bf.mask_constraint(dev(clean), dev(m)), ~measured, np.where(measured, clean, 127.5))
    for s in (2, 4):
        low = clean.astype(np.float64).reshape(1, H // s, s, W // s, s, C).mean(axis=(2, 4)).astype(np.float32)
        nearest = np.repeat(np.repeat(low, s, axis=1), s, axis=2)
        out[f"sr{s}"] = (bf.block_constraint(dev(low), s), np.ones(clean.shape, bool), nearest)
    return out


def timed_restore(module, con, **settings):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    result = bf.restore(module, con, cast_to_uint8=False, **settings)
    e1.record()
    torch.cuda.synchronize()
    return result, e0.elapsed_time(e1)


def quality_table(module, clean, args):
    rows = []
    for beta in (0.01, 1.0):
        for name, (con, where, base) in cases(clean).items():
            settings = dict(beta=beta, max_iterations=args.max_iterations, seed=args.seed)
            timed_restore(module, con, **dict(settings, max_iterations=32))           # warm-up: packing, workspaces, the status slots
            runs = [timed_restore(module, con, **settings) for _ in range(args.repeats)]
            ms = [t for _, t in runs]
            result = runs[0][0]
            rows.append({"case": name, "beta": beta, "iterations": int(result.iterations[0]), "converged": bool(result.converged[0]),
                         "sigma_end": float(result.sigma[0]), "ms_median": float(np.median(ms)), "ms_min": min(ms), "ms_max": max(ms),
                         "psnr": psnr(result.image.cpu().numpy(), clean, where), "psnr_baseline": psnr(base, clean, where)})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    return rows


def sigma_sweep(module, clean, args):
    rows = []
    for name in ("drop30", "sr2"):
        con, where, base = cases(clean)[name]
        for sigma_0 in (255.0, 128.0, 64.0, 32.0, 16.0):
            result, _ = timed_restore(module, con, beta=1.0, sigma_0=sigma_0, max_iterations=args.max_iterations, seed=args.seed)
            rows.append({"case": name, "sigma_0": sigma_0, "iterations": int(result.iterations[0]), "converged": bool(result.converged[0]),
                         "psnr": psnr(result.image.cpu().numpy(), clean, where), "psnr_baseline": psnr(base, clean, where)})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    return rows


def window_us(fn, reps: int) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def torch_update(y, D, m, a, h, beta, sigma_l, n):
    """one iteration's update with torch operators (mask constraint; the noise from torch.randn): what a user would otherwise write"""
    d = torch.where(m, a - y, D - y)
    sigma = (d.double() ** 2).sum(dim=(1, 2, 3)).div(n).sqrt()
    gamma = (((1.0 - beta * h) ** 2 - (1.0 - h) ** 2) ** 0.5 * sigma).float().view(-1, 1, 1, 1)
    moves = (sigma > sigma_l).view(-1, 1, 1, 1)
    y.copy_(torch.where(moves, y + h * d + gamma * torch.randn_like(y), y))
    return sigma


def update_cost(module, clean, args):
    """per iteration at 1 x 256 x 256 x 3, drop30: the two update entries, the denoiser call, the torch-operator update"""
    con, _, _ = cases(clean)["drop30"]
    call, _ = RS._float_denoiser(module, 3)
    B, H, W, C = con.shape
    n = H * W * C
    y = bf.restore_init(con, 255.0, args.seed)
    D = call(y)
    d, sumsq = bf.restore_direction(y, D, con)
    scratch, _ = RS.N.scratch("bf_op_restore", y.device, B, H, W, C)
    steps = torch.zeros(B, dtype=torch.int32, device="cuda")
    m, a = (con.mask != 0).expand(con.shape), con.anchor.float()
    out = {}
    for beta in (0.01, 1.0):
        def entries():
            RS._direction(y, D, con, d, sumsq, scratch)
            steps.zero_()                                                          # keeps the image moving: t = 1 every time
            RS._step(y, d, sumsq, steps, 1, 0.01, beta, 1e-6, args.seed, None, None)
        fns = {"update_entries": entries, "denoiser_call": lambda: call(y),
               "torch_update": lambda: torch_update(y, D, m, a, 0.01, beta, 1e-6, n)}
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                times[k].append(window_us(fn, args.reps))
        row = {k: {"median_us": float(np.median(t)), "min_us": min(t), "max_us": max(t)} for k, t in times.items()}
        up, den = row["update_entries"]["median_us"], row["denoiser_call"]["median_us"]
        row["update_share_of_iteration"] = up / (up + den)
        row["torch_over_entries"] = row["torch_update"]["median_us"] / up
        out[f"beta_{beta}"] = row
        y.copy_(bf.restore_init(con, 255.0, args.seed))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--max-iterations", type=int, default=2000)
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--priors", default="unet_laplacian_v5.6,resnet_1x6")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("restore_bench needs the GPU: nothing here can be measured without one")
    torch.cuda.set_device(0)
    clean = crop()
    doc = {"device": torch.cuda.get_device_name(0), "crop": "lena[128:384, 128:384]", "priors": {}}
    for prior in args.priors.split(","):
        module = train_resnet(args.epochs) if prior == "resnet_1x6" else bf.load_model(prior, device="cuda:0")
        doc["priors"][prior] = {"cases": quality_table(module, clean, args), "sigma_0_sweep": sigma_sweep(module, clean, args),
                                "update_cost": update_cost(module, clean, args)}
        if args.out:                                                               # after every prior: a long run leaves what it has
            with open(args.out, "w") as f:
                f.write(json.dumps(doc, indent=2) + "\n")
    print(json.dumps(doc, indent=2))


if __name__ == "__main__":
    main()
