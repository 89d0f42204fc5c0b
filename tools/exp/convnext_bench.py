"""What the first layer of a 7 x 7 ConvNeXt block costs, and what the shipped convnext config delivers: HIP-event
times after a warm-up, the median over windows of back-to-back calls, at 32 x 256 x 256 and C in {32, 64}.
  (a) bf_op_dwconv_ln at k = 7: depthwise + LayerNorm in one launch (csrc/dwconv7_ln.hip);
  (b) the composition that gives the same result without that kernel: bf_op_dwconv_mult (k = 7) then bf_op_dwconv_ln (k = 0).
The two are timed in alternating windows of one process, so that a drift of the machine hits both.  (a) is held against the bytes
it must move (the tensor read once and written once) at the 6.29 TB/s a float4 copy reaches on the MI355X's HBM3E.  Then the
images per second of DenoiserModule on the shipped configs/convnext_color_1x6_32x128x32_7x1x1_256x256_l1_gelu.json at batch 32
(uint8 device tensor in, uint8 out; random weights), on the exact-fp32 path and with arith = 1.  One JSON document on stdout and,
with --out, in that file.

    python tools/exp/convnext_bench.py --out convnext_bench.json"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import unet_laplacian as UL

STREAM_BYTES_PER_S = 6.29e12          # measured float4 copy rate of the MI355X's HBM3E
CONFIG = os.path.join(ROOT, "configs", "convnext_color_1x6_32x128x32_7x1x1_256x256_l1_gelu.json")


def window_us(fn, reps: int) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def alternate(fns, warmup: int, reps: int, rounds: int):
    """per function: median / min / max over `rounds` windows of `reps` back-to-back calls, the windows of the functions alternating"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(window_us(fn, reps))
    return {name: {"median_us": float(np.median(t)), "min_us": float(min(t)), "max_us": float(max(t)), "calls_per_window": reps,
                   "windows": rounds} for name, t in times.items()}


def layer(C: int, B: int, S: int, args):
    r = np.random.default_rng(C)
    x = torch.from_numpy(r.normal(size=(B, S, S, C)).astype(np.float32)).cuda()
    w = torch.from_numpy((r.normal(size=(7, 7, C, 1)) / 7.0).astype(np.float32)).cuda()
    g = torch.from_numpy(r.uniform(0.5, 1.5, C).astype(np.float32)).cuda()
    one = lambda: UL.dwconv_ln(x, w, g)
    two = lambda: UL.dwconv_ln(UL.dwconv_mult(x, w, None), None, g)
    ya, yb = one(), two()
    torch.cuda.synchronize()
    diff = float((ya - yb).abs().max())
    del ya, yb
    t = alternate({"a_dwconv_ln_k7": one, "b_dwconv_mult_then_ln": two}, args.warmup, args.reps, args.rounds)
    nbytes = 2 * x.numel() * 4
    a, b = t["a_dwconv_ln_k7"]["median_us"], t["b_dwconv_mult_then_ln"]["median_us"]
    return {"channels": C, "shape": [B, S, S, C], **t, "max_abs_difference_a_b": diff, "ratio_b_over_a": b / a,
            "algorithmic_bytes": nbytes, "a_bytes_per_s": nbytes / (a * 1e-6),
            "a_share_of_stream_rate": nbytes / (a * 1e-6) / STREAM_BYTES_PER_S}


def model(B: int, S: int, args):
    cfg = bf.load_config(CONFIG)
    m = bf.model_builder(cfg["model"], device="cuda:0", seed=0).hydra
    module = bf.DenoiserModule(m)
    x = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (B, S, S, 3), dtype=np.uint8)).cuda()
    out = {"config": os.path.basename(CONFIG), "shape": [B, S, S, 3], "parameters": m.count_params()}
    for name, arith in (("fp32", 0), ("arith1", 1)):
        m.set_option("arith", arith)
        t = alternate({name: lambda: module(x)}, args.warmup, max(1, args.reps // 4), args.rounds)[name]
        out[name] = {**t, "images_per_s": B / (t["median_us"] * 1e-6)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("convnext_bench needs the GPU: nothing here can be measured without one")
    torch.cuda.set_device(0)
    doc = {"device": torch.cuda.get_device_name(0), "layers": [layer(C, args.batch, args.size, args) for C in (32, 64)],
           "model": model(args.batch, args.size, args)}
    text = json.dumps(doc, indent=2)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
