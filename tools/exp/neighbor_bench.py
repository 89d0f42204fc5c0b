"""Timing of the Neighbor2Neighbor pairs: bf_op_neighbor_pairs alone at a training shape against the HBM rate of a
pure stream, and a training step fed by NeighborPairs (gamma = 0: the pair kernel; gamma > 0: plus the full-resolution inference
forward and the re-pack after the optimizer step) against the same train_step fed the same half-resolution batch directly.

    python tools/exp/neighbor_bench.py [--batch 32] [--size 256] [--config resnet_color_1x18_bn_16x3x3_256x256_l1_relu] [--kernel-only]"""
import argparse
import pathlib
import sys
import time

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[2]))
import blind_image_denoising_amd as bf              # noqa: E402


def kernel_time(B, S, C, with_f, y_dtype, sets, iters=200, warmup=20):
    """mean milliseconds per launch by device events; `sets` rotating buffer sets (more than the 256 MiB Infinity Cache holds: HBM)"""
    from blind_image_denoising_amd import _native as N
    dev = torch.device("cuda")
    ys = [torch.randint(0, 256, (B, S, S, C), device=dev, dtype=torch.uint8).to(y_dtype) for _ in range(sets)]
    fs = [torch.rand((B, S, S, C), device=dev) * 255 if with_f else None for _ in range(sets)]
    ins = [torch.empty((B, S // 2, S // 2, C), device=dev) for _ in range(sets)]
    tgs = [torch.empty_like(t) for t in ins]
    lib, stream = N.lib(), N.stream_ptr(ys[0])

    def launch(i):
        k = i % sets
        N.check(lib.bf_op_neighbor_pairs(N.ptr(ys[k]), int(y_dtype == torch.uint8), N.ptr(fs[k]), 0.5 if with_f else 0.0, N.ptr(ins[k]),
                                         N.ptr(tgs[k]), B, S, S, C, i, stream), None, "bf_op_neighbor_pairs")
    for i in range(warmup):
        launch(i)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        launch(i)
    stop.record()
    torch.cuda.synchronize()
    n = B * S * S * C
    moved = n * (1 if y_dtype == torch.uint8 else 4) + (4 * n if with_f else 0) + 2 * n          # y, f, two outputs of n / 4 floats
    ms = start.elapsed_time(stop) / iters
    return ms, moved


def step_times(config_name, B, S, steps=40, warmup=8):
    cfg = bf.CONFIGS_DICT[config_name]
    out = {}
    noisy = [torch.randint(0, 256, (B, S, S, 3), device="cuda", dtype=torch.uint8).float() for _ in range(4)]
    for name, gamma in (("direct", None), ("gamma=0", 0.0), ("gamma=2", 2.0)):
        model = bf.model_builder(cfg["model"], device="cuda", seed=1).hydra
        fns = bf.build_train_functions(model, bf.loss_function_builder(cfg["loss"]))
        opt, _ = bf.optimizer_builder(cfg["train"]["optimizer"])
        if gamma is None:
            half = [tuple(reversed(bf.neighbor_pairs(y, i))) for i, y in enumerate(noisy)]
            data = half * ((steps + warmup) // len(half) + 1)
        else:
            data = bf.NeighborPairs(noisy * ((steps + warmup) // len(noisy) + 1), model=model, gamma=gamma, ramp=False, seed=0)
        t0 = None
        for i, (gt, x) in enumerate(data):
            if i == warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            if i == warmup + steps:
                break
            total, _, _, _, grads = fns.train_step_single_gpu(gt, x, (1.0,), 0.0, None)
            fns.apply_grads(opt, grads, None)
        torch.cuda.synchronize()
        out[name] = (time.perf_counter() - t0) / steps * 1e3
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--config", default="resnet_color_1x18_bn_16x3x3_256x256_l1_relu")
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    B, S = args.batch, args.size
    for y_dtype in (torch.uint8, torch.float32):
        for with_f in (False, True):
            for sets, where in ((16, "HBM (16 rotating sets)"), (1, "one resident set")):
                for rep in range(2):
                    ms, moved = kernel_time(B, S, 3, with_f, y_dtype, sets)
                    print(f"bf_op_neighbor_pairs {B}x{S}x{S}x3 y={'u8' if y_dtype == torch.uint8 else 'f32'} f={'yes' if with_f else 'no'} {where}: "
                          f"{ms * 1e3:.1f} us, {moved / 1e6:.1f} MB moved, {moved / ms / 1e9:.2f} TB/s", flush=True)
    for rep in range(0 if args.kernel_only else 2):
        t = step_times(args.config, B, S)
        print(f"{args.config} step on {B}x{S // 2}x{S // 2}x3 pairs: " + ", ".join(f"{k} {v:.3f} ms" for k, v in t.items()), flush=True)


if __name__ == "__main__":
    main()
