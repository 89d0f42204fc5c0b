"""Timing of the plain unet backbone (`"type": "unet"`): DenoiserModule u8 -> u8 on a 3-level, 32-filter, [3, 3] unet (one block per
level), batch 16 at 256x256, with the fused decoder entries (fuse_upcat 1, bf_op_upcat_conv2d) and the composed ones (0: upsample +
concat + conv2d) alternated in one process; then the training step (train_step_single_gpu + Adam) at batch 16, 128x128.
Device events around repetitions that add up to >= 1 s of work per sample; several samples per variant, median and spread printed.
Run on the GPU box:  python tools/exp/unet_backbone_bench.py [--samples 5]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "..", "tests"))
import blind_image_denoising_amd as bf                     # noqa: E402
from oracle import bfcnn_oracle as O                        # noqa: E402
import unet_backbone_torch as UB                            # noqa: E402


def timed(fn, min_seconds=1.0):
    """ms per call: repetitions sized from a first estimate so that one sample covers >= min_seconds"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    reps = max(3, int(min_seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3)) + 1)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    cfg = UB.config(no_levels=3, no_layers=1, filters=32, block_kernels=[3, 3], block_filters=[32, 32])
    spec = UB.UnetSpec(cfg)
    m = bf.model_builder(cfg, device="cuda").hydra
    m.set_weights(*UB.init_params(spec, seed=1))
    mod = bf.DenoiserModule(m)
    _, base = O.synthetic_batch(4, 256, 256, seed=1)
    x = torch.from_numpy(np.concatenate([base] * 4)).cuda()
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    res = {0: [], 1: []}
    for v in (1, 0):                                          # warm-up of both variants
        m.set_option("fuse_upcat", v)
        for _ in range(3):
            mod(x)
    torch.cuda.synchronize()
    for _ in range(a.samples):
        for v in (1, 0):
            m.set_option("fuse_upcat", v)
            res[v].append(timed(lambda: mod(x)))
    for v in (1, 0):
        r = np.array(res[v])
        print(f"inference unet 3 levels 32 filters [3,3] x1, batch 16 256x256 u8->u8, fuse_upcat={v}: median {np.median(r):.3f} ms "
              f"(min {r.min():.3f}, max {r.max():.3f}, {len(r)} samples) = {16e3 / np.median(r):.0f} images/s", flush=True)
    d = np.array(res[0]) - np.array(res[1])
    print(f"composed - fused, paired per sample: median {np.median(d):.3f} ms (min {d.min():.3f}, max {d.max():.3f})", flush=True)

    m.set_option("fuse_upcat", 1)
    clean, noisy = O.synthetic_batch(4, 128, 128, seed=2)
    gt = torch.from_numpy(np.concatenate([clean] * 4).astype(np.float32)).cuda()
    nz = torch.from_numpy(np.concatenate([noisy] * 4).astype(np.float32)).cuda()
    fns = bf.build_train_functions(m, bf.loss_function_builder({"mae_multiplier": 1.0, "regularization": 0.01}))
    opt, _ = bf.optimizer_builder({"type": "Adam", "schedule": {"type": "exponential_decay", "config": {"decay_rate": 0.9,
                                   "decay_steps": 100, "learning_rate": 1e-4}}})

    def train():
        total, _, _, _, grads = fns.train_step_single_gpu(gt, nz)
        fns.apply_grads(opt, grads, None)
    for _ in range(3):
        train()
    tr = np.array([timed(train) for _ in range(a.samples)])
    print(f"training step + Adam, batch 16 128x128: median {np.median(tr):.2f} ms (min {tr.min():.2f}, max {tr.max():.2f}, "
          f"{len(tr)} samples) = {16e3 / np.median(tr):.0f} images/s", flush=True)


if __name__ == "__main__":
    main()
