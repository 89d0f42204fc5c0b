"""What non-local means costs on the GPU: HIP-event times after a warm-up, the median over windows of
back-to-back calls.
  (a) bf_op_nlm (csrc/nlm.hip), uint8 out;
  (b) the same algorithm written with torch operators on the same GPU, what a user would otherwise write: per offset of the
      search window a shifted difference, its square summed over the channels, a separable box sum, the table gather and the
      accumulation, all in integers.  Its uint8 result is asserted equal to (a) before anything is timed.
The two are timed in alternating windows of one process, so that a drift of the machine hits both.  Sizes: 32 x 256 x 256 x 3 and
1 x 2048 x 2048 x 3 at patch 1, search 10, and 8 x 256 x 256 x 3 at patch 3, search 10; sigma 20, strength 0.55 on noise over a
smooth ramp.  Next to them the time of one unet_laplacian_v5.6 call on the same batch.  One JSON document on stdout and, with
--out, in that file.

    python tools/exp/nlm_bench.py --out nlm_bench.json"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch

import blind_image_denoising_amd as bf

SIZES = ((32, 256, 256, 3, 1, 10), (1, 2048, 2048, 3, 1, 10), (8, 256, 256, 3, 3, 10))      # B, H, W, C, patch, search


def window_us(fn, reps: int) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def alternate(fns, warmup: int, reps, rounds: int):
    """per function: median / min / max over `rounds` windows of reps[name] back-to-back calls, the windows alternating"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(window_us(fn, reps[name]))
    return {name: {"median_us": float(np.median(t)), "min_us": float(min(t)), "max_us": float(max(t)), "calls_per_window": reps[name],
                   "windows": rounds} for name, t in times.items()}


def torch_nlm(images: torch.Tensor, params: torch.Tensor, table: torch.Tensor, p: int, r: int) -> torch.Tensor:
    """the definition of nlm.py with torch operators, uint8 out"""
    B, H, W, C = images.shape
    x = images.to(torch.int32)
    pad = torch.nn.functional.pad(x.permute(0, 3, 1, 2).float(), (p, p, p, p), mode="replicate").permute(0, 2, 3, 1).to(torch.int32)
    offset, mult = params[:, 0].view(B, 1, 1), params[:, 1].view(B, 1, 1)
    num = torch.zeros((B, H, W, C), dtype=torch.int32, device=images.device)
    wsum = torch.zeros((B, H, W), dtype=torch.int32, device=images.device)
    wmax = torch.zeros_like(wsum)
    k = 2 * p + 1
    for dy in range(-r, r + 1):
        ya, yb = max(0, -dy), min(H, H - dy)
        for dx in range(-r, r + 1):
            xa, xb = max(0, -dx), min(W, W - dx)
            if (dy == 0 and dx == 0) or ya >= yb or xa >= xb:
                continue
            diff = pad[:, ya:yb + 2 * p, xa:xb + 2 * p] - pad[:, ya + dy:yb + dy + 2 * p, xa + dx:xb + dx + 2 * p]
            sq = (diff * diff).sum(dim=3)
            rows = sum(sq[:, u:u + yb - ya] for u in range(k))
            D = sum(rows[:, :, v:v + xb - xa] for v in range(k))
            a = (D - offset).clamp_min(0).to(torch.int64)
            w = table[((a * mult) >> 32).clamp_max(table.numel() - 1)]
            num[:, ya:yb, xa:xb] += w.unsqueeze(3) * x[:, ya + dy:yb + dy, xa + dx:xb + dx]
            wsum[:, ya:yb, xa:xb] += w
            wmax[:, ya:yb, xa:xb] = torch.maximum(wmax[:, ya:yb, xa:xb], w)
    wc = wmax.clamp_min(1)
    num += wc.unsqueeze(3) * x
    den = (wsum + wc).unsqueeze(3)
    return ((2 * num + den) // (2 * den)).to(torch.uint8)


def size(B, H, W, C, p, r, unet, args):
    rng = np.random.default_rng(B + H)
    ramp = 40.0 + 160.0 * (np.add.outer(np.arange(H), np.arange(W)) / float(H + W))[None, :, :, None]
    x = torch.from_numpy(np.clip(np.rint(ramp + rng.normal(0.0, 20.0, (B, H, W, C))), 0, 255).astype(np.uint8)).cuda()
    params = bf.nlm_params(torch.full((B,), 20.0, dtype=torch.float64, device="cuda"), C, p, 0.55)
    table = torch.from_numpy(bf.nlm_table()).cuda()
    kernel = lambda: bf.nlm(x, params, p, r)
    composed = lambda: torch_nlm(x, params, table, p, r)
    assert torch.equal(kernel(), composed()), "the torch composition and bf_op_nlm differ"
    fns, reps = {"a_bf_op_nlm": kernel, "b_torch_operators": composed}, {"a_bf_op_nlm": args.reps, "b_torch_operators": 1}
    if unet is not None:
        fns["unet_laplacian_v5_6"], reps["unet_laplacian_v5_6"] = (lambda: unet(x)), args.reps
    t = alternate(fns, args.warmup, reps, args.rounds)
    a, b = t["a_bf_op_nlm"]["median_us"], t["b_torch_operators"]["median_us"]
    out = {"shape": [B, H, W, C], "patch": p, "search": r, **t, "ratio_b_over_a": b / a,
           "a_pixel_pairs_per_s": B * H * W * ((2 * r + 1) ** 2 - 1) / (a * 1e-6)}
    if unet is not None:
        out["a_share_of_unet_call"] = a / t["unet_laplacian_v5_6"]["median_us"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nlm_bench needs the GPU: nothing here can be measured without one")
    torch.cuda.set_device(0)
    unet = bf.load_model("unet_laplacian_v5.6", device="cuda:0") if "unet_laplacian_v5.6" in bf.models else None
    doc = {"device": torch.cuda.get_device_name(0), "sizes": [size(*s, unet, args) for s in SIZES]}
    text = json.dumps(doc, indent=2)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
