"""Records tests/golden/pair_schedule_parent.json: the sha256 of the fp32 output of bf_debug_fused_block2_h3 (fused_block2_h3w_kernel,
two residual blocks per launch) on seeded random normal inputs and weights, per (shape, walking direction), relu.  A change of the
kernel's schedule that keeps every accumulator's MFMA order must reproduce these digests; tests/test_gpu_pair_schedule.py asserts it.
Run it with the library whose bits are the reference (BFCNN_HIP_LIB=... for another one than the package's own):
usage: python tools/record_pair_golden.py [OUT.json]"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 19, 145), (1, 7, 257)]


def inputs(shape):
    """x, w4, scale2, shift2 at the scale of tests/test_gpu_kernels.py (_rand: standard normal, weights times 0.1)"""
    B, H, W = shape
    rand = lambda s, seed: np.random.default_rng(seed).standard_normal(s).astype(np.float32)
    x, w4 = rand((B, H, W, 16), 31), rand((4, 3, 3, 16, 16), 32) * 0.1
    sc2, sh2 = 1.0 + 0.25 * rand((2, 16), 33), 0.1 * rand((2, 16), 34)
    return x, w4, sc2, sh2


def key(shape, reverse):
    return "x".join(map(str, shape)) + ("-up" if reverse else "-down")


def output(shape, reverse):
    import torch
    sys.path.insert(0, ROOT)
    from blind_image_denoising_amd import _native as N
    L = N.lib()
    B, H, W = shape
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    xd, wd, sd, hd = map(up, inputs(shape))
    out = torch.full((B, H, W, 16), float("nan"), dtype=torch.float32, device="cuda")
    scratch = torch.zeros(int(L.bf_debug_fused_block2_h3_scratch_floats(B, H, W)), dtype=torch.float32, device="cuda")
    rc = L.bf_debug_fused_block2_h3(N.ptr(xd), N.ptr(wd), N.ptr(sd), N.ptr(hd), N.ptr(out), N.ptr(scratch), B, H, W, 1, reverse, N.stream_ptr(xd))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu().numpy()


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float32).tobytes()).hexdigest()


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "pair_schedule_parent.json")
    rec = {}
    for shape in SHAPES:
        for reverse in (0, 1):
            o = output(shape, reverse)
            assert np.isfinite(o).all()
            rec[key(shape, reverse)] = digest(o)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec, indent=1, sort_keys=True))
