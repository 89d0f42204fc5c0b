"""Pinned bits of everything that goes through the split-f16 weight scale (csrc/h3_weights.h): the packs, their
1/s slots, and the outputs of the three kernels that prepare their weights in the prologue and leave no intermediate to read.
Weights and inputs come from a seeded CPU torch.Generator, so they are the same on every machine.  The sha256 values are a pin,
like test_workspace_bytes_are_pinned: a deliberate change of the arithmetic updates them."""
import functools
import hashlib
import json

import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import unet_laplacian as UL
from blind_image_denoising_amd.constants import DEFAULT_BN_EPSILON
from oracle import bfcnn_oracle as O

pytestmark = pytest.mark.gpu

H3_BLOCK_FLOATS = 64 + 2 * 13 * 64 * 4        # BF_H3_BLOCK_FLOATS: the split-f16 blocks are the tail of the bf_pack_inference buffer
LAYERS = 6

# Recorded at the commit before csrc/h3_weights.h existed (every site still carried its own copy of the rule) with
#     python -m tests.test_gpu_h3_weights
# from the repository root on an MI355X; the same command prints the current table.
PINNED = {
    "base_rows_forward/6_layers_u8": "3ae67e06f503081a58621fd69a8e56d64d9b46c1b0fdd9e73038789dd199532b",
    "bf_pack_inference/ordinary": "ee41557aef7513fc9dbe9372871d275efcda7315aab13433ba839cf3e070360a",
    "bf_pack_inference/pow2": "136a45a7685b1701392d0ecaea2083ee7effc1855f36552e6effec89328b8492",
    "first_conv_h3k/k3": "2af00f3b1f2354b131fa3e49acb572a42998282e769e3afbc3c7ac787abdc1f1",
    "first_conv_h3k/k5": "aca1a8af8753bfee7dca053c5ca4fd16d8710d7e0b2e43fc4722ee394d7abd78",
    "first_conv_h3k/k7": "800dd5cd51cfb72a21f7ef37806bbd74e1bed36564396b1d8b36b9eedeed0a35",
    "head_fused_h3/C32": "1856845a7048ed97a1ec641aa6a1020f70f3514127db7da22157ce2f7e832c96",
    "head_fused_h3/C64": "2684d64e3e85bb5eaa86dabecd8c8fbc0f9b9f1b59bd0f8516c1cf8859e885d1",
    "pack_bneck_h3/ordinary": "71d7cab1ae7314785f1b6320215b178ecb3ddd2bed326cb040bbb13ea28cc014",
    "pack_bneck_h3/pow2": "2f65e6bc5f58685f0f517a7d0a423f5458d1f1184b598169e2e041bc03053005",
    "pack_mlp_h3/C32/ordinary": "81b55de7cafa7b285881e50fea60908d5e514b56f628c035790a9bfb4d5e88ea",
    "pack_mlp_h3/C32/pow2": "6b71602c44cee2dd47411cc1421f164efd46c8b75fedc071f607f2d0b888f44a",
    "pack_mlp_h3/C64/ordinary": "a3cec35363a14b36f522a9edede4b9e3a380cd6744c27af4c5e733948d7c4797",
    "pack_mlp_h3/C64/pow2": "620257d7c60ea06131ed59df2870504d76ecc29988c44b252d6b24fa660403f2",
    "pack_mlp_h3_chain/C32/ordinary": "c881c9ef726d508064a41026dbf447076f36e14dd011ff36b4fff49417bbd3da",
    "pack_mlp_h3_chain/C32/pow2": "7c8df5082de755befd185935a53abc27cc3d42d145c0720d9b45caae6f6e1a88",
}


def _sha(t) -> str:
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return hashlib.sha256(a.tobytes()).hexdigest()


def _randn(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen, dtype=torch.float32) * scale


def _pow2(w):
    """the same tensor with max |w| exactly 2^-3: x / x is 1 for every finite x, the power of two is exact"""
    return w / w.abs().max() * 0.125


def rule(m):
    """the scale rule in NumPy: 2^(14 - clip(frexp(m).exponent, -100, 100)), 1 for a zero or non-finite maximum"""
    m = np.float32(m)
    if not (m > 0 and np.isfinite(m)):
        return np.float32(1.0)
    return np.float32(np.ldexp(1.0, 14 - int(np.clip(np.frexp(m)[1], -100, 100))))


def _mlp_weights(C, pow2):
    gen = torch.Generator().manual_seed(1000 + C)
    w1, w2 = _randn(gen, C, 4 * C, scale=0.2), _randn(gen, 4 * C, C, scale=0.1)
    return (_pow2(w1), _pow2(w2)) if pow2 else (w1, w2)


def _bneck_weights(pow2):
    gen = torch.Generator().manual_seed(2000)
    w0, wd, w2 = _randn(gen, 32, 32, scale=0.2), _randn(gen, 3, 3, 32, 4, scale=0.1), _randn(gen, 128, 32, scale=0.1)
    return (_pow2(w0), wd, _pow2(w2)) if pow2 else (w0, wd, w2)


def _model_weights(pow2):
    """(spec, params, state) of the 6-layer [3,3] config: kernels N(0, 0.1^2), gamma in [0.5, 1.5], moving variance in [0.5, 1.5]"""
    cfg = O.canonical_config(no_layers=LAYERS)
    spec = O.ResnetSpec.from_config(cfg["model"])
    gen = torch.Generator().manual_seed(3000)
    params = _randn(gen, spec.param_count(), scale=0.1)
    for name, (off, shape) in spec.offsets().items():
        n = int(np.prod(shape))
        if name.endswith("gamma"):
            params[off:off + n] = 0.5 + torch.rand(n, generator=gen)
        elif pow2 and name.startswith("block"):
            params[off:off + n] = _pow2(params[off:off + n])
    state = _randn(gen, spec.state_count(), scale=0.05)
    for name, (off, shape) in spec.state_offsets().items():
        if name.endswith("moving_variance"):
            state[off:off + int(np.prod(shape))] = 0.5 + torch.rand(int(np.prod(shape)), generator=gen)
    return cfg, spec, params.numpy(), state.numpy()


def _model(pow2):
    cfg, spec, params, state = _model_weights(pow2)
    m = bf.model_builder(cfg["model"], device="cuda").hydra
    m.set_weights(params, state)
    return m


def _h3_blocks(m):
    """[LAYERS][BF_H3_BLOCK_FLOATS] fp32 view of the split-f16 part of the inference pack; the buffer starts zeroed, because the pack
    kernels leave its alignment gaps and aux[16..31] alone"""
    m._packed = torch.zeros(int(m._lib.bf_packed_bytes(m._h)), dtype=torch.uint8, device=m.device)
    m.mark_dirty()
    packed = m.packed()
    torch.cuda.synchronize()
    return packed, packed.view(torch.float32)[-H3_BLOCK_FLOATS * LAYERS:].view(LAYERS, H3_BLOCK_FLOATS)


@functools.lru_cache(maxsize=None)
def digests():
    """every pinned quantity, computed once per session"""
    d = {}
    for tag, pow2 in (("ordinary", False), ("pow2", True)):
        for C in (32, 64):
            w1, w2 = _mlp_weights(C, pow2)
            d[f"pack_mlp_h3/C{C}/{tag}"] = _sha(UL.pack_mlp_h3(w1.cuda(), w2.cuda()))
        w1, w2 = _mlp_weights(32, pow2)
        d[f"pack_mlp_h3_chain/C32/{tag}"] = _sha(UL.pack_mlp_h3_chain(w1.cuda(), w2.cuda()))
        d[f"pack_bneck_h3/{tag}"] = _sha(UL.pack_bneck_h3(*[w.cuda() for w in _bneck_weights(pow2)]))
        d[f"bf_pack_inference/{tag}"] = _sha(_h3_blocks(_model(pow2))[0])

    # ---- the kernels that scale their weights in the prologue
    # bf_op_first_conv_h3k: tiles of 8 x 64 output pixels (UF_TH, UF_TW): 12 x 80 = one full and one partial tile in both directions
    gen = torch.Generator().manual_seed(4000)
    img = torch.randint(0, 256, (1, 12, 80, 3), generator=gen, dtype=torch.uint8).cuda()
    for k in (3, 5, 7):
        w = _randn(gen, k, k, 3, 32, scale=0.2).cuda()
        d[f"first_conv_h3k/k{k}"] = _sha(UL.first_conv(img, w, 12, 80, "leaky_relu_01", True, 0.0, 255.0, arith=1))
    # bf_op_head_fused_h3: a wave carries groups of 32 pixels (16 * NP) of the flat cropped map: 7 x 9 = 63 = one full group and one
    # partial one, and the crop from 9 x 11 makes the row and the image stride differ from the map's
    for C in (32, 64):
        x, g = _randn(gen, 1, 9, 11, C, scale=1.5).cuda(), (0.5 + torch.rand(C, generator=gen)).cuda()
        w0p = UL.pack_pointwise((_randn(gen, 1, 1, C, 32) / np.sqrt(C)).cuda())
        w1 = _randn(gen, 1, 1, 32, 3, scale=0.3).cuda()
        d[f"head_fused_h3/C{C}"] = _sha(UL.head_fused(x, g, w0p, "leaky_relu_01", w1, 7, 9, False, True, 0.0, 255.0, arith=1))
    # base_conv_rows_kernel: chunks of 256 columns (BR_CW), bands of 8 rows at this size.  12 x 300 uint8 is padded to 16 x 512: the
    # source fills the first chunk and part of the second, the first band and half of the second
    m = _model(False)
    noisy = torch.randint(0, 256, (1, 12, 300, 3), generator=gen, dtype=torch.uint8).numpy()
    m.set_option("base_rows", 2)               # the row kernel wherever it can run (process-wide)
    try:
        d["base_rows_forward/6_layers_u8"] = _sha(bf.DenoiserModule(m)(noisy))
    finally:
        m.set_option("base_rows", 1)
    torch.cuda.synchronize()
    return d


@pytest.mark.parametrize("name", sorted(PINNED))
def test_bits_are_pinned(name):
    assert digests()[name] == PINNED[name]


def test_every_digest_is_pinned():
    assert sorted(digests()) == sorted(PINNED)


@pytest.mark.parametrize("C", [32, 64])
def test_mlp_pack_inverse_scales_follow_the_rule(C):
    w1, w2 = _mlp_weights(C, False)
    aux = UL.pack_mlp_h3(w1.cuda(), w2.cuda()).cpu()[-16:].view(torch.float32).numpy()
    want = np.array([1 / rule(w1.abs().max().item()), 1 / rule(w2.abs().max().item()), 0, 0], np.float32)
    assert aux.tobytes() == want.tobytes(), (aux, want)


def test_inference_pack_inverse_scales_follow_the_rule():
    """aux[0..15] = 1/s1, aux[48..63] = 1/min(s2, 2^15) with s2 from max |w2 * fold|, fold = gamma / sqrt(var + eps).  The folded maxima
    are kept clear of a binade edge by 1 %, so that a last-bit difference between sqrtf and NumPy cannot flip the exponent."""
    cfg, spec, params, state = _model_weights(False)
    blocks = _h3_blocks(_model(False))[1].cpu().numpy()
    off, soff = spec.offsets(), spec.state_offsets()
    for i in range(LAYERS):
        w1 = params[off[f"block{i}/conv0/kernel"][0]:][:2304]
        w2 = params[off[f"block{i}/conv1/kernel"][0]:][:2304].reshape(144, 16)
        gamma = params[off[f"block{i}/bn1/gamma"][0]:][:16]
        var = state[soff[f"block{i}/bn1/moving_variance"][0]:][:16]
        fold = gamma / np.sqrt(var + np.float32(DEFAULT_BN_EPSILON))
        m2 = np.abs(w2 * fold[None, :]).max()
        frac = np.frexp(m2)[0]
        assert 0.505 < frac < 0.99, f"block {i}: folded maximum {m2} sits within 1 % of a binade edge; choose another seed"
        s1, s2 = rule(np.abs(w1).max()), min(rule(m2), np.float32(32768.0))
        assert blocks[i, 0:16].tobytes() == np.full(16, 1 / s1, np.float32).tobytes(), (i, blocks[i, 0:16], 1 / s1)
        assert blocks[i, 48:64].tobytes() == np.full(16, 1 / s2, np.float32).tobytes(), (i, blocks[i, 48:64], 1 / s2)


if __name__ == "__main__":
    print(json.dumps(digests(), indent=4, sort_keys=True))
