"""CPU tests: the C-ABI library loads and exports every symbol include/bfcnn_hip.h declares,
non-compute entry points behave (layout, errors), and the host mirrors the reference's
argument / error behaviour.  No kernel is launched here."""
import ctypes as C
import json
import math
import pathlib
import re

import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import _native as N
from oracle import bfcnn_oracle as O

ROOT = pathlib.Path(__file__).resolve().parent.parent


HEADERS = ("bfcnn_hip.h", "bfcnn_hip_debug.h")      # the drop-in ABI and the single-kernel diagnostic entries


def _header_text():
    return "\n".join((ROOT / "include" / h).read_text() for h in HEADERS)


def _declared_symbols():
    text = _header_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(bf_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    lib = C.CDLL(str(N.LIB_PATH))
    declared = _declared_symbols()
    assert len(declared) >= 25
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/bfcnn_hip.h but not exported"
    # and the ctypes table binds exactly the declared functions
    assert sorted(N.SIGNATURES) == declared
    assert N.lib().bf_abi_version() == 1


def test_ctypes_signatures_match_the_header_prototypes():
    """every prototype of include/bfcnn_hip.h against _native.SIGNATURES: same number of parameters, pointers bound as pointers,
    int / int64_t / float / uint64_t as the ctypes type of that width (a binding that drifts from the header corrupts calls
    silently: ctypes does not check)."""
    text = _header_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    protos = re.findall(r"\b(?:const\s+char\s*\*|int64_t|int|void|float|bf_handle)\s*(bf_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    names = [n for n, _ in protos]
    assert sorted(set(names)) == _declared_symbols(), sorted(set(_declared_symbols()) - set(names))
    scalar = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "uint64_t": C.c_uint64, "unsigned": C.c_uint,
              "double": C.c_double}
    for name, args in protos:
        args = " ".join(args.split())
        params = [] if args in ("", "void") else [a.strip() for a in args.split(",")]
        _, argtypes = N.SIGNATURES[name]
        assert len(params) == len(argtypes), (name, len(params), len(argtypes))
        for i, (p, t) in enumerate(zip(params, argtypes)):
            words = p.replace("const", " ").replace("*", " * ").split()
            is_pointer = "*" in words or "[" in p or words[0] in ("bf_handle",)
            if is_pointer:
                assert t in (C.c_void_p, C.c_char_p) or hasattr(t, "contents") or hasattr(t, "_type_"), (name, i, p, t)
            else:
                assert words[0] in scalar, (name, i, p)
                assert C.sizeof(t) == C.sizeof(scalar[words[0]]) and (t is C.c_float) == (words[0] == "float"), (name, i, p, t)


def test_struct_layouts_match_header():
    assert C.sizeof(N.ResnetDesc) == 17 * 4 + 5 * 4
    assert C.sizeof(N.LossDesc) == 8 * 4
    assert C.sizeof(N.TensorInfo) == 104          # 100 rounded up to the int64 alignment


@pytest.mark.parametrize("n,count", [(6, 28784), (18, 84272)])
def test_parameter_inventory_matches_oracle(n, count):
    cfg = O.canonical_config(no_layers=n)["model"]
    m = bf.model_builder(cfg, device="cpu", seed=0).hydra
    spec = O.ResnetSpec.from_config(cfg)
    assert m.n_params == count == spec.param_count()
    assert m.n_state == spec.state_count() == 32 * n
    off = spec.offsets()
    names = {"block%d/conv0/kernel", "block%d/conv1/kernel"}
    for v in m.trainable_variables:
        o, s = off[v.name.replace("bn1", "bn1")]
        assert (v.offset, v.shape) == (o, tuple(s)), v.name
    for v, (name, shape) in zip(m.non_trainable_variables, spec.state_tensors()):
        assert v.name == name and v.shape == tuple(shape)


@pytest.mark.parametrize("nb", [1, 3])
def test_parameter_inventory_of_block_variants(nb):
    """block_kernels of length 1 / 3: variable order conv0, (conv j, bn j gamma) for j >= 1; one BN state pair per j >= 1."""
    cfg = O.canonical_config(no_layers=3)["model"]
    cfg["backbone"].update(block_kernels=[3] * nb, block_filters=[16] * nb)
    m = bf.model_builder(cfg, device="cpu", seed=0).hydra
    spec = O.ResnetSpec.from_config(cfg)
    assert m.n_params == spec.param_count() and m.n_state == spec.state_count() == 3 * (nb - 1) * 32
    off = spec.offsets()
    assert [v.name for v in m.trainable_variables] == [t[0] for t in spec.tensors()]
    for v in m.trainable_variables:
        assert (v.offset, v.shape) == (off[v.name][0], tuple(off[v.name][1])), v.name
    assert [(v.name, v.shape) for v in m.non_trainable_variables] == [(n, tuple(s)) for n, s in spec.state_tensors()]


def test_initial_values_follow_keras_defaults():
    m = bf.model_builder(O.canonical_config(no_layers=2)["model"], device="cpu", seed=3).hydra
    for v in m.trainable_variables:
        a = v.numpy()
        if v.kind == 1:
            assert np.all(a == 1.0)                           # gamma
        else:
            kh, kw, ci, co = a.shape
            std = math.sqrt(2.0 / (kh * kw * (ci + co))) / 0.87962566103423978
            assert np.abs(a).max() <= 2.0 * std + 1e-7        # truncated at 2 sigma
            assert 0.5 * std < a.std() < 1.2 * std
    st = {v.name: v.numpy() for v in m.non_trainable_variables}
    assert np.all(st["block0/bn1/moving_mean"] == 0) and np.all(st["block0/bn1/moving_variance"] == 1)


def test_create_rejects_what_the_reference_rejects():
    cfg = O.canonical_config(no_layers=2)["model"]
    bad = json.loads(json.dumps(cfg)); bad["backbone"]["block_kernels"] = [3, 3, 3, 3]; bad["backbone"]["block_filters"] = [16] * 4
    with pytest.raises(ValueError, match="<= 3"):
        bf.model_builder(bad, device="cpu")
    bad = json.loads(json.dumps(cfg)); bad["backbone"]["block_filters"] = [16]
    with pytest.raises(ValueError):
        bf.model_builder(bad, device="cpu")
    bad = json.loads(json.dumps(cfg)); bad["backbone"]["type"] = "nonsense"
    with pytest.raises(ValueError, match="don't know how to build model"):
        bf.model_builder(bad, device="cpu")
    bad = json.loads(json.dumps(cfg)); bad["backbone"]["type"] = "efficientnet"
    with pytest.raises(NotImplementedError):
        bf.model_builder(bad, device="cpu")
    bad = json.loads(json.dumps(cfg)); bad["backbone"]["filters"] = 48; bad["backbone"]["block_filters"] = [48, 48]
    with pytest.raises(NotImplementedError, match="16"):
        bf.model_builder(bad, device="cpu")
    # 32 / 64 / 128 filters go to the generic resnet model (operator library, inference only)
    ok = json.loads(json.dumps(cfg)); ok["backbone"]["filters"] = 32; ok["backbone"]["block_filters"] = [32, 32]
    assert type(bf.model_builder(ok, device="cpu").hydra).__name__ == "GenericResnetHydra"
    d = N.ResnetDesc()
    h = C.c_void_p()
    assert N.lib().bf_create(C.byref(d), C.byref(h)) == N.BF_EINVAL and not h.value
    assert "struct_size" in N.last_error(None)


def test_workspace_and_packed_queries():
    m = bf.model_builder(O.canonical_config(no_layers=6)["model"], device="cpu").hydra
    L = N.lib()
    assert L.bf_workspace_bytes(m._h, N.BF_MODE_INFERENCE, 64, 256, 256) == 3 * 64 * 256 * 256 * 16 * 4 + N.BF_STATUS_BYTES
    assert L.bf_workspace_bytes(m._h, N.BF_MODE_INFERENCE, 1, 200, 300) == 3 * 256 * 512 * 16 * 4 + N.BF_STATUS_BYTES   # pow2 padded
    assert L.bf_workspace_bytes(m._h, N.BF_MODE_TRAIN, 2, 32, 32) > (3 * 6 + 2) * 2 * 32 * 32 * 16 * 4
    assert L.bf_workspace_bytes(m._h, 0, 0, 8, 8) == -1
    assert L.bf_packed_bytes(m._h) % 256 == 0


def _band_plan_grid(B, H, nstrips, lead_steps, cap=256):
    """restatement of bf_band_plan (csrc/h3_bands.h): rows per band such that the slowest of `cap` workgroups finishes earliest
    (first minimum over ty = 1 .. ceil(H / 8), a ty its own rows do not reproduce is skipped); returns the launch grid"""
    best, best_cost = H, None
    for ty in range(1, (H + 7) // 8 + 1):
        rows = -(-H // ty)
        if -(-H // rows) != ty:
            continue
        cost = -(-B * ty * nstrips // cap) * (rows + lead_steps)
        if best_cost is None or cost < best_cost:
            best, best_cost = rows, cost
    return min(B * -(-H // best) * nstrips, cap)


def test_band_plan_sizes_the_block_kernel_scratch():
    """launch grid and workspace sizing of the streaming block kernels come from one planner: the scratch queries of the training
    block kernels (rows of partial sums = workgroups of the launch) against the Python restatement"""
    from test_gpu_kernels import BWD_BLOCK_SHAPES, FWD_BLOCK_SHAPES
    L = N.lib()
    rng = np.random.default_rng(20)
    shapes = sorted(set(FWD_BLOCK_SHAPES) | set(BWD_BLOCK_SHAPES)) + [(32, 256, 256), (8, 512, 512)]
    shapes += [(int(rng.integers(1, 81)), int(rng.integers(1, 601)), int(rng.integers(1, 701))) for _ in range(300)]
    P = 13 * 64 * 4 + 64
    fixed = 4 * P + 2 * 2304 + 16
    for B, H, W in shapes:
        fwd = _band_plan_grid(B, H, 1, 10)
        bwd = _band_plan_grid(B, H, -(-W // 128), 10)
        assert L.bf_debug_fwd_block_h3t_scratch_floats(B, H, W) == fixed + fwd * 32, (B, H, W)
        assert L.bf_debug_bwd_block_h3t_scratch_floats(B, H, W) == fixed + bwd * (2 * 2304 + 32), (B, H, W)


# (B, H, W) -> (training, inference) workspace bytes of the canonical 1x18 model, recorded from the build in front of the shared
# band planner: the planner and the folded forward's second statistics buffer must not move a byte
WORKSPACE_BYTES_1X18 = {
    (32, 256, 256): (8128070400, 402655232),
    (8, 512, 512): (8128070400, 402655232),
    (3, 40, 50): (30264832, 2361344),
    (70, 40, 256): (2893775872, 220203008),
    (1, 1, 1): (1876432, 2240),
}


def test_workspace_bytes_are_pinned():
    m = bf.model_builder(O.canonical_config(no_layers=18)["model"], device="cpu").hydra
    L = N.lib()
    for (B, H, W), (train, infer) in WORKSPACE_BYTES_1X18.items():
        assert L.bf_workspace_bytes(m._h, N.BF_MODE_TRAIN, B, H, W) == train, (B, H, W)
        assert L.bf_workspace_bytes(m._h, N.BF_MODE_INFERENCE, B, H, W) == infer, (B, H, W)


# ---- the forward plan (csrc/engine_infer.hip make_forward_plan, csrc/fused_h3.hip bf_select_fused_block_h3) -----------------------
PLAN_OPTIONS = {"arith": 1, "fused_blocks": 1, "h3_pair": 1, "h3_pair_head": 0, "fused_head": 0, "h3_compact": 0, "h3_zigzag": 1,
                "h3_variant": -1}           # the library's defaults


def _h3_select(B, H, W, variant, head, compact):
    """restatement of the one selection rule of a single split-f16 block: (kernel, 16 x 16 tiles, bottom-up walk forced)"""
    streams = 1 <= W <= 256 and H >= 1 and not head                # the full-row streaming kernel: up to 256 columns, no head epilogue
    if variant < 0:
        tiles32 = B * -(-H // 16) * -(-W // 32)
        if streams and B * H >= 3072 and (H >= 24 or W > 128):
            variant = 4
        else:
            variant = 2 if (not head and not compact and tiles32 < 512 and tiles32 != 256) else 1
    v = variant & 255
    if v == 4 and streams:
        return "fused_block_h3v_kernel", False, bool(variant & 256)
    return "fused_block_h3r_kernel", v == 2, bool(variant & 256)


def _forward_plan(no_layers, block_convs, head_fits, options, B, H, W):
    """restatement of make_forward_plan + its printer for a model of `no_layers` blocks of `block_convs` convolutions whose head
    is (not) linear with 3 channels, at the PADDED size H x W: (the line of bf_debug_forward_plan, block launches)"""
    o = dict(PLAN_OPTIONS, **options)
    N = no_layers
    h3 = bool(o["fused_blocks"] and o["arith"] == 1 and N > 0 and block_convs == 2)
    head_in_block = compact = pair_ok = head_in_pair = False
    if h3:
        head_in_block = bool(o["fused_head"]) and head_fits
        plain = _h3_select(B, H, W, o["h3_variant"], False, False)
        compact = bool(o["h3_compact"]) and not head_in_block and plain[0] == "fused_block_h3v_kernel"
        if o["h3_pair"] and not compact:
            if o["h3_pair"] == 2:
                pair_ok = True
            elif o["h3_variant"] >= 0:
                pair_ok = plain[0] == "fused_block_h3v_kernel"
            else:
                pair_ok = H >= 24 and B * H * -(-W // 128) >= 4096
        head_in_pair = pair_ok and not head_in_block and bool(o["h3_pair_head"]) and N >= 2 and head_fits
    tokens, launches, i = [], 0, 0
    while i < N:
        zz = bool(o["h3_zigzag"]) and launches % 2 == 1
        if pair_ok and i + 1 < N and not (head_in_block and i + 1 == N - 1) and not (i == 0 and N % 2 == 1):
            marks = (["rev"] if zz else []) + (["head"] if head_in_pair and i + 2 == N else [])
            tokens.append(",".join([f"fused_block2_h3w_kernel:{i}+{i + 1}"] + marks))
            launches, i = launches + 1, i + 2
            continue
        if h3:
            head = head_in_block and i == N - 1
            name, t16, up = _h3_select(B, H, W, 1, True, False) if head else _h3_select(B, H, W, o["h3_variant"], False, compact)
            marks = (["t16"] if t16 else []) + (["rev"] if zz or up else []) + (["head"] if head else [])
            tokens.append(",".join([f"{name}:{i}"] + marks))
            launches += 1
        elif block_convs == 2 and o["fused_blocks"]:
            tokens.append(f"fused_block_v4_kernel:{i}")
            launches += 1
        else:
            tokens += [f"conv3x3_c16_kernel:{i}.{j}" for j in range(block_convs)] if block_convs != 1 else [f"conv3x3_c16_kernel:{i}"]
            launches += block_convs
        i += 1
    layout = "compact" if compact else ("split" if h3 else "f32")
    if not (head_in_block or head_in_pair):
        tokens.append("head")
    return " ".join([layout] + tokens), launches


def _plan_totals(line):
    """(the kernel that runs most blocks -- a launch counts for the blocks it runs, of equals the one met first --, block launches)
    of a plan line: what bf_get_block_kernel reports after that forward"""
    names = [t.split(":")[0] for t in line.split()[1:] if t != "head"]
    weight = {}
    for t, name in zip([t for t in line.split()[1:] if t != "head"], names):
        weight[name] = weight.get(name, 0) + (2 if "+" in t else 1)
    best = max(weight.values(), default=0)
    return next((n for n in names if weight[n] == best), ""), len(names)


def _plan_model(no_layers, block_convs=2, head_activation="linear", output_channels=3):
    cfg = O.canonical_config(no_layers=no_layers)["model"]
    cfg["backbone"].update(block_kernels=[3] * block_convs, block_filters=[16] * block_convs)
    cfg["denoiser"].update(activation=head_activation, output_channels=output_channels)
    N.lib().bf_debug_set_h3_variant(-1)          # the process-wide override of the handle-less entries is part of the rule: off
    return bf.model_builder(cfg, device="cpu").hydra


def _pow2(n):
    return 1 << (n - 1).bit_length()


@pytest.mark.parametrize("no_layers,shape,options,kernel,launches", [
    (4, (2, 32, 32), {}, "fused_block_h3r_kernel", 4),
    (4, (16, 256, 64), {}, "fused_block2_h3w_kernel", 2),
    (4, (16, 256, 64), {"h3_pair": 0}, "fused_block_h3v_kernel", 4),
    (4, (16, 256, 64), {"arith": 0}, "fused_block_v4_kernel", 4),
    (3, (16, 256, 64), {}, "fused_block2_h3w_kernel", 2),
    (2, (6, 352, 300), {}, "fused_block2_h3w_kernel", 1),
    (3, (6, 352, 300), {}, "fused_block2_h3w_kernel", 2),
    (2, (6, 352, 300), {"h3_pair": 0}, "fused_block_h3r_kernel", None),
    (3, (6, 352, 300), {"h3_pair": 0}, "fused_block_h3r_kernel", None),
    (2, (1, 64, 300), {}, "fused_block_h3r_kernel", None),
    (3, (1, 64, 300), {}, "fused_block_h3r_kernel", None),
    (2, (2, 64, 64), {"h3_variant": 4}, "fused_block2_h3w_kernel", 1),
])
def test_forward_plan_restatement_is_pinned_to_what_the_gpu_tests_assert(no_layers, shape, options, kernel, launches):
    """the Python restatement of the selection rule, held first to the facts tests/test_gpu_inference.py asserts after real forwards
    of the canonical model on the uint8 path (sizes padded to powers of two) -- and the library to the same facts"""
    B, H, W = shape
    line, n = _forward_plan(no_layers, 2, True, options, B, _pow2(H), _pow2(W))
    assert _plan_totals(line) == (kernel, n) and (launches is None or n == launches), line
    if no_layers == 3 and kernel == "fused_block2_h3w_kernel":
        assert "+" not in line.split()[1] and "+" in line.split()[2]           # the single block is the first launch
    m = _plan_model(no_layers)
    for k, v in options.items():
        m.set_option(k, v)
    assert m.forward_plan(B, H, W) == (line, n)


def _check_plan_structure(line, launches, no_layers, block_convs):
    tokens = line.split()
    assert tokens[0] in ("f32", "split", "compact")
    runs = [t for t in tokens[1:] if t != "head"]
    assert launches == len(runs)
    seen, convs, carried = [], {}, 0
    for k, t in enumerate(runs):
        name, _, rest = t.partition(":")
        blocks, *marks = rest.split(",")
        assert marks == [mk for mk in ("t16", "rev", "head") if mk in marks], t          # known marks, once each, in order
        if "+" in blocks:
            a, b = map(int, blocks.split("+"))
            assert b == a + 1 and name == "fused_block2_h3w_kernel" and tokens[0] == "split", t     # a pair never follows compact
            seen += [a, b]
        elif "." in blocks:
            a, c = map(int, blocks.split("."))
            assert name == "conv3x3_c16_kernel", t
            convs.setdefault(a, []).append(c)
            if c == 0:
                seen.append(a)
        else:
            seen.append(int(blocks))
        if "head" in marks:
            carried += 1
            assert k == len(runs) - 1, line                                               # only the last launch carries the head
    assert seen == list(range(no_layers)), line                                           # every block once, in order
    assert all(c == list(range(block_convs)) for c in convs.values()), line               # ... and each of its convolutions
    assert carried <= 1 and (tokens[-1] == "head") == (carried == 0) and tokens.count("head") <= 1, line


def test_forward_plan_matches_the_restatement_over_a_seeded_sweep():
    """bf_debug_forward_plan -- the plan every forward runs from -- string for string against the restatement: depths 0..7 and 18,
    1 / 2 / 3 convolutions per block, heads the folded forms cannot carry, every inference option at each of its values, padded and
    unpadded sizes; and the structure every plan must have"""
    rng = np.random.default_rng(4242)
    values = {"arith": [0, 1], "fused_blocks": [0, 1], "h3_pair": [0, 1, 2], "h3_pair_head": [0, 1], "fused_head": [0, 1],
              "h3_compact": [0, 1], "h3_zigzag": [0, 1], "h3_variant": [-1, 1, 2, 4, 4 | 256]}
    models, pairs, compacts, carried = {}, 0, 0, 0
    for draw in range(400):
        no_layers = int(rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 18]))
        block_convs = int(rng.choice([1, 2, 2, 2, 2, 3]))
        head = [("linear", 3), ("linear", 3), ("relu", 3), ("linear", 1)][int(rng.integers(4))]
        key = (no_layers, block_convs) + head
        if key not in models:
            models[key] = _plan_model(*key)
        m = models[key]
        # most draws keep an option at its default, so that the interesting paths (pairs, compact) are reached often
        options = {k: int(rng.choice(v)) if rng.random() < 0.4 else PLAN_OPTIONS[k] for k, v in values.items()}
        for k, v in options.items():
            m.set_option(k, v)
        pad = bool(rng.integers(2))
        big = rng.random() < 0.5                       # both sides of the row counts where the selection changes
        H, W = int(rng.integers(1, 701)), int(rng.integers(1, 257 if rng.random() < 0.5 else 701))     # (256: the streaming kernel's width)
        B = int(rng.integers(1, 161)) if big else int(rng.integers(1, 9))
        got = m.forward_plan(B, H, W, pad_pow2=pad)
        want = _forward_plan(no_layers, block_convs, head == ("linear", 3), options, B, _pow2(H) if pad else H, _pow2(W) if pad else W)
        assert got == want, (draw, key, options, (B, H, W), pad)
        _check_plan_structure(got[0], got[1], no_layers, block_convs)
        pairs += "+" in got[0]
        compacts += got[0].startswith("compact")
        carried += ",head" in got[0]
    assert pairs >= 40 and compacts >= 10 and carried >= 10, (pairs, compacts, carried)      # the sweep did reach those paths


def test_forward_plan_error_cases():
    m = _plan_model(4)
    L = N.lib()
    buf = C.create_string_buffer(b"x" * 63, 64)
    assert L.bf_debug_forward_plan(None, 2, 32, 32, 1, buf, 64) == N.BF_EINVAL
    line, n = m.forward_plan(2, 32, 32)
    assert L.bf_debug_forward_plan(m._h, 2, 32, 32, 1, buf, 64) == N.BF_EINVAL and buf.value == b""     # too small: no truncated line
    assert "does not fit" in N.last_error(m._h)
    exact = C.create_string_buffer(len(line) + 1)
    assert L.bf_debug_forward_plan(m._h, 2, 32, 32, 1, exact, len(line) + 1) == n and exact.value.decode() == line
    assert L.bf_debug_forward_plan(m._h, 2, 32, 32, 1, exact, len(line)) == N.BF_EINVAL
    assert L.bf_debug_forward_plan(m._h, 0, 32, 32, 1, buf, 64) == N.BF_EINVAL
    assert L.bf_debug_forward_plan(m._h, 2, 32, 32, 1, None, 64) == N.BF_EINVAL


def test_load_model_errors_mirror_reference():
    with pytest.raises(ValueError, match="cannot be empty"):
        bf.load_model("")
    with pytest.raises(ValueError, match="cannot be empty"):
        bf.load_model(None)
    with pytest.raises(ValueError, match="does not exist"):
        bf.load_model("/definitely/not/here")
    with pytest.raises(ValueError, match="does not exist"):
        bf.load_denoiser_model("nope")
    with pytest.raises(ValueError, match="should not be None"):
        bf.DenoiserModule(None)


def test_denoiser_module_rejects_non_uint8_rank4(tmp_path):
    m = bf.model_builder(O.canonical_config(no_layers=1)["model"], device="cpu").hydra
    mod = bf.DenoiserModule(m)
    with pytest.raises(ValueError):
        mod(np.zeros((1, 8, 8, 3), np.float32))
    with pytest.raises(ValueError):
        mod(np.zeros((8, 8, 3), np.uint8))
    with pytest.raises(ValueError):
        mod(np.zeros((1, 8, 8, 1), np.uint8))
    assert mod(np.zeros((0, 8, 8, 3), np.uint8)).shape == (0, 8, 8, 3)       # empty batch
    with pytest.raises(RuntimeError, match="no CPU execution path"):
        mod(np.zeros((1, 8, 8, 3), np.uint8))


def test_save_and_load_model_directory(tmp_path):
    cfg = O.canonical_config(no_layers=2)
    m = bf.model_builder(cfg["model"], device="cpu", seed=5).hydra
    bf.save_model(m, str(tmp_path / "m"), cfg)
    mod = bf.load_model(str(tmp_path / "m"), device="cpu")
    p0, s0 = m.get_weights()
    p1, s1 = mod.model_hydra.get_weights()
    assert np.array_equal(p0, p1) and np.array_equal(s0, s1)
    assert bf.load_config(str(tmp_path / "m" / "pipeline.json"))["loss"]["hinge"] == 0.5


def test_load_config_and_shape_fixer():
    assert bf.input_shape_fixer(["?", "", "-1", 3]) == [None, None, None, 3]
    with pytest.raises(ValueError):
        bf.load_config(None)
    with pytest.raises(ValueError):
        bf.load_config("/no/such/file.json")
    assert bf.load_config({"a": 1}) == {"a": 1}
    assert len(bf.configs) == 3 and all("model" in c for _, c in bf.configs)


def test_schedules_match_keras_formulas():
    s = bf.schedule_builder({"type": "exponential_decay", "config": {"decay_rate": 0.9, "decay_steps": 40000, "learning_rate": 1e-3}})
    assert s(0) == 1e-3 and abs(s(20000) - 1e-3 * 0.9 ** 0.5) < 1e-15
    assert abs(s(20000) - O.exponential_decay(1e-3, 40000, 0.9, 20000)) < 1e-18
    c = bf.schedule_builder({"type": "cosine_decay", "config": {"decay_steps": 100, "learning_rate": 1.0, "alpha": 0.1}})
    assert abs(c(0) - 1.0) < 1e-12 and abs(c(100) - 0.1) < 1e-12 and abs(c(1000) - 0.1) < 1e-12
    r = bf.schedule_builder({"type": "cosine_decay_restarts", "config": {"decay_steps": 10, "learning_rate": 1.0}})
    assert abs(r(0) - 1.0) < 1e-12 and r(10) == pytest.approx(0.9 * (1 - 0.001) + 0.001)
    with pytest.raises(ValueError):
        bf.schedule_builder({"type": "nope"})
    with pytest.raises(ValueError):
        bf.schedule_builder({})
    d = bf.deep_supervision_schedule_builder({"type": "linear_low_to_high"}, 3)
    assert np.allclose(d(0.0), [1 / 6, 2 / 6, 3 / 6]) and np.allclose(d(1.0), [3 / 6, 2 / 6, 1 / 6])


def test_optimizer_builder_contract():
    cfg = O.canonical_config()["train"]["optimizer"]
    opt, sched = bf.optimizer_builder(cfg)
    assert opt.global_clipnorm == 1.0 and opt.lr() == 1e-3 and (opt.beta_1, opt.beta_2, opt.epsilon) == (0.9, 0.999, 1e-7)
    with pytest.raises(ValueError):
        bf.optimizer_builder("x")
    with pytest.raises(ValueError, match="don't know how to handle optimizer_type"):
        bf.optimizer_builder({"type": "sgd", "schedule": cfg["schedule"]})
    with pytest.raises(NotImplementedError):
        bf.optimizer_builder({"schedule": cfg["schedule"]})          # default RMSprop: outside the hot path
    # the optimizer section of the reference's shipped unet configs: per-tensor clipnorm + cosine restarts
    opt, sched = bf.optimizer_builder({"type": "ADAM", "gradient_clipping_by_norm_local": 1.0, "schedule": {
        "type": "cosine_decay_restarts", "config": {"t_mul": 1.1, "epsilon": 1e-5, "decay_rate": 0.9, "decay_steps": 40000,
                                                    "learning_rate": 0.001}}})
    assert (opt.clipnorm, opt.global_clipnorm, opt.clipvalue) == (1.0, None, None) and abs(opt.lr() - 1e-3) < 1e-9


def test_loss_builder_contract_and_monitor_values():
    fns = bf.loss_function_builder(O.canonical_config()["loss"])
    assert set(fns) == {"model", "denoiser"}
    d = fns["denoiser"].desc(0.5)
    assert (d.hinge, d.cutoff, d.mae_multiplier, d.regularization, d.depth_weight) == (0.5, 255.0, 1.0, pytest.approx(0.01), 0.5)
    gt = torch.zeros((2, 8, 8, 3))
    with pytest.raises(RuntimeError, match="GPU"):                        # monitoring values come from the HIP kernels only
        fns["denoiser"](gt, gt)


def test_pyramid_type_parsing():
    from blind_image_denoising_amd.pyramid import PyramidType
    assert PyramidType.from_string(" laplacian ") == PyramidType.LAPLACIAN
    for bad in (None, 3, "  "):
        with pytest.raises(ValueError):
            PyramidType.from_string(bad)
    with pytest.raises(KeyError):
        PyramidType.from_string("pyramid")


def test_graphed_module_argument_checks():
    import blind_image_denoising_amd as bf
    with pytest.raises(ValueError):
        bf.GraphedDenoiserModule(object())
    cfg = O.canonical_config(no_layers=1)
    m = bf.DenoiserModule(bf.model_builder(cfg["model"], device="cpu").hydra)
    with pytest.raises(ValueError):
        bf.GraphedDenoiserModule(m, max_shapes=0)
    g = bf.GraphedDenoiserModule(m)
    assert g.captured_shapes() == [] and g.name == m.name
    with pytest.raises(ValueError):
        g(np.zeros((1, 8, 8, 3), np.float32))


def test_h3_weight_scale_rule():
    """bf_debug_h3_weight_scale is a host call of the one function every split-f16 operator scales its weights with
    (csrc/h3_weights.h): s = 2^(14 - clip(exponent of m, -100, 100)) bit for bit, 1 for a zero or non-finite maximum, and
    m * s in [2^13, 2^14) wherever the clamp is not active."""
    f = N.lib().bf_debug_h3_weight_scale

    def rule(m):
        if not (m > 0 and np.isfinite(m)):
            return np.float32(1.0)
        return np.float32(np.ldexp(1.0, 14 - int(np.clip(np.frexp(m)[1], -100, 100))))

    f32 = np.float32
    edges = [f32(0.0), f32(-0.0), np.finfo(f32).tiny, f32(2.0 ** -120), f32(0.125), np.nextafter(f32(0.125), f32(0.0)), f32(1.0),
             f32(3.0), f32(2.0 ** 110), np.finfo(f32).max, f32(np.inf), f32(np.nan)]
    sweep = np.exp2(np.random.default_rng(20).uniform(-126.0, 127.99, 1000)).astype(f32)
    assert np.isfinite(sweep).all() and (sweep >= np.finfo(f32).tiny).all()
    for m in edges + list(sweep):
        got = f32(f(float(m)))
        assert got.tobytes() == rule(m).tobytes(), (m, got, rule(m))
        if m > 0 and np.isfinite(m) and -100 <= np.frexp(m)[1] <= 100:
            assert 2.0 ** 13 <= float(m) * float(got) < 2.0 ** 14, (m, got)
    for m in (0.0, np.inf, np.nan):
        assert f(m) == 1.0
