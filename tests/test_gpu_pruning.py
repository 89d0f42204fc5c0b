"""GPU tests of weight pruning (csrc/prune.hip, blind_image_denoising_amd/pruning.py) against a NumPy oracle written from the
strategies' definitions: the deterministic strategies bit for bit, the bifurcate strategy by the properties that must hold exactly,
then whole models of each class -- weights, sparsity report, and inference through the re-packed weights."""
import numpy as np
import pytest
import torch

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import pruning as P
from blind_image_denoising_amd.pruning import PruneStrategy as S
import pruning_models as PM

pytestmark = pytest.mark.gpu


# ---- the oracle: what NumPy computes on a float32 array with Python scalars ----------------------------------------------------

def oracle_minimum_threshold(x, t):
    x = x.copy()
    x[np.abs(x) < t] = 0.0
    return x


def oracle_shrinkage(x, t, shrinkage, shrinkage_threshold):
    x = x.copy()
    mask = np.abs(x) < shrinkage_threshold
    x[mask] = x[mask] * shrinkage
    x[np.abs(x) < t] = 0.0
    return x


def oracle_drop_bottom(x, percentage):
    """-> (pruned, threshold); IndexError where NumPy raises it (k == n)"""
    x = x.copy()
    s = np.sort(np.abs(x), axis=None)
    k = int(np.round(len(s) * percentage))
    threshold = s[k]
    x[np.abs(x) < threshold] = 0.0
    return x, threshold


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the synthetic flat vector -------------------------------------------------------------------------------------------------

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 4096, 70001]
GAPS = [1, 17]
SENTINEL = np.array([0x33D6BF95, 0xB3D6BF95, 0x00000001, 0x80000000, 0x7F800000], np.uint32).view(np.float32)   # +-1e-7, denormal, -0.0, inf

FILLS = {
    # name: (minimum_threshold, shrinkage, shrinkage_threshold, generator(rng, n))
    "normal": (0.01, 0.7, 0.03, lambda rng, n: (rng.standard_normal(n) * 0.05).astype(np.float32)),
    # multiples of 1/64: a few dozen distinct magnitudes, so the element of rank k sits inside a long run of ties
    "ties": (3.0 / 64.0, 0.5, 6.0 / 64.0, lambda rng, n: (np.round(rng.standard_normal(n) * 8.0) / 64.0).astype(np.float32)),
    # 1 + j 2^-23, j < 256: the three high radix bytes of every |w| are equal and only the last pass separates them
    "last_byte": (1.0 + 100 * 2.0 ** -23, 0.999, 1.0 + 200 * 2.0 ** -23,
                  lambda rng, n: ((1.0 + rng.integers(0, 256, n) * 2.0 ** -23) * rng.choice([-1.0, 1.0], n)).astype(np.float32)),
}


def layout():
    """[(begin, end)] of the pruned tensors and the total length: gap, tensor, gap, ..., tensor, gap with gaps of 1 and 17"""
    ranges, o = [], 0
    for i, n in enumerate(SIZES):
        o += GAPS[i % 2]
        ranges.append((o, o + n))
        o += n
    return ranges, o + GAPS[len(SIZES) % 2]


def build_vector(fill, seed=0):
    t, _, _, gen = FILLS[fill]
    rng = np.random.default_rng(seed)
    ranges, total = layout()
    w = np.resize(SENTINEL, total).copy()
    special = np.array([0.0, -0.0, t, -t], np.float32)                 # +0.0, -0.0 and exact hits of +-t in every fill
    for b, e in ranges:
        x = gen(rng, e - b)
        at = rng.permutation(e - b)[:4]
        x[at] = special[-len(at):]
        w[b:e] = x
    return w


def gap_mask(ranges, total):
    m = np.ones(total, bool)
    for b, e in ranges:
        m[b:e] = False
    return m


@pytest.fixture(scope="module")
def vectors():
    """the three fills and their oracle results, computed once and never modified"""
    ranges, total = layout()
    out = {}
    for fill, (t, sh, sht, _) in FILLS.items():
        w = build_vector(fill)
        w.setflags(write=False)
        ref = {"threshold": w.copy(), "shrinkage": w.copy()}
        for b, e in ranges:
            ref["threshold"][b:e] = oracle_minimum_threshold(w[b:e], t)
            ref["shrinkage"][b:e] = oracle_shrinkage(w[b:e], t, sh, sht)
        out[fill] = (w, ref)
    return ranges, total, out


def device_ranges(ranges):
    return torch.tensor(ranges, dtype=torch.int64).reshape(-1, 2).cuda()


def assert_bits_per_tensor(got, want, ranges, total, what):
    for b, e in ranges:
        assert np.array_equal(bits(got[b:e]), bits(want[b:e])), f"{what}: tensor of {e - b} elements differs"
    gaps = gap_mask(ranges, total)
    assert np.array_equal(bits(got[gaps]), bits(want[gaps])), f"{what}: an element outside every range was written"


# ---- kernel level ----------------------------------------------------------------------------------------------------------------

def test_the_fills_hold_what_they_are_meant_to(vectors):
    ranges, total, data = vectors
    for fill, (w, _) in data.items():
        t = np.float32(FILLS[fill][0])
        for b, e in ranges:
            if e - b >= 4:
                x = w[b:e]
                assert (bits(x) == 0).any() and (bits(x) == 0x80000000).any() and (x == t).any() and (x == -t).any()
    big = data["last_byte"][0][ranges[-1][0]:ranges[-1][1]]
    assert len(np.unique(bits(np.abs(big[big != 0])) >> 8)) == 1            # one value of the three high bytes
    tied = data["ties"][0][ranges[-1][0]:ranges[-1][1]]
    assert len(np.unique(np.abs(tied))) < 80


@pytest.mark.parametrize("fill", list(FILLS))
def test_elementwise_strategies_equal_numpy_bit_for_bit(vectors, fill):
    ranges, total, data = vectors
    w, ref = data[fill]
    t, sh, sht, _ = FILLS[fill]
    rd = device_ranges(ranges)
    for what, strategy, kw in (("none", S.NONE, {}),
                               ("threshold", S.MINIMUM_THRESHOLD, dict(minimum_threshold=t)),
                               ("shrinkage", S.MINIMUM_THRESHOLD_SHRINKAGE, dict(minimum_threshold=t, shrinkage=sh, shrinkage_threshold=sht))):
        d = torch.from_numpy(w.copy()).cuda()
        P.prune_tensors(d, rd, strategy, **kw)
        got = d.cpu().numpy()
        want = w if what == "none" else ref[what]
        assert_bits_per_tensor(got, want, ranges, total, f"{fill} / {what}")
        if what != "none":
            assert not np.array_equal(bits(got), bits(w))                    # the strategy did something


def largest_percentage_with_rank(n, k):
    """the largest float p with int(np.round(n * p)) == k"""
    p = (k + 0.5) / n
    while int(np.round(n * p)) > k:
        p = np.nextafter(p, 0.0)
    while int(np.round(n * np.nextafter(p, 1.0))) == k:
        p = np.nextafter(p, 1.0)
    return float(p)


@pytest.mark.parametrize("percentage", [0.0, 0.1, 0.5, 0.9, "last"])
@pytest.mark.parametrize("fill", list(FILLS))
def test_drop_bottom_equals_numpy_bit_for_bit(vectors, fill, percentage):
    ranges, total, data = vectors
    w, _ = data[fill]
    want, kth, thr, kept = w.copy(), [], [], []
    for b, e in ranges:
        n = e - b
        p = largest_percentage_with_rank(n, n - 1) if percentage == "last" else percentage
        k = int(np.round(n * p))                                             # the expression the host side uses
        if percentage == "last":
            assert k == n - 1 and int(np.round(n * np.nextafter(p, 1.0))) == n
        if k == n:
            # NumPy raises here (x_sorted[n]) and so does the host side before it launches anything: the tensor is left out of the
            # table, where it has to stay untouched like any gap
            with pytest.raises(IndexError):
                oracle_drop_bottom(w[b:e], p)
            assert percentage == 0.9 and n in (1, 2)
            continue
        want[b:e], threshold = oracle_drop_bottom(w[b:e], p)
        assert threshold == np.sort(np.abs(w[b:e]))[k]
        kept.append((b, e)); kth.append(k); thr.append(threshold)
    d = torch.from_numpy(w.copy()).cuda()
    found = P.prune_tensors(d, device_ranges(kept), S.DROP_BOTTOM, kth=torch.tensor(kth, dtype=torch.int64).cuda())
    got = d.cpu().numpy()
    assert np.array_equal(bits(found.cpu().numpy()), bits(np.array(thr, np.float32))), (found.cpu().numpy(), thr)
    assert_bits_per_tensor(got, want, kept, total, f"{fill} / drop_bottom {percentage}")
    if percentage == "last" and fill == "normal":
        b, e = ranges[-1]
        assert np.count_nonzero(got[b:e]) == 1                               # everything below the largest magnitude went


@pytest.mark.parametrize("fill", list(FILLS))
def test_count_below_equals_numpy(vectors, fill):
    ranges, total, data = vectors
    w, ref = data[fill]
    rd = device_ranges(ranges)
    for vec in (w, ref["threshold"]):
        d = torch.from_numpy(vec.copy()).cuda()
        for thr in (0.0, 0.01):
            got = P.count_below(d, rd, thr).cpu().numpy()
            want = [np.count_nonzero(np.abs(vec[b:e]) <= thr) for b, e in ranges]
            assert got.dtype == np.int64 and np.array_equal(got, want), (fill, thr, got, want)
        assert np.array_equal(bits(d.cpu().numpy()), bits(vec))              # a report writes nothing


def test_bifurcate_properties():
    ranges, total = layout()
    t = 0.01
    t32 = np.float32(t)
    w = build_vector("normal", seed=3)
    rd = device_ranges(ranges)

    def run(vec, seed, table=rd):
        d = torch.from_numpy(vec.copy()).cuda()
        P.prune_tensors(d, table, S.MINIMUM_THRESHOLD_BIFURCATE, minimum_threshold=t, seed=seed)
        return d.cpu().numpy()

    got = run(w, seed=1234)
    gaps = gap_mask(ranges, total)
    assert np.array_equal(bits(got[gaps]), bits(w[gaps]))
    inside = ~gaps
    below = inside & (np.abs(w) < t32)
    keep = inside & ~below
    assert below.sum() > 5000
    assert np.array_equal(bits(got[keep]), bits(w[keep]))                    # |w| >= t: unchanged bit for bit
    a = np.abs(got[below])
    assert ((bits(got[below]) == 0) | ((a >= t32) & (a < np.float32(2.0) * t32))).all()   # 0 (+0.0) or t <= |w| < 2t
    assert (a >= t32).sum() > 1000 and (got[below][a >= t32] > 0).any() and (got[below][a >= t32] < 0).any()
    assert np.array_equal(bits(run(w, seed=1234)), bits(got))                # same seed: same bits
    other = run(w, seed=1235)
    assert not np.array_equal(bits(other[below]), bits(got[below]))          # another seed: other draws
    assert np.array_equal(bits(other[keep]), bits(got[keep]))
    # the draw of an element depends on its position in the vector alone: the largest tensor given as two ranges
    b, e = ranges[-1]
    split = device_ranges(ranges[:-1] + [(b, b + 12345), (b + 12345, e)])
    assert np.array_equal(bits(run(w, seed=1234, table=split)), bits(got))

    # the 70 001-element tensor filled entirely below t: half of the draws land below t and become 0
    rng = np.random.default_rng(9)
    low = w.copy()
    low[b:e] = (rng.uniform(-1.0, 1.0, e - b) * 0.0099).astype(np.float32)
    assert (np.abs(low[b:e]) < t32).all()
    share = np.count_nonzero(run(low, seed=77)[b:e] == 0) / (e - b)
    print(f"bifurcate: zeroed share {share:.5f} of {e - b}")
    assert abs(share - 0.5) <= 0.0095                                        # five binomial standard deviations: 5 * 0.5 / sqrt(70 001)


def test_refused_arguments():
    ranges, total = layout()
    d = torch.zeros(total, dtype=torch.float32, device="cuda")
    rd = device_ranges(ranges)
    with pytest.raises(NotImplementedError):
        P.prune_tensors(d, rd, S.PCA_PROJECTION)
    with pytest.raises(ValueError):
        P.prune_tensors(d, rd, S.DROP_BOTTOM)                                # no ranks
    with pytest.raises(ValueError):
        P.prune_tensors(d, rd.to(torch.int32), S.MINIMUM_THRESHOLD, 0.1)


# ---- model level -----------------------------------------------------------------------------------------------------------------

IMAGE = np.random.default_rng(11).integers(0, 256, (1, 16, 16, 3), dtype=np.uint8)
MODEL_STRATEGIES = {
    "minimum_threshold": ({"type": "minimum_threshold", "config": {"minimum_threshold": 0.02}},
                          lambda x: oracle_minimum_threshold(x, 0.02)),
    "drop_bottom": ({"type": "drop_bottom", "config": {"percentage": 0.3}}, lambda x: oracle_drop_bottom(x, 0.3)[0]),
}


def state_of(model):
    w = model.get_weights()
    return w[1].copy() if isinstance(w, tuple) else None


def sparsity_numpy(w, ranges, threshold):
    tensors = {n: (int(np.count_nonzero(np.abs(w[b:e]) <= threshold)), e - b) for n, b, e in ranges}
    count, size = sum(c for c, _ in tensors.values()), sum(s for _, s in tensors.values())
    return {"tensors": tensors, "count": count, "size": size, "fraction": count / size}


@pytest.mark.parametrize("strategy", list(MODEL_STRATEGIES))
@pytest.mark.parametrize("family", list(PM.MODELS))
def test_models_are_pruned_as_numpy_prunes_them(family, strategy):
    make, cls = PM.MODELS[family]
    config, oracle = MODEL_STRATEGIES[strategy]
    model = bf.model_builder(make(), device="cuda", seed=5).hydra
    assert type(model).__name__ == cls
    module = bf.DenoiserModule(model)
    before_out = module(IMAGE)                                               # packs the unpruned weights
    w0, state = PM.params_of(model), state_of(model)
    ranges = bf.conv2d_ranges(model)
    want = w0.copy()
    for _, b, e in ranges:
        want[b:e] = oracle(w0[b:e])
    assert bf.conv2d_sparsity(model) == sparsity_numpy(w0, ranges, 0.0)

    assert bf.prune_function_builder(config)(model) is model
    w1 = PM.params_of(model)
    assert np.array_equal(bits(w1), bits(want))                              # kernels as the oracle, everything else untouched
    assert not np.array_equal(bits(w1), bits(w0))
    if state is not None:
        assert np.array_equal(bits(state_of(model)), bits(state))
    for threshold in (0.0, 0.01):
        assert bf.conv2d_sparsity(model, threshold) == sparsity_numpy(want, ranges, threshold)
    assert np.array_equal(bits(bf.get_conv2d_weights(model)), bits(np.concatenate([want[b:e] for _, b, e in ranges])))
    if strategy == "drop_bottom":
        # rank k of a tensor without ties leaves exactly k zeros; ties at the threshold survive
        ties = sum(np.count_nonzero(np.abs(w0[b:e]) == np.sort(np.abs(w0[b:e]))[int(np.round((e - b) * 0.3))]) - 1 for _, b, e in ranges)
        floor = sum(int(np.round((e - b) * 0.3)) for _, b, e in ranges) - ties
        report = bf.conv2d_sparsity(model)
        assert report["count"] >= floor and report["fraction"] >= 0.3 - (ties + 0.5 * len(ranges)) / report["size"]

    # inference reads a packed copy of the weights: it must be the pruned one
    fresh = bf.model_builder(make(), device="cuda", seed=99).hydra
    if state is None:
        fresh.set_weights(want)
    else:
        fresh.set_weights(want, state)
    after_out = module(IMAGE)
    assert after_out.dtype == np.uint8 and after_out.shape == IMAGE.shape
    assert np.array_equal(after_out, bf.DenoiserModule(fresh)(IMAGE))
    assert not np.array_equal(after_out, before_out)


def test_a_list_of_strategies_runs_in_order():
    model = bf.model_builder(PM.engine_config(), device="cuda", seed=6).hydra
    w0 = PM.params_of(model)
    prune = bf.prune_function_builder([
        {"type": "none", "config": {}},
        {"type": "minimum_threshold_shrinkage", "config": {"minimum_threshold": 0.01, "shrinkage": 0.7, "shrinkage_threshold": 0.05}},
        {"type": "drop_bottom", "config": {"percentage": 0.5}}])
    prune(model)
    want = w0.copy()
    for _, b, e in bf.conv2d_ranges(model):
        want[b:e] = oracle_drop_bottom(oracle_shrinkage(w0[b:e], 0.01, 0.7, 0.05), 0.5)[0]
    assert np.array_equal(bits(PM.params_of(model)), bits(want))
    report = bf.conv2d_sparsity(model)
    assert report["fraction"] >= 0.5 - 0.5 * len(report["tensors"]) / report["size"]       # no ties in continuous weights
    version = model.version
    bf.prune_function_builder({"type": "none", "config": {}})(model)          # NONE launches nothing and leaves the packed copy alone
    assert model.version == version


def test_a_captured_graph_is_refreshed_after_pruning():
    model = bf.model_builder(PM.engine_config(), device="cuda", seed=7).hydra
    module = bf.DenoiserModule(model)
    graphed = bf.GraphedDenoiserModule(module)
    first = graphed(IMAGE)
    assert np.array_equal(first, module(IMAGE))
    key = tuple(IMAGE.shape)
    graph_before, stamp_before = graphed._graphs[key][0], graphed._graphs[key][3]
    assert np.array_equal(graphed(IMAGE), first) and graphed._graphs[key][0] is graph_before     # replayed, not re-captured
    bf.prune_function_builder({"type": "drop_bottom", "config": {"percentage": 0.3}})(model)
    second = graphed(IMAGE)
    assert graphed._graphs[key][0] is not graph_before and graphed._graphs[key][3] != stamp_before
    assert np.array_equal(second, module(IMAGE))
    assert not np.array_equal(second, first)


def test_the_command_line_tool_prunes_a_saved_model(tmp_path, capsys):
    import importlib.util
    import pathlib
    spec = importlib.util.spec_from_file_location("prune_tool", pathlib.Path(__file__).resolve().parent.parent / "tools" / "prune.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    model = bf.model_builder(PM.engine_config(), device="cuda", seed=8).hydra
    w0 = PM.params_of(model)
    bf.save_model(model, str(tmp_path / "in"))
    before, after = tool.main([str(tmp_path / "in"), "--config", '{"type": "drop_bottom", "config": {"percentage": 0.5}}',
                               "--output", str(tmp_path / "out"), "--per-tensor"])
    want = w0.copy()
    for _, b, e in bf.conv2d_ranges(model):
        want[b:e] = oracle_drop_bottom(w0[b:e], 0.5)[0]
    pruned = bf.model.load_hydra(str(tmp_path / "out"))
    assert np.array_equal(bits(PM.params_of(pruned)), bits(want))
    assert np.array_equal(bits(PM.params_of(model)), bits(w0))                # the tool worked on its own copy
    assert before["count"] == 0 and after == bf.conv2d_sparsity(pruned) and after["fraction"] >= 0.49
    out = capsys.readouterr().out
    assert "before" in out and "after drop_bottom" in out and "saved to" in out
