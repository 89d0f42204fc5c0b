"""Host side of blind_image_denoising_amd/pruning.py (no GPU): the strategy enum, the builder's argument checks and refusals, and the
table of convolution-kernel ranges each model class hands to the device."""
import numpy as np
import pytest

import blind_image_denoising_amd as bf
from blind_image_denoising_amd import pruning as P
import pruning_models as PM


def test_strategy_enum_round_trips():
    want = {"NONE": 0, "MINIMUM_THRESHOLD": 1, "MINIMUM_THRESHOLD_BIFURCATE": 2, "MINIMUM_THRESHOLD_SHRINKAGE": 3,
            "PCA_PROJECTION": 4, "DROP_BOTTOM": 5}
    assert {s.name: s.value for s in bf.PruneStrategy} == want
    for s in bf.PruneStrategy:
        assert bf.PruneStrategy.from_string(s.to_string()) is s
        assert bf.PruneStrategy.from_string(f"  {s.name.lower()} ") is s
        assert s.to_string() == s.name


@pytest.mark.parametrize("bad, error", [(None, ValueError), (3, ValueError), ("", ValueError), ("   ", ValueError),
                                        ("no_such_strategy", KeyError)])
def test_from_string_errors(bad, error):
    with pytest.raises(error):
        bf.PruneStrategy.from_string(bad)


def test_builder_argument_checks():
    with pytest.raises(ValueError, match="None"):
        bf.prune_function_builder(None)
    for not_a_config in (3, "minimum_threshold", (1, 2)):
        with pytest.raises(ValueError, match="don't know how to handle"):
            bf.prune_function_builder(not_a_config)
    with pytest.raises(KeyError):
        bf.prune_function_builder({"type": "no_such_strategy", "config": {}})
    with pytest.raises(KeyError):
        bf.prune_function_builder({"type": "minimum_threshold", "config": {}})                    # minimum_threshold missing
    with pytest.raises(KeyError):
        bf.prune_function_builder({"type": "minimum_threshold_shrinkage", "config": {"minimum_threshold": 0.1, "shrinkage": 0.5}})
    with pytest.raises(KeyError):
        bf.prune_function_builder({"type": "drop_bottom", "config": {}})
    with pytest.raises(KeyError):
        bf.prune_function_builder({"config": {"minimum_threshold": 0.1}})                          # type missing
    with pytest.raises(KeyError):
        bf.prune_function_builder({"type": "minimum_threshold"})                                   # config missing


def test_builder_accepts_a_dict_and_a_list():
    one = bf.prune_function_builder({"type": "minimum_threshold", "config": {"minimum_threshold": 0.001}})
    assert callable(one) and one.strategies == [bf.PruneStrategy.MINIMUM_THRESHOLD]
    many = bf.prune_function_builder([
        {"type": "none", "config": {}},
        {"type": "minimum_threshold_shrinkage", "config": {"minimum_threshold": 0.001, "shrinkage": 0.9, "shrinkage_threshold": 0.01}},
        {"type": "minimum_threshold_bifurcate", "config": {"minimum_threshold": 0.001}},
        {"type": "drop_bottom", "config": {"percentage": 0.25}}], seed=1)
    assert callable(many)
    assert [s.value for s in many.strategies] == [0, 3, 2, 5]
    assert callable(bf.prune_function_builder([]))


def test_pca_projection_is_refused_when_the_function_is_built():
    with pytest.raises(NotImplementedError, match="PCA_PROJECTION"):
        bf.prune_function_builder({"type": "pca_projection", "config": {"variance": 0.9}})
    with pytest.raises(NotImplementedError, match="PCA_PROJECTION"):
        bf.prune_function_builder([{"type": "minimum_threshold", "config": {"minimum_threshold": 0.1}},
                                   {"type": "PCA_PROJECTION", "config": {"variance": 0.9, "scale": False}}])


def test_drop_bottom_of_everything_is_numpys_index_error():
    x_sorted = np.sort(np.abs(np.arange(7, dtype=np.float32)))
    with pytest.raises(IndexError):
        x_sorted[int(np.round(len(x_sorted) * 1.0))]                                               # what the reference runs into
    with pytest.raises(IndexError):
        bf.prune_function_builder({"type": "drop_bottom", "config": {"percentage": 1.0}})
    # a percentage that is out of bounds for SOME tensors only is found from the table, on the host
    m = bf.model_builder(PM.engine_config(), device="cpu", seed=0).hydra
    table = P._table(m)
    sizes = table.sizes
    assert np.array_equal(table.ranks(0.3), [int(np.round(int(n) * 0.3)) for n in sizes])
    smallest = int(sizes.min())
    p = 1.0 - 0.25 / smallest                                                                      # rounds to n for the smallest tensor
    assert int(np.round(smallest * p)) == smallest
    with pytest.raises(IndexError, match="out of bounds"):
        table.ranks(p)
    assert np.array_equal(table.ranks(-0.25), [n + int(np.round(int(n) * -0.25)) for n in sizes])  # x_sorted[-k]: from the end


RICHER = {
    "engine": {},
    "resnet_generic": dict(add_gates=True, add_initial_bn=True, add_final_bn=True, add_channelwise_scaling=True,
                           add_learnable_multiplier=True),
    "unet_backbone": dict(add_gates=True, add_channelwise_scaling=True, add_learnable_multiplier=True),
    "unet_laplacian": dict(depth=3, use_attention_gates=True),
}


@pytest.mark.parametrize("family", list(PM.MODELS))
@pytest.mark.parametrize("rich", [False, True], ids=["small", "rich"])
def test_range_table_holds_exactly_the_convolution_kernels(family, rich):
    make, cls = PM.MODELS[family]
    cfg = make(**RICHER[family]) if rich and RICHER[family] else make()
    m = bf.model_builder(cfg, device="cpu", seed=0).hydra
    assert type(m).__name__ == cls
    variables = PM.variables(m)
    ranges = bf.conv2d_ranges(m)
    want = [(n, o, o + int(np.prod(s))) for n, s, k, o in variables if k in (0, "conv", "depthwise")]
    assert ranges == want and len(ranges) > 0
    assert all(name.endswith("kernel") for name, _, _ in ranges)
    others = [(n, k) for n, s, k, o in variables if k not in (0, "conv", "depthwise")]
    assert not {n for n, _ in others} & {n for n, _, _ in ranges}
    for name, kind in others:                          # gammas, multipliers, dense gate weights: never in the table
        assert "gamma" in name or "w0" in name or name.endswith("/w") or "dense" in name, (name, kind)
    if rich and family in ("resnet_generic", "unet_backbone"):
        assert {"dense", "bn_gamma", "channelwise", "multiplier"} <= {k for _, k in others}
    if family == "unet_laplacian":
        assert {"ln_gamma", "multiplier"} <= {k for _, k in others}
        assert any(k == "depthwise" for _, _, k, _ in variables)
    if family == "resnet_generic":
        assert any(k == "depthwise" for _, _, k, _ in variables)
    if family == "engine":
        assert any(k == 1 for _, k in others)           # BatchNorm gammas
    # sorted, disjoint, inside the vector; every kernel weight is covered once and nothing else is
    table = P._table(m)
    assert table.names == [n for n, _, _ in ranges]
    assert np.array_equal(table.host, [[b, e] for _, b, e in ranges]) and table.host.dtype == np.int64
    assert (table.host[:, 0] < table.host[:, 1]).all() and table.host[0, 0] >= 0 and table.host[-1, 1] <= m.params.numel()
    assert (table.host[1:, 0] >= table.host[:-1, 1]).all()
    covered = np.zeros(m.params.numel(), np.int32)
    for _, b, e in ranges:
        covered[b:e] += 1
    kernel_mask = np.zeros(m.params.numel(), np.int32)
    for n, s, k, o in variables:
        if k in (0, "conv", "depthwise"):
            kernel_mask[o:o + int(np.prod(s))] = 1
    assert np.array_equal(covered, kernel_mask)
    assert P._table(m) is table                         # built once per model
    # get_conv2d_weights: the kernels concatenated in variable order (a plain gather: also runs on a host model)
    w = PM.params_of(m)
    assert np.array_equal(bf.get_conv2d_weights(m), np.concatenate([w[b:e] for _, b, e in ranges]))


@pytest.mark.parametrize("family", list(PM.MODELS))
def test_pruning_a_cpu_model_names_the_gpu(family):
    m = bf.model_builder(PM.MODELS[family][0](), device="cpu", seed=0).hydra
    before = PM.params_of(m)
    for cfg in ({"type": "minimum_threshold", "config": {"minimum_threshold": 0.01}},
                {"type": "drop_bottom", "config": {"percentage": 0.3}},
                {"type": "none", "config": {}}):
        with pytest.raises(RuntimeError, match="GPU"):
            bf.prune_function_builder(cfg)(m)
    with pytest.raises(RuntimeError, match="GPU"):
        bf.conv2d_sparsity(m)
    with pytest.raises(RuntimeError, match="GPU"):
        P.prune_tensors(m.params, P._table(m).ranges("cpu"), bf.PruneStrategy.MINIMUM_THRESHOLD, 0.01)
    assert np.array_equal(PM.params_of(m), before)
    with pytest.raises(ValueError):
        bf.prune_function_builder({"type": "none", "config": {}})(None)


def test_native_signatures_cover_the_new_entries():
    from blind_image_denoising_amd import _native as N
    L = N.lib()
    assert L.bf_abi_version() == 1
    for name in ("bf_op_prune_tensors", "bf_op_count_below"):
        assert name in N.SIGNATURES and hasattr(L, name)
    # NULL / empty arguments are refused before anything is launched
    assert L.bf_op_prune_tensors(None, 8, None, 1, 1, 0.1, 1.0, 0.0, 0, None, None, None) == N.BF_EINVAL
    assert L.bf_op_count_below(None, 8, None, 1, 0.0, None, None) == N.BF_EINVAL


def _tool():
    import importlib.util
    import pathlib
    spec = importlib.util.spec_from_file_location("prune_tool", pathlib.Path(__file__).resolve().parent.parent / "tools" / "prune.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_reads_its_config_and_refuses_before_loading_a_model(tmp_path):
    tool = _tool()
    cfg = {"type": "drop_bottom", "config": {"percentage": 0.5}}
    assert tool.read_config('{"type": "drop_bottom", "config": {"percentage": 0.5}}') == cfg
    path = tmp_path / "prune.json"
    path.write_text('[{"type": "drop_bottom", "config": {"percentage": 0.5}}]')
    assert tool.read_config(str(path)) == [cfg]
    with pytest.raises(SystemExit):
        tool.read_config("not json")
    with pytest.raises(NotImplementedError, match="PCA_PROJECTION"):
        tool.main(["no/such/model", "--config", '{"type": "pca_projection", "config": {"variance": 0.9}}'])
    report = {"tensors": {"a/kernel": (1, 4), "b/kernel": (0, 4)}, "count": 1, "size": 8, "fraction": 0.125}
    assert tool.format_sparsity(report, True).splitlines()[-1] == "  total  1 / 8  12.50%"
    assert len(tool.format_sparsity(report, True).splitlines()) == 3 and len(tool.format_sparsity(report, False).splitlines()) == 1
