"""Model sections the pruning tests share: the smallest instance of each of the four model classes."""
import copy

from oracle import bfcnn_oracle as O
from oracle import resnet_generic_oracle as G
from oracle import unet_oracle as U
import unet_backbone_torch as UB


def engine_config():
    """the 2-block canonical 16-filter model (HydraModel)"""
    return copy.deepcopy(O.canonical_config(no_layers=2)["model"])


def resnet_generic_config(**bb):
    """the shipped bottleneck (1x1 -> depthwise 3x3 x4 -> grouped 1x1, 32 filters) with two blocks (GenericResnetHydra)"""
    cfg = G.shipped_config()
    cfg["backbone"].update(no_layers=2, **bb)
    return cfg


def unet_backbone_config(**bb):
    """the plain unet, 32 filters, two levels (UnetHydra)"""
    return UB.config(no_levels=2, **bb)


def unet_laplacian_config(**bb):
    """unet_laplacian, depth 2, width 1, 32 filters (UnetLaplacianHydra)"""
    cfg = copy.deepcopy(U.canonical_config(depth=2, width=1, filters=32)["model"])
    cfg["backbone"].update(bb)
    return cfg


MODELS = {
    "engine": (engine_config, "HydraModel"),
    "resnet_generic": (resnet_generic_config, "GenericResnetHydra"),
    "unet_backbone": (unet_backbone_config, "UnetHydra"),
    "unet_laplacian": (unet_laplacian_config, "UnetLaplacianHydra"),
}


def variables(model):
    """[(name, shape, kind, offset)] of either model family"""
    return [(v.name, tuple(v.shape), v.kind, v.offset) if hasattr(v, "kind") else (v[0], tuple(v[1]), v[2], v[3])
            for v in model.trainable_variables]


def params_of(model):
    """the flat parameter vector as a host array (get_weights returns it alone or with the moving statistics)"""
    w = model.get_weights()
    return (w[0] if isinstance(w, tuple) else w).copy()
