"""
blind_image_denoising_amd -- MI355X-native engine for the bfcnn resnet-denoiser hot path.

Mirrors the public surface of the reference package (bfcnn/__init__.py:127-141) for that path:
`load_model`, `load_denoiser_model`, `models`, `configs`, `model_builder`, `DenoiserModule`,
`loss_function_builder`, `optimizer_builder`, `schedule_builder`, `train_loop`,
`build_pyramid_model`, `build_inverse_pyramid_model`.  All arithmetic runs in hand-written
gfx950 HIP kernels behind the C ABI of include/bfcnn_hip.h (lib/libbfcnn_hip.so); torch is
used only for device memory, streams and torch.distributed.  There is no CPU fallback.
"""
import os
import pathlib

__version__ = "0.1.0"

from .constants import *
from .custom_logger import logger
from .utilities import load_config, save_config, input_shape_fixer
from .model import (BuilderResults, HydraModel, model_builder, describe_resnet, save_model, load_hydra,
                    build_normalize_model, build_denormalize_model)
from .module_denoiser import DenoiserModule, DenoiserWrapper, GraphedDenoiserModule
from . import self_ensemble as _self_ensemble
from .self_ensemble import SelfEnsembleDenoiserModule
from .loss import loss_function_builder
from .optimizer import optimizer_builder, schedule_builder, deep_supervision_schedule_builder
from .train_loop import (train_loop, build_train_functions, DataParallelTrainer, NativeCommunicator, shard_batch,
                         allreduce_gradients)
from .checkpoint import Checkpoint, CheckpointManager
from .resnet_generic import squeeze_and_excite_block, selector_block
from .pyramid import (build_pyramid_model, build_inverse_pyramid_model, multiscales_generator_fn)
from .dataset import dataset_builder, PrepareData, noise_augment
from .export_model import export_model
from .file_operations import load_image
from . import metrics
from .metrics import ImageMetrics, image_metrics, image_metric_sums, psnr, ssim, mae, evaluate
from .noise_estimate import NoiseEstimate, noise_statistics, noise_summary, estimate_noise, evaluate_blind
from . import noise_level
from .noise_level import NoiseLevelFunction, noise_level_statistics, noise_level_function, camera_noise
from . import risk
from .risk import RiskEstimate, risk_probe_stack_u8, risk_sums, estimate_risk, evaluate_blind_risk, format_risk_report
from .risk import risk_sums_affine, risk_from_affine_sums, estimate_risk_affine
from . import vst
from .vst import StabilisedDenoiserModule, stabilise_u8, unstabilise, evaluate_camera, format_camera_report
from . import tiling
from .tiling import TilePlan, TiledDenoiserModule, tile_plan, tile_split_u8, tile_blend, receptive_radius
from . import pixel_shuffle
from .pixel_shuffle import (NoiseCorrelation, PixelShuffleDenoiserModule, noise_correlation, noise_correlation_statistics,
                            pd_split_u8, pd_merge, pd_replace_u8, pd_mean)
from .pixel_shuffle import parse_setting as pixel_shuffle_settings
from . import burst
from .burst import BurstDenoiserModule, burst_pyramid, burst_align, burst_thresholds, burst_merge
from .burst import parse_setting as burst_settings
from . import video as _video
from .video import VideoDenoiserModule, VideoState, video_state, video_update
from .video import parse_setting as video_settings
from . import nlm as _nlm
from .nlm import NlmDenoiserModule, nlm, nlm_params, nlm_table, nlm_tune
from .nlm import parse_setting as nlm_settings
from . import bm3d as _bm3d
from .bm3d import Bm3dDenoiserModule, bm3d, bm3d_params, bm3d_step
from .bm3d import parse_setting as bm3d_settings
from . import restore as _restore
from .restore import (RestoreConstraint, RestoreResult, mask_constraint, block_constraint, restore_init, restore_direction,
                      restore_step, restore_finish, restore, inpaint, super_resolve, bayer_mask)
from . import degrade
from .degrade import Degradations, degrade_jpeg, degrade_blur, degrade_pointwise, gaussian_taps
from . import neighbor
from .neighbor import neighbor_pairs, NeighborPairs, RiskValidator, parse_self_supervised_config
from . import regularizers
from . import pruning
from .pruning import (PruneStrategy, prune_function_builder, get_conv2d_weights, conv2d_sparsity, conv2d_ranges)
from .custom_layers import RandomOnOff, Multiplier, ChannelwiseMultiplier

current_dir = pathlib.Path(__file__).parent.resolve()

# ---- configs (bfcnn/__init__.py:29-44): every *.json in configs/ ------------------------------
configs_dir = current_dir / "configs"
configs = []
if configs_dir.is_dir():
    for _f in sorted(configs_dir.glob("*.json")):
        try:
            configs.append((os.path.basename(str(_f)), load_config(str(_f))))
        except Exception as _e:     # a broken config must not break import
            logger.error(f"failed to load config [{_f}]: {_e}")

CONFIGS_DICT = {os.path.splitext(name)[0]: cfg for name, cfg in configs}          # bfcnn/__init__.py:41-44

# ---- pretrained registry (bfcnn/__init__.py:48-75) --------------------------------------------
pretrained_dir = current_dir / "pretrained"
models = {}


def _make_loader(directory):
    # bound per directory (the reference closure late-binds its loop variable, __init__.py:58-64)
    def load_denoiser_module():
        return DenoiserModule(load_hydra(str(directory)))
    return load_denoiser_module


if pretrained_dir.is_dir():
    for _d in [d for d in sorted(pretrained_dir.iterdir()) if d.is_dir()]:
        models[str(_d.name)] = {
            "directory": _d,
            DENOISER_STR: _make_loader(_d),
            "configuration": str(_d / PIPELINE_FILE_STR),
            "saved_model_path": str(_d),
        }


# load_model's wrappers, innermost first: (keyword, its parse_setting: the option's value -> the keyword arguments of the wrapper,
# or None for no wrapper, ValueError for a bad one; the wrapper).  burst and video both go outermost: one of them at most
_WRAPPERS = (("self_ensemble", _self_ensemble.parse_setting, SelfEnsembleDenoiserModule),
             ("tiled", tiling.parse_setting, TiledDenoiserModule),
             ("pixel_shuffle", pixel_shuffle_settings, PixelShuffleDenoiserModule),
             ("stabilise", vst.parse_setting, StabilisedDenoiserModule),
             ("burst", burst_settings, BurstDenoiserModule),
             ("video", video_settings, VideoDenoiserModule))


def load_model(model_path: str, device=None, self_ensemble=None, stabilise=None, tiled=None, pixel_shuffle=None, burst=None,
               nlm=None, video=None, bm3d=None):
    """bfcnn/__init__.py:81-97: a registry name, a model directory (pipeline.json + weights.npz written by
    `save_model`), or a `.keras` archive of a trained unet_laplacian hydra / the directory holding `model_hydra.keras`
    (the layout of the reference's bfcnn/pretrained/<name>/).  Returns a callable uint8 [B,H,W,C] -> uint8 [B,H,W,C]: a
    DenoiserModule, inside one wrapper for every option of `_WRAPPERS` that is set, in the table's order; each wrapper's module
    says what its option does and may set:

        self_ensemble  "d4", "flips" or transform numbers 0..7: the mean over flips and rotations of the image (self_ensemble.py)
        tiled          True or a dict (tile, overlap, margin, tile_batch): the frame runs as overlapping tiles (tiling.py)
        pixel_shuffle  a stride, "auto" (so is True) or a dict (stride, max_stride, threshold, refine, replace, seed): for noise
                       correlated over a few pixels, the sub-images of every s-th pixel run as one batch (pixel_shuffle.py)
        stabilise      True (fitted per frame) or a (gain, offset) pair: camera noise of variance gain x + offset; outside
                       the three above, so that the noise fit sees the whole frame (vst.py)
        burst          True or a dict (reference, levels, search, sigma, k): the callable takes uint8 [B,T,H,W,C] bursts,
                       aligns and merges their frames and denoises the merged frame (burst.py)
        video          True or a dict (n_max, levels, search, sigma, k): the callable takes the next uint8 [B,H,W,C] frame of B
                       parallel streams, filters it along the motion and denoises the filtered frame (video.py)

    `burst` and `video` both wrap outermost: both together are a ValueError.  The name "nlm" is no network: it returns a
    NlmDenoiserModule (non-local means, nlm.py; any channel count 1..4, no weights) under the same wrappers; `nlm` = None or a
    dict of its settings (sigma, patch, search, strength), a ValueError with any other `model_path`.  The name "bm3d" likewise
    returns a Bm3dDenoiserModule (block matching and collaborative filtering, bm3d.py); `bm3d` = None or a dict of its settings
    (sigma, search, step, threshold, wiener).  Every option is checked before anything is loaded."""
    options = {"self_ensemble": self_ensemble, "tiled": tiled, "pixel_shuffle": pixel_shuffle, "stabilise": stabilise, "burst": burst,
               "video": video}
    # the filters that are no network: name -> (the option that sets it, its value, its parse_setting, its module)
    filters = {_nlm.MODEL_NAME: ("nlm", nlm, nlm_settings, NlmDenoiserModule),
               _bm3d.MODEL_NAME: ("bm3d", bm3d, bm3d_settings, Bm3dDenoiserModule)}
    for name, (keyword, value, _, _) in filters.items():
        if value is not None and model_path != name:
            raise ValueError(f"{keyword} sets the filter of load_model({name!r}), got it with model_path {model_path!r}")
    filter_settings = filters[model_path][2](filters[model_path][1]) if model_path in filters else None
    settings = {keyword: parse(options[keyword]) for keyword, parse, _ in _WRAPPERS}
    if settings["burst"] is not None and settings["video"] is not None:
        raise ValueError("burst and video both wrap outermost: set one of them")
    module = _load_module(model_path, device) if filter_settings is None else filters[model_path][3](**filter_settings)
    for keyword, _, wrapper in _WRAPPERS:
        if settings[keyword] is not None:
            module = wrapper(module, **settings[keyword])
    return module


def _load_module(model_path: str, device=None) -> DenoiserModule:
    # --- argument checking
    if model_path is None or len(model_path) <= 0:
        raise ValueError("model_path cannot be empty")
    # --- load from pretrained
    if model_path in models:
        return DenoiserModule(load_hydra(models[model_path]["saved_model_path"], device=device))
    # --- load from any directory
    if not os.path.exists(model_path):
        raise ValueError("model_path [{0}] does not exist".format(model_path))
    # --- a trained hydra as keras wrote it (bfcnn/export_model.py:106-110), or the directory holding one
    archive = os.path.join(model_path, "model_hydra.keras") if os.path.isdir(model_path) else str(model_path)
    if archive.endswith(".keras") and os.path.isfile(archive):
        from .unet_laplacian import UnetLaplacianHydra
        return DenoiserModule(UnetLaplacianHydra.from_keras_archive(archive, device=device))
    return DenoiserModule(load_hydra(str(model_path), device=device))


def load_denoiser_model(model_path: str):
    """bfcnn/__init__.py:103-112."""
    if model_path is None or len(model_path) <= 0:
        raise ValueError("model_path cannot be empty")
    if model_path in models:
        return models[model_path][DENOISER_STR]()
    raise ValueError("model_path [{0}] does not exist".format(model_path))


# offer a decent pretrained model (bfcnn/__init__.py:118-122)
load_default_denoiser = list(models.values())[0][DENOISER_STR] if len(models) > 0 else None
