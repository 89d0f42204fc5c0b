"""The host side the operator-graph models share (`GenericResnetHydra`, `UnetHydra`, `UnetLaplacianHydra`): the flat parameter /
moving-statistics storage and its views, weights in and out, options, the status word, input placement and the padded uint8
entry point.  Each family adds its config parsing, its inventory, `_pack`, the forward walk (`_features` or `backbone`) and the
training graph it is trained by (`train_graph_class`)."""
from typing import Dict, Optional

import numpy as np
import torch

from . import _native as N
from ._native import call

BN_EPSILON = 1e-3          # DEFAULT_BN_EPSILON (bfcnn/constants.py:9)


def concat_input(f: torch.Tensor, x: torch.Tensor, H: int, W: int, cp: int, v_min: float, v_max: float) -> torch.Tensor:
    """Concatenate([features f, the input x normalised and zero-padded to [H,W]]) with zero channels up to cp, the width the
    head's matrix kernel takes"""
    B, Hs, Ws, cin = x.shape
    cat = torch.empty((B, H, W, cp), dtype=torch.float32, device=f.device)
    call("bf_op_concat_input", N.ptr(f), N.ptr(x), int(x.dtype == torch.uint8), N.ptr(cat), B, H, W, Hs, Ws, int(f.shape[-1]), cin, cp,
         v_min, v_max, N.stream_ptr(f))
    return cat


class OpGraphModel:
    """A hydra on the operator library: trainable tensors in one flat float32 vector (`params`), BatchNorm moving statistics in
    another (`state`), both in graph-construction order; `trainable_variables` lists (name, shape, kind, offset),
    `non_trainable_variables` (name, shape, offset)."""

    multi_output = False
    auto_exact_fallback = False
    FAMILY = ""                  # the family's name in error messages
    OPTIONS = ()                 # what set_option accepts, each 0 / 1
    TRAINING_CALL = "hydra(x, training=True) on its own is not built here; use train_loop's train_step_single_gpu"

    class _Desc:
        def __init__(self, cin, cout):
            self.in_channels, self.out_channels = cin, cout
            self.denormalize = 1

    # -- config keys the resnet and the unet builders read alike ----------------------------------------------------------------
    @staticmethod
    def _check_block_count(nb: int):
        if nb <= 0:
            raise ValueError("len(block_kernels) must be >= 0 ")                 # backbone_resnet.py:110-113
        if nb > 3:
            raise ValueError("len(block_kernels) must be <= 3")

    def _parse_dropout(self, bb: Dict):
        self.dropout_rate = float(bb.get("dropout_rate", -1))                  # RandomOnOff (:231-235): identity at inference
        if self.dropout_rate != -1 and not 0.0 <= self.dropout_rate < 1.0:
            raise ValueError("dropout_rate must be in [0, 1)")

    def _parse_bn_gates(self, bb: Dict, nb: int):
        self.use_bn = bool(bb.get("use_bn", True))
        self.add_gates = bool(bb.get("add_gates", False))
        if self.add_gates and nb < 2:
            raise ValueError("don't know what to do here")                       # backbone_blocks.py:131-141 (gate_no_filters)

    def _parse_io(self, bb: Dict, dn: Dict):
        self.in_channels = int(bb["input_shape"][-1])
        vr = bb.get("value_range", [0, 255])
        self.v_min, self.v_max = float(vr[0]), float(vr[1])
        self.head_filters = int(dn.get("filters", 32))
        self.head_activation = dn.get("activation", "linear")
        self.out_channels = int(dn.get("output_channels", 3))

    @staticmethod
    def _refuse_head_options(dn: Dict):
        if dn.get("use_bias", False) or dn.get("use_bn", False) or dn.get("use_ln", False):
            raise NotImplementedError("denoiser head: use_bias / use_bn / use_ln are outside the built graph")

    # -- storage ----------------------------------------------------------------------------------------------------------------
    def _init_storage(self, device, seed: Optional[int]):
        """desc, device, inventory (`_build_inventory` returns (trainable, state) lists) and the two flat vectors"""
        self.desc = self._Desc(self.in_channels, self.out_channels)
        self.device = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self._inventory, self._state_inventory = self._build_inventory()
        self.n_params = sum(int(np.prod(s)) for _, s, _ in self._inventory)
        self.n_state = sum(int(np.prod(s)) for _, s in self._state_inventory)
        self.params = torch.from_numpy(self._initial_values(seed)).to(self.device)
        st = np.concatenate([np.zeros(s, np.float32).ravel() if n.endswith("mean") else np.ones(s, np.float32).ravel()
                             for n, s in self._state_inventory]) if self._state_inventory else np.zeros(0, np.float32)
        self.state = torch.from_numpy(st).to(self.device)
        self.version = 0
        self._packed = None

    @property
    def trainable_variables(self):
        o, res = 0, []
        for name, shape, kind in self._inventory:
            res.append((name, shape, kind, o))
            o += int(np.prod(shape))
        return res

    @property
    def non_trainable_variables(self):
        o, res = 0, []
        for name, shape in self._state_inventory:
            res.append((name, shape, o))
            o += int(np.prod(shape))
        return res

    def count_params(self) -> int:
        return self.n_params

    def _initial_value(self, shape, kind: str, rng) -> np.ndarray:
        """keras' initialisers: glorot normal kernels, BatchNorm gamma 1, multipliers' w0 0"""
        from .model import glorot_normal
        if kind == "bn_gamma":
            return np.ones(shape)
        if kind in ("channelwise", "multiplier"):
            return np.zeros(shape)
        return glorot_normal((1, 1) + tuple(shape), rng).reshape(shape) if kind == "dense" else glorot_normal(shape, rng)

    def _initial_values(self, seed) -> np.ndarray:
        rng = np.random.default_rng(seed)
        return np.concatenate([np.asarray(self._initial_value(s, kind, rng), np.float32).ravel() for _, s, kind in self._inventory])

    def get_weights(self):
        return self.params.detach().cpu().numpy(), self.state.detach().cpu().numpy()

    def set_weights(self, params: np.ndarray, state: Optional[np.ndarray] = None):
        params = np.ascontiguousarray(params, np.float32).ravel()
        if params.size != self.n_params:
            raise ValueError(f"expected {self.n_params} parameters, got {params.size}")
        self.params.copy_(torch.from_numpy(params))
        if state is not None:
            state = np.ascontiguousarray(state, np.float32).ravel()
            if state.size != self.n_state:
                raise ValueError(f"expected {self.n_state} state values, got {state.size}")
            self.state.copy_(torch.from_numpy(state))
        self.mark_dirty()

    def mark_dirty(self):
        """parameters or moving statistics changed in place (optimizer / training step): drop the packed operands"""
        self._packed = None
        self.version += 1

    def set_option(self, key: str, value: int):
        if key not in self.OPTIONS or int(value) not in (0, 1):
            raise ValueError(f"unknown option {key}={value}")
        setattr(self, key, int(value))
        self.version += 1

    # -- status word ------------------------------------------------------------------------------------------------------------
    def _status(self) -> torch.Tensor:
        """int32 status word on the device, cleared (bf_op_fill32) at the start of a forward, OR-ed by the head kernels."""
        if getattr(self, "_status_word", None) is None:
            self._status_word = torch.empty(1, dtype=torch.int32, device=self.device)
        call("bf_op_fill32", N.ptr(self._status_word), 0, 1, N.stream_ptr(self._status_word))
        return self._status_word

    def status_tensor(self) -> Optional[torch.Tensor]:
        return getattr(self, "_status_word", None)

    def check_status(self, raise_on_overflow: bool = True) -> bool:
        """synchronises and reads the status word of the last forward (see HydraModel.check_status); True without one."""
        st = self.status_tensor()
        if st is None or not (int(st.item()) & N.BF_STATUS_F16_RANGE):
            return True
        if raise_on_overflow:
            raise FloatingPointError("an activation left the f16 range inside the split-f16 operators; "
                                     "call set_option('arith', 0) to run the exact-fp32 operators")
        return False

    # -- packing ----------------------------------------------------------------------------------------------------------------
    def _host_weights(self):
        """the `_pack` preamble: W / S = float64 host copies of the parameters / moving statistics by name, dev(a) = a float32
        device tensor, bn_affine(base) = the inference BatchNorm (center=False) as a per-channel (scale, shift)"""
        w, st = self.get_weights()
        W = {n: w[o:o + int(np.prod(s))].reshape(s).astype(np.float64) for n, s, _, o in self.trainable_variables}
        S = {n: st[o:o + int(np.prod(s))].reshape(s).astype(np.float64) for n, s, o in self.non_trainable_variables}
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.device)

        def bn_affine(base):
            sc = W[base + "/gamma"] / np.sqrt(S[base + "/moving_variance"] + BN_EPSILON)
            return sc, -sc * S[base + "/moving_mean"]
        return W, S, dev, bn_affine

    # -- forward ----------------------------------------------------------------------------------------------------------------
    def _require_gpu(self):
        if self.device.type != "cuda":
            raise RuntimeError(f"{self.FAMILY} inference needs the GPU: there is no CPU execution path")

    def _as_device(self, x):
        was_numpy = isinstance(x, np.ndarray)
        if was_numpy:
            x = torch.from_numpy(np.ascontiguousarray(x))
        if x.dim() != 4 or x.shape[-1] != self.in_channels:
            raise ValueError(f"expected [B,H,W,{self.in_channels}], got {tuple(x.shape)}")
        if x.dtype != torch.uint8:
            x = x.to(torch.float32)
        return x.to(self.device).contiguous(), was_numpy

    def _outputs(self, x: torch.Tensor, H: int, W: int, crop=None, as_uint8: bool = False):
        """the head on the features of x (padded to [H,W]), cropped to crop = (Ho, Wo) (default: [H,W])"""
        from .unet_laplacian import head_fused
        P = self._pack()
        Ho, Wo = crop or (H, W)
        return head_fused(self._features(x, H, W), None, P["head0"], self.head_activation, P["head1"], Ho, Wo, as_uint8, True,
                          self.v_min, self.v_max, arith=self.arith)

    def __call__(self, x, training: bool = False):
        """float32 (or uint8) [B,H,W,cin] on the value_range scale -> the denoised image (a list of them, full resolution first,
        for a multi-output model); host arrays in, host arrays out."""
        if training:
            raise NotImplementedError(self.TRAINING_CALL)
        self._require_gpu()
        x, was_numpy = self._as_device(x)
        B, H, W, _ = x.shape
        out = self._outputs(x, H, W)
        if not was_numpy:
            return out
        torch.cuda.synchronize(self.device)
        if not self.check_status(raise_on_overflow=not (self.auto_exact_fallback and self.arith != 0)):
            self.set_option("arith", 0)
            return self(x.cpu().numpy())
        return [o.cpu().numpy() for o in out] if self.multi_output else out.cpu().numpy()

    def predict(self, x):
        return self(x)

    def infer_u8(self, image: torch.Tensor, cast_to_uint8: bool = True) -> torch.Tensor:
        """DenoiserModule.__call__ for this model (module_denoiser.py:46-75): pad to a power of two, hydra, (first) output, crop,
        round half to even, cast."""
        from .utilities import next_power_of_2
        self._require_gpu()
        B, Hs, Ws, _ = image.shape
        return self._outputs(image, next_power_of_2(Hs), next_power_of_2(Ws), (Hs, Ws), bool(cast_to_uint8))
