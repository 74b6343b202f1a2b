"""HiFi-GAN multi-scale discriminator on the MI355X (include/genvox_amd.h, "HiFi-GAN scale discriminators"; kernels in
csrc/hifigan_msd.hip).

The module holds weights in PyTorch's ``Conv1d`` layout [out, in / groups, k] under the published names
(``discriminators.<s>.convs.<i>.weight / .bias``, ``discriminators.<s>.conv_post.*``).  A scale listed in the config's
``spectral_norm_scales`` (the published first scale) keeps spectral norm live, in torch: its layers hold ``weight_orig``, ``weight_u``
and ``weight_v`` as ``torch.nn.utils.spectral_norm`` does, a training-mode forward does one power iteration, and the effective weight
``weight_orig / sigma`` goes into the autograd node as a tensor, so that torch itself carries the kernels' weight gradient back to
``weight_orig``.  Weight norm (the other published scales) is a reparametrisation and is folded on load.  The kernels read a packed
blob of the effective weights that is built on the device whenever they change; ``forward`` is one autograd node whose backward is one
call of gvx_hifigan_msd_backward.  There is no CPU or eager path.  No trained discriminator checkpoint ships with the project;
``load_state_dict`` reads the published ``{"mpd": ..., "msd": ...}`` file itself."""
from __future__ import annotations

import ctypes as C
import re
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from .configs import BaseConfig, HiFiGANScaleDiscriminatorConfig
from .melgan import _Layer, fold_weight_norm

SPECTRAL_EPS = 1e-12


def dims_from_config(dc: HiFiGANScaleDiscriminatorConfig) -> _lib.gvx_hifigan_msd_dims:
    arrays = []
    for values in (dc.channels, dc.kernel_sizes, dc.strides, dc.groups):
        a = (C.c_int32 * 8)()
        for i, v in enumerate(values):
            a[i] = v
        arrays.append(a)
    return _lib.gvx_hifigan_msd_dims(dc.n_scales, len(dc.channels), *arrays, float(dc.leaky_slope))


def feature_lengths(config: HiFiGANScaleDiscriminatorConfig, n: int) -> List[List[int]]:
    """Per scale, the length of each of the len(channels) + 1 maps of a row of ``n`` samples (host arithmetic)."""
    out = []
    for _s in range(config.n_scales):
        length, ls = n, []
        for _cin, _cout, _k, stride, _pad, _g in config.layer_shapes():
            length = (length - 1) // stride + 1 if length > 0 else 0
            ls.append(length)
        out.append(ls)
        n = n // 2 + 1 if n > 0 else 0
    return out


def map_published_keys(state_dict) -> Dict[str, torch.Tensor]:
    """The published checkpoint file ``{"mpd": ..., "msd": ...}`` -> its ``msd`` part; this project's own checkpoint form
    (``{"model_statedict": ...}``) -> its inner dict; anything else passes through."""
    if "msd" in state_dict and isinstance(state_dict["msd"], dict):
        return dict(state_dict["msd"])
    if "model_statedict" in state_dict and isinstance(state_dict["model_statedict"], dict):
        return dict(state_dict["model_statedict"])
    return dict(state_dict)


def spectral_sigma(weight_orig: torch.Tensor, u: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """sigma = u . (W v) with W = weight_orig as [c_out, -1]: the estimate of the largest singular value that spectral norm divides by."""
    return torch.dot(u, torch.mv(weight_orig.reshape(weight_orig.shape[0], -1), v))


class _SpectralLayer(nn.Module):
    """One layer under spectral norm, with ``torch.nn.utils.spectral_norm``'s names and shapes: ``weight_orig`` [c_out, c_in / groups,
    k], the buffers ``weight_u`` [c_out] and ``weight_v`` [c_in / groups * k], and ``bias``."""

    def __init__(self, shape, n_out: int, fan_in: int) -> None:
        super().__init__()
        self.weight_orig = nn.Parameter(torch.randn(*shape) * fan_in ** -0.5)
        self.bias = nn.Parameter(torch.zeros(n_out))
        self.register_buffer("weight_u", F.normalize(torch.randn(shape[0]), dim=0, eps=SPECTRAL_EPS))
        self.register_buffer("weight_v", F.normalize(torch.randn(shape[1] * shape[2]), dim=0, eps=SPECTRAL_EPS))

    def effective_weight(self) -> torch.Tensor:
        """``weight_orig / sigma``.  In training mode one power iteration first: v = normalize(W^T u), u = normalize(W v), without
        gradient, in place in the buffers, and clones of them from there on; in eval mode the buffers as they are."""
        u, v = self.weight_u, self.weight_v
        if self.training:
            with torch.no_grad():
                w = self.weight_orig.reshape(self.weight_orig.shape[0], -1)
                v = F.normalize(torch.mv(w.t(), u), dim=0, eps=SPECTRAL_EPS, out=v)
                u = F.normalize(torch.mv(w, v), dim=0, eps=SPECTRAL_EPS, out=u)
            u, v = u.clone(memory_format=torch.contiguous_format), v.clone(memory_format=torch.contiguous_format)
        return self.weight_orig / spectral_sigma(self.weight_orig, u, v)


class _Scale(nn.Module):
    def __init__(self, config: HiFiGANScaleDiscriminatorConfig, spectral: bool) -> None:
        super().__init__()
        make = _SpectralLayer if spectral else _Layer
        shapes = config.layer_shapes()
        self.convs = nn.ModuleList([make((cout, cin // g, k), cout, cin // g * k) for cin, cout, k, _s, _p, g in shapes[:-1]])
        cin, cout, k, _s, _p, g = shapes[-1]
        self.conv_post = make((cout, cin // g, k), cout, cin // g * k)

    def layers(self):
        return [(f"convs.{i}", layer) for i, layer in enumerate(self.convs)] + [("conv_post", self.conv_post)]


class _ScaleFunction(torch.autograd.Function):
    """gvx_hifigan_msd_forward / gvx_hifigan_msd_backward as one autograd node.  The inputs after ``lens_dev`` are the EFFECTIVE weights
    and the biases in the packer's order (a parameter itself, or ``weight_orig / sigma`` of a spectral layer); they go through
    ``save_for_backward``, so an in-place change between forward and backward raises torch's own version error.  The features buffer
    is the tape, and the node keeps it - and the blob its forward ran on; the returned maps are views of the tape and go through
    ``save_for_backward`` as well."""

    @staticmethod
    def forward(ctx, model, wav, lens_dev, *weights):
        blob = model._ensure_packed(weights)
        features, maps = model._run_forward(wav, lens_dev)
        ctx.model, ctx.lens_dev, ctx.features, ctx.blob = model, lens_dev, features, blob
        ctx.n_weights = len(weights)
        ctx.save_for_backward(wav, *weights, *maps)
        return tuple(maps)

    @staticmethod
    def backward(ctx, *d_maps):
        wav, *rest = ctx.saved_tensors   # raises if a weight - or a returned map, which is the tape - was changed in place
        weights = rest[:ctx.n_weights]
        model = ctx.model
        if ctx.blob.device != model._device():
            raise RuntimeError("the discriminator was moved between this forward and its backward")
        lib, dims, dev = _lib.load(), model.dims(), wav.device
        B, n_max = wav.shape
        want_params = any(ctx.needs_input_grad[3:])
        d_wav = torch.empty_like(wav) if ctx.needs_input_grad[1] else None
        if not want_params and d_wav is None:
            return (None, None, None) + (None,) * len(weights)
        d_features = torch.empty_like(ctx.features)
        for view, g in zip(model._views(d_features, B, n_max), d_maps):
            if g is None:
                view.zero_()
            else:
                view.copy_(g)
        grads, table = [], None
        if want_params:
            names = model.weight_names()
            grads = [torch.empty(w.shape, dtype=torch.float32, device=dev) for w in weights]
            table = (_lib.gvx_weight_desc * len(grads))()
            for i, (k, g) in enumerate(zip(names, grads)):
                table[i] = _lib.gvx_weight_desc(k.encode(), g.data_ptr(), g.numel())
        need = lib.gvx_hifigan_msd_workspace_bytes(C.byref(dims), B, n_max, 1)
        if model._train_workspace is None or model._train_workspace.numel() < need or model._train_workspace.device != dev:
            model._train_workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        ws = model._train_workspace
        _lib.check(lib.gvx_hifigan_msd_bind(model._handle, ctx.blob.data_ptr()))   # the weights this node's forward ran on
        _lib.check(lib.gvx_hifigan_msd_backward(model._handle, wav.data_ptr(), ctx.lens_dev.data_ptr() if ctx.lens_dev is not None else None, B, n_max,
                                                ctx.features.data_ptr(), d_features.data_ptr(), table, len(grads),
                                                d_wav.data_ptr() if d_wav is not None else None, ws.data_ptr(), ws.numel(), model._stream()))
        if model._blob is not None:
            _lib.check(lib.gvx_hifigan_msd_bind(model._handle, model._blob.data_ptr()))
        return (None, d_wav, None, *(grads if want_params else [None] * len(weights)))


class HiFiGANScaleDiscriminator(nn.Module):
    model_name = "hifigan_scale_discriminator"

    def __init__(self, model_config: Optional[HiFiGANScaleDiscriminatorConfig] = None) -> None:
        super().__init__()
        self.model_config = model_config if model_config is not None else HiFiGANScaleDiscriminatorConfig()
        spectral = set(self.model_config.spectral_norm_scales)
        self.discriminators = nn.ModuleList([_Scale(self.model_config, s in spectral) for s in range(self.model_config.n_scales)])
        self._handle: Optional[int] = None
        self._blob: Optional[torch.Tensor] = None
        self._packed_key = None
        self._workspace: Optional[torch.Tensor] = None
        self._train_workspace: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------ C-ABI plumbing
    def __del__(self):
        try:
            if self._handle is not None:
                _lib.load().gvx_hifigan_msd_destroy(self._handle)
        except Exception:
            pass

    def dims(self) -> _lib.gvx_hifigan_msd_dims:
        return dims_from_config(self.model_config)

    @property
    def min_samples(self) -> int:
        return self.model_config.min_samples

    @property
    def maps_per_scale(self) -> int:
        return len(self.model_config.channels) + 1

    def _device(self) -> torch.device:
        return self.discriminators[0].conv_post.bias.device

    def _require_gpu(self) -> torch.device:
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError("genvox_amd.HiFiGANScaleDiscriminator runs on an MI355X only: move the model with .to('cuda:0'). There is no CPU fallback.")
        return dev

    def _stream(self) -> int:
        return torch.cuda.current_stream(self._device()).cuda_stream

    def weight_names(self) -> List[str]:
        """The packer's names, scale by scale and layer by layer: ``<layer>.weight``, ``<layer>.bias``."""
        return [f"discriminators.{s}.{name}.{part}" for s, scale in enumerate(self.discriminators) for name, _ in scale.layers()
                for part in ("weight", "bias")]

    def effective_weights(self) -> List[torch.Tensor]:
        """The tensors the kernels see, in ``weight_names()`` order.  A spectral layer's weight is ``weight_orig / sigma`` - in training
        mode after one power iteration, which updates ``weight_u`` and ``weight_v`` in place."""
        out = []
        for scale in self.discriminators:
            for _name, layer in scale.layers():
                out.append(layer.effective_weight() if isinstance(layer, _SpectralLayer) else layer.weight)
                out.append(layer.bias)
        return out

    def _weights_key(self):
        tensors = list(self.parameters()) + list(self.buffers())
        return (str(self._device()),) + tuple((t.data_ptr(), t._version) for t in tensors)

    def _ensure_packed(self, weights) -> torch.Tensor:
        """The blob of ``weights`` (``effective_weights()``), bound to the handle.  Packed again - into a NEW blob, an earlier forward's
        node keeps its own - whenever a parameter or a spectral buffer has changed."""
        dev = self._require_gpu()
        lib, dims = _lib.load(), self.dims()
        if self._handle is None:
            h = C.c_void_p()
            _lib.check(lib.gvx_hifigan_msd_create(C.byref(dims), C.byref(h)))
            self._handle = h.value
        key = self._weights_key()
        if self._packed_key != key or self._blob is None:
            srcs = [w.detach().to(device=dev, dtype=torch.float32).contiguous() for w in weights]
            table = (_lib.gvx_weight_desc * len(srcs))()
            for i, (k, v) in enumerate(zip(self.weight_names(), srcs)):
                table[i] = _lib.gvx_weight_desc(k.encode(), v.data_ptr(), v.numel())
            blob = torch.empty(lib.gvx_hifigan_msd_blob_floats(C.byref(dims)), dtype=torch.float32, device=dev)
            _lib.check(lib.gvx_hifigan_msd_pack_weights_device(C.byref(dims), table, len(srcs), blob.data_ptr(), self._stream()))
            self._blob, self._packed_key = blob, key
        _lib.check(lib.gvx_hifigan_msd_bind(self._handle, self._blob.data_ptr()))
        return self._blob

    # ------------------------------------------------------------------ host arithmetic
    def feature_lengths(self, n: int) -> List[List[int]]:
        """Per scale, the length of each of the maps of a row of ``n`` samples (host arithmetic)."""
        return feature_lengths(self.model_config, n)

    def map_lengths(self, sample_lengths) -> List[List[List[int]]]:
        """[scale][map] -> the length of that map in every row, for the losses' per-row means (host arithmetic)."""
        host = [int(v) for v in (sample_lengths.tolist() if isinstance(sample_lengths, torch.Tensor) else sample_lengths)]
        per_row = [self.feature_lengths(n) for n in host]
        return [[[row[s][i] for row in per_row] for i in range(self.maps_per_scale)] for s in range(self.model_config.n_scales)]

    def layout(self, B: int, n_max: int):
        """gvx_hifigan_msd_layout: per scale a list of (byte offset, channels, length, (stride_b, stride_c, stride_l))."""
        dims = self.dims()
        per, count = self.maps_per_scale, self.model_config.n_scales * self.maps_per_scale
        entries = (_lib.gvx_hifigan_msd_entry * count)()
        got = _lib.load().gvx_hifigan_msd_layout(C.byref(dims), B, n_max, entries, count)
        if got != count:
            raise ValueError(f"no layout for B = {B}, n_max = {n_max}: a row needs {self.min_samples} sample or more")
        flat = [(e.byte_offset, e.channels, e.length, (e.stride_b, e.stride_c, e.stride_l)) for e in entries]
        return [flat[s * per:(s + 1) * per] for s in range(self.model_config.n_scales)]

    def _views(self, features: torch.Tensor, B: int, n_max: int) -> List[torch.Tensor]:
        """The maps of a features buffer (uint8) as float32 [B, C, L] views of its channels-last storage, scale after scale."""
        out = []
        for scale in self.layout(B, n_max):
            for off, c, length, strides in scale:
                flat = features[off:off + 4 * B * c * length].view(torch.float32)
                out.append(flat.as_strided((B, c, length), strides))
        return out

    # ------------------------------------------------------------------ the call
    def _check_call(self, wav: torch.Tensor, sample_lengths):
        dev = self._require_gpu()
        if not isinstance(wav, torch.Tensor) or wav.dim() != 2:
            raise ValueError(f"wav must be [B, n_max], got {tuple(wav.shape) if isinstance(wav, torch.Tensor) else type(wav)}")
        if wav.device != dev or wav.dtype != torch.float32:
            raise ValueError(f"wav must be float32 on {dev}, got {wav.dtype} on {wav.device}")
        B, n_max = wav.shape
        if B < 1 or n_max < self.min_samples:
            raise ValueError(f"a batch of {B} rows and {n_max} samples: every row needs at least {self.min_samples} sample")
        lens_dev = None
        if sample_lengths is not None:
            host = [int(v) for v in (sample_lengths.tolist() if isinstance(sample_lengths, torch.Tensor) else sample_lengths)]
            if len(host) != B:
                raise ValueError(f"{len(host)} lengths for {B} rows")
            for b, n in enumerate(host):
                if not self.min_samples <= n <= n_max:
                    raise ValueError(f"row {b}: {n} samples are outside [{self.min_samples}, {n_max}]")
            lens_dev = (sample_lengths if isinstance(sample_lengths, torch.Tensor) else torch.tensor(host)).to(dev, torch.int32).contiguous()
        return lens_dev

    def _run_forward(self, wav: torch.Tensor, lens_dev):
        """One gvx_hifigan_msd_forward on the blob that is bound (``_ensure_packed`` comes first)."""
        lib, dims, dev = _lib.load(), self.dims(), wav.device
        B, n_max = wav.shape
        features = torch.empty(lib.gvx_hifigan_msd_features_bytes(C.byref(dims), B, n_max), dtype=torch.uint8, device=dev)
        need = lib.gvx_hifigan_msd_workspace_bytes(C.byref(dims), B, n_max, 0)
        if self._workspace is None or self._workspace.numel() < need or self._workspace.device != dev:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        workspace = self._workspace
        _lib.check(lib.gvx_hifigan_msd_forward(self._handle, wav.data_ptr(), lens_dev.data_ptr() if lens_dev is not None else None, B, n_max,
                                               features.data_ptr(), features.numel(), workspace.data_ptr(), workspace.numel(), self._stream()))
        return features, self._views(features, B, n_max)

    def forward(self, wav: torch.Tensor, sample_lengths=None) -> List[List[torch.Tensor]]:
        """wav float32 [B, n_max] on the device -> per scale the list of its len(channels) + 1 maps [B, C, L]: the post-activation
        features, then the score.  The shape is the contract; the strides are those of the kernels' channels-last storage.
        ``sample_lengths`` ([B], host or device): every row at its own length - bit for bit that row run alone - and exact zeros behind
        its own lengths (``feature_lengths``); the padded samples may hold anything.  In training mode a spectral scale does its power
        iteration first (``weight_u`` and ``weight_v`` change); in eval mode nothing of the module changes.  With gradients enabled and
        something that requires one, ``backward()`` through any of the maps fills ``.grad`` of the parameters that require it
        (``weight_orig`` through sigma), and of ``wav`` if it does, in one call of the device's backward - ``d_wav`` alone when no
        parameter requires a gradient; under ``torch.no_grad()`` it is the plain forward with the same bits.  The returned maps are
        views of the buffer the backward reads as its tape: changing one in place before ``backward()`` raises torch's version error
        (clone it first)."""
        lens_dev = self._check_call(wav, sample_lengths)
        wav = wav.contiguous()
        per = self.maps_per_scale
        if not torch.is_grad_enabled() or not (wav.requires_grad or any(p.requires_grad for p in self.parameters())):
            with torch.no_grad():
                self._ensure_packed(self.effective_weights())
                _, maps = self._run_forward(wav, lens_dev)
        else:
            for k, p in self.named_parameters():
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise ValueError(f"{k}: training needs contiguous float32 parameters")
            maps = list(_ScaleFunction.apply(self, wav, lens_dev, *self.effective_weights()))
        return [maps[s * per:(s + 1) * per] for s in range(self.model_config.n_scales)]

    # ------------------------------------------------------------------ checkpoints and configs
    _LAYER_KEY = re.compile(r"^(discriminators\.(\d+)\.(?:convs\.\d+|conv_post))\.(weight_orig|weight_u|weight_v|weight)$")

    def _convert_state_dict(self, state_dict) -> Dict[str, torch.Tensor]:
        """Any of the three checkpoint forms -> this module's own keys.  Weight-norm pairs (``weight_g`` with a ``weight_v`` of the
        weight's own shape) are folded; spectral triples (``weight_orig`` with vector ``weight_u`` and ``weight_v``) go to a spectral
        scale as they are and are folded to ``weight_orig / sigma`` for a scale without spectral norm; a plain ``weight`` given to a
        spectral scale becomes its ``weight_orig`` and the scale keeps its ``u`` and ``v``.  The two meanings of ``weight_v`` are told
        apart by the key beside it."""
        sd = map_published_keys(state_dict)
        spectral_prefixes = {k[:-len(".weight_orig")] for k in sd if k.endswith(".weight_orig")}
        triples: Dict[str, Dict[str, torch.Tensor]] = {}
        rest = {}
        for k, v in sd.items():
            m = self._LAYER_KEY.match(k)
            if m and m.group(1) in spectral_prefixes and m.group(3) != "weight":
                triples.setdefault(m.group(1), {})[m.group(3)] = v
            else:
                rest[k] = v
        out = fold_weight_norm(rest)
        spectral = set(self.model_config.spectral_norm_scales)
        own = dict(super().state_dict())
        for prefix, parts in triples.items():
            if set(parts) != {"weight_orig", "weight_u", "weight_v"}:
                raise KeyError(f"{prefix}: a spectrally normalised layer needs weight_orig, weight_u and weight_v")
            s = int(self._LAYER_KEY.match(prefix + ".weight").group(2))
            if s in spectral:
                for name, v in parts.items():
                    out[f"{prefix}.{name}"] = v
            else:
                w = parts["weight_orig"]
                out[f"{prefix}.weight"] = w / spectral_sigma(w, parts["weight_u"].to(w.dtype), parts["weight_v"].to(w.dtype))
        for k in list(out):
            m = self._LAYER_KEY.match(k)
            if m and m.group(3) == "weight" and int(m.group(2)) in spectral:
                prefix = m.group(1)
                out[f"{prefix}.weight_orig"] = out.pop(k)
                for name in ("weight_u", "weight_v"):
                    if f"{prefix}.{name}" in own:
                        out.setdefault(f"{prefix}.{name}", own[f"{prefix}.{name}"])
        return out

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        out = super().load_state_dict(self._convert_state_dict(state_dict), strict=strict, assign=assign)
        self._packed_key = None
        return out

    def get_checkpoint_statedicts(self, optimizer: Optional[Dict] = None) -> Dict:
        return {"model_statedict": self.state_dict()}

    def load_checkpoint_statedicts(self, statedicts: Dict, save_optimizer_dict: bool = False, optimizer: Optional[Dict] = None) -> None:
        self.load_state_dict(statedicts["model_statedict"])

    @staticmethod
    def load_from_config(config_path: str) -> "HiFiGANScaleDiscriminator":
        configs = BaseConfig.load_configs_from_file(path=config_path, config_map={"discriminator_config": HiFiGANScaleDiscriminatorConfig})
        return HiFiGANScaleDiscriminator(configs.get("discriminator_config"))
