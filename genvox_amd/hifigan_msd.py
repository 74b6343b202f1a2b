"""HiFi-GAN multi-scale discriminator on the MI355X (include/genvox_amd.h, "HiFi-GAN scale discriminators"; kernels in
csrc/hifigan_msd.hip).

The module holds weights in PyTorch's ``Conv1d`` layout [out, in / groups, k] under the published names
(``discriminators.<s>.convs.<i>.weight / .bias``, ``discriminators.<s>.conv_post.*``).  A scale listed in the config's
``spectral_norm_scales`` (the published first scale) keeps spectral norm live, in torch: its layers hold ``weight_orig``, ``weight_u``
and ``weight_v`` as ``torch.nn.utils.spectral_norm`` does, a training-mode forward does one power iteration, and the effective weight
``weight_orig / sigma`` goes into the autograd node as a tensor, so that torch itself carries the kernels' weight gradient back to
``weight_orig``.  Weight norm (the other published scales) is a reparametrisation and is folded on load.  The kernels read a packed
blob of the effective weights that is built on the device whenever they change; ``forward`` is ``DeviceDiscriminator``'s, one autograd
node whose backward is one call of gvx_hifigan_msd_backward, and this module's part in it is ``weight_names()`` and
``effective_weights()``.  There is no CPU or eager path.  No trained discriminator checkpoint ships with the project;
``load_state_dict`` reads the published ``{"mpd": ..., "msd": ...}`` file itself."""
from __future__ import annotations

import ctypes as C
import re
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from ._device_module import DeviceDiscriminator, _Layer, fold_weight_norm
from .configs import HiFiGANScaleDiscriminatorConfig

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


class HiFiGANScaleDiscriminator(DeviceDiscriminator):
    """``forward`` gives per scale its len(channels) + 1 maps [B, C, L], views of the kernels' channels-last storage.  In training
    mode a spectral scale does its power iteration first, with or without gradients (``weight_u`` and ``weight_v`` change, so every
    such forward packs a new blob); in eval mode nothing of the module changes.  ``backward()`` reaches ``weight_orig`` through sigma."""
    model_name = "hifigan_scale_discriminator"
    _abi, _config_class = "gvx_hifigan_msd", HiFiGANScaleDiscriminatorConfig
    _samples = "sample"

    def __init__(self, model_config: Optional[HiFiGANScaleDiscriminatorConfig] = None) -> None:
        super().__init__(model_config)
        spectral = set(self.model_config.spectral_norm_scales)
        self.discriminators = nn.ModuleList([_Scale(self.model_config, s in spectral) for s in range(self.model_config.n_scales)])

    def dims(self) -> _lib.gvx_hifigan_msd_dims:
        return dims_from_config(self.model_config)

    @property
    def maps_per_scale(self) -> int:
        return len(self.model_config.channels) + 1

    def _grid(self):
        return self.model_config.n_scales, self.maps_per_scale

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

    def feature_lengths(self, n: int) -> List[List[int]]:
        """Per scale, the length of each of the maps of a row of ``n`` samples (host arithmetic)."""
        return feature_lengths(self.model_config, n)

    _row_lengths = feature_lengths

    @staticmethod
    def _entry(e):
        return e.byte_offset, e.channels, e.length, (e.stride_b, e.stride_c, e.stride_l)

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
