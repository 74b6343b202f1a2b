"""MelGAN multi-scale discriminator on the MI355X (include/genvox_amd.h, "MelGAN discriminators"; kernels in csrc/melgan_disc.hip).

The module holds plain weights in PyTorch's ``Conv1d`` layout [out, in / groups, k] under the names the C ABI's packer reads
(``scales.<k>.layers.<i>.weight / .bias``); the kernels read a packed blob that is rebuilt on the device whenever the parameters change.
``forward`` is ``DeviceDiscriminator``'s: one autograd node whose backward is one call of gvx_melgan_disc_backward.  There is no CPU or
eager path.  No trained discriminator checkpoint ships with the project; ``load_state_dict`` reads the published implementation's key
names as well."""
from __future__ import annotations

import re
from typing import Dict, List, Optional

import torch
from torch import nn

from . import _lib
from ._device_module import DeviceDiscriminator, _Layer, fold_weight_norm
from .configs import MelGANDiscriminatorConfig


def dims_from_config(dc: MelGANDiscriminatorConfig) -> _lib.gvx_melgan_disc_dims:
    return _lib.gvx_melgan_disc_dims(dc.n_scales, dc.base_channels, dc.n_layers, dc.downsampling_factor, dc.max_channels, float(dc.leaky_slope))


# the published checkpoints: model.discriminator_<k>.model.layer_<i>.<j>.<what>, layer 0's convolution behind its ReflectionPad1d
_PUBLISHED = re.compile(r"^(?:model\.)?discriminator_(\d+)\.model\.layer_(\d+)\.(\d+)\.(.+)$")


def map_published_keys(state_dict) -> Dict[str, torch.Tensor]:
    """Keys of the published implementation -> this module's (``scales.<k>.layers.<i>.<what>``); other keys pass through.  Layer 0's
    convolution sits at index 1 of its ``Sequential`` (behind the reflection padding), every other layer's at index 0."""
    out = {}
    for key, val in state_dict.items():
        m = _PUBLISHED.match(key)
        if m:
            k, i, j, what = int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4)
            if j != (1 if i == 0 else 0):
                raise KeyError(f"{key}: layer {i}'s convolution is expected at index {1 if i == 0 else 0} of its Sequential")
            key = f"scales.{k}.layers.{i}.{what}"
        out[key] = val
    return out


class _Scale(nn.Module):
    def __init__(self, config: MelGANDiscriminatorConfig) -> None:
        super().__init__()
        self.layers = nn.ModuleList([_Layer((cout, cin // g, k), cout, (cin // g) * k) for cin, cout, k, _s, _p, g in config.layer_shapes()])


class MelGANDiscriminator(DeviceDiscriminator):
    """``forward`` gives per scale its n_layers + 3 maps [B, C, L], contiguous."""
    model_name = "melgan_discriminator"
    _abi, _config_class = "gvx_melgan_disc", MelGANDiscriminatorConfig
    _short_hint = " (the last scale reflects 7)"
    _range_hint = " (the last scale reflects 7 samples)"

    def __init__(self, model_config: Optional[MelGANDiscriminatorConfig] = None) -> None:
        super().__init__(model_config)
        self.scales = nn.ModuleList([_Scale(self.model_config) for _ in range(self.model_config.n_scales)])

    def dims(self) -> _lib.gvx_melgan_disc_dims:
        return dims_from_config(self.model_config)

    def _grid(self):
        return self.model_config.n_scales, self.model_config.n_layers + 3

    def feature_lengths(self, n: int) -> List[List[int]]:
        """Per scale, the length of each of the n_layers + 3 maps of a row of ``n`` samples (host arithmetic)."""
        mc = self.model_config
        out = []
        for k in range(mc.n_scales):
            length, lens = n >> k, []
            for _cin, _cout, _k, stride, _p, _g in mc.layer_shapes():
                if stride > 1:
                    length = (length - 1) // stride + 1 if length > 0 else 0
                lens.append(length)
            out.append(lens)
        return out

    _row_lengths = feature_lengths

    @staticmethod
    def _entry(e):
        return e.byte_offset, e.channels, e.positions

    def _convert_state_dict(self, state_dict) -> Dict[str, torch.Tensor]:
        return fold_weight_norm(map_published_keys(state_dict))
