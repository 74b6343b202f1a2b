"""HiFi-GAN multi-period discriminator on the MI355X (include/genvox_amd.h, "HiFi-GAN period discriminators"; kernels in
csrc/hifigan_disc.hip).

The module holds plain weights in PyTorch's ``Conv2d`` layout [out, in, k, 1] under the published names
(``discriminators.<j>.convs.<i>.weight / .bias``, ``discriminators.<j>.conv_post.*``); the kernels read a packed blob that is rebuilt on
the device whenever the parameters change.  ``forward`` is ``DeviceDiscriminator``'s: one autograd node whose backward is one call of
gvx_hifigan_mpd_backward.  There is no CPU or eager path.  No trained discriminator checkpoint ships with the project;
``load_state_dict`` reads the published checkpoints (weight-normalised, and the ``{"mpd": ...}`` file itself) as well."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import torch
from torch import nn

from . import _lib
from ._device_module import DeviceDiscriminator, _Layer, fold_weight_norm
from .configs import HiFiGANPeriodDiscriminatorConfig


def dims_from_config(dc: HiFiGANPeriodDiscriminatorConfig) -> _lib.gvx_hifigan_mpd_dims:
    periods, channels = (C.c_int32 * 8)(), (C.c_int32 * 8)()
    for i, p in enumerate(dc.periods):
        periods[i] = p
    for i, c in enumerate(dc.channels):
        channels[i] = c
    return _lib.gvx_hifigan_mpd_dims(len(dc.periods), periods, len(dc.channels), channels, dc.kernel_size, dc.stride, float(dc.leaky_slope))


def feature_heights(config: HiFiGANPeriodDiscriminatorConfig, n: int) -> List[List[int]]:
    """Per period, the height of each of the len(channels) + 1 maps of a row of ``n`` samples (host arithmetic)."""
    out = []
    for p in config.periods:
        h, hs = -(-n // p), []
        for _cin, _cout, _k, stride, _pad in config.layer_shapes():
            if stride > 1:
                h = (h - 1) // stride + 1 if h > 0 else 0
            hs.append(h)
        out.append(hs)
    return out


def map_published_keys(state_dict) -> Dict[str, torch.Tensor]:
    """The published checkpoint file ``{"mpd": ..., "msd": ...}`` -> its ``mpd`` part; this project's own checkpoint form
    (``{"model_statedict": ...}``) -> its inner dict; anything else passes through."""
    if "mpd" in state_dict and isinstance(state_dict["mpd"], dict):
        return dict(state_dict["mpd"])
    if "model_statedict" in state_dict and isinstance(state_dict["model_statedict"], dict):
        return dict(state_dict["model_statedict"])
    return dict(state_dict)


class _Period(nn.Module):
    def __init__(self, config: HiFiGANPeriodDiscriminatorConfig) -> None:
        super().__init__()
        shapes = config.layer_shapes()
        self.convs = nn.ModuleList([_Layer((cout, cin, k, 1), cout, cin * k) for cin, cout, k, _s, _p in shapes[:-1]])
        cin, cout, k, _s, _p = shapes[-1]
        self.conv_post = _Layer((cout, cin, k, 1), cout, cin * k)


class HiFiGANPeriodDiscriminator(DeviceDiscriminator):
    """``forward`` gives per period its len(channels) + 1 maps [B, C, H, p], views of the kernels' channels-last storage."""
    model_name = "hifigan_period_discriminator"
    _abi, _config_class = "gvx_hifigan_mpd", HiFiGANPeriodDiscriminatorConfig
    _short_hint = _range_hint = " (the largest period's reflection)"

    def __init__(self, model_config: Optional[HiFiGANPeriodDiscriminatorConfig] = None) -> None:
        super().__init__(model_config)
        self.discriminators = nn.ModuleList([_Period(self.model_config) for _ in self.model_config.periods])

    def dims(self) -> _lib.gvx_hifigan_mpd_dims:
        return dims_from_config(self.model_config)

    @property
    def maps_per_period(self) -> int:
        return len(self.model_config.channels) + 1

    def _grid(self):
        return len(self.model_config.periods), self.maps_per_period

    def feature_heights(self, n: int) -> List[List[int]]:
        """Per period, the height of each of the maps of a row of ``n`` samples (host arithmetic)."""
        return feature_heights(self.model_config, n)

    _row_lengths = feature_heights

    @staticmethod
    def _entry(e):
        return e.byte_offset, e.channels, e.height, e.period, (e.stride_b, e.stride_c, e.stride_h, e.stride_p)

    def _convert_state_dict(self, state_dict) -> Dict[str, torch.Tensor]:
        return fold_weight_norm(map_published_keys(state_dict))
