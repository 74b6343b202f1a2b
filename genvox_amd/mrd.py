"""Multi-resolution spectrogram discriminator on the MI355X (UnivNet's MRD, the discriminator the published BigVGAN recipe trains with
next to MPD; include/genvox_amd.h, "Multi-resolution spectrogram discriminator"; kernels in csrc/mrd.hip).

The module holds plain weights in PyTorch's ``Conv2d`` layout [out, in, 3, 9] / [out, in, 3, 3] under the published names
(``discriminators.<j>.convs.<i>.weight / .bias``, ``discriminators.<j>.conv_post.*``); the kernels read a packed blob that is rebuilt on
the device whenever the parameters change.  ``forward`` is ``DeviceDiscriminator``'s: one autograd node whose backward is one call of
gvx_mrd_backward.  There is no CPU or eager path.  ``load_state_dict`` reads a plain dict, this project's ``{"model_statedict": ...}``,
the published discriminator file ``{"mpd": ..., "mrd": ...}`` (its ``mrd`` part) and weight-normalised tensors; spectral-norm
checkpoints (``weight_orig`` / ``weight_u`` keys) are refused."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import torch
from torch import nn

from . import _lib
from ._device_module import DeviceDiscriminator, _Layer, fold_weight_norm
from .configs import MultiResolutionDiscriminatorConfig


def dims_from_config(dc: MultiResolutionDiscriminatorConfig) -> _lib.gvx_mrd_dims:
    n_fft, hop, win = (C.c_int32 * 8)(), (C.c_int32 * 8)(), (C.c_int32 * 8)()
    for i, (n, h, w) in enumerate(dc.resolutions):
        n_fft[i], hop[i], win[i] = n, h, w
    return _lib.gvx_mrd_dims(len(dc.resolutions), n_fft, hop, win, dc.channels, dc.WINDOWS.index(dc.window), float(dc.leaky_slope))


def map_widths(config: MultiResolutionDiscriminatorConfig, n: int) -> List[List[int]]:
    """Per resolution, the frames of each of the six maps of a row of ``n`` samples (host arithmetic): W_0 = 1 + (n + 2p - n_fft) // hop
    with p = (n_fft - hop) // 2, halved (rounding up) by each of the three strided layers; 0 for a row without a whole frame."""
    out = []
    for n_fft, hop, _win in config.resolutions:
        p = (n_fft - hop) // 2
        w = 1 + (n + 2 * p - n_fft) // hop if n > p and n + 2 * p >= n_fft else 0
        ws = []
        for _cin, _cout, _k, stride in config.layer_shapes():
            if stride > 1 and w > 0:
                w = (w - 1) // stride + 1
            ws.append(w)
        out.append(ws)
    return out


def map_published_keys(state_dict) -> Dict[str, torch.Tensor]:
    """The published discriminator file ``{"mpd": ..., "mrd": ...}`` -> its ``mrd`` part; this project's own checkpoint form
    (``{"model_statedict": ...}``) -> its inner dict; anything else passes through.  A spectral-norm key raises ValueError."""
    if "mrd" in state_dict and isinstance(state_dict["mrd"], dict):
        state_dict = state_dict["mrd"]
    elif "model_statedict" in state_dict and isinstance(state_dict["model_statedict"], dict):
        state_dict = state_dict["model_statedict"]
    for key in state_dict:
        if key.endswith((".weight_orig", ".weight_u")):
            raise ValueError(f"{key}: a spectral-norm checkpoint of the multi-resolution discriminator is not supported")
    return dict(state_dict)


class _Resolution(nn.Module):
    def __init__(self, config: MultiResolutionDiscriminatorConfig) -> None:
        super().__init__()
        shapes = config.layer_shapes()
        self.convs = nn.ModuleList([_Layer((cout, cin, kf, kt), cout, cin * kf * kt) for cin, cout, (kf, kt), _s in shapes[:-1]])
        cin, cout, (kf, kt), _s = shapes[-1]
        self.conv_post = _Layer((cout, cin, kf, kt), cout, cin * kf * kt)


class MultiResolutionDiscriminator(DeviceDiscriminator):
    """``forward`` gives per resolution its six maps [B, C, W, F] - frames in front of bins, the TRANSPOSE of the published
    [B, C, F, W] - as views of the kernels' channels-last storage [B][W][F][C].  The ragged axis is dim 2, so the losses' per-row means
    (``losses._row_mean_any``) take ``map_lengths`` as they are; means and feature matching do not depend on the order of the axes."""
    model_name = "multi_resolution_discriminator"
    _abi, _config_class = "gvx_mrd", MultiResolutionDiscriminatorConfig
    _short_hint = _range_hint = " (the widest reflection, (n_fft - hop) // 2 samples, needs one sample more)"

    def __init__(self, model_config: Optional[MultiResolutionDiscriminatorConfig] = None) -> None:
        super().__init__(model_config)
        self.discriminators = nn.ModuleList([_Resolution(self.model_config) for _ in self.model_config.resolutions])

    def dims(self) -> _lib.gvx_mrd_dims:
        return dims_from_config(self.model_config)

    def _grid(self):
        return len(self.model_config.resolutions), self.model_config.MAPS

    def map_widths(self, n: int) -> List[List[int]]:
        """Per resolution, the frames of each of the six maps of a row of ``n`` samples (host arithmetic)."""
        return map_widths(self.model_config, n)

    _row_lengths = map_widths

    @staticmethod
    def _entry(e):
        return e.byte_offset, e.channels, e.frames, e.bins, (e.stride_b, e.stride_c, e.stride_w, e.stride_f)

    def _convert_state_dict(self, state_dict) -> Dict[str, torch.Tensor]:
        return fold_weight_norm(map_published_keys(state_dict))
