"""MelGAN generator: mel -> waveform on the MI355X (include/genvox_amd.h, "Neural vocoder"; kernels in csrc/melgan.hip).

The module holds the parameters in PyTorch's own layouts - ``Conv1d`` as [out, in, k], ``ConvTranspose1d`` as [in, out, k] - under the
names the C ABI's packer reads (``pre``, ``ups.<i>``, ``res.<i>.<j>.conv / .shortcut / .mix``, ``post``); the kernels read a packed
blob that is rebuilt on the device whenever the parameters change.  The calls - ``vocode``, ``vocode_with_grad`` (kernels in
csrc/melgan_train.hip), ``inference`` - are ``DeviceGenerator``'s.  There is no CPU or eager path."""
from __future__ import annotations

import ctypes as C

from torch import nn

from . import _lib
from ._device_module import DeviceGenerator, _Layer, _VocodeWithGrad, fold_weight_norm  # noqa: F401  (imported from here as well)
from .configs import AudioConfig, MelGANConfig

MIN_FRAMES = 4   # GVX_MELGAN_MIN_FRAMES: the first convolution reflects 3 frames


def dims_from_config(mc: MelGANConfig, ac: AudioConfig) -> _lib.gvx_melgan_dims:
    ratios = (C.c_int32 * 8)(*mc.upsample_ratios)
    return _lib.gvx_melgan_dims(ac.n_mels, mc.base_channels, len(mc.upsample_ratios), ratios, mc.n_residual_layers, mc.dilation_base,
                                float(mc.leaky_slope))


class _ResidualLayer(nn.Module):
    def __init__(self, channels: int) -> None:
        super().__init__()
        self.conv = _Layer((channels, channels, 3), channels, 3 * channels)
        self.shortcut = _Layer((channels, channels, 1), channels, channels)
        self.mix = _Layer((channels, channels, 1), channels, channels)


class MelGANGenerator(DeviceGenerator):
    """``vocode`` takes mels on the model's own dB scale, as ``mel_outputs_postnet``; a row needs 4 frames.  With the default
    config the workspace is 98,624 bytes per frame and row, and ``vocode_with_grad``'s tape 747,840."""
    model_name = "melgan"
    _abi, _config_class = "gvx_melgan", MelGANConfig
    _min_frames = MIN_FRAMES
    _range_hint = " (the first convolution reflects 3 frames)"
    _short_tail = f"{MIN_FRAMES} frames (the first convolution reflects 3)"

    def __init__(self, model_config: MelGANConfig, audio_config: AudioConfig) -> None:
        super().__init__(model_config, audio_config)
        c = model_config.base_channels
        self.pre = _Layer((c, audio_config.n_mels, 7), c, 7 * audio_config.n_mels)
        self.ups, self.res = nn.ModuleList(), nn.ModuleList()
        for r in model_config.upsample_ratios:
            self.ups.append(_Layer((c, c // 2, 2 * r), c // 2, 2 * c))   # ConvTranspose1d: [in, out, k]; two taps of c inputs reach an output
            c //= 2
            self.res.append(nn.ModuleList([_ResidualLayer(c) for _ in range(model_config.n_residual_layers)]))
        self.post = _Layer((1, c, 7), 1, 7 * c)

    def dims(self) -> _lib.gvx_melgan_dims:
        return dims_from_config(self.model_config, self.audio_config)

    def _stage_shapes(self):
        return self.model_config.base_channels, self.model_config.upsample_ratios
