"""BigVGAN generator: mel -> waveform on the MI355X, inference (include/genvox_amd.h, "BigVGAN generator"; kernels in csrc/bigvgan.hip
on HiFi-GAN's convolution kernels).

The module holds the parameters in PyTorch's own layouts under the published implementation's names (``conv_pre``, ``ups.<i>.0``,
``resblocks.<n>.convs1.<m>`` / ``.convs2.<m>`` or ``.convs.<m>``, ``resblocks.<n>.activations.<p>.act.alpha`` / ``.beta``,
``activation_post.act.alpha`` / ``.beta``, ``conv_post``), so a published generator checkpoint loads as it is: weight normalisation is
folded on load, and the anti-aliasing filter buffers such a checkpoint carries are compared with the filter computed here and dropped.
The kernels read a packed blob that is rebuilt on the device whenever the parameters change; every activation's per-channel constants
``a`` and ``g`` are derived from ``alpha`` / ``beta`` in float64 at that point.  The calls are ``DeviceGenerator``'s.  There is no
backward yet: ``vocode_with_grad`` is ``vocode`` when nothing asks for a gradient and raises ``NotImplementedError`` otherwise.  There
is no CPU or eager path.

As with the other vocoders, the model vocodes whatever mel scale its checkpoint was trained on; no conversion is part of this module."""
from __future__ import annotations

import math
import re
from typing import Dict, Optional

import torch
from torch import nn

from . import _lib
from ._device_module import DeviceGenerator, _Layer, _ptr, fold_weight_norm
from .configs import AudioConfig, BigVGANConfig
from .hifigan import structure_dims

FILTER_TAPS = 12                      # GVX_BIGVGAN_FILTER_TAPS
ACT_TILE = 32                         # GVX_BIGVGAN_ACT_TILE: positions per workgroup of the activation kernel
_FILTER_KEY = re.compile(r"\.(upsample\.filter|downsample\.lowpass\.filter)$")


def kaiser_sinc_filter() -> torch.Tensor:
    """The activation's fixed 12-tap low-pass filter, float64 on the host: a sinc of cutoff 0.25 under a symmetric Kaiser window of
    half-width 0.3, normalised to sum 1.  The same filter serves the 2x upsampling and the 2x downsampling."""
    cutoff, half_width, n = 0.25, 0.3, FILTER_TAPS
    a_k = 2.285 * (n // 2 - 1) * math.pi * (4 * half_width) + 7.95   # ~51.02: the > 50 branch of Kaiser's formula
    beta = 0.1102 * (a_k - 8.7)
    j = torch.arange(n, dtype=torch.float64)
    ratio = 2.0 * j / (n - 1) - 1.0
    window = torch.special.i0(beta * torch.sqrt(1.0 - ratio * ratio)) / torch.special.i0(torch.tensor(beta, dtype=torch.float64))
    f = 2 * cutoff * window * torch.sinc(2 * cutoff * (j - n // 2 + 0.5))
    return f / f.sum()


def snake_constants(alpha: torch.Tensor, beta: Optional[torch.Tensor], activation: str, logscale: bool):
    """``alpha`` / ``beta`` [C] -> the kernel's per-channel constants (a, g) in float32, computed in float64: ``z = u + g sin(a u)^2``."""
    a = alpha.detach().double()
    a = a.exp() if logscale else a
    if activation == "snakebeta":
        b = beta.detach().double()
        b = b.exp() if logscale else b
    else:
        b = a
    return a.float(), (1.0 / (b + 1e-9)).float()


def antialiased_snake(x: torch.Tensor, alpha: torch.Tensor, beta: Optional[torch.Tensor] = None, lengths=None, activation: str = "snakebeta",
                      logscale: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """BigVGAN's anti-aliased activation on its own (gvx_snake_antialiased): x float32 [B, n_max, C] channels-last on the device, alpha
    (and beta for "snakebeta") [C] -> [B, n_max, C].  ``lengths`` ([B], host or device): every row at its own length, bit for bit that
    row run alone; ``out`` is exact zeros at and behind a row's length, and ``x`` is never read there.  ``out``: a float32 contiguous
    tensor of x's shape to write into, every element of which is written."""
    if x.dim() != 3 or x.device.type != "cuda" or x.dtype != torch.float32:
        raise ValueError(f"x must be float32 [B, n_max, C] on the device, got {x.dtype} {tuple(x.shape)} on {x.device}")
    if activation not in ("snake", "snakebeta"):
        raise ValueError(f"activation must be 'snake' or 'snakebeta', not {activation!r}")
    B, n_max, C = x.shape
    if alpha.shape != (C,) or (activation == "snakebeta" and (beta is None or beta.shape != (C,))):
        raise ValueError(f"alpha (and beta for 'snakebeta') must be [{C}]")
    dev = x.device
    x = x.contiguous()
    lens = None
    if lengths is not None:
        host = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
        if len(host) != B or any(not 0 <= n <= n_max for n in host):
            raise ValueError(f"lengths must be {B} values in [0, {n_max}]")
        lens = torch.tensor(host, dtype=torch.int32, device=dev)
    a, g = snake_constants(alpha.to(dev), beta.to(dev) if beta is not None else None, activation, logscale)
    f = kaiser_sinc_filter().to(dev, torch.float32)
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous() or out.data_ptr() == x.data_ptr():
        raise ValueError("out must be a contiguous float32 tensor of x's shape on x's device, and not x")
    _lib.check(_lib.load().gvx_snake_antialiased(x.data_ptr(), _ptr(lens), B, n_max, C, f.data_ptr(), a.contiguous().data_ptr(),
                                                 g.contiguous().data_ptr(), out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return out


def dims_from_config(mc: BigVGANConfig, ac: AudioConfig) -> _lib.gvx_bigvgan_dims:
    d = _lib.gvx_bigvgan_dims()
    d.net = structure_dims(mc, ac)
    d.snakebeta, d.tanh_at_final, d.bias_at_final = int(mc.activation == "snakebeta"), int(mc.use_tanh_at_final), int(mc.use_bias_at_final)
    return d


class _Snake(nn.Module):
    """The learned per-channel frequency ``alpha`` and, for "snakebeta", magnitude ``beta``: zeros in log scale, ones otherwise."""

    def __init__(self, channels: int, mc: BigVGANConfig) -> None:
        super().__init__()
        start = torch.zeros if mc.snake_logscale else torch.ones
        self.alpha = nn.Parameter(start(channels))
        if mc.activation == "snakebeta":
            self.beta = nn.Parameter(start(channels))


class _Activation(nn.Module):
    """The anti-aliased activation's parameters, under the published ``Activation1d``'s name ``act``; its filters are not parameters."""

    def __init__(self, channels: int, mc: BigVGANConfig) -> None:
        super().__init__()
        self.act = _Snake(channels, mc)


class _AMPBlock1(nn.Module):
    def __init__(self, channels: int, k: int, n: int, mc: BigVGANConfig) -> None:
        super().__init__()
        self.convs1 = nn.ModuleList([_Layer((channels, channels, k), channels, k * channels) for _ in range(n)])
        self.convs2 = nn.ModuleList([_Layer((channels, channels, k), channels, k * channels) for _ in range(n)])
        self.activations = nn.ModuleList([_Activation(channels, mc) for _ in range(2 * n)])


class _AMPBlock2(nn.Module):
    def __init__(self, channels: int, k: int, n: int, mc: BigVGANConfig) -> None:
        super().__init__()
        self.convs = nn.ModuleList([_Layer((channels, channels, k), channels, k * channels) for _ in range(n)])
        self.activations = nn.ModuleList([_Activation(channels, mc) for _ in range(n)])


class BigVGANGenerator(DeviceGenerator):
    """A row needs 1 frame; ``stage_outputs`` are x after every stage's average over its resblocks.  The workspace is five tensors of
    the widest stage and the transposed mel: 164,160 bytes per frame and row for the base model."""
    model_name = "bigvgan"
    _abi, _config_class = "gvx_bigvgan", BigVGANConfig
    _min_frames = 1
    _range_hint = ""
    _short_tail = "1 of the frames"

    def __init__(self, model_config: BigVGANConfig, audio_config: AudioConfig) -> None:
        super().__init__(model_config, audio_config)
        c = model_config.upsample_initial_channel
        self.conv_pre = _Layer((c, audio_config.n_mels, 7), c, 7 * audio_config.n_mels)
        self.ups, self.resblocks = nn.ModuleList(), nn.ModuleList()
        block = _AMPBlock1 if model_config.resblock == "1" else _AMPBlock2
        for r in model_config.upsample_rates:
            self.ups.append(nn.ModuleList([_Layer((c, c // 2, 2 * r), c // 2, 2 * c)]))   # ConvTranspose1d [in, out, k], published as ups.<i>.0
            c //= 2
            for k, ds in zip(model_config.resblock_kernel_sizes, model_config.resblock_dilation_sizes):
                self.resblocks.append(block(c, k, len(ds), model_config))
        self.activation_post = _Activation(c, model_config)
        self.conv_post = _Layer((1, c, 7), 1, 7 * c)
        if not model_config.use_bias_at_final:
            self.conv_post.bias = None

    def dims(self) -> _lib.gvx_bigvgan_dims:
        return dims_from_config(self.model_config, self.audio_config)

    def _stage_shapes(self):
        return self.model_config.upsample_initial_channel, self.model_config.upsample_rates

    def _pack_items(self, held=None):
        """The convolutions under the packer's names (``ups.<i>``; a zero ``conv_post.bias`` where the model has none), the filter, and
        per activation ``<its name>.a`` / ``.g``."""
        mc = self.model_config
        state = self.state_dict()
        items = []
        for k, v in state.items():
            if ".act." in k:
                continue
            items.append((re.sub(r"^ups\.(\d+)\.0\.", r"ups.\1.", k), v))
        if not mc.use_bias_at_final:
            items.append(("conv_post.bias", torch.zeros(1, device=self._device())))
        items.append(("filter", kaiser_sinc_filter()))
        for k, alpha in state.items():
            if k.endswith(".act.alpha"):
                name = k[:-len(".act.alpha")]
                a, g = snake_constants(alpha, state.get(name + ".act.beta"), mc.activation, mc.snake_logscale)
                items += [(name + ".a", a), (name + ".g", g)]
        return items

    def _convert_state_dict(self, state_dict) -> Dict[str, torch.Tensor]:
        """Folds weight normalisation; a published checkpoint's filter buffers (``...upsample.filter``, ``...downsample.lowpass.filter``,
        [1, 1, 12]) are compared with the computed filter and dropped, a mismatch beyond 1e-6 is a ValueError that names the key."""
        f = kaiser_sinc_filter()
        out = {}
        for k, v in fold_weight_norm(state_dict).items():
            if _FILTER_KEY.search(k):
                got = v.detach().double().cpu().reshape(-1)
                if got.numel() != FILTER_TAPS or not bool(((got - f).abs() <= 1e-6).all()):
                    raise ValueError(f"{k}: the checkpoint's anti-aliasing filter is not the 12-tap Kaiser-sinc filter this model computes")
                continue
            out[k] = v
        return out

    def vocode_with_grad(self, mel: torch.Tensor, mel_lengths=None) -> torch.Tensor:
        """``vocode`` when gradients are off or nothing requires one; otherwise NotImplementedError: BigVGAN's backward is not built."""
        if torch.is_grad_enabled() and (mel.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError("BigVGANGenerator has no backward on the device yet: vocode_with_grad runs only under torch.no_grad() or "
                                      "when neither the mel nor a parameter requires a gradient")
        return self.vocode(mel, mel_lengths)

    def load_checkpoint_statedicts(self, statedicts: Dict, save_optimizer_dict: bool = False, optimizer: Optional[Dict] = None) -> None:
        """Our own ``{"model_statedict": ...}`` or the published generator file's ``{"generator": ...}`` (weight-normalised)."""
        if "model_statedict" in statedicts:
            self.load_state_dict(statedicts["model_statedict"])
        elif "generator" in statedicts:
            self.load_state_dict(statedicts["generator"])
        else:
            raise KeyError("a BigVGAN checkpoint holds its weights under 'model_statedict' or, in the published form, under 'generator'")
