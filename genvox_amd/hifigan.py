"""HiFi-GAN generator: mel -> waveform on the MI355X (include/genvox_amd.h, "HiFi-GAN generator"; kernels in csrc/hifigan.hip).

The module holds the parameters in PyTorch's own layouts - ``Conv1d`` as [out, in, k], ``ConvTranspose1d`` as [in, out, k] - under the
published implementation's names (``conv_pre``, ``ups.<i>``, ``resblocks.<n>.convs1.<m>`` / ``.convs2.<m>`` or ``.convs.<m>``,
``conv_post``), so a published V1, V2 or V3 generator checkpoint loads as it is; weight normalisation is folded on load.  The kernels
read a packed blob that is rebuilt on the device whenever the parameters change.  The calls are ``DeviceGenerator``'s: ``vocode`` is
inference; ``vocode_with_grad`` (kernels in csrc/hifigan_train.hip) is the same call attached to autograd, for training or fine-tuning
the generator with any loss written in torch (``MultiResolutionSTFTLoss``, a discriminator).  There is no CPU or eager path.

The model vocodes whatever mel scale its checkpoint was trained on.  A checkpoint trained on the published recipe's natural-log mels
is NOT matched to this package's Tacotron2 mels (log10, dB-scaled: ``AudioProcessor``), and no conversion is part of this module: pair
the Tacotron2 with a HiFi-GAN trained on its own mels."""
from __future__ import annotations

from typing import Dict, List, Optional

import torch
from torch import nn

from . import _lib
from ._device_module import DeviceGenerator, _Layer, _ptr
from .configs import AudioConfig, HiFiGANConfig


def conv_layer(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, dilation: int = 1, stride: int = 1, lengths=None,
               in_mul: int = 1, act: bool = False, slope: float = 0.1, res: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
               accumulate: bool = False, divide: float = 0.0, zero_tail: bool = False, tanh_out: bool = False, gradient: bool = False,
               mask: Optional[torch.Tensor] = None, add2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One layer of the generators on its own (gvx_hifigan_layer, which states the arithmetic): x float32 [B, L, C] channels-last on the
    device -> [B, L * stride, Cout].  ``weight`` is in PyTorch's layout and brought into the device order here, in torch (this wrapper is
    for tests): ``Conv1d`` [Cout, Cin, k] with ``dilation`` and padding (k - 1) dilation / 2; with ``stride`` r > 1 ``ConvTranspose1d``
    [Cin, Cout, 2 r] of stride r and padding r / 2; with ``gradient`` the FORWARD convolution's [N, C, k], x being dY [B, L, N] and the
    result dX [B, L, C] = (lrelu'(mask) * conv^T(dY) + res + add2) / divide.  ``lengths`` ([B], host or device) count units of ``in_mul``
    positions.  ``out``: the tensor to write (what it holds behind a row stays unless ``zero_tail``; ``accumulate`` adds to what it holds),
    or None for a new one.  The library refuses what the kernels cannot take."""
    if x.dim() != 3 or x.device.type != "cuda" or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"x must be contiguous float32 [B, L, C] on the device, got {x.dtype} {tuple(x.shape)} on {x.device}")
    if weight.dim() != 3:
        raise ValueError(f"weight must have three dimensions, got {tuple(weight.shape)}")
    B, L, C = x.shape
    dev = x.device
    prep = lambda t: t.detach().to(dev, torch.float32).contiguous()
    phases, taps = 1, weight.shape[2]
    if gradient:
        if stride != 1 or weight.shape[0] != C:
            raise ValueError(f"a gradient takes stride 1 and the forward weight [{C}, C, k], got {tuple(weight.shape)}")
        w, c_out = prep(weight.flip(2).permute(1, 2, 0)), weight.shape[1]               # [C][k][N], the taps reversed
    elif stride > 1:
        if stride % 2 or tuple(weight.shape[::2]) != (C, 2 * stride):
            raise ValueError(f"with stride {stride} (even) weight must be [{C}, Cout, {2 * stride}], got {tuple(weight.shape)}")
        half = stride // 2
        tap = torch.tensor([[ph + half, ph + half + stride if ph < half else ph + half - stride] for ph in range(stride)])
        w, c_out = prep(weight.permute(2, 1, 0)[tap].permute(0, 2, 1, 3)), weight.shape[1]   # [r][Cout][2][Cin]
        phases, taps = stride, 2
    else:
        if weight.shape[1] != C:
            raise ValueError(f"weight must be [Cout, {C}, k], got {tuple(weight.shape)}")
        w, c_out = prep(weight.permute(0, 2, 1)), weight.shape[0]                         # [Cout][k][Cin]
    if bias is not None and tuple(bias.shape) != (c_out,):
        raise ValueError(f"bias must be [{c_out}], got {tuple(bias.shape)}")
    if in_mul < 1 or L % in_mul:
        raise ValueError(f"in_mul must divide the {L} positions")
    T = L // in_mul
    lens = None
    if lengths is not None:
        host = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
        if len(host) != B or any(not 0 <= n <= T for n in host):
            raise ValueError(f"lengths must be {B} values in [0, {T}]")
        lens = torch.tensor(host, dtype=torch.int32, device=dev)
    for name, t, shape in (("res", res, (B, L, c_out)), ("mask", mask, (B, L, c_out)), ("add2", add2, (B, L, c_out)), ("out", out, (B, L * phases, c_out))):
        if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous()):
            raise ValueError(f"{name} must be contiguous float32 {list(shape)} on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    if out is None:
        out = torch.empty(B, L * phases, c_out, device=dev)
    b = prep(bias) if bias is not None else None
    _lib.check(_lib.load().gvx_hifigan_layer(x.data_ptr(), w.data_ptr(), _ptr(b), _ptr(res), _ptr(mask), _ptr(add2), out.data_ptr(), _ptr(lens), B, T,
                                             int(in_mul), C, c_out, taps, int(dilation), phases, int(act), int(accumulate), float(divide), int(zero_tail),
                                             int(tanh_out), float(slope), int(gradient), torch.cuda.current_stream(dev).cuda_stream))
    return out


def structure_dims(mc: HiFiGANConfig, ac: AudioConfig) -> _lib.gvx_hifigan_dims:
    """The network's structure, which BigVGAN shares; the slopes stay 0."""
    d = _lib.gvx_hifigan_dims()
    d.n_mels, d.upsample_initial_channel, d.n_stages = ac.n_mels, mc.upsample_initial_channel, len(mc.upsample_rates)
    for i, (r, k) in enumerate(zip(mc.upsample_rates, mc.upsample_kernel_sizes)):
        d.upsample_rates[i], d.upsample_kernel_sizes[i] = r, k
    d.resblock, d.n_resblocks = int(mc.resblock), len(mc.resblock_kernel_sizes)
    d.n_dilations = len(mc.resblock_dilation_sizes[0])
    for j, (k, ds) in enumerate(zip(mc.resblock_kernel_sizes, mc.resblock_dilation_sizes)):
        d.resblock_kernel_sizes[j] = k
        for m, dil in enumerate(ds):
            d.resblock_dilation_sizes[j][m] = dil
    return d


def dims_from_config(mc: HiFiGANConfig, ac: AudioConfig) -> _lib.gvx_hifigan_dims:
    d = structure_dims(mc, ac)
    d.slope, d.post_slope = float(mc.leaky_slope), float(mc.post_leaky_slope)
    return d


class _ResBlock1(nn.Module):
    def __init__(self, channels: int, k: int, n: int) -> None:
        super().__init__()
        self.convs1 = nn.ModuleList([_Layer((channels, channels, k), channels, k * channels) for _ in range(n)])
        self.convs2 = nn.ModuleList([_Layer((channels, channels, k), channels, k * channels) for _ in range(n)])


class _ResBlock2(nn.Module):
    def __init__(self, channels: int, k: int, n: int) -> None:
        super().__init__()
        self.convs = nn.ModuleList([_Layer((channels, channels, k), channels, k * channels) for _ in range(n)])


class HiFiGANGenerator(DeviceGenerator):
    """A row needs 1 frame; ``stage_outputs`` are x after every stage's average over its resblocks.  The workspace is 131,392 bytes
    per frame and row for V1; ``vocode_with_grad``'s tape is 1,812,800 for V1, 453,440 for V2 and 267,584 for V3."""
    model_name = "hifigan"
    _abi, _config_class = "gvx_hifigan", HiFiGANConfig
    _min_frames = 1
    _range_hint = ""
    _short_tail = "1 of the frames"

    def __init__(self, model_config: HiFiGANConfig, audio_config: AudioConfig) -> None:
        super().__init__(model_config, audio_config)
        c = model_config.upsample_initial_channel
        self.conv_pre = _Layer((c, audio_config.n_mels, 7), c, 7 * audio_config.n_mels)
        self.ups, self.resblocks = nn.ModuleList(), nn.ModuleList()
        block = _ResBlock1 if model_config.resblock == "1" else _ResBlock2
        for r in model_config.upsample_rates:
            self.ups.append(_Layer((c, c // 2, 2 * r), c // 2, 2 * c))   # ConvTranspose1d: [in, out, k]; two taps of c inputs reach an output
            c //= 2
            for k, ds in zip(model_config.resblock_kernel_sizes, model_config.resblock_dilation_sizes):
                self.resblocks.append(block(c, k, len(ds)))
        self.conv_post = _Layer((1, c, 7), 1, 7 * c)

    def dims(self) -> _lib.gvx_hifigan_dims:
        return dims_from_config(self.model_config, self.audio_config)

    def _stage_shapes(self):
        return self.model_config.upsample_initial_channel, self.model_config.upsample_rates

    def backward_stage_times_ms(self) -> List[float]:
        """Durations of the last ``vocode_with_grad`` backward's parts, in the order they ran: the weight transposes, conv_post,
        every stage from the last to the first, conv_pre (synchronises)."""
        return self._times_ms("backward_stage_times_ms", 12)

    def load_checkpoint_statedicts(self, statedicts: Dict, save_optimizer_dict: bool = False, optimizer: Optional[Dict] = None) -> None:
        """Our own ``{"model_statedict": ...}`` or the published generator file's ``{"generator": ...}`` (weight-normalised)."""
        if "model_statedict" in statedicts:
            self.load_state_dict(statedicts["model_statedict"])
        elif "generator" in statedicts:
            self.load_state_dict(statedicts["generator"])
        else:
            raise KeyError("a HiFi-GAN checkpoint holds its weights under 'model_statedict' or, in the published form, under 'generator'")
