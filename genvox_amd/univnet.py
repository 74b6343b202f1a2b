"""UnivNet generator: (mel, noise) -> waveform on the MI355X, inference (include/genvox_amd.h, "UnivNet generator"; kernels in
csrc/univnet.hip on the dense fp32 GEMM and HiFi-GAN's layer kernels).

Noise at the frame rate, upsampled through blocks whose convolutions carry weights of their own for every mel frame: a small network
predicts them from the mel (location-variable convolution).  The module holds the parameters in PyTorch's own layouts under the published
implementation's names (``conv_pre``, ``res_stack.<i>.convt_pre.1``, ``.conv_blocks.<m>.1``, ``.kernel_predictor.input_conv.0`` /
``.residual_convs.<j>.1`` / ``.3`` / ``.kernel_conv`` / ``.bias_conv``, ``conv_post.1``), so a published state dict loads as it is, its
weight normalisation folded.  The kernels read a packed blob that is rebuilt on the device whenever the parameters change; the output
channels of ``kernel_conv`` and ``bias_conv`` are permuted at that point into the order the LVC kernel reads (``device_order``), so
nothing is permuted per call.  The calls are ``DeviceGenerator``'s, with the noise beside the mel.  There is no backward yet:
``vocode_with_grad`` is ``vocode`` when nothing asks for a gradient and raises ``NotImplementedError`` otherwise.  There is no CPU or
eager path.

As with the other vocoders, the model vocodes whatever mel scale its checkpoint was trained on; no conversion is part of this module."""
from __future__ import annotations

from typing import Dict, Optional

import torch
from torch import nn

from . import _lib
from ._device_module import DeviceGenerator, _Layer, _ptr, fold_weight_norm
from .configs import AudioConfig, UnivNetConfig

LVC_KERNEL = 3    # the LVC kernel size
MIN_FRAMES = 4    # GVX_UNIVNET_MIN_FRAMES


def device_order(channel_size: int, n_dilations: int) -> torch.Tensor:
    """int64 [n_dilations * 6 C^2]: for every output channel of ``kernel_conv`` in the DEVICE order - [layer][2C out][3 taps][C in] -
    its index in the published order, [layer][C in][2C out][3 taps] (the view ``[B, n_dil, C_in, 2C, 3, T]``)."""
    c = channel_size
    pub = torch.arange(n_dilations * c * 2 * c * LVC_KERNEL).view(n_dilations, c, 2 * c, LVC_KERNEL)
    return pub.permute(0, 2, 3, 1).reshape(-1)


def tconv_phase_taps(stride: int) -> torch.Tensor:
    """int64 [stride, 2]: the tap of ``ConvTranspose1d(kernel 2 s, stride s, padding s / 2)`` that connects output ``s q + phase`` with
    input ``q`` (column 0) and with input ``q - 1`` (phase < s / 2) or ``q + 1`` (column 1): hifigan.hip's two-tap phase split."""
    half = stride // 2
    return torch.tensor([[ph + half, ph + half + stride if ph < half else ph + half - stride] for ph in range(stride)])


def _lens_on(lengths, B: int, T: int, dev) -> Optional[torch.Tensor]:
    if lengths is None:
        return None
    host = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
    if len(host) != B or any(not 0 <= n <= T for n in host):
        raise ValueError(f"lengths must be {B} values in [0, {T}]")
    return torch.tensor(host, dtype=torch.int32, device=dev)


def lvc_gated(x: torch.Tensor, kernels: torch.Tensor, bias: torch.Tensor, conv_weight: Optional[torch.Tensor] = None,
              conv_bias: Optional[torch.Tensor] = None, dilation: int = 1, lengths=None, slope: float = 0.2, in_place: bool = False) -> torch.Tensor:
    """One gated LVC layer on its own (gvx_lvc_gated): x float32 [B, T * cum, C] channels-last on the device, ``kernels`` in the
    PUBLISHED layout [B, C in, 2C out, 3, T] and ``bias`` [B, 2C, T] (permuted into the device order here, in torch: this wrapper is for
    tests), ``conv_weight`` [C, C, 3] and ``conv_bias`` [C] of the dilated convolution in front, or both None ->
    ``x + sigmoid(o[:C]) * tanh(o[C:])`` with ``o = bias + LVC(y)`` and ``y = lrelu(conv(lrelu(x)))`` (``lrelu(x)`` without a
    convolution), [B, T * cum, C].  ``lengths`` ([B] frames, host or device): every row at its own ``T_b * cum`` positions, bit for bit
    that row run alone; x is returned as it is behind them and never read there.  ``in_place``: the result is written into ``x``
    (contiguous) itself, which the layer allows with a convolution only - without one it reads its neighbours' positions of x, and the
    library refuses."""
    if x.dim() != 3 or x.device.type != "cuda" or x.dtype != torch.float32:
        raise ValueError(f"x must be float32 [B, T * cum, C] on the device, got {x.dtype} {tuple(x.shape)} on {x.device}")
    B, L, C = x.shape
    if kernels.dim() != 5 or tuple(kernels.shape[:4]) != (B, C, 2 * C, LVC_KERNEL) or kernels.shape[4] < 1 or L % kernels.shape[4]:
        raise ValueError(f"kernels must be [{B}, {C}, {2 * C}, {LVC_KERNEL}, T] with T dividing {L}, got {tuple(kernels.shape)}")
    T = kernels.shape[4]
    if tuple(bias.shape) != (B, 2 * C, T):
        raise ValueError(f"bias must be [{B}, {2 * C}, {T}], got {tuple(bias.shape)}")
    if (conv_weight is None) != (conv_bias is None) or (conv_weight is not None and (tuple(conv_weight.shape) != (C, C, 3) or tuple(conv_bias.shape) != (C,))):
        raise ValueError(f"conv_weight and conv_bias must be [{C}, {C}, 3] and [{C}], or both None")
    dev = x.device
    prep = lambda t: t.detach().to(dev, torch.float32).contiguous()
    kern = torch.cat([prep(kernels).permute(0, 4, 2, 3, 1).reshape(B, T, -1), prep(bias).permute(0, 2, 1)], dim=2).contiguous()
    w = prep(conv_weight.permute(0, 2, 1)) if conv_weight is not None else None   # [C][3][C]
    b = prep(conv_bias) if conv_bias is not None else None
    lens = _lens_on(lengths, B, T, dev)
    if in_place and not x.is_contiguous():
        raise ValueError("in_place needs a contiguous x")
    x = x.contiguous()
    out = x if in_place else torch.empty_like(x)
    scratch = torch.empty_like(x) if w is not None else None
    _lib.check(_lib.load().gvx_lvc_gated(x.data_ptr(), kern.data_ptr(), 1, 0, _ptr(w), _ptr(b), int(dilation), _ptr(lens), B, T, L // T, C, float(slope),
                                         _ptr(scratch), out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return out


def dims_from_config(mc: UnivNetConfig, ac: AudioConfig) -> _lib.gvx_univnet_dims:
    d = _lib.gvx_univnet_dims()
    d.n_mels, d.noise_dim, d.channel_size = int(ac.n_mels), mc.noise_dim, mc.channel_size
    d.n_dilations, d.n_blocks = len(mc.dilations), len(mc.strides)
    for i, v in enumerate(mc.dilations):
        d.dilations[i] = v
    for i, v in enumerate(mc.strides):
        d.strides[i] = v
    d.kpnet_hidden_channels, d.kpnet_conv_size, d.slope = mc.kpnet_hidden_channels, mc.kpnet_conv_size, mc.lReLU_slope
    return d


def _at(index: int, layer: nn.Module) -> nn.ModuleDict:
    """``layer`` under the name of its place in the published ``nn.Sequential``."""
    return nn.ModuleDict({str(index): layer})


class _KernelPredictor(nn.Module):
    def __init__(self, mc: UnivNetConfig, n_mels: int) -> None:
        super().__init__()
        h, c, k, n = mc.kpnet_hidden_channels, mc.channel_size, mc.kpnet_conv_size, len(mc.dilations)
        self.input_conv = _at(0, _Layer((h, n_mels, 5), h, 5 * n_mels))
        self.residual_convs = nn.ModuleList([nn.ModuleDict({"1": _Layer((h, h, k), h, k * h), "3": _Layer((h, h, k), h, k * h)}) for _ in range(3)])
        # the predicted kernels multiply 3 C values each: the start keeps the LVC's output at the scale of its input
        self.kernel_conv = _Layer((c * 2 * c * LVC_KERNEL * n, h, k), c * 2 * c * LVC_KERNEL * n, k * h * LVC_KERNEL * c)
        self.bias_conv = _Layer((2 * c * n, h, k), 2 * c * n, k * h)


class _LVCBlock(nn.Module):
    def __init__(self, mc: UnivNetConfig, n_mels: int, stride: int) -> None:
        super().__init__()
        c = mc.channel_size
        self.convt_pre = _at(1, _Layer((c, c, 2 * stride), c, 2 * c))   # ConvTranspose1d [in, out, k]
        self.conv_blocks = nn.ModuleList([_at(1, _Layer((c, c, 3), c, 3 * c)) for _ in mc.dilations])
        self.kernel_predictor = _KernelPredictor(mc, n_mels)


class UnivNetGenerator(DeviceGenerator):
    """A row needs 4 frames (the reflections by 3).  ``vocode`` takes the noise beside the mel, or draws it; ``stage_outputs`` are x
    after ``conv_pre`` [B, T, C], after every block [B, T * cum_i, C] and the output layer before its tanh [B, T * hop, 1].  The
    workspace is 199,312 bytes per frame and row for c32 with 100 mels - 99,328 of them one block's predicted kernels, a slot the
    three blocks share - so a batch of 32 x 800 frames runs in groups of rows under ``WORKSPACE_CAP_BYTES``."""
    model_name = "univnet"
    _abi, _config_class = "gvx_univnet", UnivNetConfig
    _min_frames = MIN_FRAMES
    _range_hint = " (a row needs 4 frames: the first and the last layer reflect by 3)"
    _short_tail = "4 of the frames"

    def __init__(self, model_config: UnivNetConfig, audio_config: AudioConfig) -> None:
        super().__init__(model_config, audio_config)
        mc, n_mels = model_config, int(audio_config.n_mels)
        self.conv_pre = _Layer((mc.channel_size, mc.noise_dim, 7), mc.channel_size, 7 * mc.noise_dim)
        self.res_stack = nn.ModuleList([_LVCBlock(mc, n_mels, s) for s in mc.strides])
        self.conv_post = _at(1, _Layer((1, mc.channel_size, 7), 1, 7 * mc.channel_size))
        self._noise_seed = 0
        self._noise_generator: Optional[torch.Generator] = None

    def dims(self) -> _lib.gvx_univnet_dims:
        return dims_from_config(self.model_config, self.audio_config)

    def _stage_tensor_shapes(self, T: int):
        mc = self.model_config
        shapes, cum = [(T, mc.channel_size)], 1
        for s in mc.strides:
            cum *= s
            shapes.append((T * cum, mc.channel_size))
        return shapes + [(T * cum, 1)]

    def stage_times_ms(self):
        """Durations of the last call's parts: ``conv_pre``, per block its kernel predictor and then its layers, ``conv_post``
        (synchronises)."""
        return self._times_ms("stage_times_ms", 2 * len(self.model_config.strides) + 2)

    # ------------------------------------------------------------------ the noise
    def manual_seed(self, seed: int) -> None:
        """Seeds the generator the module draws its noise from: the calls behind it with ``noise=None`` repeat."""
        self._noise_seed, self._noise_generator = int(seed), None

    def draw_noise(self, B: int, T: int) -> torch.Tensor:
        """The next ``torch.randn`` [B, noise_dim, T] of the module's own generator, on the module's device."""
        dev = self._require_gpu()
        if self._noise_generator is None or self._noise_generator.device != dev:
            self._noise_generator = torch.Generator(device=dev)
            self._noise_generator.manual_seed(self._noise_seed)
        return torch.randn(B, self.model_config.noise_dim, T, generator=self._noise_generator, device=dev, dtype=torch.float32)

    def _check_extra(self, noise, dev, B: int, T: int) -> torch.Tensor:
        """The noise of a call whose mel and lengths have passed their checks: drawn, or held to [B, noise_dim, T] float32 on ``dev``."""
        if noise is None:
            return self.draw_noise(B, T)
        if not isinstance(noise, torch.Tensor) or tuple(noise.shape) != (B, self.model_config.noise_dim, T):
            raise ValueError(f"noise must be [{B}, {self.model_config.noise_dim}, {T}], got {tuple(noise.shape) if isinstance(noise, torch.Tensor) else type(noise)}")
        if noise.device != dev or noise.dtype != torch.float32:
            raise ValueError(f"noise must be float32 on {dev}, got {noise.dtype} on {noise.device}")
        return noise.contiguous()

    def _forward_extra(self, extra, lo: int, n: int):
        return (extra[lo:lo + n].data_ptr(),)

    def vocode(self, mel: torch.Tensor, mel_lengths=None, stage_outputs: bool = False, workspace: Optional[torch.Tensor] = None,
               noise: Optional[torch.Tensor] = None):
        """``DeviceGenerator.vocode`` with ``noise`` float32 [B, noise_dim, T] on the mel's device; None draws it from the module's own
        generator (``manual_seed``) once the mel and the lengths have passed their checks.  What lies behind a row's frames is never
        read, in mel or noise.  A row split by ``WORKSPACE_CAP_BYTES`` slices the noise with the rows.  No padding is done here: see
        ``vocode_utterances``."""
        return super().vocode(mel, mel_lengths, stage_outputs, workspace, _extra=noise)

    def vocode_utterances(self, mel: torch.Tensor, mel_lengths=None) -> torch.Tensor:
        """The published inference: ``tail_pad_frames`` frames of ``tail_pad_value`` behind every row's own frames, ``vocode``, and the
        padding's samples dropped - it hides the artefact at an utterance's end.  -> [B, T * hop], a row's ``T_b * hop`` samples in front
        and zeros behind them.  The padding counts towards the 4 frames a row needs."""
        mc = self.model_config
        pad = mc.tail_pad_frames
        if pad == 0:
            return self.vocode(mel, mel_lengths)
        dev = self._require_gpu()
        if mel.dim() != 3 or mel.shape[1] != self.audio_config.n_mels or mel.shape[0] < 1 or mel.shape[2] < 1:
            raise ValueError(f"mel must be [B, {self.audio_config.n_mels}, T] with at least one row and one frame, got {tuple(mel.shape)}")
        if mel.device != dev or mel.dtype != torch.float32:
            raise ValueError(f"mel must be float32 on {dev}, got {mel.dtype} on {mel.device}")
        B, _, T = mel.shape
        host = [T] * B if mel_lengths is None else self._host_lengths(mel_lengths)   # the one look at the lengths: vocode gets a host list
        if len(host) != B:
            raise ValueError(f"{len(host)} lengths for {B} rows")
        least = max(1, MIN_FRAMES - pad)
        for b, n in enumerate(host):
            if not least <= n <= T:
                raise ValueError(f"row {b}: {n} frames are outside [{least}, {T}]")
        lens = torch.tensor(host, dtype=torch.int32, device=dev)
        padded = torch.cat([mel, mel.new_empty(B, mel.shape[1], pad)], dim=2)
        behind = torch.arange(T + pad, device=dev)[None, :] >= lens[:, None]
        padded = torch.where(behind[:, None, :], torch.full_like(padded, mc.tail_pad_value), padded)
        wav = self.vocode(padded, [n + pad for n in host])[:, :T * self.hop]
        keep = torch.arange(T * self.hop, device=dev)[None, :] < (lens * self.hop)[:, None]
        return torch.where(keep, wav, torch.zeros_like(wav)).contiguous()

    # ------------------------------------------------------------------ weights
    def _pack_items(self, held=None):
        """The tensors under the packer's names and in its layouts: every convolution tap-major [out][k][in] (``conv_pre`` and
        ``input_conv`` with their input channels padded to a multiple of 4), ``convt_pre`` as its two-tap phases [s][out][2][in],
        ``conv_post`` [7][C], and ``kernel_conv`` + ``bias_conv`` as ONE layer ``kernel_predictor.kb`` whose output channels stand in
        the device order (``device_order``)."""
        mc = self.model_config
        state = {k: v.detach() for k, v in self.state_dict().items()}
        tap_major = lambda w, to=4: nn.functional.pad(w.permute(0, 2, 1), (0, -w.shape[1] % to))
        items = [("conv_pre.weight", tap_major(state["conv_pre.weight"])), ("conv_pre.bias", state["conv_pre.bias"])]
        order = device_order(mc.channel_size, len(mc.dilations))
        for i, s in enumerate(mc.strides):
            base, kp = f"res_stack.{i}.", f"res_stack.{i}.kernel_predictor."
            w = state[base + "convt_pre.1.weight"].permute(2, 1, 0)                              # [tap, out, in]
            items.append((base + "convt_pre.weight", w[tconv_phase_taps(s).to(w.device)].permute(0, 2, 1, 3)))   # [s, out, 2, in]
            items.append((base + "convt_pre.bias", state[base + "convt_pre.1.bias"]))
            items.append((kp + "input_conv.weight", tap_major(state[kp + "input_conv.0.weight"])))
            items.append((kp + "input_conv.bias", state[kp + "input_conv.0.bias"]))
            for j in range(3):
                for part in ("1", "3"):
                    items.append((kp + f"residual_convs.{j}.{part}.weight", tap_major(state[kp + f"residual_convs.{j}.{part}.weight"], 1)))
                    items.append((kp + f"residual_convs.{j}.{part}.bias", state[kp + f"residual_convs.{j}.{part}.bias"]))
            rows = order.to(state[kp + "kernel_conv.weight"].device)
            items.append((kp + "kb.weight", torch.cat([tap_major(state[kp + "kernel_conv.weight"][rows], 1), tap_major(state[kp + "bias_conv.weight"], 1)])))
            items.append((kp + "kb.bias", torch.cat([state[kp + "kernel_conv.bias"][rows], state[kp + "bias_conv.bias"]])))
            for m in range(len(mc.dilations)):
                items.append((base + f"conv_blocks.{m}.weight", tap_major(state[base + f"conv_blocks.{m}.1.weight"], 1)))
                items.append((base + f"conv_blocks.{m}.bias", state[base + f"conv_blocks.{m}.1.bias"]))
        items.append(("conv_post.weight", state["conv_post.1.weight"][0].t()))
        items.append(("conv_post.bias", state["conv_post.1.bias"]))
        return items

    def _convert_state_dict(self, state_dict) -> Dict[str, torch.Tensor]:
        """Folds weight normalisation; a key this model does not have is refused by name."""
        out = fold_weight_norm(state_dict)
        own = set(self.state_dict())
        for k in out:
            if k not in own:
                raise KeyError(f"{k}: not a tensor of the UnivNet generator with this config")
        return out

    def vocode_with_grad(self, mel: torch.Tensor, mel_lengths=None, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``vocode`` when gradients are off or nothing requires one; otherwise NotImplementedError: UnivNet's backward is not built."""
        if torch.is_grad_enabled() and (mel.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError("UnivNetGenerator has no backward on the device yet: vocode_with_grad runs only under torch.no_grad() or "
                                      "when neither the mel nor a parameter requires a gradient")
        return self.vocode(mel, mel_lengths, noise=noise)

    def load_checkpoint_statedicts(self, statedicts: Dict, save_optimizer_dict: bool = False, optimizer: Optional[Dict] = None) -> None:
        """Our own ``{"model_statedict": ...}``, the published checkpoint file's ``{"model_g": ...}`` (weight-normalised), or a plain
        state dict (its keys start with ``conv_pre.`` / ``res_stack.`` / ``conv_post.``)."""
        if "model_statedict" in statedicts:
            self.load_state_dict(statedicts["model_statedict"])
        elif "model_g" in statedicts:
            self.load_state_dict(statedicts["model_g"])
        elif any(k.startswith("res_stack.") for k in statedicts):
            self.load_state_dict(statedicts)
        else:
            raise KeyError("a UnivNet checkpoint holds its weights under 'model_statedict' or 'model_g', or is the state dict itself")
