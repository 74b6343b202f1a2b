"""Vocos generator, mel variant: mel -> waveform on the MI355X, inference (include/genvox_amd.h, "Vocos generator"; kernels in
csrc/vocos.hip on the dense fp32 GEMM and the in-LDS FFT).

A ConvNeXt backbone at the frame rate and an inverse STFT.  The module holds the parameters in PyTorch's own layouts under the
published implementation's names (``backbone.embed``, ``backbone.norm``, ``backbone.convnext.<i>.dwconv`` / ``.norm`` / ``.pwconv1`` /
``.pwconv2`` / ``.gamma``, ``backbone.final_layer_norm``, ``head.out``), so a published state dict loads as it is: the window buffer it
carries (``head.istft.window``) is compared with the Hann window computed here and dropped, its ``feature_extractor.*`` buffers are
dropped, and the conditioned ``AdaLayerNorm`` of the EnCodec variant (``backbone.norm.scale`` / ``.shift``) is refused by name.  The
kernels read a packed blob that is rebuilt on the device whenever the parameters change; ``gamma`` is folded into ``pwconv2`` in float64
at that point.  The calls are ``DeviceGenerator``'s.  The backward (gvx_vocos_forward_train / gvx_vocos_backward, csrc/vocos_train.hip)
is opt-in: with ``trainable=False``, the default, ``vocode_with_grad`` is ``vocode`` when nothing asks for a gradient and raises
``NotImplementedError`` otherwise; with ``trainable=True`` it is ``DeviceGenerator``'s autograd node, and the gradients of ``gamma`` and
``pwconv2`` are unfolded on the device from those of the folded tensors.  There is no CPU or eager path.

As with the other vocoders, the model vocodes whatever mel scale its checkpoint was trained on; no conversion is part of this module."""
from __future__ import annotations

import re
from typing import Dict, Optional

import torch
from torch import nn

from . import _lib
from ._device_module import DeviceGenerator, _Layer, _ptr, _weight_table
from .configs import AudioConfig, VocosConfig

TILE = 16          # GVX_VOCOS_TILE: frames per workgroup of the filter + LayerNorm kernel
LN_EPS = 1e-6
_WINDOW_KEY = "head.istft.window"
_ADA_KEY = re.compile(r"\.norm\.(scale|shift)\.")


def hann_window(n_fft: int) -> torch.Tensor:
    """The periodic Hann window of ``n_fft`` points, float64 on the host."""
    return torch.hann_window(n_fft, periodic=True, dtype=torch.float64)


def _lens_on(lengths, B: int, T: int, dev) -> Optional[torch.Tensor]:
    if lengths is None:
        return None
    host = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
    if len(host) != B or any(not 0 <= n <= T for n in host):
        raise ValueError(f"lengths must be {B} values in [0, {T}]")
    return torch.tensor(host, dtype=torch.int32, device=dev)


def dwconv_layernorm(x: torch.Tensor, ln_weight: torch.Tensor, ln_bias: torch.Tensor, weight: Optional[torch.Tensor] = None,
                     bias: Optional[torch.Tensor] = None, lengths=None, eps: float = LN_EPS) -> torch.Tensor:
    """"k = 7 channel-wise filter, then LayerNorm" on its own (gvx_dwconv_layernorm): x float32 [B, T, C] channels-last on the device,
    ``weight`` [C, 1, 7] and ``bias`` [C] of ``Conv1d(C, C, 7, padding=3, groups=C)`` (both None: the LayerNorm alone), ``ln_weight`` and
    ``ln_bias`` [C] -> [B, T, C].  ``lengths`` ([B], host or device): every row at its own length, bit for bit that row run alone; the
    result is exact zeros at and behind a row's length, and ``x`` is never read there."""
    if x.dim() != 3 or x.device.type != "cuda" or x.dtype != torch.float32:
        raise ValueError(f"x must be float32 [B, T, C] on the device, got {x.dtype} {tuple(x.shape)} on {x.device}")
    B, T, C = x.shape
    dev = x.device
    taps = 0 if weight is None else 7
    if (weight is None) != (bias is None) or (weight is not None and (tuple(weight.shape) != (C, 1, 7) or tuple(bias.shape) != (C,))):
        raise ValueError(f"weight and bias must be [{C}, 1, 7] and [{C}], or both None")
    prep = lambda t: t.detach().to(dev, torch.float32).contiguous()
    w = prep(weight.reshape(C, 7).t()) if taps else None   # tap-major [7][C]
    b = prep(bias) if taps else None
    lw, lb = prep(ln_weight), prep(ln_bias)
    lens = _lens_on(lengths, B, T, dev)
    x = x.contiguous()
    out = torch.empty_like(x)
    _lib.check(_lib.load().gvx_dwconv_layernorm(x.data_ptr(), _ptr(lens), B, T, C, taps, _ptr(w), _ptr(b), lw.data_ptr(), lb.data_ptr(), float(eps),
                                                out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return out


def istft_head(coeffs: torch.Tensor, n_fft: int, hop_length: int, padding: str = "center", lengths=None) -> torch.Tensor:
    """The ISTFT head behind its Linear (gvx_istft_head): coeffs float32 [B, T, n_fft + 2] on the device - per frame the n_fft / 2 + 1
    log-magnitudes, then as many phases - -> waveform float32 [B, T * hop_length], a row's samples in front (``T_b * hop`` for "same",
    ``(T_b - 1) * hop`` for "center") and exact zeros behind them."""
    if coeffs.dim() != 3 or coeffs.device.type != "cuda" or coeffs.dtype != torch.float32 or coeffs.shape[2] != n_fft + 2:
        raise ValueError(f"coeffs must be float32 [B, T, {n_fft + 2}] on the device, got {coeffs.dtype} {tuple(coeffs.shape)} on {coeffs.device}")
    if padding not in ("center", "same"):
        raise ValueError(f"padding must be 'center' or 'same', not {padding!r}")
    B, T, _ = coeffs.shape
    dev = coeffs.device
    lib = _lib.load()
    need = lib.gvx_istft_head_workspace_bytes(B, T, int(n_fft))
    if need == 0:
        raise ValueError(f"no ISTFT for B = {B}, T = {T}, n_fft = {n_fft}")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    win = hann_window(int(n_fft)).to(dev, torch.float32)
    lens = _lens_on(lengths, B, T, dev)
    coeffs = coeffs.contiguous()
    wav = torch.empty(B, T * int(hop_length), dtype=torch.float32, device=dev)
    _lib.check(lib.gvx_istft_head(coeffs.data_ptr(), _ptr(lens), B, T, int(n_fft), int(hop_length), int(padding == "center"), win.data_ptr(),
                                  ws.data_ptr(), wav.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return wav


def dwconv_layernorm_backward(x: torch.Tensor, dy: torch.Tensor, ln_weight: torch.Tensor, weight: Optional[torch.Tensor] = None,
                              bias: Optional[torch.Tensor] = None, d_res: Optional[torch.Tensor] = None, lengths=None, eps: float = LN_EPS,
                              workspace: Optional[torch.Tensor] = None, out=None):
    """The backward of ``dwconv_layernorm`` on its own (gvx_dwconv_layernorm_backward): x (the layer's input) and dy (the gradient at the
    LayerNorm's output) float32 [B, T, C] on the device, ``d_res`` the residual path's gradient or None -> (dx [B, T, C], d ln_weight,
    d ln_bias, d weight [C, 1, 7] or None, d bias or None).  Rows are ragged as in the forward: dx is exact zeros at and behind a row's
    length and neither x, dy nor d_res is read there.  ``workspace``: a uint8 tensor to use as it is; ``out``: the five results' own
    tensors (contiguous float32 on the device, None where the result is None), written in place and returned (tests fill them first)."""
    if x.dim() != 3 or x.device.type != "cuda" or x.dtype != torch.float32 or dy.shape != x.shape or dy.dtype != torch.float32 or dy.device != x.device:
        raise ValueError(f"x and dy must be float32 [B, T, C] on the device, got {tuple(x.shape)} and {tuple(dy.shape)}")
    B, T, C = x.shape
    dev = x.device
    taps = 0 if weight is None else 7
    if (weight is None) != (bias is None) or (weight is not None and (tuple(weight.shape) != (C, 1, 7) or tuple(bias.shape) != (C,))):
        raise ValueError(f"weight and bias must be [{C}, 1, 7] and [{C}], or both None")
    if d_res is not None and (d_res.shape != x.shape or d_res.dtype != torch.float32 or d_res.device != dev):
        raise ValueError("d_res must be like x")
    if tuple(ln_weight.shape) != (C,):
        raise ValueError(f"ln_weight must be [{C}], got {tuple(ln_weight.shape)}")
    prep = lambda t: t.detach().to(dev, torch.float32).contiguous()
    w = prep(weight.reshape(C, 7).t()) if taps else None
    b = prep(bias) if taps else None
    lw = prep(ln_weight)
    lens = _lens_on(lengths, B, T, dev)
    lib = _lib.load()
    need = lib.gvx_dwconv_layernorm_backward_workspace_bytes(B, T, C, taps)
    if need == 0:
        raise ValueError(f"no filter + LayerNorm backward for B = {B}, T = {T}, C = {C}")
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if workspace is None else workspace
    x, dy = x.contiguous(), dy.contiguous()
    d_res = d_res.contiguous() if d_res is not None else None
    new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    shapes = [(B, T, C), (C,), (C,)] + ([(C, 1, 7), (C,)] if taps else [None, None])
    if out is None:
        out = [None if sh is None else new(*sh) for sh in shapes]
    for t, sh in zip(out, shapes):
        if (t is None) != (sh is None) or (t is not None and (tuple(t.shape) != sh or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous())):
            raise ValueError(f"out must be contiguous float32 tensors of shapes {shapes} on {dev}")
    dx, d_lw, d_lb, d_w, d_b = out
    _lib.check(lib.gvx_dwconv_layernorm_backward(x.data_ptr(), dy.data_ptr(), _ptr(d_res), _ptr(lens), B, T, C, taps, _ptr(w), _ptr(b), lw.data_ptr(),
                                                 float(eps), dx.data_ptr(), _ptr(d_w), _ptr(d_b), d_lw.data_ptr(), d_lb.data_ptr(), ws.data_ptr(),
                                                 ws.numel(), torch.cuda.current_stream(dev).cuda_stream))
    return dx, d_lw, d_lb, d_w, d_b


def istft_head_backward(coeffs: torch.Tensor, d_wav: torch.Tensor, n_fft: int, hop_length: int, padding: str = "center", lengths=None,
                        workspace: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The backward of ``istft_head`` on its own (gvx_istft_head_backward): coeffs float32 [B, T, n_fft + 2] and the waveform's gradient
    d_wav [B, T * hop_length] on the device -> d_coeffs [B, T, n_fft + 2], exact zeros at and behind a row's frames; d_wav is not read
    behind a row's delivered samples.  ``out``: the result's own tensor, written in place and returned (tests fill it first)."""
    if coeffs.dim() != 3 or coeffs.device.type != "cuda" or coeffs.dtype != torch.float32 or coeffs.shape[2] != n_fft + 2:
        raise ValueError(f"coeffs must be float32 [B, T, {n_fft + 2}] on the device, got {coeffs.dtype} {tuple(coeffs.shape)} on {coeffs.device}")
    if padding not in ("center", "same"):
        raise ValueError(f"padding must be 'center' or 'same', not {padding!r}")
    B, T, _ = coeffs.shape
    dev = coeffs.device
    if tuple(d_wav.shape) != (B, T * int(hop_length)) or d_wav.dtype != torch.float32 or d_wav.device != dev:
        raise ValueError(f"d_wav must be float32 [{B}, {T * int(hop_length)}] on {dev}")
    lib = _lib.load()
    need = lib.gvx_istft_head_backward_workspace_bytes(B, T, int(n_fft), int(hop_length))
    if need == 0:
        raise ValueError(f"no ISTFT backward for B = {B}, T = {T}, n_fft = {n_fft}, hop = {hop_length}")
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if workspace is None else workspace
    win = hann_window(int(n_fft)).to(dev, torch.float32)
    lens = _lens_on(lengths, B, T, dev)
    coeffs, d_wav = coeffs.contiguous(), d_wav.contiguous()
    if out is None:
        out = torch.empty_like(coeffs)
    elif out.shape != coeffs.shape or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
        raise ValueError(f"out must be contiguous float32 {tuple(coeffs.shape)} on {dev}")
    _lib.check(lib.gvx_istft_head_backward(coeffs.data_ptr(), d_wav.data_ptr(), _ptr(lens), B, T, int(n_fft), int(hop_length), int(padding == "center"),
                                           win.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return out


def dims_from_config(mc: VocosConfig, ac: AudioConfig) -> _lib.gvx_vocos_dims:
    d = _lib.gvx_vocos_dims()
    d.n_mels, d.dim, d.intermediate_dim, d.num_layers = int(ac.n_mels), mc.dim, mc.intermediate_dim, mc.num_layers
    d.n_fft, d.hop_length, d.center = mc.n_fft, mc.hop_length, int(mc.padding == "center")
    return d


class _Norm(nn.Module):
    """LayerNorm's parameters: ones and zeros."""

    def __init__(self, dim: int) -> None:
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.bias = nn.Parameter(torch.zeros(dim))


class _ConvNeXtBlock(nn.Module):
    def __init__(self, dim: int, intermediate_dim: int, layer_scale: float) -> None:
        super().__init__()
        self.dwconv = _Layer((dim, 1, 7), dim, 7)
        self.norm = _Norm(dim)
        self.pwconv1 = _Layer((intermediate_dim, dim), intermediate_dim, dim)
        self.pwconv2 = _Layer((dim, intermediate_dim), dim, intermediate_dim)
        self.gamma = nn.Parameter(layer_scale * torch.ones(dim))


class _Backbone(nn.Module):
    def __init__(self, mc: VocosConfig, n_mels: int) -> None:
        super().__init__()
        self.embed = _Layer((mc.dim, n_mels, 7), mc.dim, 7 * n_mels)
        self.norm = _Norm(mc.dim)
        self.convnext = nn.ModuleList([_ConvNeXtBlock(mc.dim, mc.intermediate_dim, mc.layer_scale) for _ in range(mc.num_layers)])
        self.final_layer_norm = _Norm(mc.dim)


class _Head(nn.Module):
    def __init__(self, mc: VocosConfig) -> None:
        super().__init__()
        self.out = _Layer((mc.n_fft + 2, mc.dim), mc.n_fft + 2, mc.dim)


class VocosGenerator(DeviceGenerator):
    """A row needs 1 frame ("same") or 2 ("center").  ``vocode`` returns [B, T * hop] for both paddings: a row of ``T_b`` frames has
    ``sample_counts(T_b)`` samples in front - ``T_b * hop``, or ``(T_b - 1) * hop`` for "center" - and exact zeros behind them.
    ``stage_outputs`` are x after embed + norm, after every block and after the final norm, [B, T, dim] each, then the head product
    [B, T, n_fft + 2].  The workspace is 18,840 bytes per frame and row for the default model with 100 mels."""
    model_name = "vocos"
    _abi, _config_class = "gvx_vocos", VocosConfig
    _range_hint = ""

    def __init__(self, model_config: VocosConfig, audio_config: AudioConfig, trainable: bool = False) -> None:
        super().__init__(model_config, audio_config)
        self.backbone = _Backbone(model_config, int(audio_config.n_mels))
        self.head = _Head(model_config)
        self.trainable = bool(trainable)   # opt-in: vocode_with_grad builds an autograd node only when this is set

    @property
    def _min_frames(self) -> int:
        return 2 if self.model_config.padding == "center" else 1

    @property
    def _short_tail(self) -> str:
        return f"{self._min_frames} of the frames"

    def dims(self) -> _lib.gvx_vocos_dims:
        return dims_from_config(self.model_config, self.audio_config)

    def _stage_tensor_shapes(self, T: int):
        mc = self.model_config
        return [(T, mc.dim)] * (mc.num_layers + 2) + [(T, mc.n_fft + 2)]

    def sample_counts(self, frame_lengths):
        if self.model_config.padding != "center":
            return super().sample_counts(frame_lengths)
        if isinstance(frame_lengths, torch.Tensor):
            return (frame_lengths - 1).clamp(min=0) * self.hop
        if isinstance(frame_lengths, int):
            return max(frame_lengths - 1, 0) * self.hop
        return [max(int(t) - 1, 0) * self.hop for t in frame_lengths]

    def stage_times_ms(self):
        """Durations of the last call's parts: embed + norm, the blocks, final norm + head product, the ISTFT (synchronises)."""
        return self._times_ms("stage_times_ms", 4)

    def _pack_items(self, held=None):
        """The tensors under the packer's names and in its layouts: ``embed.weight`` [dim][7][n_mels padded to a multiple of 4],
        ``dwconv.weight`` tap-major [7][dim], and ``pwconv2`` with ``gamma`` folded in, in float64."""
        state = {k: v.detach() for k, v in self.state_dict().items()}
        n_mels = int(self.audio_config.n_mels)
        items = []
        w = state["backbone.embed.weight"].permute(0, 2, 1)                      # [dim, 7, n_mels]
        items.append(("embed.weight", nn.functional.pad(w, (0, -n_mels % 4))))
        items.append(("embed.bias", state["backbone.embed.bias"]))
        for part in ("weight", "bias"):
            items.append((f"norm.{part}", state[f"backbone.norm.{part}"]))
        for i in range(self.model_config.num_layers):
            src, dst = f"backbone.convnext.{i}.", f"convnext.{i}."
            gamma = state[src + "gamma"].double()
            items.append((dst + "dwconv.weight", state[src + "dwconv.weight"].reshape(-1, 7).t()))
            for name in ("dwconv.bias", "norm.weight", "norm.bias", "pwconv1.weight", "pwconv1.bias"):
                items.append((dst + name, state[src + name]))
            items.append((dst + "pwconv2.weight", (gamma[:, None] * state[src + "pwconv2.weight"].double()).float()))
            items.append((dst + "pwconv2.bias", (gamma * state[src + "pwconv2.bias"].double()).float()))
        for part in ("weight", "bias"):
            items.append((f"final_layer_norm.{part}", state[f"backbone.final_layer_norm.{part}"]))
            items.append((f"head.{part}", state[f"head.out.{part}"]))
        return items

    def _convert_state_dict(self, state_dict) -> Dict[str, torch.Tensor]:
        """A published state dict -> this module's keys: ``head.istft.window`` is compared with the computed Hann window and dropped (a
        mismatch beyond 1e-6 is a ValueError that names the key), ``feature_extractor.*`` is dropped, and the EnCodec variant's
        conditioned norms (``...norm.scale.*`` / ``.shift.*``) are refused by name."""
        out = {}
        for k, v in state_dict.items():
            if _ADA_KEY.search(k + "."):
                raise ValueError(f"{k}: the conditioned AdaLayerNorm of the EnCodec variant is not supported, only the mel variant's LayerNorm")
            if k == _WINDOW_KEY:
                got = v.detach().double().cpu().reshape(-1)
                want = hann_window(self.model_config.n_fft)
                if got.numel() != want.numel() or not bool(((got - want).abs() <= 1e-6).all()):
                    raise ValueError(f"{k}: the checkpoint's window is not the periodic Hann window of {self.model_config.n_fft} points this model computes")
                continue
            if k.startswith("feature_extractor."):
                continue
            out[k] = v
        return out

    def _forward_train_scratch(self, B: int, T: int, dev: torch.device):
        return self._scratch("_workspace", self.workspace_bytes(B, T), dev)

    def _backward_extra(self, params):
        """The raw ``gamma``, ``pwconv2.weight`` and ``pwconv2.bias`` of every block: the blob holds only their product."""
        wanted = re.compile(r"\.convnext\.\d+\.(gamma|pwconv2\.weight|pwconv2\.bias)$")
        return _weight_table((k, p) for (k, _), p in zip(self.named_parameters(), params) if wanted.search(k))

    def vocode_with_grad(self, mel: torch.Tensor, mel_lengths=None) -> torch.Tensor:
        """``trainable=True``: ``DeviceGenerator.vocode_with_grad`` - the waveform with ``vocode``'s bits, whose ``backward()`` fills
        ``.grad`` of every parameter (``gamma`` and ``pwconv2`` unfolded) and of ``mel`` on the device's own kernels.  ``trainable=False``
        (the default): ``vocode`` when gradients are off or nothing requires one; otherwise NotImplementedError."""
        if self.trainable:
            return super().vocode_with_grad(mel, mel_lengths)
        if torch.is_grad_enabled() and (mel.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError("this VocosGenerator was built without its backward: vocode_with_grad runs only under torch.no_grad() or "
                                      "when neither the mel nor a parameter requires a gradient. Construct it with trainable=True, or set "
                                      "model.trainable = True, to train it on the device")
        return self.vocode(mel, mel_lengths)

    def load_checkpoint_statedicts(self, statedicts: Dict, save_optimizer_dict: bool = False, optimizer: Optional[Dict] = None) -> None:
        """Our own ``{"model_statedict": ...}`` or a plain published state dict (its keys start with ``backbone.`` / ``head.``)."""
        if "model_statedict" in statedicts:
            self.load_state_dict(statedicts["model_statedict"])
        elif any(k.startswith("backbone.") for k in statedicts):
            self.load_state_dict(statedicts)
        else:
            raise KeyError("a Vocos checkpoint holds its weights under 'model_statedict' or is the published state dict itself")
