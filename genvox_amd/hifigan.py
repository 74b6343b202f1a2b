"""HiFi-GAN generator: mel -> waveform on the MI355X (include/genvox_amd.h, "HiFi-GAN generator"; kernels in csrc/hifigan.hip).

The module holds the parameters in PyTorch's own layouts - ``Conv1d`` as [out, in, k], ``ConvTranspose1d`` as [in, out, k] - under the
published implementation's names (``conv_pre``, ``ups.<i>``, ``resblocks.<n>.convs1.<m>`` / ``.convs2.<m>`` or ``.convs.<m>``,
``conv_post``), so a published V1, V2 or V3 generator checkpoint loads as it is; weight normalisation is folded on load.  The kernels
read a packed blob that is rebuilt on the device whenever the parameters change.  ``vocode`` is inference; ``vocode_with_grad`` is the
same call attached to autograd, for training or fine-tuning the generator.  There is no CPU or eager path.

The model vocodes whatever mel scale its checkpoint was trained on.  A checkpoint trained on the published recipe's natural-log mels
is NOT matched to this package's Tacotron2 mels (log10, dB-scaled: ``AudioProcessor``), and no conversion is part of this module: pair
the Tacotron2 with a HiFi-GAN trained on its own mels."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import torch
from torch import nn

from . import _lib
from .configs import AudioConfig, BaseConfig, HiFiGANConfig
from .melgan import _Layer, _VocodeWithGrad, fold_weight_norm


def dims_from_config(mc: HiFiGANConfig, ac: AudioConfig) -> _lib.gvx_hifigan_dims:
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


class HiFiGANGenerator(nn.Module):
    model_name = "hifigan"
    WORKSPACE_CAP_BYTES = 1 << 30   # a call whose workspace would pass this is split by rows (131,392 bytes per frame and row for V1)

    def __init__(self, model_config: HiFiGANConfig, audio_config: AudioConfig) -> None:
        super().__init__()
        model_config.check_hop(audio_config.hop_length)
        self.model_config, self.audio_config = model_config, audio_config
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
        self._handle: Optional[int] = None
        self._blob: Optional[torch.Tensor] = None
        self._packed_key = None
        self._workspace: Optional[torch.Tensor] = None
        self._train_workspace: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------ C-ABI plumbing
    def __del__(self):
        try:
            if self._handle is not None:
                _lib.load().gvx_hifigan_destroy(self._handle)
        except Exception:
            pass

    @property
    def hop(self) -> int:
        return self.model_config.hop

    def dims(self) -> _lib.gvx_hifigan_dims:
        return dims_from_config(self.model_config, self.audio_config)

    def blob_numel(self) -> int:
        return _lib.load().gvx_hifigan_blob_floats(C.byref(self.dims()))

    def workspace_bytes(self, B: int, T: int) -> int:
        return _lib.load().gvx_hifigan_workspace_bytes(C.byref(self.dims()), B, T)

    def _device(self) -> torch.device:
        return self.conv_pre.weight.device

    def _require_gpu(self) -> torch.device:
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError("genvox_amd.HiFiGANGenerator runs on an MI355X only: move the model with .to('cuda:0'). There is no CPU fallback.")
        return dev

    def _stream(self) -> int:
        return torch.cuda.current_stream(self._device()).cuda_stream

    def _weights_key(self):
        return (str(self._device()),) + tuple((p.data_ptr(), p._version) for p in self.parameters())

    def _ensure_packed(self) -> int:
        dev = self._require_gpu()
        lib = _lib.load()
        dims = self.dims()
        if self._handle is None:
            h = C.c_void_p()
            _lib.check(lib.gvx_hifigan_create(C.byref(dims), C.byref(h)))
            self._handle = h.value
        key = self._weights_key()
        if self._packed_key != key:
            srcs = {k: v.detach().to(device=dev, dtype=torch.float32).contiguous() for k, v in self.state_dict().items()}
            table = (_lib.gvx_weight_desc * len(srcs))()
            for i, (k, v) in enumerate(srcs.items()):
                table[i] = _lib.gvx_weight_desc(k.encode(), v.data_ptr(), v.numel())
            blob = torch.empty(self.blob_numel(), dtype=torch.float32, device=dev)
            _lib.check(lib.gvx_hifigan_pack_weights_device(C.byref(dims), table, len(srcs), blob.data_ptr(), self._stream()))
            _lib.check(lib.gvx_hifigan_bind(self._handle, blob.data_ptr()))
            self._blob, self._packed_key = blob, key
        return self._handle

    def enable_stage_timing(self, enable: bool = True) -> None:
        _lib.check(_lib.load().gvx_hifigan_timing_enable(self._ensure_packed(), int(enable)))

    def stage_times_ms(self) -> List[float]:
        """Durations of the last call's parts: conv_pre, every stage, conv_post (synchronises)."""
        out, n = (C.c_float * 10)(), C.c_int()
        _lib.check(_lib.load().gvx_hifigan_stage_times_ms(self._ensure_packed(), out, C.byref(n)))
        return [out[i] for i in range(n.value)]

    def backward_stage_times_ms(self) -> List[float]:
        """Durations of the last ``vocode_with_grad`` backward's parts, in the order they ran: the weight transposes, conv_post,
        every stage from the last to the first, conv_pre (synchronises)."""
        out, n = (C.c_float * 12)(), C.c_int()
        _lib.check(_lib.load().gvx_hifigan_backward_stage_times_ms(self._ensure_packed(), out, C.byref(n)))
        return [out[i] for i in range(n.value)]

    # ------------------------------------------------------------------ the call
    def _check_call(self, mel: torch.Tensor, mel_lengths):
        """The argument checks of ``vocode`` -> (device, B, T, the lengths as int32 on the device or None)."""
        dev = self._require_gpu()
        if mel.dim() != 3 or mel.shape[1] != self.audio_config.n_mels:
            raise ValueError(f"mel must be [B, {self.audio_config.n_mels}, T], got {tuple(mel.shape)}")
        if mel.device != dev or mel.dtype != torch.float32:
            raise ValueError(f"mel must be float32 on {dev}, got {mel.dtype} on {mel.device}")
        B, _, T = mel.shape
        lens_dev = None
        if mel_lengths is not None:
            host = [int(v) for v in (mel_lengths.tolist() if isinstance(mel_lengths, torch.Tensor) else mel_lengths)]
            if len(host) != B:
                raise ValueError(f"{len(host)} lengths for {B} rows")
            for b, t in enumerate(host):
                if not 1 <= t <= T:
                    raise ValueError(f"row {b}: {t} frames are outside [1, {T}]")
            lens_dev = (mel_lengths if isinstance(mel_lengths, torch.Tensor) else torch.tensor(host)).to(dev, torch.int32).contiguous()
        if B < 1 or T < 1:
            raise ValueError(f"a mel of {B} rows and {T} frames: every row needs at least 1 of the frames")
        return dev, B, T, lens_dev

    def vocode(self, mel: torch.Tensor, mel_lengths=None, stage_outputs: bool = False, workspace: Optional[torch.Tensor] = None):
        """mel float32 [B, n_mels, T] on the device, on the mel scale the checkpoint was trained on (see the module's docstring: a
        published natural-log checkpoint is not matched to this package's Tacotron2 mels) -> waveform float32 [B, T * hop].
        ``mel_lengths`` ([B], host or device): every row at its own frames - bit for bit that row run alone - and exact zeros behind
        ``T_b * hop`` samples; the padded frames of ``mel`` may hold anything.  A row outside [1, T] frames raises ValueError before
        anything is launched.  A batch whose workspace would pass ``WORKSPACE_CAP_BYTES`` is run in groups of rows; rows do not
        depend on each other, so the split changes no bit.  ``stage_outputs``: also the list of x after every stage's average,
        [B, len_i, C_i] channels-last (tests).  ``workspace``: a uint8 tensor to use as it is, of at least ``workspace_bytes(B, T)``
        (tests of the workspace contract; no row split then)."""
        dev, B, T, lens_dev = self._check_call(mel, mel_lengths)
        h = self._ensure_packed()
        lib = _lib.load()
        mel = mel.contiguous()
        wav = torch.empty(B, T * self.hop, dtype=torch.float32, device=dev)
        stages = None
        if stage_outputs:
            stages, mul, c = [], 1, self.model_config.upsample_initial_channel
            for r in self.model_config.upsample_rates:
                mul, c = mul * r, c // 2
                stages.append(torch.empty(B, T * mul, c, dtype=torch.float32, device=dev))
        rows = B
        if workspace is None:
            while rows > 1 and self.workspace_bytes(rows, T) > self.WORKSPACE_CAP_BYTES:
                rows = (rows + 1) // 2
            need = self.workspace_bytes(rows, T)
            if self._workspace is None or self._workspace.numel() < need or self._workspace.device != dev:
                self._workspace = torch.empty(need, dtype=torch.uint8, device=dev)
            workspace = self._workspace
        for lo in range(0, B, rows):
            n = min(rows, B - lo)
            ptrs = None
            if stages is not None:
                ptrs = (C.c_void_p * len(stages))(*[s[lo:lo + n].data_ptr() for s in stages])
            _lib.check(lib.gvx_hifigan_forward(h, mel[lo:lo + n].data_ptr(), lens_dev[lo:lo + n].data_ptr() if lens_dev is not None else None, n, T,
                                               wav[lo:lo + n].data_ptr(), ptrs, workspace.data_ptr(), workspace.numel(), self._stream()))
        return (wav, stages) if stage_outputs else wav

    def vocode_with_grad(self, mel: torch.Tensor, mel_lengths=None) -> torch.Tensor:
        """``vocode`` attached to autograd: mel float32 [B, n_mels, T] on the device -> waveform float32 [B, T * hop] whose
        ``backward()`` fills ``.grad`` of every parameter of the generator - and of ``mel`` if ``mel.requires_grad`` - on the device's
        own kernels (gvx_hifigan_forward_train / gvx_hifigan_backward, csrc/hifigan_train.hip), so a plain torch loop with any loss
        written in torch (``MultiResolutionSTFTLoss``, a discriminator) and any torch optimizer trains or fine-tunes the vocoder.  The
        waveform has ``vocode``'s bits; under ``torch.no_grad()`` (or when nothing requires a gradient) the call IS ``vocode``.  Rows
        are ragged as in ``vocode``; gradient that arrives behind ``T_b * hop`` samples is never read, and ``mel.grad`` is 0 at and
        behind a row's frames.  The call keeps a tape of every layer's pre-activations (1,812,800 bytes per frame and row for V1,
        453,440 for V2, 267,584 for V3) until its backward has run; a parameter changed in place between the two raises torch's version
        error, and packing the weights again between the two raises RuntimeError.  Two backward calls give the same bits.

        Training is on plain weights: a weight-normalised checkpoint is folded when it is loaded and stays folded, and the module
        has no weight-norm parametrisation of its own.  Parameters must be contiguous float32."""
        if not torch.is_grad_enabled() or not (mel.requires_grad or any(p.requires_grad for p in self.parameters())):
            return self.vocode(mel, mel_lengths)
        _, _, _, lens_dev = self._check_call(mel, mel_lengths)
        for k, p in self.named_parameters():
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError(f"{k}: training needs contiguous float32 parameters")
        return _VocodeWithGrad.apply(self, mel.contiguous(), lens_dev, *self.parameters())

    def inference(self, inputs: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """{"mel": [B, n_mels, T], "mel_lengths": optional [B]} -> {"waveform": float32 [B, T * hop] on the device, "lengths": int32 [B]
        sample counts}."""
        mel, lens = inputs["mel"], inputs.get("mel_lengths")
        wav = self.vocode(mel, lens)
        if lens is None:
            lengths = torch.full((mel.shape[0],), mel.shape[2] * self.hop, dtype=torch.int32, device=wav.device)
        else:
            lengths = torch.as_tensor(lens).to(wav.device, torch.int32) * self.hop
        return {"waveform": wav, "lengths": lengths}

    def forward(self, inputs: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        return self.inference(inputs)

    # ------------------------------------------------------------------ checkpoints and configs
    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        out = super().load_state_dict(fold_weight_norm(state_dict), strict=strict, assign=assign)
        self._packed_key = None
        return out

    def get_checkpoint_statedicts(self, optimizer: Optional[Dict] = None) -> Dict:
        return {"model_statedict": self.state_dict()}

    def load_checkpoint_statedicts(self, statedicts: Dict, save_optimizer_dict: bool = False, optimizer: Optional[Dict] = None) -> None:
        """Our own ``{"model_statedict": ...}`` or the published generator file's ``{"generator": ...}`` (weight-normalised)."""
        if "model_statedict" in statedicts:
            self.load_state_dict(statedicts["model_statedict"])
        elif "generator" in statedicts:
            self.load_state_dict(statedicts["generator"])
        else:
            raise KeyError("a HiFi-GAN checkpoint holds its weights under 'model_statedict' or, in the published form, under 'generator'")

    @staticmethod
    def load_from_config(config_path: str) -> "HiFiGANGenerator":
        configs = BaseConfig.load_configs_from_file(path=config_path, config_map={"audio_config": AudioConfig, "model_config": HiFiGANConfig})
        return HiFiGANGenerator(**configs)
