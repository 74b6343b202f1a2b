"""MelGAN generator: mel -> waveform on the MI355X (include/genvox_amd.h, "Neural vocoder"; kernels in csrc/melgan.hip).

The module holds the parameters in PyTorch's own layouts - ``Conv1d`` as [out, in, k], ``ConvTranspose1d`` as [in, out, k] - under the
names the C ABI's packer reads (``pre``, ``ups.<i>``, ``res.<i>.<j>.conv / .shortcut / .mix``, ``post``); the kernels read a packed
blob that is rebuilt on the device whenever the parameters change.  There is no CPU or eager path."""
from __future__ import annotations

import ctypes as C
import re
from typing import Dict, List, Optional

import torch
from torch import nn

from . import _lib
from .configs import AudioConfig, BaseConfig, MelGANConfig

MIN_FRAMES = 4   # GVX_MELGAN_MIN_FRAMES: the first convolution reflects 3 frames


def dims_from_config(mc: MelGANConfig, ac: AudioConfig) -> _lib.gvx_melgan_dims:
    ratios = (C.c_int32 * 8)(*mc.upsample_ratios)
    return _lib.gvx_melgan_dims(ac.n_mels, mc.base_channels, len(mc.upsample_ratios), ratios, mc.n_residual_layers, mc.dilation_base,
                                float(mc.leaky_slope))


class _Layer(nn.Module):
    """One layer's parameters; the weight starts as N(0, 1 / fan_in), the bias at 0."""

    def __init__(self, shape, n_out: int, fan_in: int) -> None:
        super().__init__()
        self.weight = nn.Parameter(torch.randn(*shape) * fan_in ** -0.5)
        self.bias = nn.Parameter(torch.zeros(n_out))


class _ResidualLayer(nn.Module):
    def __init__(self, channels: int) -> None:
        super().__init__()
        self.conv = _Layer((channels, channels, 3), channels, 3 * channels)
        self.shortcut = _Layer((channels, channels, 1), channels, channels)
        self.mix = _Layer((channels, channels, 1), channels, channels)


_WN_OLD = re.compile(r"^(.*)\.weight_(g|v)$")
_WN_NEW = re.compile(r"^(.*)\.parametrizations\.weight\.original(0|1)$")


def fold_weight_norm(state_dict) -> Dict[str, torch.Tensor]:
    """A state dict whose layers may carry weight normalisation -> plain weights, as ``torch.nn.utils.remove_weight_norm`` folds them:
    ``w = v * (g / ||v||)`` with the norm over all axes but the first.  Both spellings are read: ``X.weight_g`` / ``X.weight_v`` and
    ``X.parametrizations.weight.original0`` (g) / ``original1`` (v).  Every other entry passes through."""
    out, parts = {}, {}
    for key, val in state_dict.items():
        m = _WN_OLD.match(key)
        if m:
            parts.setdefault(m.group(1), {})[m.group(2)] = val
            continue
        m = _WN_NEW.match(key)
        if m:
            parts.setdefault(m.group(1), {})["g" if m.group(2) == "0" else "v"] = val
            continue
        out[key] = val
    for name, gv in parts.items():
        if set(gv) != {"g", "v"}:
            raise KeyError(f"{name}: a weight-normalised layer needs both its g and its v")
        g, v = gv["g"], gv["v"]
        norm = torch.linalg.vector_norm(v.reshape(v.shape[0], -1), dim=1).reshape(-1, *([1] * (v.dim() - 1)))
        out[f"{name}.weight"] = v * (g / norm)
    return out


class _VocodeWithGrad(torch.autograd.Function):
    """gvx_<model_name>_forward_train / gvx_<model_name>_backward as one autograd node, for the generators whose C ABI has that pair
    (MelGAN, HiFi-GAN).  The inputs after ``lens_dev`` are the model's parameters in ``named_parameters()`` order; they go through
    ``save_for_backward``, so an in-place change between forward and backward raises torch's own version error, and the tape is a
    tensor the node keeps."""

    @staticmethod
    def forward(ctx, model, mel, lens_dev, *params):
        lib, dims = _lib.load(), model.dims()
        h = model._ensure_packed()
        B, _, T = mel.shape
        dev = mel.device
        wav = torch.empty(B, T * model.hop, dtype=torch.float32, device=dev)
        abi = "gvx_" + model.model_name
        tape = torch.empty(getattr(lib, abi + "_tape_bytes")(C.byref(dims), B, T), dtype=torch.uint8, device=dev)
        _lib.check(getattr(lib, abi + "_forward_train")(h, mel.data_ptr(), lens_dev.data_ptr() if lens_dev is not None else None, B, T, wav.data_ptr(),
                                                tape.data_ptr(), tape.numel(), None, 0, model._stream()))
        ctx.model, ctx.lens_dev, ctx.shape, ctx.tape, ctx.packed_key = model, lens_dev, (B, T), tape, model._packed_key
        ctx.save_for_backward(*params)
        return wav

    @staticmethod
    def backward(ctx, d_wav):
        params = ctx.saved_tensors   # raises if a parameter was changed in place since the forward
        model, (B, T) = ctx.model, ctx.shape
        lib, dims = _lib.load(), model.dims()
        if model._packed_key != ctx.packed_key:
            raise RuntimeError("the generator's weights were packed again between this forward and its backward")
        dev = d_wav.device
        d_wav = d_wav.to(torch.float32).contiguous()
        names = [k for k, _ in model.named_parameters()]
        grads = [torch.empty_like(p, dtype=torch.float32, memory_format=torch.contiguous_format) for p in params]
        table = (_lib.gvx_weight_desc * len(grads))()
        for i, (k, g) in enumerate(zip(names, grads)):
            table[i] = _lib.gvx_weight_desc(k.encode(), g.data_ptr(), g.numel())
        d_mel = torch.empty(B, model.audio_config.n_mels, T, dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        abi = "gvx_" + model.model_name
        need = getattr(lib, abi + "_backward_workspace_bytes")(C.byref(dims), B, T)
        if model._train_workspace is None or model._train_workspace.numel() < need or model._train_workspace.device != dev:
            model._train_workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        ws = model._train_workspace
        _lib.check(getattr(lib, abi + "_backward")(model._handle, d_wav.data_ptr(), ctx.lens_dev.data_ptr() if ctx.lens_dev is not None else None, B, T,
                                           ctx.tape.data_ptr(), ctx.tape.numel(), table, len(grads), d_mel.data_ptr() if d_mel is not None else None,
                                           ws.data_ptr(), ws.numel(), model._stream()))
        return (None, d_mel, None, *grads)


class MelGANGenerator(nn.Module):
    model_name = "melgan"
    WORKSPACE_CAP_BYTES = 1 << 30   # a call whose workspace would pass this is split by rows (98,624 bytes per frame and row with the defaults)

    def __init__(self, model_config: MelGANConfig, audio_config: AudioConfig) -> None:
        super().__init__()
        model_config.check_hop(audio_config.hop_length)
        self.model_config, self.audio_config = model_config, audio_config
        c = model_config.base_channels
        self.pre = _Layer((c, audio_config.n_mels, 7), c, 7 * audio_config.n_mels)
        self.ups, self.res = nn.ModuleList(), nn.ModuleList()
        for r in model_config.upsample_ratios:
            self.ups.append(_Layer((c, c // 2, 2 * r), c // 2, 2 * c))   # ConvTranspose1d: [in, out, k]; two taps of c inputs reach an output
            c //= 2
            self.res.append(nn.ModuleList([_ResidualLayer(c) for _ in range(model_config.n_residual_layers)]))
        self.post = _Layer((1, c, 7), 1, 7 * c)
        self._handle: Optional[int] = None
        self._blob: Optional[torch.Tensor] = None
        self._packed_key = None
        self._workspace: Optional[torch.Tensor] = None
        self._train_workspace: Optional[torch.Tensor] = None   # the backward's scratch (vocode_with_grad)
        self._timing = False

    # ------------------------------------------------------------------ C-ABI plumbing
    def __del__(self):
        try:
            if self._handle is not None:
                _lib.load().gvx_melgan_destroy(self._handle)
        except Exception:
            pass

    @property
    def hop(self) -> int:
        return self.model_config.hop

    def dims(self) -> _lib.gvx_melgan_dims:
        return dims_from_config(self.model_config, self.audio_config)

    def blob_numel(self) -> int:
        return _lib.load().gvx_melgan_blob_floats(C.byref(self.dims()))

    def workspace_bytes(self, B: int, T: int) -> int:
        return _lib.load().gvx_melgan_workspace_bytes(C.byref(self.dims()), B, T)

    def _device(self) -> torch.device:
        return self.pre.weight.device

    def _require_gpu(self) -> torch.device:
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError("genvox_amd.MelGANGenerator runs on an MI355X only: move the model with .to('cuda:0'). There is no CPU fallback.")
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
            _lib.check(lib.gvx_melgan_create(C.byref(dims), C.byref(h)))
            self._handle = h.value
        key = self._weights_key()
        if self._packed_key != key:
            srcs = {k: v.detach().to(device=dev, dtype=torch.float32).contiguous() for k, v in self.state_dict().items()}
            table = (_lib.gvx_weight_desc * len(srcs))()
            for i, (k, v) in enumerate(srcs.items()):
                table[i] = _lib.gvx_weight_desc(k.encode(), v.data_ptr(), v.numel())
            blob = torch.empty(self.blob_numel(), dtype=torch.float32, device=dev)
            _lib.check(lib.gvx_melgan_pack_weights_device(C.byref(dims), table, len(srcs), blob.data_ptr(), self._stream()))
            _lib.check(lib.gvx_melgan_bind(self._handle, blob.data_ptr()))
            self._blob, self._packed_key = blob, key
        return self._handle

    def enable_stage_timing(self, enable: bool = True) -> None:
        _lib.check(_lib.load().gvx_melgan_timing_enable(self._ensure_packed(), int(enable)))

    def stage_times_ms(self) -> List[float]:
        """Durations of the last call's parts: first convolution, every stage, output layer (synchronises)."""
        out, n = (C.c_float * 10)(), C.c_int()
        _lib.check(_lib.load().gvx_melgan_stage_times_ms(self._ensure_packed(), out, C.byref(n)))
        return [out[i] for i in range(n.value)]

    # ------------------------------------------------------------------ the call
    def _check_call(self, mel: torch.Tensor, mel_lengths):
        """The argument checks of ``vocode`` and ``vocode_with_grad`` -> (device, B, T, the lengths as int32 on the device or None)."""
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
                if not MIN_FRAMES <= t <= T:
                    raise ValueError(f"row {b}: {t} frames are outside [{MIN_FRAMES}, {T}] (the first convolution reflects 3 frames)")
            lens_dev = (mel_lengths if isinstance(mel_lengths, torch.Tensor) else torch.tensor(host)).to(dev, torch.int32).contiguous()
        if B < 1 or T < MIN_FRAMES:
            raise ValueError(f"a mel of {B} rows and {T} frames: every row needs at least {MIN_FRAMES} frames (the first convolution reflects 3)")
        return dev, B, T, lens_dev

    def vocode(self, mel: torch.Tensor, mel_lengths=None, stage_outputs: bool = False, workspace: Optional[torch.Tensor] = None):
        """mel float32 [B, n_mels, T] on the device (the model's own dB scale, as ``mel_outputs_postnet``) -> waveform float32
        [B, T * hop].  ``mel_lengths`` ([B], host or device): every row at its own frames - bit for bit that row run alone - and
        exact zeros behind ``T_b * hop`` samples; the padded frames of ``mel`` may hold anything.  A row below 4 frames raises
        ValueError before anything is launched.  A batch whose workspace would pass ``WORKSPACE_CAP_BYTES`` is run in groups of rows;
        rows do not depend on each other, so the split changes no bit.  ``stage_outputs``: also the list of x after every stage,
        [B, len_i, C_i] channels-last (tests).  ``workspace``: a uint8 tensor to use as it is, of at least ``workspace_bytes(B, T)``
        (tests of the workspace contract; no row split then)."""
        dev, B, T, lens_dev = self._check_call(mel, mel_lengths)
        h = self._ensure_packed()
        lib = _lib.load()
        mel = mel.contiguous()
        wav = torch.empty(B, T * self.hop, dtype=torch.float32, device=dev)
        stages = None
        if stage_outputs:
            stages, mul, c = [], 1, self.model_config.base_channels
            for r in self.model_config.upsample_ratios:
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
            _lib.check(lib.gvx_melgan_forward(h, mel[lo:lo + n].data_ptr(), lens_dev[lo:lo + n].data_ptr() if lens_dev is not None else None, n, T,
                                              wav[lo:lo + n].data_ptr(), ptrs, workspace.data_ptr(), workspace.numel(), self._stream()))
        return (wav, stages) if stage_outputs else wav

    def vocode_with_grad(self, mel: torch.Tensor, mel_lengths=None) -> torch.Tensor:
        """``vocode`` attached to autograd: mel float32 [B, n_mels, T] on the device -> waveform float32 [B, T * hop] whose
        ``backward()`` fills ``.grad`` of every parameter of the generator - and of ``mel`` if ``mel.requires_grad`` - on the device's
        own kernels (gvx_melgan_forward_train / gvx_melgan_backward, csrc/melgan_train.hip), so a plain torch loop with any loss
        written in torch and any torch optimizer trains or fine-tunes the vocoder.  The waveform has ``vocode``'s bits; under
        ``torch.no_grad()`` (or when nothing requires a gradient) the call IS ``vocode``.  Rows are ragged as in ``vocode``; gradient
        that arrives behind ``T_b * hop`` samples is never read, and ``mel.grad`` is 0 at and behind a row's frames.  The call keeps a
        tape of every layer's pre-activations (747,840 bytes per frame and row with the defaults) until its backward has run; a
        parameter changed in place between the two raises torch's version error.  Two backward calls give the same bits.

        Training is on plain weights: a weight-normalised checkpoint is folded when it is loaded and stays folded, and the module
        has no weight-norm parametrisation of its own."""
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
        self.load_state_dict(statedicts["model_statedict"])

    @staticmethod
    def load_from_config(config_path: str) -> "MelGANGenerator":
        configs = BaseConfig.load_configs_from_file(path=config_path, config_map={"audio_config": AudioConfig, "model_config": MelGANConfig})
        return MelGANGenerator(**configs)
