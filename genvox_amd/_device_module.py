"""What the vocoder modules share in front of their C ABIs (include/genvox_amd.h): ``DeviceModule`` - handle, packed blob, scratch,
argument checks, checkpoints - and on it ``DeviceGenerator`` (mel -> waveform, with ``_VocodeWithGrad``) and ``DeviceDiscriminator``
(waveform -> feature maps, with ``_DiscriminatorNode``).  A module states its ABI prefix (``_abi``: its calls are
``<_abi>_create``, ``<_abi>_forward``, ...) and its ``dims()``, and fills in the hooks its base names.  DESIGN.md, "The Python
surface of the vocoder modules"."""
from __future__ import annotations

import ctypes as C
import math
import re
from typing import Dict, List, Optional

import torch
from torch import nn

from . import _lib
from .configs import AudioConfig, BaseConfig


class _Layer(nn.Module):
    """One layer's parameters; the weight starts as N(0, 1 / fan_in), the bias at 0."""

    def __init__(self, shape, n_out: int, fan_in: int) -> None:
        super().__init__()
        self.weight = nn.Parameter(torch.randn(*shape) * fan_in ** -0.5)
        self.bias = nn.Parameter(torch.zeros(n_out))


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


def _weight_table(named):
    """(name, tensor) pairs -> the C ABI's table of ``gvx_weight_desc`` and its length.  The caller keeps the tensors alive."""
    named = list(named)
    table = (_lib.gvx_weight_desc * len(named))()
    for i, (k, v) in enumerate(named):
        table[i] = _lib.gvx_weight_desc(k.encode(), v.data_ptr(), v.numel())
    return table, len(named)


def _ptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


class DeviceModule(nn.Module):
    """A module whose kernels read a packed blob of its weights through a handle of the C ABI ``_abi``.  The blob is rebuilt on the
    device whenever a parameter or a buffer changes.  A subclass sets ``_abi`` and ``dims()``; ``_pack_items`` and
    ``_convert_state_dict`` are the hooks it may replace."""
    _abi: str

    def __init__(self) -> None:
        super().__init__()
        self._handle: Optional[int] = None
        self._blob: Optional[torch.Tensor] = None
        self._packed_key = None
        self._workspace: Optional[torch.Tensor] = None
        self._train_workspace: Optional[torch.Tensor] = None   # the backward's scratch

    def __del__(self):
        try:
            if self._handle is not None:
                self._c("destroy")(self._handle)
        except Exception:
            pass

    # ------------------------------------------------------------------ C-ABI plumbing
    def _c(self, name: str):
        """The C ABI's call ``<_abi>_<name>``; a call the ABI does not have is an AttributeError."""
        return getattr(_lib.load(), f"{self._abi}_{name}")

    def dims(self):
        raise NotImplementedError

    def _device(self) -> torch.device:
        return next(self.parameters()).device

    def _require_gpu(self) -> torch.device:
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError(f"genvox_amd.{type(self).__name__} runs on an MI355X only: move the model with .to('cuda:0'). There is no CPU fallback.")
        return dev

    def _stream(self, dev: Optional[torch.device] = None) -> int:
        """The current stream of ``dev``, the module's device for a caller that has already asked for it."""
        return torch.cuda.current_stream(dev if dev is not None else self._device()).cuda_stream

    def _weights_key(self):
        """Where every parameter and buffer lies and at which version.  One walk over the modules' own tables, module by module in
        ``parameters()``'s order: ``parameters()`` and ``buffers()`` would each walk the tree and name every tensor on the way, and
        this runs in front of every call."""
        tensors = [t for m in self.modules() for table in (m._parameters, m._buffers) for t in table.values() if t is not None]
        return (str(tensors[0].device),) + tuple((t.data_ptr(), t._version) for t in tensors)

    def _pack_items(self, held=None):
        """The (name, tensor) pairs the packer reads.  ``held`` is what the caller gave ``_ensure_packed``: the tensors it already
        holds, for a module whose kernels see something other than its state dict."""
        return self.state_dict().items()

    def _ensure_packed(self, held=None) -> int:
        """-> the handle, with the module's current blob bound.  The weights are packed again - into a NEW blob, an autograd node may
        keep the old one - whenever ``_weights_key()`` has changed."""
        dev = self._require_gpu()
        dims = self.dims()
        if self._handle is None:
            h = C.c_void_p()
            _lib.check(self._c("create")(C.byref(dims), C.byref(h)))
            self._handle = h.value
        key = self._weights_key()
        if self._packed_key != key or self._blob is None:
            srcs = [(k, v.detach().to(device=dev, dtype=torch.float32).contiguous()) for k, v in self._pack_items(held)]
            table, n = _weight_table(srcs)
            blob = torch.empty(self._c("blob_floats")(C.byref(dims)), dtype=torch.float32, device=dev)
            _lib.check(self._c("pack_weights_device")(C.byref(dims), table, n, blob.data_ptr(), self._stream(dev)))
            self._blob, self._packed_key = blob, key
        _lib.check(self._c("bind")(self._handle, self._blob.data_ptr()))
        return self._handle

    def _scratch(self, attr: str, need: int, dev: torch.device) -> torch.Tensor:
        """The scratch buffer kept under ``attr``, grown to ``need`` bytes on ``dev``."""
        buf = getattr(self, attr)
        if buf is None or buf.numel() < need or buf.device != dev:
            buf = torch.empty(need, dtype=torch.uint8, device=dev)
            setattr(self, attr, buf)
        return buf

    # ------------------------------------------------------------------ argument checks
    @staticmethod
    def _host_lengths(lengths) -> List[int]:
        return [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]

    def _ragged_lengths(self, lengths, B: int, lo: int, hi: int, unit: str, hint: str, dev: torch.device) -> Optional[torch.Tensor]:
        """Per-row lengths (host or device, or None) -> int32 [B] on the device, or None; ValueError unless there are ``B`` of them and
        each lies in [lo, hi].  ``unit`` and ``hint`` word the message: "row b: n <unit> are outside [lo, hi]<hint>"."""
        if lengths is None:
            return None
        host = self._host_lengths(lengths)
        if len(host) != B:
            raise ValueError(f"{len(host)} lengths for {B} rows")
        for b, n in enumerate(host):
            if not lo <= n <= hi:
                raise ValueError(f"row {b}: {n} {unit} are outside [{lo}, {hi}]{hint}")
        return (lengths if isinstance(lengths, torch.Tensor) else torch.tensor(host)).to(dev, torch.int32).contiguous()

    def _check_trainable(self) -> None:
        for k, p in self.named_parameters():
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError(f"{k}: training needs contiguous float32 parameters")

    # ------------------------------------------------------------------ checkpoints
    def _convert_state_dict(self, state_dict) -> Dict[str, torch.Tensor]:
        """A checkpoint's state dict -> this module's own keys and plain weights."""
        return fold_weight_norm(state_dict)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        out = super().load_state_dict(self._convert_state_dict(state_dict), strict=strict, assign=assign)
        self._packed_key = None
        return out

    def get_checkpoint_statedicts(self, optimizer: Optional[Dict] = None) -> Dict:
        return {"model_statedict": self.state_dict()}

    def load_checkpoint_statedicts(self, statedicts: Dict, save_optimizer_dict: bool = False, optimizer: Optional[Dict] = None) -> None:
        self.load_state_dict(statedicts["model_statedict"])


# ====================================================================== generators
class _VocodeWithGrad(torch.autograd.Function):
    """<_abi>_forward_train / <_abi>_backward as one autograd node, for the generators.  The inputs after ``lens_dev`` are the model's
    parameters in ``named_parameters()`` order; they go through ``save_for_backward``, so an in-place change between forward and
    backward raises torch's own version error, and the tape is a tensor the node keeps.  The node keeps no blob: a backward after the
    weights were packed again is refused."""

    @staticmethod
    def forward(ctx, model, mel, lens_dev, *params):
        dims = model.dims()
        h = model._ensure_packed()
        B, _, T = mel.shape
        dev = mel.device
        wav = torch.empty(B, T * model.hop, dtype=torch.float32, device=dev)
        tape = torch.empty(model._c("tape_bytes")(C.byref(dims), B, T), dtype=torch.uint8, device=dev)
        scratch = model._forward_train_scratch(B, T, dev)
        _lib.check(model._c("forward_train")(h, mel.data_ptr(), _ptr(lens_dev), B, T, wav.data_ptr(), tape.data_ptr(), tape.numel(), _ptr(scratch),
                                             scratch.numel() if scratch is not None else 0, model._stream(dev)))
        ctx.model, ctx.lens_dev, ctx.shape, ctx.tape, ctx.packed_key = model, lens_dev, (B, T), tape, model._packed_key
        ctx.save_for_backward(*params)
        return wav

    @staticmethod
    def backward(ctx, d_wav):
        params = ctx.saved_tensors   # raises if a parameter was changed in place since the forward
        model, (B, T) = ctx.model, ctx.shape
        dims = model.dims()
        if model._packed_key != ctx.packed_key:
            raise RuntimeError("the generator's weights were packed again between this forward and its backward")
        dev = d_wav.device
        d_wav = d_wav.to(torch.float32).contiguous()
        grads = [torch.empty_like(p, dtype=torch.float32, memory_format=torch.contiguous_format) for p in params]
        table, n = _weight_table(zip((k for k, _ in model.named_parameters()), grads))
        d_mel = torch.empty(B, model.audio_config.n_mels, T, dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        ws = model._scratch("_train_workspace", model._c("backward_workspace_bytes")(C.byref(dims), B, T), dev)
        extra = model._backward_extra(params)
        _lib.check(model._c("backward")(model._handle, d_wav.data_ptr(), _ptr(ctx.lens_dev), B, T, ctx.tape.data_ptr(), ctx.tape.numel(), *extra,
                                        table, n, _ptr(d_mel), ws.data_ptr(), ws.numel(), model._stream(dev)))
        return (None, d_mel, None, *grads)


class DeviceGenerator(DeviceModule):
    """mel -> waveform.  A subclass builds its layers, and states ``_config_class``, ``dims()``, ``_stage_shapes()`` and the least
    frame count of a row with its two messages (``_min_frames``, ``_range_hint``, ``_short_tail``)."""
    WORKSPACE_CAP_BYTES = 1 << 30   # a call whose workspace would pass this is split by rows
    _config_class: type
    _min_frames: int
    _range_hint: str    # behind "row b: t frames are outside [lo, T]"
    _short_tail: str    # behind "every row needs at least "

    def __init__(self, model_config, audio_config: AudioConfig) -> None:
        super().__init__()
        model_config.check_hop(audio_config.hop_length)
        self.model_config, self.audio_config = model_config, audio_config

    def _stage_shapes(self):
        """-> (the channels in front of the first upsampling stage, every stage's rate); a stage halves the channels."""
        raise NotImplementedError

    def _stage_tensor_shapes(self, T: int):
        """-> the (positions, channels) of every ``stage_outputs`` tensor of a call on ``T`` frames, in the C ABI's order.  The default
        is the upsampling generators' arithmetic on ``_stage_shapes()``: a stage multiplies the positions by its rate and halves the
        channels."""
        c, rates = self._stage_shapes()
        shapes, mul = [], 1
        for r in rates:
            mul, c = mul * r, c // 2
            shapes.append((T * mul, c))
        return shapes

    @property
    def hop(self) -> int:
        return self.model_config.hop

    def sample_counts(self, frame_lengths):
        """Frame counts (an int, a list or a tensor) -> the samples a row of that many frames delivers: ``t * hop`` unless the model
        says otherwise."""
        if isinstance(frame_lengths, torch.Tensor):
            return frame_lengths * self.hop
        if isinstance(frame_lengths, int):
            return frame_lengths * self.hop
        return [int(t) * self.hop for t in frame_lengths]

    def blob_numel(self) -> int:
        return self._c("blob_floats")(C.byref(self.dims()))

    def workspace_bytes(self, B: int, T: int) -> int:
        return self._c("workspace_bytes")(C.byref(self.dims()), B, T)

    def enable_stage_timing(self, enable: bool = True) -> None:
        _lib.check(self._c("timing_enable")(self._ensure_packed(), int(enable)))

    def _times_ms(self, call: str, most: int) -> List[float]:
        out, n = (C.c_float * most)(), C.c_int()
        _lib.check(self._c(call)(self._ensure_packed(), out, C.byref(n)))
        return [out[i] for i in range(n.value)]

    def stage_times_ms(self) -> List[float]:
        """Durations of the last call's parts: first convolution, every stage, output layer (synchronises)."""
        return self._times_ms("stage_times_ms", 10)

    # ------------------------------------------------------------------ the call
    def _check_call(self, mel: torch.Tensor, mel_lengths):
        """The argument checks of ``vocode`` and ``vocode_with_grad`` -> (device, B, T, the lengths as int32 on the device or None)."""
        dev = self._require_gpu()
        if mel.dim() != 3 or mel.shape[1] != self.audio_config.n_mels:
            raise ValueError(f"mel must be [B, {self.audio_config.n_mels}, T], got {tuple(mel.shape)}")
        if mel.device != dev or mel.dtype != torch.float32:
            raise ValueError(f"mel must be float32 on {dev}, got {mel.dtype} on {mel.device}")
        B, _, T = mel.shape
        lens_dev = self._ragged_lengths(mel_lengths, B, self._min_frames, T, "frames", self._range_hint, dev)
        if B < 1 or T < self._min_frames:
            raise ValueError(f"a mel of {B} rows and {T} frames: every row needs at least {self._short_tail}")
        return dev, B, T, lens_dev

    def _check_extra(self, extra, dev: torch.device, B: int, T: int):
        """``vocode``'s ``_extra``, checked behind the mel and the lengths -> what ``_forward_extra`` is handed.  The default takes none."""
        return extra

    def _forward_extra(self, extra, lo: int, n: int):
        """The arguments of ``<_abi>_forward`` between ``mel`` and the frame lengths for rows [lo, lo + n) of ``vocode``'s ``_extra``:
        none, unless the model takes a second per-row input (UnivNet's noise)."""
        return ()

    def _forward_train_scratch(self, B: int, T: int, dev: torch.device) -> Optional[torch.Tensor]:
        """The scratch ``<_abi>_forward_train`` needs besides its tape: none, unless the model says otherwise (Vocos)."""
        return None

    def _backward_extra(self, params):
        """The arguments of ``<_abi>_backward`` in front of the gradient table, from the node's saved parameters (``named_parameters()``
        order): none, unless the kernels see something other than the parameters (Vocos folds ``gamma`` into ``pwconv2``)."""
        return ()

    def vocode(self, mel: torch.Tensor, mel_lengths=None, stage_outputs: bool = False, workspace: Optional[torch.Tensor] = None, _extra=None):
        """mel float32 [B, n_mels, T] on the device, on the mel scale the weights were trained on -> waveform float32 [B, T * hop].
        ``mel_lengths`` ([B], host or device): every row at its own frames - bit for bit that row run alone - and exact zeros behind
        ``T_b * hop`` samples; the padded frames of ``mel`` may hold anything.  A row outside [the least frame count, T] raises
        ValueError before anything is launched.  A batch whose workspace would pass ``WORKSPACE_CAP_BYTES`` is run in groups of rows;
        rows do not depend on each other, so the split changes no bit.  ``stage_outputs``: also the list of x after every stage,
        [B, len_i, C_i] channels-last (tests).  ``workspace``: a uint8 tensor to use as it is, of at least ``workspace_bytes(B, T)``
        (tests of the workspace contract; no row split then).  ``_extra``: what a subclass hands its own ``_check_extra`` and ``_forward_extra``."""
        dev, B, T, lens_dev = self._check_call(mel, mel_lengths)
        _extra = self._check_extra(_extra, dev, B, T)
        h = self._ensure_packed()
        forward = self._c("forward")
        mel = mel.contiguous()
        wav = torch.empty(B, T * self.hop, dtype=torch.float32, device=dev)
        stages = None
        if stage_outputs:
            stages = [torch.empty(B, n, c, dtype=torch.float32, device=dev) for n, c in self._stage_tensor_shapes(T)]
        rows = B
        if workspace is None:
            while rows > 1 and self.workspace_bytes(rows, T) > self.WORKSPACE_CAP_BYTES:
                rows = (rows + 1) // 2
            workspace = self._scratch("_workspace", self.workspace_bytes(rows, T), dev)
        for lo in range(0, B, rows):
            n = min(rows, B - lo)
            ptrs = None
            if stages is not None:
                ptrs = (C.c_void_p * len(stages))(*[s[lo:lo + n].data_ptr() for s in stages])
            _lib.check(forward(h, mel[lo:lo + n].data_ptr(), *self._forward_extra(_extra, lo, n),
                               lens_dev[lo:lo + n].data_ptr() if lens_dev is not None else None, n, T,
                               wav[lo:lo + n].data_ptr(), ptrs, workspace.data_ptr(), workspace.numel(), self._stream(dev)))
        return (wav, stages) if stage_outputs else wav

    def vocode_with_grad(self, mel: torch.Tensor, mel_lengths=None) -> torch.Tensor:
        """``vocode`` attached to autograd: mel float32 [B, n_mels, T] on the device -> waveform float32 [B, T * hop] whose
        ``backward()`` fills ``.grad`` of every parameter of the generator - and of ``mel`` if ``mel.requires_grad`` - on the device's
        own kernels (<_abi>_forward_train / <_abi>_backward), so a plain torch loop with any loss written in torch and any torch
        optimizer trains or fine-tunes the vocoder.  The waveform has ``vocode``'s bits; under ``torch.no_grad()`` (or when nothing
        requires a gradient) the call IS ``vocode``.  Rows are ragged as in ``vocode``; gradient that arrives behind ``T_b * hop``
        samples is never read, and ``mel.grad`` is 0 at and behind a row's frames.  The call keeps a tape of every layer's
        pre-activations until its backward has run; a parameter changed in place between the two raises torch's version error, and
        packing the weights again between the two raises RuntimeError.  Two backward calls give the same bits.

        Training is on plain weights: a weight-normalised checkpoint is folded when it is loaded and stays folded, and the module
        has no weight-norm parametrisation of its own.  Parameters must be contiguous float32."""
        if not torch.is_grad_enabled() or not (mel.requires_grad or any(p.requires_grad for p in self.parameters())):
            return self.vocode(mel, mel_lengths)
        _, _, _, lens_dev = self._check_call(mel, mel_lengths)
        self._check_trainable()
        return _VocodeWithGrad.apply(self, mel.contiguous(), lens_dev, *self.parameters())

    def vocode_utterances(self, mel: torch.Tensor, mel_lengths=None) -> torch.Tensor:
        """What ``inference`` and ``Synthesizer`` call on whole utterances: ``vocode``, unless the model's published inference does more
        (UnivNet pads every utterance's end and drops the padding's samples)."""
        return self.vocode(mel, mel_lengths)

    def inference(self, inputs: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """{"mel": [B, n_mels, T], "mel_lengths": optional [B]} -> {"waveform": float32 [B, T * hop] on the device, "lengths": int32 [B]
        sample counts}."""
        mel, lens = inputs["mel"], inputs.get("mel_lengths")
        wav = self.vocode_utterances(mel, lens)
        if lens is None:
            lengths = torch.full((mel.shape[0],), self.sample_counts(int(mel.shape[2])), dtype=torch.int32, device=wav.device)
        else:
            lengths = self.sample_counts(torch.as_tensor(lens).to(wav.device, torch.int32))
        return {"waveform": wav, "lengths": lengths}

    def forward(self, inputs: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        return self.inference(inputs)

    @classmethod
    def load_from_config(cls, config_path: str):
        return cls(**BaseConfig.load_configs_from_file(path=config_path, config_map={"audio_config": AudioConfig, "model_config": cls._config_class}))


# ====================================================================== discriminators
class _DiscriminatorNode(torch.autograd.Function):
    """<_abi>_forward / <_abi>_backward as one autograd node, for every discriminator.  The inputs after ``lens_dev`` are the tensors
    the kernels see, in ``weight_names()`` order (``effective_weights()``); they go through ``save_for_backward``, so an in-place
    change between forward and backward raises torch's own version error.  A node owns the blob and the tape of its forward: the
    features buffer is the tape, the returned maps are views of it and go through ``save_for_backward`` as well, and the backward
    binds the node's own blob, whatever the module has packed since, and binds the module's current one back."""

    @staticmethod
    def forward(ctx, model, wav, lens_dev, *weights):
        model._ensure_packed(weights)
        features, maps = model._run_forward(wav, lens_dev)
        ctx.model, ctx.lens_dev, ctx.features, ctx.blob = model, lens_dev, features, model._blob
        ctx.n_weights = len(weights)
        ctx.save_for_backward(wav, *weights, *maps)
        return tuple(maps)

    @staticmethod
    def backward(ctx, *d_maps):
        wav, *rest = ctx.saved_tensors   # raises if a weight - or a returned map, which is the tape - was changed in place
        weights = rest[:ctx.n_weights]
        model = ctx.model
        if ctx.blob.device != model._device():
            raise RuntimeError("the discriminator was moved between this forward and its backward")
        dims, dev = model.dims(), wav.device
        B, n_max = wav.shape
        want_params = any(ctx.needs_input_grad[3:])
        d_wav = torch.empty_like(wav) if ctx.needs_input_grad[1] else None
        if not want_params and d_wav is None:
            return (None, None, None) + (None,) * len(weights)
        d_features = torch.empty_like(ctx.features)
        for view, g in zip(model._views(d_features, B, n_max), d_maps):
            if g is None:
                view.zero_()
            else:
                view.copy_(g)
        grads, table, n = [None] * len(weights), None, 0
        if want_params:
            grads = [torch.empty(w.shape, dtype=torch.float32, device=dev) for w in weights]
            table, n = _weight_table(zip(model.weight_names(), grads))
        ws = model._scratch("_train_workspace", model._c("workspace_bytes")(C.byref(dims), B, n_max, 1), dev)
        bind = model._c("bind")
        _lib.check(bind(model._handle, ctx.blob.data_ptr()))   # the weights this node's forward ran on
        _lib.check(model._c("backward")(model._handle, wav.data_ptr(), _ptr(ctx.lens_dev), B, n_max, ctx.features.data_ptr(), d_features.data_ptr(),
                                        table, n, _ptr(d_wav), ws.data_ptr(), ws.numel(), model._stream(dev)))
        if model._blob is not None:
            _lib.check(bind(model._handle, model._blob.data_ptr()))
        return (None, d_wav, None, *grads)


class DeviceDiscriminator(DeviceModule):
    """waveform -> per sub-discriminator its feature maps and its score, all views of one features buffer.  A subclass builds its
    layers, and states ``_config_class``, ``dims()``, ``_grid()``, ``_row_lengths(n)``, ``_entry(e)`` and the hints of its messages."""
    _config_class: type
    _samples = "samples"   # the unit behind "at least <min_samples>"
    _short_hint = ""       # behind "every row needs at least <min_samples> samples"
    _range_hint = ""       # behind "row b: n samples are outside [lo, n_max]"

    def __init__(self, model_config=None) -> None:
        super().__init__()
        self.model_config = model_config if model_config is not None else self._config_class()

    @property
    def min_samples(self) -> int:
        return self.model_config.min_samples

    def _grid(self):
        """-> (the number of sub-discriminators, the maps of each)."""
        raise NotImplementedError

    def _row_lengths(self, n: int) -> List[List[int]]:
        """Per sub-discriminator, the extent of each map of a row of ``n`` samples."""
        raise NotImplementedError

    @staticmethod
    def _entry(e):
        """One entry of <_abi>_layout -> ``layout()``'s tuple: (byte offset, every extent behind the batch ..., and the strides as a
        tuple where the storage is not the contiguous one)."""
        raise NotImplementedError

    def weight_names(self) -> List[str]:
        """The packer's names, in the order of ``effective_weights()``."""
        return [k for k, _ in self.named_parameters()]

    def effective_weights(self):
        """The tensors the kernels see, in ``weight_names()`` order: the autograd node's inputs."""
        return self.parameters()

    def _pack_items(self, held=None):
        return zip(self.weight_names(), self.effective_weights() if held is None else held)

    # ------------------------------------------------------------------ host arithmetic
    def map_lengths(self, sample_lengths) -> List[List[List[int]]]:
        """[sub-discriminator][map] -> the extent of that map in every row, for the losses' per-row means (host arithmetic)."""
        count, per = self._grid()
        per_row = [self._row_lengths(n) for n in self._host_lengths(sample_lengths)]
        return [[[row[j][i] for row in per_row] for i in range(per)] for j in range(count)]

    def layout(self, B: int, n_max: int):
        """<_abi>_layout: per sub-discriminator the list of its maps' places inside the features buffer (``_entry``)."""
        count, per = self._grid()
        entries = (getattr(_lib, self._abi + "_entry") * (count * per))()
        got = self._c("layout")(C.byref(self.dims()), B, n_max, entries, count * per)
        if got != count * per:
            raise ValueError(f"no layout for B = {B}, n_max = {n_max}: a row needs {self.min_samples} {self._samples} or more")
        flat = [self._entry(e) for e in entries]
        return [flat[j * per:(j + 1) * per] for j in range(count)]

    def _views(self, features: torch.Tensor, B: int, n_max: int) -> List[torch.Tensor]:
        """The maps of a features buffer (uint8) as float32 [B, ...] views of its storage, one sub-discriminator after the other."""
        out = []
        for sub in self.layout(B, n_max):
            for off, *shape in sub:
                strides = shape.pop() if isinstance(shape[-1], tuple) else None
                flat = features[off:off + 4 * B * math.prod(shape)].view(torch.float32)
                out.append(flat.view(B, *shape) if strides is None else flat.as_strided((B, *shape), strides))
        return out

    # ------------------------------------------------------------------ the call
    def _check_call(self, wav: torch.Tensor, sample_lengths):
        dev = self._require_gpu()
        if not isinstance(wav, torch.Tensor) or wav.dim() != 2:
            raise ValueError(f"wav must be [B, n_max], got {tuple(wav.shape) if isinstance(wav, torch.Tensor) else type(wav)}")
        if wav.device != dev or wav.dtype != torch.float32:
            raise ValueError(f"wav must be float32 on {dev}, got {wav.dtype} on {wav.device}")
        B, n_max = wav.shape
        if B < 1 or n_max < self.min_samples:
            raise ValueError(f"a batch of {B} rows and {n_max} samples: every row needs at least {self.min_samples} {self._samples}{self._short_hint}")
        return self._ragged_lengths(sample_lengths, B, self.min_samples, n_max, "samples", self._range_hint, dev)

    def _run_forward(self, wav: torch.Tensor, lens_dev):
        """One <_abi>_forward on the blob that is bound (``_ensure_packed`` comes first) -> (the features buffer, its maps)."""
        dims, dev = self.dims(), wav.device
        B, n_max = wav.shape
        features = torch.empty(self._c("features_bytes")(C.byref(dims), B, n_max), dtype=torch.uint8, device=dev)
        workspace = self._scratch("_workspace", self._c("workspace_bytes")(C.byref(dims), B, n_max, 0), dev)
        _lib.check(self._c("forward")(self._handle, wav.data_ptr(), _ptr(lens_dev), B, n_max, features.data_ptr(), features.numel(),
                                      workspace.data_ptr(), workspace.numel(), self._stream(dev)))
        return features, self._views(features, B, n_max)

    def forward(self, wav: torch.Tensor, sample_lengths=None) -> List[List[torch.Tensor]]:
        """wav float32 [B, n_max] on the device -> per sub-discriminator the list of its maps [B, C, ...]: the post-activation features,
        then the score.  The shape is the contract; the strides are those of the kernels' storage.  ``sample_lengths`` ([B], host or
        device): every row at its own length - bit for bit that row run alone - and exact zeros behind its own extents
        (``_row_lengths``); the padded samples may hold anything.  A row below ``min_samples`` raises ValueError before anything is
        launched.  With gradients enabled and something that requires one, ``backward()`` through any of the maps fills ``.grad`` of
        the parameters that require it, and of ``wav`` if it does, in one call of the device's backward - ``d_wav`` alone when no
        parameter requires a gradient - on the weights this forward ran on, whatever the module has packed since; under
        ``torch.no_grad()`` it is the plain forward with the same bits.  The returned maps are views of the buffer the backward reads
        as its tape: changing one in place before ``backward()`` raises torch's version error (clone it first)."""
        lens_dev = self._check_call(wav, sample_lengths)
        wav = wav.contiguous()
        count, per = self._grid()
        if not torch.is_grad_enabled() or not (wav.requires_grad or any(p.requires_grad for p in self.parameters())):
            with torch.no_grad():
                self._ensure_packed(self.effective_weights())
                _, maps = self._run_forward(wav, lens_dev)
        else:
            self._check_trainable()
            maps = list(_DiscriminatorNode.apply(self, wav, lens_dev, *self.effective_weights()))
        return [maps[j * per:(j + 1) * per] for j in range(count)]

    @classmethod
    def load_from_config(cls, config_path: str):
        configs = BaseConfig.load_configs_from_file(path=config_path, config_map={"discriminator_config": cls._config_class})
        return cls(configs.get("discriminator_config"))
