"""FastPitch acoustic model: tokens -> mel on the MI355X, inference (include/genvox_amd.h, "FastPitch acoustic model"; kernels in
csrc/fastpitch.hip on the dense fp32 GEMM).

A non-autoregressive text-to-mel model: an FFT encoder over the tokens, duration, pitch and energy predictors, a length regulator that
repeats every token for its duration, an FFT decoder over the frames and a projection onto the mel bins.  The module holds the
parameters in PyTorch's own layouts under the published NVIDIA implementation's names (``encoder.word_emb``,
``encoder.layers.<i>.dec_attn.qkv_net`` / ``.o_net`` / ``.layer_norm``, ``.pos_ff.CoreNet.0`` / ``.2`` / ``.layer_norm``,
``duration_predictor.layers.<i>.conv`` / ``.norm``, ``.fc``, ``pitch_emb``, ``energy_emb``, ``proj``), so a published single-speaker
state dict loads as it is: a leading ``module.`` is stripped, ``*.pos_emb.inv_freq`` and the training-only aligner ``attention.*`` are
dropped, ``pitch_mean`` / ``pitch_std`` load as buffers, and ``speaker_emb.*`` is refused by name.  The kernels read a packed blob that is
rebuilt on the device whenever the parameters change.  There is no training, no CPU and no eager path.

Every row is the row alone: every convolution sees zeros outside a row's own positions and keys behind its length get no weight, so a
row of a ragged batch has, bit for bit, the result of that row run alone.  This matches the published single-utterance inference, not its
padded batch, which lets a padded row's last positions see non-zero values behind the row's end (the ReLU output in front of
``CoreNet.2`` and the predictors' second convolution).

``inference`` returns Tacotron2's keys, so ``Synthesizer(tts_model_class=FastPitch, ...)`` - ``tts``, ``tts_batch``, diagnostics, timings,
rate control, pitch tracking, every vocoder - works unchanged."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch
from torch import nn

from . import _lib
from ._device_module import DeviceModule, _Layer, _ptr
from .configs import AudioConfig, BaseConfig, FastPitchConfig, TextConfig

Q_TILE, K_TILE = 128, 64   # GVX_ATTN_Q_TILE, GVX_ATTN_K_TILE: queries per workgroup, keys per LDS tile
LN_EPS = 1e-5
LN_POSITIONS, MAX_DIM = 16, 512   # GVX_ADD_LN_POSITIONS: positions per workgroup of the LayerNorm kernel; GVX_FASTPITCH_MAX_DIM
PACE_MIN, PACE_MAX = 0.125, 8.0


def self_attention(qkv: torch.Tensor, lengths=None, n_head: int = 1, d_head: int = 64, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Masked multi-head self-attention on its own (gvx_self_attention): qkv float32 [B, T, 3 * n_head * d_head] on the device, its
    columns ``[q | k | v]``, each ``[n_head][d_head]`` -> ``softmax(q k^T / sqrt(d_head)) v`` per head, [B, T, n_head * d_head].
    ``lengths`` ([B], host or device): every row over its own keys - bit for bit that row run alone, whatever ``B`` and ``T`` are; the
    result is exact zeros at and behind a row's length, and ``qkv`` is never read there.  ``d_head`` must be 32 or 64.  ``out``: the
    tensor to write, every element of it."""
    if qkv.dim() != 3 or qkv.device.type != "cuda" or qkv.dtype != torch.float32:
        raise ValueError(f"qkv must be float32 [B, T, 3 * n_head * d_head] on the device, got {qkv.dtype} {tuple(qkv.shape)} on {qkv.device}")
    B, T, W = qkv.shape
    if d_head not in (32, 64) or n_head < 1 or W != 3 * n_head * d_head:
        raise ValueError(f"qkv has {W} columns for n_head = {n_head}, d_head = {d_head} (d_head must be 32 or 64)")
    dev = qkv.device
    lens = None
    if lengths is not None:
        host = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
        if len(host) != B or any(not 0 <= n <= T for n in host):
            raise ValueError(f"lengths must be {B} values in [0, {T}]")
        lens = torch.tensor(host, dtype=torch.int32, device=dev)
    qkv = qkv.contiguous()
    if out is None:
        out = torch.empty(B, T, n_head * d_head, dtype=torch.float32, device=dev)
    elif out.shape != (B, T, n_head * d_head) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
        raise ValueError(f"out must be contiguous float32 [{B}, {T}, {n_head * d_head}] on {dev}")
    _lib.check(_lib.load().gvx_self_attention(qkv.data_ptr(), _ptr(lens), B, T, int(n_head), int(d_head), out.data_ptr(),
                                              torch.cuda.current_stream(dev).cuda_stream))
    return out


def add_layernorm(x: torch.Tensor, ln_weight: torch.Tensor, ln_bias: torch.Tensor, y: Optional[torch.Tensor] = None, lengths=None,
                  out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The residual + LayerNorm launch on its own (gvx_add_layer_norm): x and ``y`` (or None) float32 [B, N, C] on the device,
    ``ln_weight`` and ``ln_bias`` float32 [C] on the device -> ``(haloed, plain)``: ``LN(x + y) * ln_weight + ln_bias`` with eps 1e-5 as
    [B, N + 2, C] between two rows of exact zeros (the layout the k-tap products read) and as [B, N, C], the same bits.  ``C`` must be a
    multiple of 32 in [32, MAX_DIM].  ``lengths`` ([B], host or device): every row at its own length - bit for bit that row run alone;
    both results are exact zeros at and behind a row's length, and ``x`` and ``y`` are never read there.  ``out``: the two tensors to
    write, every element of them."""
    if x.dim() != 3 or x.device.type != "cuda" or x.dtype != torch.float32:
        raise ValueError(f"x must be float32 [B, N, C] on the device, got {x.dtype} {tuple(x.shape)} on {x.device}")
    B, N, Cm = x.shape
    dev = x.device
    if B < 1 or N < 1 or Cm < 32 or Cm > MAX_DIM or Cm % 32:
        raise ValueError(f"x is {tuple(x.shape)}: B and N must be >= 1 and C a multiple of 32 in [32, {MAX_DIM}]")
    if y is not None and (y.shape != x.shape or y.dtype != torch.float32 or y.device != dev):
        raise ValueError(f"y must be float32 {tuple(x.shape)} on {dev}, got {y.dtype} {tuple(y.shape)} on {y.device}")
    for name, t in (("ln_weight", ln_weight), ("ln_bias", ln_bias)):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (Cm,) or t.dtype != torch.float32 or t.device != dev:
            raise ValueError(f"{name} must be a float32 tensor [{Cm}] on {dev}")
    lens = None
    if lengths is not None:
        host = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
        if len(host) != B or any(not 0 <= n <= N for n in host):
            raise ValueError(f"lengths must be {B} values in [0, {N}]")
        lens = torch.tensor(host, dtype=torch.int32, device=dev)
    x, y = x.contiguous(), None if y is None else y.contiguous()
    lw, lb = ln_weight.detach().contiguous(), ln_bias.detach().contiguous()
    if out is None:
        out = (torch.empty(B, N + 2, Cm, dtype=torch.float32, device=dev), torch.empty(B, N, Cm, dtype=torch.float32, device=dev))
    haloed, plain = out
    for t, shape in ((haloed, (B, N + 2, Cm)), (plain, (B, N, Cm))):
        if tuple(t.shape) != shape or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
            raise ValueError(f"out must be contiguous float32 [{B}, {N + 2}, {Cm}] and [{B}, {N}, {Cm}] on {dev}")
    _lib.check(_lib.load().gvx_add_layer_norm(x.data_ptr(), _ptr(y), _ptr(lens), B, N, Cm, lw.data_ptr(), lb.data_ptr(), haloed.data_ptr(),
                                              plain.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return haloed, plain


def dims_from_config(mc: FastPitchConfig, ac: AudioConfig, n_tokens: int) -> _lib.gvx_fastpitch_dims:
    d = _lib.gvx_fastpitch_dims()
    d.n_tokens, d.n_mels, d.d_model = int(n_tokens), int(ac.n_mels), mc.d_model
    for stack, s in ((d.enc, "enc"), (d.dec, "dec")):
        stack.n_layers, stack.n_head, stack.d_head = getattr(mc, f"{s}_n_layers"), getattr(mc, f"{s}_n_head"), getattr(mc, f"{s}_d_head")
        stack.d_inner, stack.kernel_size = getattr(mc, f"{s}_d_inner"), getattr(mc, f"{s}_kernel_size")
    d.pred_filter, d.pred_layers, d.energy = mc.predictor_filter_size, mc.predictor_n_layers, int(mc.energy_conditioning)
    d.max_tokens, d.max_decoder_steps, d.max_duration, d.min_token_frames = mc.max_tokens, mc.max_decoder_steps, mc.max_duration, mc.min_token_frames
    return d


class _Norm(nn.Module):
    def __init__(self, dim: int) -> None:
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.bias = nn.Parameter(torch.zeros(dim))


class _Attn(nn.Module):
    def __init__(self, d_model: int, n_head: int, d_head: int) -> None:
        super().__init__()
        self.qkv_net = _Layer((3 * n_head * d_head, d_model), 3 * n_head * d_head, d_model)
        self.o_net = nn.Module()
        self.o_net.weight = nn.Parameter(torch.randn(d_model, n_head * d_head) * (n_head * d_head) ** -0.5)
        self.layer_norm = _Norm(d_model)


class _PosFF(nn.Module):
    def __init__(self, d_model: int, d_inner: int, k: int) -> None:
        super().__init__()
        self.CoreNet = nn.Module()
        self.CoreNet.add_module("0", _Layer((d_inner, d_model, k), d_inner, k * d_model))
        self.CoreNet.add_module("2", _Layer((d_model, d_inner, k), d_model, k * d_inner))
        self.layer_norm = _Norm(d_model)


class _FFTLayer(nn.Module):
    def __init__(self, d_model: int, n_head: int, d_head: int, d_inner: int, k: int) -> None:
        super().__init__()
        self.dec_attn = _Attn(d_model, n_head, d_head)
        self.pos_ff = _PosFF(d_model, d_inner, k)


class _FFTStack(nn.Module):
    def __init__(self, mc: FastPitchConfig, s: str, n_tokens: Optional[int]) -> None:
        super().__init__()
        if n_tokens is not None:
            self.word_emb = nn.Module()
            self.word_emb.weight = nn.Parameter(torch.randn(n_tokens, mc.d_model))
        self.layers = nn.ModuleList([_FFTLayer(mc.d_model, getattr(mc, f"{s}_n_head"), getattr(mc, f"{s}_d_head"), getattr(mc, f"{s}_d_inner"),
                                               getattr(mc, f"{s}_kernel_size")) for _ in range(getattr(mc, f"{s}_n_layers"))])


class _PredLayer(nn.Module):
    def __init__(self, c_in: int, width: int) -> None:
        super().__init__()
        self.conv = _Layer((width, c_in, 3), width, 3 * c_in)
        self.norm = _Norm(width)


class _Predictor(nn.Module):
    def __init__(self, d_model: int, width: int, n_layers: int) -> None:
        super().__init__()
        self.layers = nn.ModuleList([_PredLayer(d_model if i == 0 else width, width) for i in range(n_layers)])
        self.fc = _Layer((1, width), 1, width)


class FastPitch(DeviceModule):
    """``FastPitch(model_config, audio_config, text_config)``; ``text_config.n_tokens`` sizes the embedding table.  A row needs one
    token; a batch is ragged through ``token_lengths``.  The workspace of either phase is ``workspace_bytes(B, N)`` at its ``N``
    positions (tokens for the encoder and the predictors, frames for the decoder)."""
    model_name = "FastPitch"
    _abi = "gvx_fastpitch"

    def __init__(self, model_config: FastPitchConfig, audio_config: AudioConfig, text_config: TextConfig) -> None:
        super().__init__()
        if text_config.n_tokens is None or int(text_config.n_tokens) < 1:
            raise ValueError("text_config.n_tokens sizes the embedding table and must be set")
        self.model_config, self.audio_config, self.text_config = model_config, audio_config, text_config
        mc = model_config
        self.encoder = _FFTStack(mc, "enc", int(text_config.n_tokens))
        self.decoder = _FFTStack(mc, "dec", None)
        self.duration_predictor = _Predictor(mc.d_model, mc.predictor_filter_size, mc.predictor_n_layers)
        self.pitch_predictor = _Predictor(mc.d_model, mc.predictor_filter_size, mc.predictor_n_layers)
        self.pitch_emb = _Layer((mc.d_model, 1, 3), mc.d_model, 3)
        if mc.energy_conditioning:
            self.energy_predictor = _Predictor(mc.d_model, mc.predictor_filter_size, mc.predictor_n_layers)
            self.energy_emb = _Layer((mc.d_model, 1, 3), mc.d_model, 3)
        self.proj = _Layer((int(audio_config.n_mels), mc.d_model), int(audio_config.n_mels), mc.d_model)
        self.register_buffer("pitch_mean", torch.zeros(1))
        self.register_buffer("pitch_std", torch.ones(1))
        for p in self.parameters():
            p.requires_grad_(False)

    # ------------------------------------------------------------------ C-ABI plumbing
    def dims(self) -> _lib.gvx_fastpitch_dims:
        return dims_from_config(self.model_config, self.audio_config, int(self.text_config.n_tokens))

    def blob_numel(self) -> int:
        return self._c("blob_floats")(C.byref(self.dims()))

    def workspace_bytes(self, B: int, N: int) -> int:
        return self._c("workspace_bytes")(C.byref(self.dims()), B, N)

    def enable_stage_timing(self, enable: bool = True) -> None:
        _lib.check(self._c("timing_enable")(self._ensure_packed(), int(enable)))

    def stage_times_ms(self) -> List[float]:
        """Durations of the last call's parts: embedding + encoder, predictors + plan + regulator, decoder, projection (synchronises)."""
        out, n = (C.c_float * 4)(), C.c_int()
        _lib.check(self._c("stage_times_ms")(self._ensure_packed(), out, C.byref(n)))
        return [out[i] for i in range(n.value)]

    def _pack_items(self, held=None):
        """The tensors under the packer's names and in its layouts: the convolutions' weights tap-major, ``[out][k][in]``."""
        items = []
        for k, v in self.state_dict().items():
            if k in ("pitch_mean", "pitch_std"):
                continue
            v = v.detach()
            if v.dim() == 3:
                v = v.permute(0, 2, 1)
            items.append((k, v))
        return items

    # ------------------------------------------------------------------ checkpoints
    def _convert_state_dict(self, state_dict) -> Dict[str, torch.Tensor]:
        """A published state dict -> this module's keys: a leading ``module.`` is stripped, ``*.pos_emb.inv_freq`` and the aligner
        ``attention.*`` are dropped, and a multi-speaker model's ``speaker_emb.*`` is refused by name."""
        out = {}
        for k, v in state_dict.items():
            if k.startswith("module."):
                k = k[len("module."):]
            if k.startswith("speaker_emb") or ".speaker_emb" in k:
                raise ValueError(f"{k}: a multi-speaker FastPitch is not supported, only the single-speaker model")
            if k.endswith("pos_emb.inv_freq") or k.startswith("attention."):
                continue
            out[k] = v
        return out

    def load_checkpoint_statedicts(self, statedicts: Dict, save_optimizer_dict: bool = False, optimizer: Optional[Dict] = None) -> None:
        """Our own ``{"model_statedict": ...}``, the published ``{"state_dict": ...}``, or a plain state dict."""
        if "model_statedict" in statedicts:
            self.load_state_dict(statedicts["model_statedict"])
        elif "state_dict" in statedicts:
            self.load_state_dict(statedicts["state_dict"])
        elif any(k.endswith("encoder.word_emb.weight") for k in statedicts):
            self.load_state_dict(statedicts)
        else:
            raise KeyError("a FastPitch checkpoint holds its weights under 'model_statedict' or 'state_dict', or is the state dict itself")

    @classmethod
    def load_from_config(cls, config_path: str) -> "FastPitch":
        return cls(**BaseConfig.load_configs_from_file(path=config_path, config_map={"text_config": TextConfig, "audio_config": AudioConfig,
                                                                                      "model_config": FastPitchConfig}))

    # ------------------------------------------------------------------ the call
    def _check_inputs(self, inputs: Dict):
        dev = self._require_gpu()
        if inputs.get("attention_window") is not None:
            raise ValueError("attention_window: FastPitch has no attention between tokens and frames to window")
        tokens = inputs["tokens"]
        if not isinstance(tokens, torch.Tensor) or tokens.dim() != 2 or tokens.shape[0] < 1 or tokens.shape[1] < 1:
            raise ValueError("tokens must be a [B, L] tensor with B, L >= 1")
        B, L = tokens.shape
        if L > self.model_config.max_tokens:
            raise ValueError(f"{L} tokens in a row are beyond max_tokens = {self.model_config.max_tokens}")
        tokens = tokens.to(dev, torch.int32).contiguous()
        lens = inputs.get("token_lengths")
        if lens is not None:
            if isinstance(lens, torch.Tensor) and lens.device.type == "cuda":   # no read-back: the kernels clamp a length to [0, L]
                if lens.numel() != B:
                    raise ValueError(f"{lens.numel()} lengths for {B} rows")
                lens = lens.to(dev, torch.int32).clamp(1, L).contiguous()
            else:
                lens = self._ragged_lengths(lens, B, 1, L, "tokens", "", dev)
        pace = float(inputs.get("pace", 1.0))
        if not PACE_MIN <= pace <= PACE_MAX:
            raise ValueError(f"pace = {pace} is outside [{PACE_MIN}, {PACE_MAX}]")
        durations, pitch = inputs.get("durations"), inputs.get("pitch")
        if durations is not None:
            durations = torch.as_tensor(durations)
            if tuple(durations.shape) != (B, L) or durations.dtype.is_floating_point or durations.dtype == torch.bool:
                raise ValueError(f"durations must be an integer tensor [{B}, {L}], got {durations.dtype} {tuple(durations.shape)}")
            if durations.device.type != "cuda" and bool((durations < 0).any()):
                raise ValueError("durations must be >= 0")
            durations = durations.to(dev, torch.int32).clamp(min=0).contiguous()
        if pitch is not None:
            pitch = torch.as_tensor(pitch)
            if tuple(pitch.shape) != (B, L):
                raise ValueError(f"pitch must be [{B}, {L}], got {tuple(pitch.shape)}")
            pitch = pitch.to(dev, torch.float32).contiguous()
        return dev, tokens, lens, pace, durations, pitch

    def _run(self, inputs: Dict, stage_outputs: bool = False, workspace: Optional[torch.Tensor] = None):
        """Both phases -> the outputs of ``inference`` (and, with ``stage_outputs``, the list of x after the embedding and after every
        encoder layer [B, L, d_model], ``log_durations``, ``pitch_pred``, ``energy_pred`` [B, L], the regulated sequence and x after
        every decoder layer [B, T, d_model], and the mel [B, n_mels, T]).  ``workspace``: a uint8 tensor to use as it is in both phases,
        of at least ``workspace_bytes(B, L)`` and ``workspace_bytes(B, T)`` (tests of the workspace contract)."""
        dev, tokens, lens, pace, durations, pitch = self._check_inputs(inputs)
        mc = self.model_config
        B, L = tokens.shape
        Cm, M = mc.d_model, int(self.audio_config.n_mels)
        h = self._ensure_packed()
        f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
        enc_out, log_dur, pitch_pred, energy_pred = f32(B, L + 2, Cm), f32(B, L), f32(B, L), f32(B, L)
        reps, starts, counts = i32(B, L), i32(B, L), i32(B)
        stages, ptrs = None, None
        if stage_outputs:
            stages = [f32(B, L, Cm) for _ in range(mc.enc_n_layers + 1)]
            ptrs = (C.c_void_p * len(stages))(*[s.data_ptr() for s in stages])
        ws = workspace if workspace is not None else self._scratch("_workspace", self.workspace_bytes(B, L), dev)
        _lib.check(self._c("encode")(h, tokens.data_ptr(), _ptr(lens), B, L, pace, _ptr(durations), _ptr(pitch), enc_out.data_ptr(), log_dur.data_ptr(),
                                     pitch_pred.data_ptr(), energy_pred.data_ptr(), reps.data_ptr(), starts.data_ptr(), counts.data_ptr(), ptrs,
                                     ws.data_ptr(), ws.numel(), self._stream(dev)))
        T = max(counts.tolist())   # the one synchronisation of a call: the decoder's length
        mel, gate, align = f32(B, M, T), f32(B, T), f32(B, T, L)
        dec_stages, ptrs = None, None
        if stage_outputs:
            dec_stages = [f32(B, T, Cm) for _ in range(mc.dec_n_layers + 1)]
            ptrs = (C.c_void_p * len(dec_stages))(*[s.data_ptr() for s in dec_stages])
        ws = workspace if workspace is not None else self._scratch("_workspace", self.workspace_bytes(B, T), dev)
        _lib.check(self._c("decode")(h, enc_out.data_ptr(), reps.data_ptr(), starts.data_ptr(), counts.data_ptr(), _ptr(lens), B, L, T, mel.data_ptr(),
                                     gate.data_ptr(), align.data_ptr(), ptrs, ws.data_ptr(), ws.numel(), self._stream(dev)))
        out = {"mel_outputs": mel, "mel_outputs_postnet": mel, "gate_outputs": gate, "alignments": align}
        if B > 1:
            out["mel_lengths"] = counts
        out.update({"durations": reps, "log_durations": log_dur, "pitch_pred": pitch_pred, "energy_pred": energy_pred})
        if stage_outputs:
            return out, stages + [log_dur, pitch_pred, energy_pred] + dec_stages + [mel]
        return out

    @torch.no_grad()
    def inference(self, inputs: Dict) -> Dict[str, torch.Tensor]:
        """``{"tokens": [B, L], "token_lengths": optional [B], "pace": optional float in [0.125, 8] (2 = twice as fast), "durations":
        optional int [B, L] used instead of the predicted ones, "pitch": optional float [B, L] used instead of the predicted pitch (in
        the model's normalised units)}`` -> Tacotron2's keys: ``mel_outputs_postnet`` and ``mel_outputs`` (the same tensor, float32
        [B, n_mels, T], exact zeros behind a row's frames), ``gate_outputs`` [B, T] (-1e3 on a row's frames but its last, +1e3 on the last
        and behind), ``alignments`` [B, T, L] (the exact 0 / 1 matrix of the durations), ``mel_lengths`` int32 [B] for B > 1 - and
        ``durations`` int32 [B, L] (the frames every token got, after ``pace``, ``min_token_frames`` and the cut at
        ``max_decoder_steps``), ``log_durations``, ``pitch_pred`` and ``energy_pred`` float32 [B, L].  A token id outside
        ``[0, n_tokens)`` is read as id 0.  ``attention_window`` raises ValueError.  The call waits for the device once, for the frame counts."""
        return self._run(inputs)

    def forward(self, inputs: Dict) -> Dict[str, torch.Tensor]:
        return self.inference(inputs)
