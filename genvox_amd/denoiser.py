"""Vocoder denoiser, on the device: the post-filter that the usual neural-vocoder inference scripts apply.

A GAN vocoder - a freshly trained or fine-tuned one above all - hums: it makes a steady tonal artefact whatever the mel says.  The
filter vocodes a constant mel once, keeps the magnitude spectrum of that hum (the vocoder's bias spectrum), takes ``strength`` times
it off the STFT magnitudes of every vocoded waveform, clamped at 0, and transforms back with the phase kept - one call of gvx_denoise
(definition in include/genvox_amd.h, restatement in tests/denoise_ref64.py):

    denoiser = Denoiser.from_vocoder(vocoder)            # once per vocoder
    wav = denoiser(vocoder.vocode(mel, mel_lengths), sample_lengths)

``Synthesizer.tts(text, denoise=0.01)`` does both.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np
import torch

from . import _lib

SUPPORTED_N_FFT = (512, 1024, 2048)


def check_strength(strength, what: str = "strength") -> float:
    """A finite number >= 0, not a bool (no GPU needed)."""
    if isinstance(strength, bool) or not isinstance(strength, (int, float, np.integer, np.floating)) or not math.isfinite(strength) or strength < 0:
        raise ValueError(f"{what} must be a finite number >= 0, not {strength!r}")
    return float(strength)


class Denoiser(torch.nn.Module):
    """out = istft(stft(wav) * max(0, |stft(wav)| - strength * bias) / |stft(wav)|): torch.stft / torch.istft with center=True, reflect
    padding and the periodic Hann of ``n_fft`` points, every row at its own length.  ``bias`` [n_fft / 2 + 1], finite and >= 0, is a
    buffer: ``state_dict`` carries it.  No parameters.

    forward(wav, sample_lengths=None, strength=None): float32 [B, n] on the device -> [B, n], exact zeros behind a row's length;
    ``strength`` None: the module's.  A row needs at least ``min_samples`` = n_fft / 2 + 1 samples for the reflection.
    magnitudes(wav, sample_lengths=None): the STFT magnitudes [B, 1 + n // hop_length, n_fft / 2 + 1], zeros behind a row's frames."""

    def __init__(self, bias, n_fft: int = 1024, hop_length: int = 256, strength: float = 0.01):
        super().__init__()
        n_fft, hop_length = int(n_fft), int(hop_length)
        if n_fft not in SUPPORTED_N_FFT:
            raise ValueError(f"n_fft = {n_fft}: supported are {SUPPORTED_N_FFT}")
        if not 1 <= hop_length <= n_fft // 2:
            raise ValueError(f"hop_length = {hop_length}: 1 <= hop_length <= n_fft / 2 = {n_fft // 2} is required")
        bias = torch.as_tensor(bias).detach().to(torch.float32)
        if bias.shape != (n_fft // 2 + 1,) or not bool(torch.isfinite(bias).all()) or bool((bias < 0).any()):
            raise ValueError(f"bias must be a finite [n_fft / 2 + 1] = [{n_fft // 2 + 1}] spectrum >= 0, got shape {tuple(bias.shape)}")
        self.n_fft, self.hop_length, self.strength = n_fft, hop_length, check_strength(strength)
        self.min_samples = n_fft // 2 + 1
        self.register_buffer("bias", bias.clone().contiguous())
        self._handle = None
        self._workspace: Optional[torch.Tensor] = None

    def __del__(self):
        try:
            if self._handle is not None:
                _lib.load().gvx_denoise_destroy(self._handle)
        except Exception:
            pass

    def __getstate__(self):   # a copy makes its own plan: the handle is destroyed once, by its owner
        state = dict(self.__dict__)
        state.update(_handle=None, _workspace=None)
        return state

    # ---- checks, all before anything is launched
    def _check(self, wav, sample_lengths):
        if not isinstance(wav, torch.Tensor) or wav.dim() != 2 or wav.dtype != torch.float32:
            raise ValueError(f"wav must be a float32 tensor [B, n], got {getattr(wav, 'dtype', type(wav))} {tuple(getattr(wav, 'shape', ()))}")
        B, n_max = wav.shape
        if B < 1 or n_max < self.min_samples:
            raise ValueError(f"a row needs at least n_fft / 2 + 1 = {self.min_samples} samples for the reflection, got [B, n] = [{B}, {n_max}]")
        host = None
        on_device = isinstance(sample_lengths, torch.Tensor) and sample_lengths.device.type == "cuda"
        if sample_lengths is not None and not on_device:   # lengths the host has: refused here, with the row named
            host = [int(v) for v in (sample_lengths.tolist() if isinstance(sample_lengths, torch.Tensor) else sample_lengths)]
            if len(host) != B:
                raise ValueError(f"{len(host)} sample lengths for a batch of {B} rows")
            for b, n in enumerate(host):
                if not self.min_samples <= n <= n_max:
                    raise ValueError(f"row {b} has {n} samples: outside [{self.min_samples}, n = {n_max}]")
        elif on_device and sample_lengths.shape != (B,):
            raise ValueError(f"sample lengths of shape {tuple(sample_lengths.shape)} for a batch of {B} rows")
        if wav.device.type != "cuda":
            raise RuntimeError("genvox_amd.Denoiser runs on an MI355X only: pass tensors on 'cuda:0'. There is no CPU fallback.")
        if self.bias.device != wav.device:
            raise ValueError(f"wav is on {wav.device}, the bias on {self.bias.device}: move the module with .to('{wav.device}')")
        if sample_lengths is None:
            return None
        if host is not None:
            return torch.tensor(host, dtype=torch.int32, device=wav.device)
        return sample_lengths.to(device=wav.device, dtype=torch.int32).contiguous()   # checked by the call itself (GvxError naming the row)

    # ---- the call
    def _plan(self):
        if self._handle is None:
            h = C.c_void_p()
            _lib.check(_lib.load().gvx_denoise_create(self.n_fft, self.hop_length, C.byref(h)))
            self._handle = h.value
        return self._handle

    def _call(self, wav, lens_dev, strength, want_out: bool, want_mag: bool):
        lib = _lib.load()
        dev = wav.device
        B, n_max = wav.shape
        with torch.cuda.device(dev):
            plan = self._plan()
            need = lib.gvx_denoise_workspace_bytes(plan, B, n_max)
            if need == 0:
                _lib.check(-1)
            if self._workspace is None or self._workspace.device != dev or self._workspace.numel() < need:
                self._workspace = torch.empty(need, dtype=torch.uint8, device=dev)
            wav = wav.detach().contiguous()
            out = torch.empty_like(wav) if want_out else None
            mag = torch.empty(B, 1 + n_max // self.hop_length, self.n_fft // 2 + 1, dtype=torch.float32, device=dev) if want_mag else None
            bias = self.bias.contiguous()
            _lib.check(lib.gvx_denoise(plan, wav.data_ptr(), None if lens_dev is None else lens_dev.data_ptr(), B, n_max, bias.data_ptr(), strength,
                                       None if out is None else out.data_ptr(), None if mag is None else mag.data_ptr(),
                                       self._workspace.data_ptr(), self._workspace.numel(), torch.cuda.current_stream(dev).cuda_stream))
        return out, mag

    def forward(self, wav: torch.Tensor, sample_lengths=None, strength: Optional[float] = None) -> torch.Tensor:
        strength = self.strength if strength is None else check_strength(strength)
        return self._call(wav, self._check(wav, sample_lengths), strength, True, False)[0]

    def magnitudes(self, wav: torch.Tensor, sample_lengths=None) -> torch.Tensor:
        return self._call(wav, self._check(wav, sample_lengths), 0.0, False, True)[1]

    @classmethod
    def from_vocoder(cls, vocoder, n_fft: int = 1024, hop_length: Optional[int] = None, frames: int = 88, mel_value: float = 0.0,
                     reduce: str = "first", strength: float = 0.01) -> "Denoiser":
        """The denoiser of ``vocoder`` (``MelGANGenerator``, ``HiFiGANGenerator``, ``BigVGANGenerator``, ``VocosGenerator``, ``UnivNetGenerator``: anything with ``vocode`` and ``n_mels``, its own or
        its ``audio_config``'s): one constant mel [1, n_mels, frames] of ``mel_value`` is vocoded under ``no_grad``, and the bias is
        frame 0 of that waveform's magnitudes (``reduce="first"``, the usual recipe) or their mean over the frames (``"mean"``).
        ``hop_length`` None: ``n_fft // 4``."""
        if reduce not in ("first", "mean"):
            raise ValueError(f"reduce must be 'first' or 'mean', not {reduce!r}")
        hop_length = int(n_fft) // 4 if hop_length is None else int(hop_length)
        frames = int(frames)
        if frames < 1:
            raise ValueError(f"frames = {frames}: at least 1 frame of mel is needed")
        if not math.isfinite(mel_value):
            raise ValueError(f"mel_value must be finite, not {mel_value!r}")
        n_mels = getattr(vocoder, "n_mels", None)
        if n_mels is None:
            n_mels = vocoder.audio_config.n_mels
        dev = next(vocoder.parameters()).device
        probe = cls(torch.zeros(int(n_fft) // 2 + 1), n_fft, hop_length, strength).to(dev)
        with torch.no_grad():
            hum = vocoder.vocode(torch.full((1, int(n_mels), frames), float(mel_value), dtype=torch.float32, device=dev))
            mag = probe.magnitudes(hum.to(torch.float32))[0]
        probe.bias.copy_(mag[0] if reduce == "first" else mag.mean(dim=0))
        return probe
