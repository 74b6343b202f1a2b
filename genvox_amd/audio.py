"""Host-side mirror of the reference's ``AudioProcessor`` mel->wav path (core/processors.py:55-96) on the MI355X.

One-off host work stays on the host exactly as in the reference: the Slaney mel filterbank and its pseudo-inverse
(utils/audio/base.py:90-137; float64 intermediates, float32 result), the Hann window and the Butterworth
coefficients (scipy.signal.butter, base.py:164-166).  Everything per utterance - dB->amplitude, pseudo-inverse
projection, fast Griffin-Lim, inverse STFT, clip/trim/normalise/low-pass - runs batched on the GPU through the
C ABI (include/genvox_amd.h, vocoder section; FFTs in LDS at n_fft 1024 / hop 256, rocFFT at other sizes).  There is no
CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import scipy.signal
import torch

from . import _lib
from . import resample as rs
from .configs import AudioConfig
from .resample import resample_filter, resample_ratio, resampled_length   # noqa: F401  (part of this module's surface)


def hz_to_mel(hz: float) -> float:
    """Slaney mel scale: linear below 1 kHz, logarithmic above (reference: utils/audio/base.py:90-102)."""
    lin_step, knee_hz = 200.0 / 3.0, 1000.0
    if hz < knee_hz:
        return hz / lin_step
    return knee_hz / lin_step + np.log(hz / knee_hz) * 27.0 / np.log(6.4)


def mel_to_hz(mel: float) -> float:
    """Inverse of :func:`hz_to_mel` (reference: utils/audio/base.py:104-115)."""
    lin_step, knee_hz = 200.0 / 3.0, 1000.0
    knee_mel = knee_hz / lin_step
    if mel < knee_mel:
        return lin_step * mel
    return knee_hz * np.exp((np.log(6.4) / 27.0) * (mel - knee_mel))


def get_mel_filter(fs: int, n_fft: int, n_mels: int, fmin: float, fmax: float) -> np.ndarray:
    """Triangular mel filterbank with Slaney area normalisation, float32 [n_mels, 1 + n_fft/2]
    (reference: utils/audio/base.py:117-134)."""
    bins = 1 + n_fft // 2
    bin_hz = np.linspace(0, fs / 2, bins)
    edges_hz = np.array([mel_to_hz(m) for m in np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2)])
    widths = np.diff(edges_hz)
    dist = np.subtract.outer(edges_hz, bin_hz)
    bank = np.zeros((n_mels, bins), dtype=np.float32)
    for i in range(n_mels):
        rising, falling = -dist[i] / widths[i], dist[i + 2] / widths[i + 1]
        bank[i] = np.maximum(0, np.minimum(rising, falling))
    bank *= (2.0 / (edges_hz[2:] - edges_hz[:-2]))[:, np.newaxis]
    return bank


def get_inverse_mel_filter(mel_basis: np.ndarray) -> np.ndarray:
    """Moore-Penrose pseudo-inverse [bins, n_mels] (reference: utils/audio/base.py:136-137)."""
    return np.linalg.pinv(mel_basis)


def keep_by_duration(durations: Sequence[float], config: AudioConfig) -> List[int]:
    """Indices of the recordings whose duration (seconds, after trimming) lies in ``[min_wav_duration, max_wav_duration]``: the
    filter of the reference's ``DataPreprocessor`` (core/processors.py:152)."""
    return [i for i, d in enumerate(durations) if config.min_wav_duration <= d and d <= config.max_wav_duration]


def _int_list(x) -> List[int]:
    """A [B] tensor, array or sequence of counts as host ints."""
    return [int(v) for v in (x.tolist() if isinstance(x, (torch.Tensor, np.ndarray)) else x)]


class _RowLengths(NamedTuple):
    """Frame counts of a ragged batch that passed AudioProcessor._check_lengths: host ints and the device int32 [B] the kernels read."""
    host: List[int]
    dev: torch.Tensor


class AudioProcessor:
    TRIM = 500          # samples dropped at both ends (core/processors.py:93)
    LOWPASS_HZ = 6000   # utils/audio/base.py:168-169
    LOWPASS_ORDER = 6

    def __init__(self, config: AudioConfig, device: Union[str, torch.device] = "cuda:0"):
        self.config = config
        c = config
        self.mel_basis = get_mel_filter(fs=c.sampling_rate, n_fft=c.filter_length, n_mels=c.n_mels, fmin=c.mel_fmin, fmax=c.mel_fmax)
        self.inverse_mel_basis = get_inverse_mel_filter(mel_basis=self.mel_basis)
        self.window = scipy.signal.get_window("hann", c.filter_length, fftbins=True).astype(np.float32)
        self._b, self._a = scipy.signal.butter(self.LOWPASS_ORDER, self.LOWPASS_HZ, fs=c.sampling_rate, btype="low", analog=False)
        self.device = torch.device(device)
        self._plan: Optional[int] = None
        self._ws: Optional[torch.Tensor] = None
        self._window_dev = self._inv_basis_dev = self._mel_basis_dev = None   # device copies, made in _ensure
        self._rs_tables: dict = {}   # (src, dst, float64?) -> (up, down, K, polyphase table on the device), made on first use

    def __del__(self):
        try:
            if self._plan is not None:
                _lib.load().gvx_gl_plan_destroy(self._plan)
        except Exception:
            pass

    # ------------------------------------------------------------------ plumbing
    def _ensure(self):
        if self.device.type != "cuda":
            raise RuntimeError("genvox_amd.AudioProcessor's mel->wav path runs on an MI355X only (no CPU fallback)")
        lib = _lib.load()
        if self._plan is None:
            h = C.c_void_p()
            _lib.check(lib.gvx_gl_plan_create(self.config.filter_length, self.config.hop_length, C.byref(h)))
            self._plan = h.value
        if self._window_dev is None:
            self._window_dev = torch.from_numpy(self.window).to(self.device)
            self._inv_basis_dev = torch.from_numpy(np.ascontiguousarray(self.inverse_mel_basis, dtype=np.float32)).to(self.device)
            self._mel_basis_dev = torch.from_numpy(np.ascontiguousarray(self.mel_basis)).to(self.device)
        return lib

    def _workspace_for(self, what: str, size_fn, *args) -> torch.Tensor:
        """The shared workspace, grown to what ``size_fn(plan, *args)`` of the C ABI asks for."""
        need = size_fn(self._plan, *args)
        if need == 0:
            raise _lib.GvxError(f"could not plan the {what} workspace: " + _lib.load().gvx_last_error().decode())
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def _workspace(self, B: int, T: int, ragged: bool = False) -> torch.Tensor:
        lib = _lib.load()
        return self._workspace_for("vocoder", lib.gvx_gl_workspace_bytes_ragged if ragged else lib.gvx_gl_workspace_bytes, B, T, self.config.n_mels)

    @property
    def _dev_consts(self) -> Tuple[Optional[torch.Tensor], ...]:
        """(window, inverse mel basis, mel basis) on the device: the tuple earlier callers indexed, kept readable for them."""
        return self._window_dev, self._inv_basis_dev, self._mel_basis_dev

    @property
    def _log_kind(self) -> int:
        """log10_kind of the C ABI: 0 natural logarithm, 1 base 10."""
        return 0 if self.config.log_func == "np.log" else 1

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def row_samples(self, frame_lengths: Sequence[int], trimmed: bool = True) -> List[int]:
        """Samples of rows of the given frame counts: n_fft + (T_b-1)*hop, less the TRIM samples `finalize` drops at both ends."""
        c = self.config
        return [c.filter_length + (int(t) - 1) * c.hop_length - (2 * self.TRIM if trimmed else 0) for t in frame_lengths]

    def _check_lengths(self, frame_lengths, B: int, T: int, trimmed: bool) -> _RowLengths:
        """Validate per-row frame counts on the host (nothing is launched for a bad batch): (host list, device int32 [B])."""
        if isinstance(frame_lengths, _RowLengths):   # checked by the caller (convert_mel2wav_batch), with trimmed=True
            return frame_lengths
        host = _int_list(frame_lengths)
        if len(host) != B:
            raise ValueError(f"{len(host)} frame lengths for a batch of {B} rows")
        for b, t in enumerate(host):
            if not 1 <= t <= T:
                raise ValueError(f"frame length {t} of row {b} is outside [1, {T}]")
        if trimmed:
            for b, n in enumerate(self.row_samples(host)):
                if n <= 0:
                    raise ValueError(f"row {b}: {host[b]} frames are {n + 2 * self.TRIM} samples, too short to drop {self.TRIM} at both ends")
        if isinstance(frame_lengths, torch.Tensor) and frame_lengths.device == self.device and frame_lengths.dtype == torch.int32:
            return _RowLengths(host, frame_lengths.contiguous())
        return _RowLengths(host, torch.tensor(host, dtype=torch.int32, device=self.device))

    # ------------------------------------------------------------------ device stages (batched, reference layouts)
    def stft(self, signal: torch.Tensor) -> torch.Tensor:
        """[B, n] float32 -> complex64 [B, bins, T] (reference stft, utils/audio/base.py:58-69, per row)."""
        lib = self._ensure()
        x = signal.to(self.device, torch.float32).contiguous()
        B, n = x.shape
        c = self.config
        T = (n - c.filter_length) // c.hop_length + 1
        out = torch.empty(B, c.filter_length // 2 + 1, T, 2, device=self.device)
        ws = self._workspace(B, T)
        _lib.check(lib.gvx_stft(self._plan, x.data_ptr(), self._window_dev.data_ptr(), B, n, out.data_ptr(), ws.data_ptr(),
                                ws.numel(), self._stream()))
        return torch.view_as_complex(out)

    def istft(self, spec: torch.Tensor) -> torch.Tensor:
        """complex64 [B, bins, T] -> [B, n_fft + (T-1)*hop] (reference istft, utils/audio/base.py:71-88)."""
        lib = self._ensure()
        z = torch.view_as_real(spec.to(self.device, torch.complex64).contiguous()).contiguous()
        B, bins, T, _ = z.shape
        c = self.config
        out = torch.empty(B, c.filter_length + (T - 1) * c.hop_length, device=self.device)
        ws = self._workspace(B, T)
        _lib.check(lib.gvx_istft(self._plan, z.data_ptr(), self._window_dev.data_ptr(), B, T, out.data_ptr(), ws.data_ptr(),
                                 ws.numel(), self._stream()))
        return out

    def mel_to_magnitude(self, mel_db: torch.Tensor) -> torch.Tensor:
        """db_to_amplitude + mel2fft: [B, n_mels, T] -> [B, bins, T]."""
        lib = self._ensure()
        x = mel_db.to(self.device, torch.float32).contiguous()
        B, M, T = x.shape
        c = self.config
        out = torch.empty(B, c.filter_length // 2 + 1, T, device=self.device)
        ws = self._workspace(B, T)
        _lib.check(lib.gvx_mel_to_magnitude(self._plan, x.data_ptr(), self._inv_basis_dev.data_ptr(), B, M, T, self._log_kind,
                                            float(c.ref_level_db), out.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()))
        return out

    def griffin_lim(self, mag: torch.Tensor, n_iter: int = 32, momentum: float = 0.99, want_phase: bool = True,
                    want_wav: bool = True, frame_lengths=None) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
        """[B, bins, T] magnitude -> (phase [B, bins, T], waveform [B, n]) (reference griffin_lim + final istft).

        ``frame_lengths`` ([B] ints, tensor or sequence, each in [1, T]): row b has only its first T_b frames; its phase and
        waveform up to n_fft + (T_b-1)*hop samples equal a call on ``mag[b:b+1, :, :T_b]`` bit for bit, whatever the padded
        frames hold, and are 0 behind."""
        lib = self._ensure()
        m = mag.to(self.device, torch.float32).contiguous()
        B, bins, T = m.shape
        c = self.config
        lens = self._check_lengths(frame_lengths, B, T, trimmed=False).dev if frame_lengths is not None else None
        phase = torch.empty_like(m) if want_phase else None
        wav = torch.empty(B, c.filter_length + (T - 1) * c.hop_length, device=self.device) if want_wav else None
        ws = self._workspace(B, T, ragged=lens is not None)
        call, rows = (lib.gvx_griffin_lim, ()) if lens is None else (lib.gvx_griffin_lim_ragged, (lens.data_ptr(),))
        _lib.check(call(self._plan, m.data_ptr(), self._window_dev.data_ptr(), B, T, *rows, n_iter, float(momentum),
                        phase.data_ptr() if want_phase else None, wav.data_ptr() if want_wav else None, ws.data_ptr(), ws.numel(),
                        self._stream()))
        return phase, wav

    def finalize(self, wav: torch.Tensor, frame_lengths=None) -> torch.Tensor:
        """clip / trim 500 / peak-normalise / Butterworth low-pass -> float64 [B, n - 1000] (core/processors.py:91-95).

        ``frame_lengths``: row b is the signal of T_b frames (n_fft + (T_b-1)*hop samples at the start of the padded row); it is
        trimmed, normalised and filtered as a signal of that length and the result is 0 behind its n_b - 1000 samples."""
        lib = self._ensure()
        y = wav.to(self.device, torch.float32).contiguous()
        B, n = y.shape
        c = self.config
        lens = None
        if frame_lengths is not None:
            if n < c.filter_length or (n - c.filter_length) % c.hop_length:
                raise ValueError(f"{n} samples per row are not n_fft + (T-1)*hop for any frame count T")
            lens = self._check_lengths(frame_lengths, B, (n - c.filter_length) // c.hop_length + 1, trimmed=True).dev
        out = torch.empty(B, n - 2 * self.TRIM, dtype=torch.float64, device=self.device)
        scratch = torch.empty(B, dtype=torch.int32, device=self.device)
        nb = len(self._b)
        b = (C.c_double * nb)(*[float(v) for v in self._b])
        a = (C.c_double * nb)(*[float(v) for v in self._a])
        call, rows = (lib.gvx_wav_finalize, ()) if lens is None else (lib.gvx_wav_finalize_ragged, (lens.data_ptr(), c.filter_length, c.hop_length))
        _lib.check(call(y.data_ptr(), B, n, *rows, self.TRIM, b, a, nb - 1, out.data_ptr(), scratch.data_ptr(), self._stream()))
        return out

    def wav_to_mel(self, signal: torch.Tensor) -> torch.Tensor:
        """[B, n] normalised float32 signals -> mel (dB) [B, n_mels, T] (reference convert_wav2mel chain, per row)."""
        lib = self._ensure()
        x = signal.to(self.device, torch.float32).contiguous()
        B, n = x.shape
        c = self.config
        T = (n - c.filter_length) // c.hop_length + 1
        out = torch.empty(B, c.n_mels, T, device=self.device)
        ws = self._workspace(B, T)
        _lib.check(lib.gvx_wav_to_mel(self._plan, x.data_ptr(), self._window_dev.data_ptr(), self._mel_basis_dev.data_ptr(), B, n, c.n_mels,
                                      self._log_kind, float(c.ref_level_db), out.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()))
        return out

    def convert_wav2mel(self, input_path: str, output_path: str) -> None:
        """Reference signature (core/processors.py:70-79): read a wav file, write the mel (dB) as .npy."""
        import scipy.io.wavfile

        fs, sig = scipy.io.wavfile.read(input_path)
        assert fs == self.config.sampling_rate, f"wav file ({input_path}) sampling rate ({fs}) does not match with config ({self.config.sampling_rate})"
        if self.config.normalize:
            sig = (sig / max(np.abs(np.min(sig)), np.abs(np.max(sig)))).astype(np.float32)   # utils/audio/base.py:20-22
        mel = self.wav_to_mel(torch.from_numpy(np.ascontiguousarray(sig, dtype=np.float32))[None])
        np.save(output_path, mel[0].cpu().numpy())

    # ------------------------------------------------------------------ recordings -> mel batch (rows of different lengths)
    ROW_EMPTY, ROW_SHORT, ROW_SILENT, ROW_CUT = 1, 2, 4, 8   # GVX_WAV_ROW_* of include/genvox_amd.h
    _ROW_WHY = {1: "nothing is left of it after trimming silence", 2: "it is shorter than one frame ({n_fft} samples)",
                4: "every sample of it is zero", 8: "it has more frames than the output was sized for"}

    def _pcm_batch(self, pcm, sample_lengths=None) -> Tuple[torch.Tensor, List[int]]:
        """Padded PCM batch on the device and the rows' sample counts on the host.  ``pcm``: a [B, n_max] tensor / array (int16,
        or floating point with full scale 1.0) with ``sample_lengths``, or a list of 1-D arrays of their own lengths."""
        if isinstance(pcm, (list, tuple)):
            rows = [np.asarray(r.cpu() if isinstance(r, torch.Tensor) else r) for r in pcm]
            if not rows:
                raise ValueError("an empty batch of recordings")
            for b, r in enumerate(rows):
                if r.ndim != 1:
                    raise ValueError(f"row {b}: a recording is a 1-D array of samples, got shape {r.shape} (mix channels down first)")
            kinds = {np.int16 if r.dtype == np.int16 else (np.float32 if r.dtype.kind == "f" else None) for r in rows}
            if None in kinds or len(kinds) != 1:
                raise ValueError("recordings must all be int16 or all be floating point, got " + ", ".join(sorted({str(r.dtype) for r in rows})))
            if sample_lengths is not None:
                raise ValueError("sample_lengths goes with a padded [B, n_max] batch; a list of arrays carries its own lengths")
            lengths = [int(r.shape[0]) for r in rows]
            host = np.zeros((len(rows), max(1, max(lengths))), dtype=kinds.pop())
            for b, r in enumerate(rows):
                host[b, : lengths[b]] = r
            return torch.from_numpy(host).to(self.device), lengths
        x = torch.as_tensor(pcm)
        if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError(f"a PCM batch is [B, n_max], got shape {tuple(x.shape)}")
        if x.dtype != torch.int16:
            if not x.dtype.is_floating_point:
                raise ValueError(f"PCM samples must be int16 or floating point, got {x.dtype}")
            x = x.to(torch.float32)
        if sample_lengths is None:
            raise ValueError("a padded PCM batch needs sample_lengths")
        lengths = _int_list(sample_lengths)
        if len(lengths) != x.shape[0]:
            raise ValueError(f"{len(lengths)} sample lengths for a batch of {x.shape[0]} rows")
        for b, n in enumerate(lengths):
            if not 0 <= n <= x.shape[1]:
                raise ValueError(f"sample length {n} of row {b} is outside [0, {x.shape[1]}]")
        return x.to(self.device).contiguous(), lengths

    def _trim_bounds(self, x: torch.Tensor, lengths: List[int], trim: bool, fs: Optional[int] = None) -> torch.Tensor:
        lib = self._ensure()
        B, n_max = x.shape
        lens = torch.tensor(lengths, dtype=torch.int32, device=self.device)
        bounds = torch.empty(B, 2, dtype=torch.int32, device=self.device)
        _lib.check(lib.gvx_wav_trim_bounds(x.data_ptr(), 0 if x.dtype == torch.int16 else 1, B, n_max, lens.data_ptr(),
                                           int(self.config.sampling_rate if fs is None else fs), float(self.config.trim_dbfs) if trim else float("nan"),
                                           bounds.data_ptr(), self._stream()))
        return bounds

    def trim_bounds(self, pcm, sample_lengths=None) -> torch.Tensor:
        """Silence bounds of every row: int32 [B, 2] on the device, row b keeps ``pcm[b, left:right]``.

        The reference's ``get_non_silent_boundary`` (utils/__init__.py:56-76) at ``config.trim_dbfs``: 20 ms chunks walked from the
        row's start and, aligned to its last sample, from its end.  A row in which no chunk reaches the threshold comes back with
        ``left >= right`` (the reference asserts on it).  Nothing synchronises."""
        x, lengths = self._pcm_batch(pcm, sample_lengths)
        return self._trim_bounds(x, lengths, True)

    def wav_to_mel_ragged(self, pcm, sample_lengths=None, trim: Optional[bool] = None, normalize: Optional[bool] = None,
                          drop_bad: bool = False, _durations: bool = False, sample_rates=None):
        """Recordings of different lengths -> ``(mel_padded [B, n_mels, T], mel_lengths [B] int64, gate_padded [B, T])`` on the
        device: the mel side of the batch ``Tacotron2.forward`` / ``train_step`` consume, in one set of launches.

        ``pcm`` is a padded ``[B, n_max]`` batch with ``sample_lengths`` (what lies behind a row's length may hold anything), or a
        list of 1-D arrays; int16 (full scale 32767, as ``scipy.io.wavfile.read`` gives) or floating point (full scale 1.0).
        ``trim`` / ``normalize`` default to ``config.trim_silence`` / ``config.normalize``.  Per row: the reference's silence bounds
        (see ``trim_bounds``), peak normalisation over the kept samples as ``float32(double(y) / double(peak))`` fused into the
        STFT's loads (``normalize_signal``, utils/audio/base.py:20-22 - except that the peak of an int16 row that holds -32768 is
        32768: the reference's int16 ``abs`` wraps to -32768 there and flips the signal, which is not reproduced), then the
        ``convert_wav2mel`` chain.  Row b equals ``wav_to_mel`` on its own trimmed, normalised signal bit for bit; frames behind
        ``mel_lengths[b]`` are exact zeros and ``gate_padded`` is 1 from each row's last frame on, as ``TextMelCollateFn`` lays them out.

        The outputs' time stride is computed on the host from the UNTRIMMED lengths (an upper bound), so no launch waits for the
        device; the one synchronisation of the call is the copy of the B frame counts and status words back to the host at the end,
        after which the result is narrowed to the longest row.

        A row that is empty after trimming, shorter than one frame or all zeros raises ``ValueError`` naming the row (its output is
        zeros, never NaN).  With ``drop_bad=True`` such rows are left out instead and the return value gains a fourth member, the
        list of their indices.

        ``sample_rates`` (one int, or one per recording; default: every recording is at ``config.sampling_rate``) and rows of shape
        ``(n, channels)`` open the call to recordings as they arrive: the reference's order of operations (core/processors.py:136-164)
        with its ffmpeg stage on the device.  Channels are mixed down (``gvx_wav_mixdown``), the silence bounds are taken on the
        mono signal at the SOURCE rate, ``[left, right)`` is resampled to the model's rate (``resample``; one call per group of
        recordings of one rate, channel count and sample type, each writing its rows of one padded float32 batch), and one
        ``gvx_wav_to_mel_ragged`` call over all rows follows with the bounds ``[0, n_out_b)``.  Results come back in input order,
        the call still synchronises once, and a recording that is mono and already at the model's rate goes through exactly as
        it does without these arguments.  A list may then mix int16 and floating point recordings; each keeps its own full scale
        (which peak normalisation removes)."""
        lib = self._ensure()
        c = self.config
        trim = c.trim_silence if trim is None else trim
        normalize = c.normalize if normalize is None else normalize
        rows = src_bounds = None   # recordings at other rates / with channels: the batch's row of each input, source bounds and rates
        if self._is_foreign(pcm, sample_rates):
            x, bounds, longest, rows, src_bounds, row_rates = self._gather_recordings(pcm, sample_lengths, sample_rates, bool(trim))
            B, n_max = x.shape
        else:
            x, lengths = self._pcm_batch(pcm, sample_lengths)
            B, n_max = x.shape
            longest = max(lengths)
        T = max(1, (longest - c.filter_length) // c.hop_length + 1)
        if rows is None:
            bounds = self._trim_bounds(x, lengths, bool(trim))
        ws = self._workspace_for("wav -> mel", lib.gvx_wav_to_mel_ragged_workspace_bytes, B, n_max, c.n_mels)
        mel = torch.empty(B, c.n_mels, T, device=self.device)
        gate = torch.empty(B, T, device=self.device)
        words = torch.empty(2, B, dtype=torch.int32, device=self.device)   # frame counts, status words
        _lib.check(lib.gvx_wav_to_mel_ragged(self._plan, x.data_ptr(), 0 if x.dtype == torch.int16 else 1, self._window_dev.data_ptr(),
                                             self._mel_basis_dev.data_ptr(), B, n_max, bounds.data_ptr(), int(bool(normalize)), c.n_mels,
                                             self._log_kind, float(c.ref_level_db), T, mel.data_ptr(), gate.data_ptr(),
                                             words[0].data_ptr(), words[1].data_ptr(), ws.data_ptr(), ws.numel(), self._stream()))
        at_source = bounds if src_bounds is None else src_bounds
        host = torch.cat([words, at_source.t()]).cpu() if _durations else words.cpu()   # the call's one synchronisation
        if rows is not None:   # back to input order: recording i is row rows[i] of the batch
            host = host[:, rows]
            if rows != list(range(B)):
                idx = torch.tensor(rows, dtype=torch.long, device=self.device)
                mel, gate = mel.index_select(0, idx), gate.index_select(0, idx)
        frames, status = host[0].tolist(), host[1].tolist()
        bad = [b for b in range(B) if status[b] != 0]
        if bad and not drop_bad:
            b = bad[0]
            why = self._ROW_WHY.get(status[b], f"status {status[b]}").format(n_fft=c.filter_length)
            raise ValueError(f"row {b} of the batch gives no mel: {why}" + (f" (and {len(bad) - 1} more: rows {bad[1:]})" if len(bad) > 1 else ""))
        keep = [b for b in range(B) if status[b] == 0]
        if bad:
            idx = torch.tensor(keep, dtype=torch.long, device=self.device)
            mel, gate = mel.index_select(0, idx), gate.index_select(0, idx)
        T_used = max([frames[b] for b in keep], default=0)
        if T_used < T:
            mel, gate = mel[:, :, :T_used].contiguous(), gate[:, :T_used].contiguous()
        out = (mel, torch.tensor([frames[b] for b in keep], dtype=torch.long, device=self.device), gate)
        if drop_bad:
            out = out + (bad,)
        if _durations:
            rate = [c.sampling_rate] * B if rows is None else [row_rates[r] for r in rows]
            out = out + ([(host[3][b].item() - host[2][b].item()) / rate[b] for b in range(B)],)
        return out

    # ------------------------------------------------------------------ recordings at any rate, with channels
    _PCM_KINDS = {torch.int16: 0, torch.float32: 1, torch.float64: 2}   # GVX_PCM_* of include/genvox_amd.h

    def _resample_table(self, src: int, dst: int, float64: bool):
        """(up, down, K, table on the device) of src -> dst: designed on first use (``resample.resample_filter``), kept per pair."""
        key = (int(src), int(dst), bool(float64))
        if key not in self._rs_tables:
            up, down = rs.resample_ratio(src, dst)
            table = rs.polyphase_table(rs.resample_filter(up, down), up, np.float64 if float64 else np.float32)
            self._rs_tables[key] = (up, down, table.shape[1], torch.from_numpy(table).to(self.device))
        return self._rs_tables[key]

    def _mixdown(self, x: torch.Tensor) -> torch.Tensor:
        """[B, n_max, C] interleaved -> float32 mono [B, n_max]: the mean of the channels (int16 keeps its full scale)."""
        lib = self._ensure()
        B, n_max, C_ = x.shape
        mono = torch.empty(B, n_max, dtype=torch.float32, device=self.device)
        _lib.check(lib.gvx_wav_mixdown(x.data_ptr(), self._PCM_KINDS[x.dtype], B, n_max, C_, mono.data_ptr(), self._stream()))
        return mono

    def _resample_into(self, x: torch.Tensor, bounds: torch.Tensor, src: int, dst: int, out: torch.Tensor) -> torch.Tensor:
        """Rows ``x[b, left_b:right_b]`` at ``src`` Hz -> ``out[b]`` at ``dst`` Hz (``out``: contiguous rows of a float32 - float64
        for float64 samples - buffer at least ``resampled_length(n_max)`` wide); returns the rows' new lengths, device int32 [B]."""
        lib = self._ensure()
        up, down, K, table = self._resample_table(src, dst, x.dtype == torch.float64)
        B, n_max = x.shape
        assert out.is_contiguous() and out.shape[0] == B and out.dtype == (torch.float64 if x.dtype == torch.float64 else torch.float32)
        lengths = torch.empty(B, dtype=torch.int32, device=self.device)
        _lib.check(lib.gvx_wav_resample_ragged(x.data_ptr(), self._PCM_KINDS[x.dtype], B, n_max, bounds.data_ptr(), up, down, table.data_ptr(),
                                               K, out.data_ptr(), out.shape[1], lengths.data_ptr(), self._stream()))
        return lengths

    def _pcm_batch_any(self, pcm, sample_lengths=None, keep_float64: bool = False) -> Tuple[torch.Tensor, List[int]]:
        """``_pcm_batch`` for recordings that may have channels: ``[B, n_max]`` or interleaved ``[B, n_max, C]`` on the device (int16,
        float32, or float64 where the caller keeps it) and the rows' sample counts.  A list holds arrays of one shape kind
        (all ``(n,)`` or all ``(n, C)`` with one C) and one sample type."""
        if isinstance(pcm, (list, tuple)):
            arrs = [np.asarray(r.cpu() if isinstance(r, torch.Tensor) else r) for r in pcm]
            if not arrs:
                raise ValueError("an empty batch of recordings")
            if sample_lengths is not None:
                raise ValueError("sample_lengths goes with a padded [B, n_max] batch; a list of arrays carries its own lengths")
            shapes = {r.shape[1:] for r in arrs}
            if any(r.ndim not in (1, 2) for r in arrs) or len(shapes) != 1:
                raise ValueError("recordings of one call are all (n,) or all (n, channels) with one channel count, got shapes "
                                 + ", ".join(sorted({str(r.shape) for r in arrs})))
            kinds = {np.dtype(np.int16) if r.dtype == np.int16 else (np.dtype(np.float64) if keep_float64 and r.dtype == np.float64 else
                                                                    (np.dtype(np.float32) if r.dtype.kind == "f" else None)) for r in arrs}
            if None in kinds or len(kinds) != 1:
                raise ValueError("recordings must all be int16 or all be floating point, got " + ", ".join(sorted({str(r.dtype) for r in arrs})))
            lengths = [int(r.shape[0]) for r in arrs]
            host = np.zeros((len(arrs), max(1, max(lengths))) + tuple(shapes.pop()), dtype=kinds.pop())
            for b, r in enumerate(arrs):
                host[b, : lengths[b]] = r
            x = torch.from_numpy(host).to(self.device)
        else:
            x = torch.as_tensor(pcm)
            if x.dim() not in (2, 3) or min(x.shape) < 1:
                raise ValueError(f"a PCM batch is [B, n_max] or [B, n_max, channels], got shape {tuple(x.shape)}")
            if x.dtype != torch.int16:
                if not x.dtype.is_floating_point:
                    raise ValueError(f"PCM samples must be int16 or floating point, got {x.dtype}")
                x = x.to(torch.float64 if keep_float64 and x.dtype == torch.float64 else torch.float32)
            if sample_lengths is None:
                raise ValueError("a padded PCM batch needs sample_lengths")
            lengths = _int_list(sample_lengths)
            if len(lengths) != x.shape[0]:
                raise ValueError(f"{len(lengths)} sample lengths for a batch of {x.shape[0]} rows")
            for b, n in enumerate(lengths):
                if not 0 <= n <= x.shape[1]:
                    raise ValueError(f"sample length {n} of row {b} is outside [0, {x.shape[1]}]")
            x = x.to(self.device).contiguous()
        if x.dim() == 3 and not 2 <= x.shape[2] <= 8:
            if x.shape[2] == 1:
                x = x[:, :, 0].contiguous()
            else:
                raise ValueError(f"{x.shape[2]} channels: the mix-down takes 2 to 8")
        return x, lengths

    def resample(self, pcm, src_rate: int, dst_rate: Optional[int] = None, sample_lengths=None, bounds=None):
        """Recordings at ``src_rate`` Hz -> ``(signal [B, n_out], lengths)`` at ``dst_rate`` (default ``config.sampling_rate``) on the
        device; ``lengths`` is the device int32 [B] of the rows' new sample counts, ``resampled_length(n_b, up, down)`` each, and a
        row is exact zeros behind its own.  Nothing synchronises.

        ``pcm`` is what ``wav_to_mel_ragged`` takes (a padded ``[B, n_max]`` batch with ``sample_lengths``, or a list of arrays),
        also as float64 and with channels - ``(n, channels)`` rows, ``[B, n_max, channels]`` batches - which are mixed down first
        (the mean of the channels).  int16 and float32 give float32, float64 gives float64; int16 keeps its full scale of 32767.
        ``bounds`` (int32 ``[B, 2]``): row b is ``pcm[b, left_b:right_b]``, as ``trim_bounds`` returns them for the mono signal.
        The filter is ``resample.resample_filter``: a Kaiser-windowed sinc of this project's own choice, no delay (output 0 sits on
        input 0), the signal taken as zero outside its bounds.  A mono batch that is already at ``dst_rate`` comes back as it is,
        as floating point, without a launch."""
        dst = int(self.config.sampling_rate if dst_rate is None else dst_rate)
        src = int(src_rate)
        up, down = rs.resample_ratio(src, dst)
        rs.check_ratio(up, down)
        self._ensure()
        x, lengths = self._pcm_batch_any(pcm, sample_lengths, keep_float64=True)
        if x.dim() == 3:
            x = self._mixdown(x)
        if bounds is None:
            bounds_dev = torch.tensor([[0, n] for n in lengths], dtype=torch.int32, device=self.device)
        else:
            bounds_dev = torch.as_tensor(bounds).to(self.device, torch.int32).contiguous()
            if tuple(bounds_dev.shape) != (x.shape[0], 2):
                raise ValueError(f"bounds are [B, 2] = [{x.shape[0]}, 2], got shape {tuple(bounds_dev.shape)}")
        if src == dst:
            if bounds is not None:
                raise ValueError("bounds go with a rate change: slice a batch that is already at the rate asked for")
            return (x if x.dtype.is_floating_point else x.to(torch.float32)), torch.tensor(lengths, dtype=torch.int32, device=self.device)
        out = torch.empty(x.shape[0], rs.resampled_length(x.shape[1], up, down), dtype=torch.float64 if x.dtype == torch.float64 else torch.float32,
                          device=self.device)
        return out, self._resample_into(x, bounds_dev, src, dst, out)

    def _is_foreign(self, pcm, sample_rates) -> bool:
        """Does a wav -> mel call need the mix-down / resampling stage: a rate other than the model's, or a recording with channels?"""
        if sample_rates is not None:
            rates = [sample_rates] if isinstance(sample_rates, (int, np.integer)) else sample_rates
            if any(int(r) != self.config.sampling_rate for r in rates):
                return True
        if isinstance(pcm, (list, tuple)):
            return any(getattr(r, "ndim", 1) == 2 for r in pcm)
        return getattr(pcm, "ndim", 2) == 3

    def _gather_recordings(self, pcm, sample_lengths, sample_rates, trim: bool):
        """The stage in front of ``gvx_wav_to_mel_ragged`` for recordings of any rate and channel count: one padded float32 batch at
        the model's rate.  Returns ``(x [B, W], bounds [B, 2], longest row (host upper bound), rows, source bounds [B, 2], source
        rate of each batch row)``; recording i is row ``rows[i]`` of the batch (groups are laid out one after the other)."""
        model_rate = int(self.config.sampling_rate)
        if isinstance(pcm, (list, tuple)):
            items = [np.asarray(r.cpu() if isinstance(r, torch.Tensor) else r) for r in pcm]
            if not items:
                raise ValueError("an empty batch of recordings")
            if sample_lengths is not None:
                raise ValueError("sample_lengths goes with a padded [B, n_max] batch; a list of arrays carries its own lengths")
            n_rec = len(items)
        else:
            n_rec = int(pcm.shape[0])
        if sample_rates is None or isinstance(sample_rates, (int, np.integer)):
            rates = [model_rate if sample_rates is None else int(sample_rates)] * n_rec
        else:
            rates = [int(r) for r in sample_rates]
            if len(rates) != n_rec:
                raise ValueError(f"{len(rates)} sample rates for {n_rec} recordings")
        for r in set(rates):
            rs.check_ratio(*rs.resample_ratio(r, model_rate))
        if isinstance(pcm, (list, tuple)):
            for i, a in enumerate(items):
                if a.ndim not in (1, 2) or not (a.dtype == np.int16 or a.dtype.kind == "f"):
                    raise ValueError(f"row {i}: a recording is an int16 or floating point array of shape (n,) or (n, channels), got {a.dtype} {a.shape}")
            keys = [(rates[i], 1 if a.ndim == 1 or a.shape[1] == 1 else a.shape[1], "i" if a.dtype == np.int16 else "f") for i, a in enumerate(items)]
            groups = rs.plan_groups(keys)
            batches = [self._pcm_batch_any([items[i] for i in idx]) for _, idx in groups]
        else:
            if len(set(rates)) != 1:
                raise ValueError("a padded batch is at one sampling rate; pass recordings of different rates as a list")
            groups = [((rates[0],), list(range(n_rec)))]
            batches = [self._pcm_batch_any(pcm, sample_lengths)]
        widths = [x.shape[1] if key[0] == model_rate else rs.resampled_length(x.shape[1], *rs.resample_ratio(key[0], model_rate))
                  for (key, _), (x, _) in zip(groups, batches)]
        B, W = n_rec, max(widths)
        big = torch.empty(B, W, dtype=torch.float32, device=self.device)
        rows, bounds, src_bounds, row_rates, longest, row0 = [0] * B, [], [], [], 1, 0
        for (key, idx), (x, lengths) in zip(groups, batches):
            rate, b = key[0], len(idx)
            mono = self._mixdown(x) if x.dim() == 3 else x
            # silence bounds on the mono signal at the source rate; a mixed-down int16 batch is float32 at full scale 32767
            heard = mono * (1.0 / 32767.0) if trim and x.dim() == 3 and x.dtype == torch.int16 else mono
            sb = self._trim_bounds(heard, lengths, trim, fs=rate)
            part = big[row0:row0 + b]
            if rate == model_rate:
                part[:, : mono.shape[1]] = mono
                bounds.append(sb)
                longest = max(longest, max(lengths))
            else:
                n_out = self._resample_into(mono, sb, rate, model_rate, part)
                bounds.append(torch.stack([torch.zeros_like(n_out), n_out], dim=1))
                longest = max(longest, rs.resampled_length(max(lengths), *rs.resample_ratio(rate, model_rate)))
            src_bounds.append(sb)
            row_rates += [rate] * b
            for k, i in enumerate(idx):
                rows[i] = row0 + k
            row0 += b
        return big, torch.cat(bounds).contiguous(), longest, rows, torch.cat(src_bounds), row_rates

    def format_audio2wav(self, input_path: str, output_path: str) -> None:
        """Reference signature (core/processors.py:62-68, there an ffmpeg process): a wav file of any supported rate and channel
        count -> 16-bit mono at ``config.sampling_rate``.  Mix down, resample (``resample``), round to int16 with saturation,
        write.  Only wav input is decoded here (16-bit PCM or floating point); other containers raise ``ValueError``."""
        import scipy.io.wavfile

        try:
            fs, sig = scipy.io.wavfile.read(input_path)
        except ValueError as e:
            raise ValueError(f"{input_path} is not a wav file this project can decode ({e}); convert other containers to wav first") from e
        if not (sig.dtype == np.int16 or sig.dtype.kind == "f"):
            raise ValueError(f"{input_path} holds {sig.dtype} samples; 16-bit PCM and floating point wav files are supported")
        y, _ = self.resample([sig], fs)
        if sig.dtype != np.int16:
            y = y * 32767.0
        pcm16 = torch.clamp(torch.round(y[0]), -32768.0, 32767.0).to(torch.int16)
        scipy.io.wavfile.write(output_path, int(self.config.sampling_rate), pcm16.cpu().numpy())

    def convert_wav2mel_batch(self, inputs: Sequence, output_paths: Optional[Sequence[str]] = None, trim: Optional[bool] = None,
                              normalize: Optional[bool] = None, drop_bad: bool = False, sample_rates=None):
        """The many-files form of ``convert_wav2mel``: wav paths or sample arrays -> ``(mels, durations)``.

        ``mels[i]`` is the float32 ``[n_mels, T_i]`` array ``convert_wav2mel`` would have written for recording i after the
        reference's silence trimming (``None`` for a recording that gives no mel, with ``drop_bad=True``; otherwise such a
        recording raises ``ValueError``), written to ``output_paths[i]`` as .npy when paths are given.  ``durations[i]`` is the
        recording's length in seconds after trimming, the number the reference's ``DataPreprocessor`` holds against
        ``min_wav_duration`` / ``max_wav_duration`` (core/processors.py:143-152): see ``keep_by_duration``.  All recordings go
        through one ``wav_to_mel_ragged`` call.

        A wav file carries its own rate and channel count; arrays are at ``sample_rates`` (one int, or one per input; default the
        model's rate; the entry of a path is ignored) and may be ``(n, channels)``.  What is not mono at ``config.sampling_rate`` is
        mixed down and resampled on the device first (``wav_to_mel_ragged``), where the single-file ``convert_wav2mel`` asserts;
        ``durations`` stay those of the trimmed recording at its source rate."""
        import scipy.io.wavfile

        model_rate = int(self.config.sampling_rate)
        if sample_rates is None or isinstance(sample_rates, (int, np.integer)):
            rates = [model_rate if sample_rates is None else int(sample_rates)] * len(inputs)
        else:
            rates = [int(r) for r in sample_rates]
            if len(rates) != len(inputs):
                raise ValueError(f"{len(rates)} sample rates for {len(inputs)} recordings")
        rows = []
        for i, item in enumerate(inputs):
            if isinstance(item, (str, bytes)) or hasattr(item, "__fspath__"):
                rates[i], item = scipy.io.wavfile.read(item)
            rows.append(item)
        if output_paths is not None and len(output_paths) != len(rows):
            raise ValueError(f"{len(output_paths)} output paths for {len(rows)} recordings")
        foreign = {} if all(r == model_rate for r in rates) else {"sample_rates": rates}   # rows with channels are seen by the call itself
        mel, mel_lengths, _, dropped, durations = self.wav_to_mel_ragged(rows, trim=trim, normalize=normalize, drop_bad=True, _durations=True, **foreign)
        if dropped and not drop_bad:
            raise ValueError(f"recordings {dropped} give no mel (empty after trimming, shorter than one frame, or all zeros)")
        host, counts = mel.cpu().numpy(), mel_lengths.tolist()
        mels: List[Optional[np.ndarray]] = [None] * len(rows)
        for k, i in enumerate(i for i in range(len(rows)) if i not in set(dropped)):
            mels[i] = np.ascontiguousarray(host[k, :, : counts[k]])
            if output_paths is not None:
                np.save(output_paths[i], mels[i])
        return mels, durations

    # ------------------------------------------------------------------ reference surface
    def convert_mel2wav_batch(self, mels: torch.Tensor, n_iter: int = 32, mel_lengths=None, out_rate: Optional[int] = None):
        """[B, n_mels, T] mel (dB) -> float64 waveforms [B, n_fft + (T-1)*hop - 1000] on the device.

        ``out_rate`` (Hz; default and ``config.sampling_rate``: nothing changes): the float64 waveforms are resampled on the device,
        every row at its own sample count, to ``[B, resampled_length(n)]``; with ``mel_lengths`` the sample counts returned are the
        resampled ones.

        With ``mel_lengths`` ([B] frame counts in [1, T]) the rows are vocoded at their own lengths in the same launches and the
        return value is ``(waveforms, sample_counts)``: row b is valid up to ``sample_counts[b] = n_fft + (T_b-1)*hop - 1000``
        samples - bit for bit the result of a call on ``mels[b:b+1, :, :T_b]`` - and 0 behind.  The padded frames of ``mels`` may
        hold anything.  Bad lengths raise ValueError before anything is launched."""
        lens = None
        if mel_lengths is not None:
            B, _, T = mels.shape
            lens = self._check_lengths(mel_lengths, B, T, trimmed=True)
        mag = self.mel_to_magnitude(mels)   # frame-wise: the padded frames' magnitudes of a ragged batch are simply never used
        _, wav = self.griffin_lim(mag, n_iter=n_iter, want_phase=False, frame_lengths=lens)
        out = self.finalize(wav, frame_lengths=lens)
        samples = self.row_samples(lens.host) if lens is not None else None
        out, samples = self.deliver_at(out, samples, out_rate)
        return out if lens is None else (out, samples)

    def deliver_at(self, wav: torch.Tensor, samples: Optional[List[int]], out_rate: Optional[int]):
        """The last stage of ``convert_mel2wav_batch`` on its own: waveforms [B, n] at ``config.sampling_rate`` (float64 or float32; row
        b of ``samples[b]`` samples, None: all n) -> ``(waveforms at out_rate, their sample counts or None)``, resampled on the device
        in the waveforms' own dtype.  ``out_rate`` None or the model's: both come back as they are.  A caller that needs the
        model-rate waveform as well (``Synthesizer`` tracks pitch on it) vocodes without ``out_rate`` and calls this: the same
        launches as the one call, hence the same bits."""
        if out_rate is None or int(out_rate) == self.config.sampling_rate:
            return wav, samples
        up, down = rs.resample_ratio(self.config.sampling_rate, int(out_rate))
        rs.check_ratio(up, down)
        counts = samples if samples is not None else [wav.shape[1]] * wav.shape[0]
        bounds = torch.tensor([[0, n] for n in counts], dtype=torch.int32, device=self.device)
        resampled = torch.empty(wav.shape[0], rs.resampled_length(wav.shape[1], up, down), dtype=wav.dtype, device=self.device)
        self._resample_into(wav, bounds, self.config.sampling_rate, int(out_rate), resampled)
        samples = [rs.resampled_length(n, up, down) for n in samples] if samples is not None else None
        return resampled, samples

    def convert_mel2wav(self, mel: Union[np.ndarray, str, torch.Tensor], n_iter: int = 32) -> Tuple[int, np.ndarray]:
        """Reference signature (core/processors.py:81-96): one mel [n_mels, T] (array or .npy path) -> (fs, float64 signal)."""
        if isinstance(mel, str):
            mel = np.load(mel)
        x = torch.as_tensor(mel, dtype=torch.float32)
        wav = self.convert_mel2wav_batch(x.unsqueeze(0), n_iter=n_iter)
        return self.config.sampling_rate, wav[0].cpu().numpy()
