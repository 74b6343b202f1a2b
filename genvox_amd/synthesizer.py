"""Mirror of the reference's ``core.synthesizer.Synthesizer`` (core/synthesizer.py:9-45): config + checkpoint
loading, text -> tokens, autoregressive Tacotron2 on the GPU, mel -> waveform on the GPU."""
from __future__ import annotations

import math
from typing import Dict, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .audio import AudioProcessor
from .text import TextProcessor


def plan_tts_batches(token_lists: Sequence[Sequence[int]], batch_size: int = 32) -> List[Tuple[List[int], torch.Tensor, torch.Tensor]]:
    """The host half of ``Synthesizer.tts_batch`` (no GPU needed): sentences as token-id lists -> decoder calls.

    Returns one ``(indices, tokens, token_lengths)`` per call: ``indices`` are positions in ``token_lists``, ``tokens`` int32
    [b, L] holds those sentences padded with 0 to the longest of the call, ``token_lengths`` int32 [b].  Sentences are sorted by
    token length, longest first (ties in input order, like ``dist.plan_shards``), and dealt in runs of at most ``batch_size``,
    so the rows of a call are of similar length.  A sentence without tokens raises ValueError naming its index."""
    if batch_size < 1:
        raise ValueError(f"batch_size must be >= 1, not {batch_size}")
    for i, toks in enumerate(token_lists):
        if len(toks) == 0:
            raise ValueError(f"sentence {i} has no tokens after cleaning")
    order = sorted(range(len(token_lists)), key=lambda i: -len(token_lists[i]))
    calls = []
    for lo in range(0, len(order), batch_size):
        idx = order[lo:lo + batch_size]
        lens = torch.tensor([len(token_lists[i]) for i in idx], dtype=torch.int32)
        tokens = torch.zeros(len(idx), int(lens[0]), dtype=torch.int32)
        for r, i in enumerate(idx):
            tokens[r, :len(token_lists[i])] = torch.as_tensor(list(token_lists[i]), dtype=torch.int32)
        calls.append((idx, tokens, lens))
    return calls


def group_words(tokens: Sequence[str], starts: Sequence[float], ends: Sequence[float]) -> List[Tuple[str, float, float]]:
    """Token timings -> word timings (no GPU needed).  ``tokens`` are the characters of the cleaned text with their ``starts`` and
    ``ends``; a word is a maximal run of non-space tokens (punctuation stays on the word it touches) and lasts from its first
    token's start to its last token's end.  Spaces, and the silence they carry, belong to no word: leading, trailing and
    repeated spaces produce nothing."""
    if not len(tokens) == len(starts) == len(ends):
        raise ValueError(f"{len(tokens)} tokens with {len(starts)} starts and {len(ends)} ends")
    words: List[Tuple[str, float, float]] = []
    first = None
    for i, tok in enumerate(tokens):
        if tok.isspace():
            if first is not None:
                words.append(("".join(tokens[first:i]), starts[first], ends[i - 1]))
                first = None
        elif first is None:
            first = i
    if first is not None:
        words.append(("".join(tokens[first:]), starts[first], ends[-1]))
    return words


def token_times(start_frames: Sequence[int], hop_length: int, trim: int, n_samples: int, model_rate: int, end_s: float):
    """Seconds in the delivered waveform from the first frame of every token (no GPU needed): ``(starts, ends)``.  Frame f begins at
    sample ``f * hop_length - trim`` of the model-rate signal of ``n_samples`` samples (the vocoder drops ``trim`` samples at both
    ends), clamped to ``[0, n_samples]`` and divided by ``model_rate`` - a time, so it holds at whatever rate the waveform is
    delivered.  A token ends where the next starts; the last ends at ``end_s``, the delivered waveform's own duration."""
    starts = [min(max(int(f) * hop_length - trim, 0), n_samples) / model_rate for f in start_frames]
    return starts, starts[1:] + [end_s]


def token_pitch(start_frames: Sequence[int], n_frames: int, f0: Sequence[float]) -> List[Tuple[Optional[float], float]]:
    """Pitch per token from a contour per frame (no GPU needed): ``start_frames`` are the first frames of the tokens (what the
    timings are made of), token l owns the frames ``[start_frames[l], start_frames[l + 1])`` and the last one those up to
    ``n_frames``, each bound clamped to ``[0, min(n_frames, len(f0))]``; ``f0`` is in Hz with 0 for an unvoiced frame.  Returns one
    ``(mean_hz, voiced_fraction)`` per token: the mean of its voiced frames (None when it has none) and their share of its frames
    (0.0 for a token without frames)."""
    f0 = np.asarray(f0, dtype=np.float64)
    if f0.ndim != 1:
        raise ValueError(f"f0 must be one contour, got shape {f0.shape}")
    if n_frames < 0:
        raise ValueError(f"n_frames must be >= 0, not {n_frames}")
    n = min(int(n_frames), len(f0))
    bounds = [min(max(int(s), 0), n) for s in start_frames] + [n]
    out: List[Tuple[Optional[float], float]] = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        seg = f0[lo:hi]
        voiced = seg[seg > 0]
        out.append((float(voiced.mean()) if len(voiced) else None, len(voiced) / len(seg) if len(seg) else 0.0))
    return out


RATE_MIN, RATE_MAX = 0.125, 8.0   # GVX_RATE_MIN / GVX_RATE_MAX of include/genvox_amd.h: the range of speed and of speed * rate


def _check_rate(rate, what: str) -> float:
    if isinstance(rate, bool) or not isinstance(rate, (int, float, np.integer, np.floating)) or not math.isfinite(rate) or rate <= 0:
        raise ValueError(f"{what} must be a finite number above 0, not {rate!r}")
    return float(rate)


def token_rates(token_strs: Sequence[str], word_speed: Union[Sequence[float], Mapping[int, float], None]) -> List[float]:
    """Rates per word -> rates per token (no GPU needed).  Words are ``group_words``' segmentation of ``token_strs``: maximal runs of
    non-space tokens, counted from 0.  ``word_speed`` is a sequence with one rate per word or a ``{word_index: rate}`` dict (None:
    no word is named); every token of a word gets the word's rate, spaces and unnamed words get 1.0.  A wrong count, an index that
    is not the number of a word, or a rate that is not a finite number above 0 raises ValueError."""
    word_of: List[int] = []   # per token: its word's number, -1 for a space
    n_words, inside = 0, False
    for tok in token_strs:
        if tok.isspace():
            word_of.append(-1)
            inside = False
        else:
            if not inside:
                n_words, inside = n_words + 1, True
            word_of.append(n_words - 1)
    by_word = [1.0] * n_words
    if word_speed is None:
        pass
    elif isinstance(word_speed, Mapping):
        for w, rate in word_speed.items():
            if isinstance(w, bool) or not isinstance(w, (int, np.integer)) or not 0 <= w < n_words:
                raise ValueError(f"word index {w!r} is outside the sentence's {n_words} words")
            by_word[int(w)] = _check_rate(rate, f"the rate of word {w}")
    else:
        rates = list(word_speed)
        if len(rates) != n_words:
            raise ValueError(f"{len(rates)} word rates for a sentence of {n_words} words")
        by_word = [_check_rate(rate, f"the rate of word {w}") for w, rate in enumerate(rates)]
    return [1.0 if w < 0 else by_word[w] for w in word_of]


def _check_denoise(denoise, has_vocoder: bool) -> float:
    """The ``denoise`` of ``tts`` / ``tts_batch`` (no GPU needed): a finite number >= 0, not a bool; above 0 it needs a vocoder model."""
    if isinstance(denoise, bool) or not isinstance(denoise, (int, float, np.integer, np.floating)) or not math.isfinite(denoise) or denoise < 0:
        raise ValueError(f"denoise must be a finite number >= 0, not {denoise!r}")
    if denoise > 0 and not has_vocoder:
        raise ValueError(f"denoise = {denoise} needs a vocoder model: Griffin-Lim has no bias to subtract")
    return float(denoise)


PITCH_MAX_SEMITONES = 12.0   # a shift of an octave either way: the ratios 0.5 and 2 of GVX_PSOLA_RATIO_MIN / GVX_PSOLA_RATIO_MAX


def _check_semitones(v, what: str) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
        raise ValueError(f"{what} must be a finite number of semitones, not {v!r}")
    return float(v)


def semitones_to_ratio(semitones: float) -> float:
    """The factor on a frequency that ``semitones`` equal-tempered semitones are: 2 ** (semitones / 12) (no GPU needed)."""
    return 2.0 ** (_check_semitones(semitones, "a pitch shift") / 12.0)


def token_semitones(token_strs: Sequence[str], word_pitch: Union[Sequence[float], Mapping[int, float], None]) -> List[float]:
    """Semitones per word -> semitones per token (no GPU needed): ``token_rates`` for pitch.  Words are ``group_words``' segmentation
    of ``token_strs``, counted from 0; ``word_pitch`` is a sequence with one shift per word or a ``{word_index: semitones}`` dict
    (None: no word is named); every token of a word gets the word's shift, spaces and unnamed words get 0.0.  A wrong count, an
    index that is not the number of a word, or a shift that is not a finite number raises ValueError."""
    word_of: List[int] = []   # per token: its word's number, -1 for a space
    n_words, inside = 0, False
    for tok in token_strs:
        if tok.isspace():
            word_of.append(-1)
            inside = False
        else:
            if not inside:
                n_words, inside = n_words + 1, True
            word_of.append(n_words - 1)
    by_word = [0.0] * n_words
    if word_pitch is None:
        pass
    elif isinstance(word_pitch, Mapping):
        for w, semis in word_pitch.items():
            if isinstance(w, bool) or not isinstance(w, (int, np.integer)) or not 0 <= w < n_words:
                raise ValueError(f"word index {w!r} is outside the sentence's {n_words} words")
            by_word[int(w)] = _check_semitones(semis, f"the pitch of word {w}")
    else:
        shifts = list(word_pitch)
        if len(shifts) != n_words:
            raise ValueError(f"{len(shifts)} word pitches for a sentence of {n_words} words")
        by_word = [_check_semitones(semis, f"the pitch of word {w}") for w, semis in enumerate(shifts)]
    return [0.0 if w < 0 else by_word[w] for w in word_of]


def frame_ratios(start_frames: Sequence[int], n_frames: int, per_token_semitones: Sequence[float], base_semitones: float = 0.0) -> np.ndarray:
    """Pitch ratios per frame from semitones per token (no GPU needed): float32 [n_frames].  Token l owns the frames
    ``[start_frames[l], start_frames[l + 1])`` and the last one those up to ``n_frames``, each bound clamped to ``[0, n_frames]``
    (the frames of ``token_pitch``); its frames get ``semitones_to_ratio(base_semitones + per_token_semitones[l])``, frames of no
    token ``semitones_to_ratio(base_semitones)``."""
    if n_frames < 0:
        raise ValueError(f"n_frames must be >= 0, not {n_frames}")
    if len(start_frames) != len(per_token_semitones):
        raise ValueError(f"{len(start_frames)} start frames for {len(per_token_semitones)} tokens")
    out = np.full(int(n_frames), semitones_to_ratio(base_semitones), dtype=np.float32)
    bounds = [min(max(int(s), 0), int(n_frames)) for s in start_frames] + [int(n_frames)]
    for l, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
        out[lo:hi] = semitones_to_ratio(base_semitones + per_token_semitones[l])
    return out


class Synthesizer:
    def __init__(self, tts_model_class, tts_config_path: str, tts_checkpoint_path: str, use_cuda: bool = True, vocoder_model_class=None,
                 vocoder_config_path: Optional[str] = None, vocoder_checkpoint_path: Optional[str] = None) -> None:
        """``vocoder_model_class`` (``MelGANGenerator``, ``HiFiGANGenerator``, ``BigVGANGenerator``, ``VocosGenerator`` or ``UnivNetGenerator``) with its config and checkpoint paths: ``tts`` and ``tts_batch`` vocode the mel
        through that model instead of Griffin-Lim.  The waveform is then float32 of exactly ``frames * hop_length`` samples (``(frames - 1) * hop_length`` from a Vocos model with padding "center"; no trim,
        no low-pass), and every result carries ``"vocoder"``: the model's name.  All three or none: with none nothing changes."""
        if not (use_cuda and torch.cuda.is_available()):
            raise RuntimeError("genvox_amd.Synthesizer needs an MI355X (use_cuda=True and a visible GPU); it has no CPU path")
        self.device = "cuda:0"
        self.tts_model = tts_model_class.load_from_config(config_path=tts_config_path)
        self.tts_model.to(self.device)
        self.tts_model.eval()
        ckpt = torch.load(tts_checkpoint_path, map_location="cpu")
        print(f"[genvox_amd] {self.tts_model.model_name} on {self.device} (MI355X HIP path); "
              f"checkpoint {tts_checkpoint_path} at iteration {ckpt.get('iteration')}")
        self.tts_model.load_checkpoint_statedicts(statedicts=ckpt, save_optimizer_dict=False, optimizer=None)
        self.text_processor = TextProcessor(config=self.tts_model.text_config)
        self.audio_processor = AudioProcessor(config=self.tts_model.audio_config, device=self.device)
        given = [vocoder_model_class, vocoder_config_path, vocoder_checkpoint_path]
        self.vocoder = None
        self._denoiser = None   # made on the first denoise > 0: the vocoder's bias spectrum is taken once
        if any(g is not None for g in given):
            if any(g is None for g in given):
                raise ValueError("a vocoder needs vocoder_model_class, vocoder_config_path and vocoder_checkpoint_path, all three")
            voc = vocoder_model_class.load_from_config(config_path=vocoder_config_path)
            ac, mine = voc.audio_config, self.tts_model.audio_config
            for field in ("n_mels", "hop_length", "sampling_rate"):
                if getattr(ac, field) != getattr(mine, field):
                    raise ValueError(f"the vocoder's {field} = {getattr(ac, field)} is not the text-to-mel model's {getattr(mine, field)}")
            voc.to(self.device)
            voc.eval()
            voc.load_checkpoint_statedicts(statedicts=torch.load(vocoder_checkpoint_path, map_location="cpu"), save_optimizer_dict=False, optimizer=None)
            self.vocoder = voc

    def _out_rate(self, sampling_rate: Optional[int]) -> int:
        return self.audio_processor.config.sampling_rate if sampling_rate is None else int(sampling_rate)

    def _diagnose(self, outputs: Dict[str, torch.Tensor], frames: Optional[torch.Tensor], token_lengths: Optional[torch.Tensor]) -> List[Dict]:
        """Per row of a decoded batch: {"alignment_stats": {...Python numbers}, "stopped": bool}.  The statistics are computed on the
        device from the alignments already there; what comes to the host is one small table per batch."""
        from . import metrics

        st = metrics.alignment_stats(outputs["alignments"], frames, token_lengths)
        n = st["focus"].shape[0]
        if frames is None:
            frames = torch.full((n,), outputs["alignments"].shape[1], dtype=torch.int32, device=st["focus"].device)
        stopped = frames < self.tts_model.model_config.max_decoder_steps
        floats = torch.stack([st["focus"], st["monotonic_fraction"], st["coverage"]]).cpu().tolist()
        ints = torch.stack([st["max_jump"], st["first_pos"], st["last_pos"], stopped.to(torch.int32)]).cpu().tolist()
        return [{"alignment_stats": {"focus": floats[0][r], "monotonic_fraction": floats[1][r], "max_jump": ints[0][r],
                                     "coverage": floats[2][r], "first_pos": ints[1][r], "last_pos": ints[2][r]},
                 "stopped": bool(ints[3][r])} for r in range(n)]

    def _align(self, outputs: Dict[str, torch.Tensor], frames: Optional[torch.Tensor], token_lengths: Optional[torch.Tensor]):
        """Monotonic alignment search over a decoded batch, on the device from the alignments already there: per row the first frame
        of every token and the row's status, as host lists (one small copy)."""
        from . import metrics

        al = metrics.monotonic_align(outputs["alignments"], frames, token_lengths)
        host = torch.cat([al["starts"], al["status"][:, None]], dim=1).cpu().tolist()
        return [row[:-1] for row in host], [row[-1] for row in host]

    def _timings(self, token_strs: Sequence[str], start_frames: Sequence[int], status: int, n_frames: int, n_delivered: int,
                 out_rate: int) -> Dict:
        """The three timing keys of one sentence: ``start_frames`` and ``status`` from ``_align``, ``n_delivered`` samples at ``out_rate``."""
        if status != 0:   # fewer frames than tokens: a collapsed decode is for the diagnostics to report, not an error here
            return {"token_timings": [], "word_timings": [], "timings_status": "infeasible"}
        ap = self.audio_processor
        # a neural vocoder delivers frames * hop samples untrimmed: frame f starts at sample f * hop
        trim, n_samples = (ap.TRIM, ap.row_samples([n_frames])[0]) if self.vocoder is None else (0, self.vocoder.sample_counts(int(n_frames)))
        starts, ends = token_times(start_frames[:len(token_strs)], ap.config.hop_length, trim, n_samples, ap.config.sampling_rate, n_delivered / out_rate)
        return {"token_timings": list(zip(token_strs, starts, ends)), "word_timings": group_words(token_strs, starts, ends),
                "timings_status": "ok"}

    def _vocode(self, mel: torch.Tensor, frames, sampling_rate: Optional[int]):
        """mel [B, M, T] on the device -> ``(waveforms on the device, sample counts per row or None)``; ``frames`` (None: all T) are the
        rows' own lengths.  Without a vocoder model this is ``AudioProcessor.convert_mel2wav_batch`` (Griffin-Lim), call for call.
        With one, the rows go through it in one ragged call - float32 [B, T * hop], row b of ``vocoder.sample_counts(frames[b])`` samples, ``frames[b] * hop`` unless the model says otherwise - and are
        resampled like Griffin-Lim's, every row at its own sample count."""
        wav, counts, _, _ = self._vocode_and_track(mel, frames, sampling_rate, False)
        return wav, counts

    def _denoise(self, wav: torch.Tensor, counts, strength: float) -> torch.Tensor:
        """The vocoder's waveforms with ``strength`` times its bias spectrum taken off (``Denoiser.from_vocoder`` at its defaults, made
        on first use and kept): the ragged batch in one call, every row at its own sample count.  Rows below the denoiser's
        ``min_samples`` (513: fewer than 3 frames at a hop of 256) pass through unchanged."""
        if self._denoiser is None:
            from .denoiser import Denoiser

            self._denoiser = Denoiser.from_vocoder(self.vocoder)
        dn = self._denoiser
        if wav.shape[1] < dn.min_samples:
            return wav
        if counts is None:
            return dn(wav, None, strength)
        keep = [b for b, n in enumerate(counts) if n >= dn.min_samples]
        if len(keep) == len(counts):
            return dn(wav, counts, strength)
        if not keep:
            return wav
        out = wav.clone()
        out[keep] = dn(wav[keep], [counts[b] for b in keep], strength)
        return out

    def _vocode_and_track(self, mel: torch.Tensor, frames, sampling_rate: Optional[int], pitch: bool, control: Optional[Dict] = None,
                          denoise: float = 0.0):
        """``_vocode`` with the pitch contour of what it made: ``(waveforms, sample counts or None, f0 or None)``.  The waveform is
        vocoded at the model's rate, tracked there when ``pitch`` asks (``metrics.pitch_track`` with the model's hop, every row at
        its own sample count; frame 0 centred on sample ``-TRIM`` of a Griffin-Lim waveform, which lost ``TRIM`` samples at its
        head, and on sample 0 of a neural vocoder's), and only then resampled by ``AudioProcessor.deliver_at`` - the launches of
        ``convert_mel2wav_batch(..., out_rate=...)``, so tracking changes no bit of what is delivered.  f0 is float32 [B, T] on the
        device, one value per frame of ``mel``: Hz, 0 for an unvoiced frame and behind a row's own frames.

        ``control`` (pitch control; None: nothing of it runs) is ``{"ratios": float32 [B, T] on the host, the factor on the pitch of
        every frame that the shifts in semitones ask for (``frame_ratios``), "range": float}``.  The vocoded waveform is then
        tracked, repitched at the model's rate by ``metrics.pitch_shift`` - ratio per frame = that table times, for a ``range``
        other than 1, 2 ** ((range - 1) * (log2 f0 - the row's mean log2 f0 over its voiced frames)) on the voiced frames, clamped
        to [0.5, 2], torch operations on the device - and tracked again when ``pitch`` asks, so that f0 is the contour of what is
        delivered.  A fourth value is returned: the ratios applied, float32 [B, T] on the device (1 where the waveform has no
        frame), or None.

        ``denoise`` > 0 (a vocoder model only): the vocoded waveform goes through ``_denoise`` directly behind ``vocode``, before
        tracking, pitch control and resampling, so that f0 and the pitch control see what is delivered."""
        ap = self.audio_processor
        if self.vocoder is None:
            if frames is None:
                wav, counts = ap.convert_mel2wav_batch(mel), None
            else:
                wav, counts = ap.convert_mel2wav_batch(mel, mel_lengths=frames)
            first_centre = -ap.TRIM
        else:
            host = None if frames is None else [int(t) for t in (frames.tolist() if isinstance(frames, torch.Tensor) else frames)]
            wav = self.vocoder.vocode_utterances(mel.contiguous(), host)
            counts = None if host is None else self.vocoder.sample_counts(host)
            if host is None and self.vocoder.sample_counts(int(mel.shape[2])) != wav.shape[1]:   # a model that delivers fewer than T * hop samples
                wav = wav[:, :self.vocoder.sample_counts(int(mel.shape[2]))].contiguous()
            if denoise > 0.0:
                wav = self._denoise(wav, counts, denoise)
            first_centre = 0
        f0 = ratios = None
        if pitch or control is not None:
            from . import metrics

            T = mel.shape[2]
            fit = lambda t, fill=0.0: t[:, :T] if t.shape[1] >= T else torch.nn.functional.pad(t, (0, T - t.shape[1]), value=fill)
            grid = dict(sampling_rate=int(ap.config.sampling_rate), hop_length=int(ap.config.hop_length), first_centre=first_centre)
            lengths = None if counts is None else torch.tensor(counts, dtype=torch.int32, device=self.device)
            tracked = metrics.pitch_track(wav, lengths, **grid)
            if control is not None:
                F = tracked["f0"].shape[1]
                ratio = torch.from_numpy(np.ascontiguousarray(control["ratios"], dtype=np.float32)).to(self.device)   # [B, T]
                ratio = ratio[:, :F] if F <= T else torch.nn.functional.pad(ratio, (0, F - T), value=1.0)
                if control["range"] != 1.0:
                    ratio = ratio * self._range_ratios(tracked["f0"], float(control["range"]))
                ratio = ratio.clamp(metrics.PSOLA_RATIO_MIN, metrics.PSOLA_RATIO_MAX).contiguous()
                wav = metrics.pitch_shift(wav, lengths, tracked["lag"], ratio, **grid)["wav"].to(wav.dtype)   # float32 inside; the vocoder's dtype is kept
                ratios = fit(ratio, 1.0)
                if pitch:
                    tracked = metrics.pitch_track(wav, lengths, **grid)
            if pitch:
                f0 = fit(tracked["f0"])
        wav, counts = ap.deliver_at(wav, counts, sampling_rate)
        return wav, counts, f0, ratios

    @staticmethod
    def _range_ratios(f0: torch.Tensor, pitch_range: float) -> torch.Tensor:
        """The ratio per frame that scales every voiced frame's distance from its row's mean log-F0 by ``pitch_range``: f0 is float32
        [B, F] on the device, Hz, 0 where unvoiced.  The mean is a sum of integers (log2 f0 in units of 2^-20 octave), so a row has
        the same mean whatever batch it is in; unvoiced frames and rows without a voiced frame get 1."""
        voiced = f0 > 0
        logf = torch.where(voiced, torch.log2(torch.where(voiced, f0, torch.ones_like(f0))), torch.zeros_like(f0))
        total = (logf.to(torch.float64) * 2.0 ** 20).round().to(torch.int64).sum(dim=1, keepdim=True)
        count = voiced.sum(dim=1, keepdim=True)
        mean = (total.to(torch.float64) / count.clamp(min=1).to(torch.float64) / 2.0 ** 20).to(torch.float32)
        return torch.where(voiced, torch.exp2((pitch_range - 1.0) * (logf - mean)), torch.ones_like(f0))

    @staticmethod
    def _check_pitch_control(pitch_shift, pitch_range) -> Tuple[float, float]:
        pitch_shift = _check_semitones(pitch_shift, "pitch_shift")
        if abs(pitch_shift) > PITCH_MAX_SEMITONES:
            raise ValueError(f"pitch_shift = {pitch_shift} is outside [-{PITCH_MAX_SEMITONES}, {PITCH_MAX_SEMITONES}] semitones")
        if isinstance(pitch_range, bool) or not isinstance(pitch_range, (int, float, np.integer, np.floating)) or not math.isfinite(pitch_range) \
                or pitch_range < 0:
            raise ValueError(f"pitch_range must be a finite number >= 0, not {pitch_range!r}")
        return pitch_shift, float(pitch_range)

    @staticmethod
    def _sentence_semitones(token_strs: Sequence[str], word_pitch, pitch_shift: float, name: str) -> List[float]:
        """One shift per token of a sentence, on top of ``pitch_shift``: ``token_semitones`` of ``word_pitch``, each sum within an octave."""
        per_token = token_semitones(token_strs, word_pitch)
        for tok, semis in zip(token_strs, per_token):
            if abs(pitch_shift + semis) > PITCH_MAX_SEMITONES:
                raise ValueError(f"{name}: pitch_shift {pitch_shift} plus {semis} semitones on the word of {tok!r} is outside "
                                 f"[-{PITCH_MAX_SEMITONES}, {PITCH_MAX_SEMITONES}]")
        return per_token

    @staticmethod
    def _ratio_rows(starts, statuses, n_frames: int, per_token: Sequence[Sequence[float]], pitch_shift: float) -> np.ndarray:
        """The factor on the pitch of every frame, float32 [rows, n_frames]: ``frame_ratios`` of every row's shifts per token on top
        of ``pitch_shift`` (``starts``: first frames of the tokens per row, ``statuses``: of the search that found them; None, or a
        row whose search was infeasible: ``pitch_shift`` alone)."""
        table = np.full((len(per_token), n_frames), semitones_to_ratio(pitch_shift), dtype=np.float32)
        if starts is not None:
            for r, row in enumerate(per_token):
                if statuses[r] == 0:
                    table[r] = frame_ratios(starts[r][:len(row)], n_frames, row, pitch_shift)
        return table

    @staticmethod
    def _pitch_keys(f0: np.ndarray) -> Dict:
        """The two pitch keys of one sentence from its contour on the host."""
        f0 = np.ascontiguousarray(f0, dtype=np.float32)
        return {"f0": f0, "voiced_fraction": float((f0 > 0).mean()) if len(f0) else 0.0}

    @staticmethod
    def _sentence_rates(token_strs: Sequence[str], word_speed, token_speed) -> List[float]:
        """One rate per token of a sentence: ``token_rates`` of ``word_speed`` times ``token_speed`` (a sequence per token, or None)."""
        rates = token_rates(token_strs, word_speed)
        if token_speed is not None:
            per_token = list(token_speed)
            if len(per_token) != len(token_strs):
                raise ValueError(f"{len(per_token)} token rates for a sentence of {len(token_strs)} tokens")
            rates = [a * _check_rate(b, f"the rate of token {l}") for l, (a, b) in enumerate(zip(rates, per_token))]
        return rates

    @staticmethod
    def _check_speed(speed) -> float:
        speed = _check_rate(speed, "speed")
        if not RATE_MIN <= speed <= RATE_MAX:
            raise ValueError(f"speed = {speed} is outside [{RATE_MIN}, {RATE_MAX}]")
        return speed

    def _rate_control(self, outputs: Dict[str, torch.Tensor], frames: Optional[torch.Tensor], token_lengths: Optional[torch.Tensor],
                      speed: float, rates: Sequence[Sequence[float]], names: Sequence[str]):
        """The rate-controlled mel of a decoded batch, on the device: monotonic alignment search over the alignments already there,
        the plan at ``speed`` times the rows' per-token ``rates`` (``metrics.scale_durations``), the token-wise time warp of
        ``mel_outputs_postnet`` (``metrics.time_warp``).  A row whose search is infeasible (fewer frames than tokens) is warped as
        one token of all its frames at ``speed`` alone.  Returns ``(mel [B, M, max T'], T' int32 [B] on the device, host)``, host =
        per row (target start frames, status of the search, T') from one small copy.  A row the plan refuses raises ValueError with
        its name from ``names``."""
        from . import metrics

        mel, a = outputs["mel_outputs_postnet"], outputs["alignments"]
        B, L, dev = a.shape[0], a.shape[2], a.device
        al = metrics.monotonic_align(a, frames, token_lengths)
        feasible = al["status"] == 0
        Tb = frames.to(torch.int32) if frames is not None else torch.full((B,), a.shape[1], dtype=torch.int32, device=dev)
        Lb = token_lengths.to(torch.int32) if token_lengths is not None else torch.full((B,), L, dtype=torch.int32, device=dev)
        whole = torch.zeros(B, L, dtype=torch.int32, device=dev)
        whole[:, 0] = Tb
        table = torch.ones(B, L, dtype=torch.float32)
        for r, row in enumerate(rates):
            table[r, :len(row)] = torch.tensor(row, dtype=torch.float32)
        durations = torch.where(feasible[:, None], al["durations"], whole)
        n_tokens = torch.where(feasible, Lb, torch.ones_like(Lb))
        table = torch.where(feasible[:, None], table.to(dev), torch.ones((), dtype=torch.float32, device=dev))
        plan = metrics.scale_durations(durations, n_tokens, speed, table)
        host = torch.cat([plan["starts"], al["status"][:, None], plan["status"][:, None], plan["out_lengths"][:, None]], dim=1).cpu().tolist()
        for r, row in enumerate(host):
            if row[-2] != 0:
                raise ValueError(f"{names[r]}: the rate plan is {metrics.WARP_STATUS_NAMES[row[-2]]} - speed {speed} times a token's rate "
                                 f"is outside [{RATE_MIN}, {RATE_MAX}], or the result is longer than the warp's limit of frames")
        warped = metrics.time_warp(mel, durations, plan["durations"], n_tokens, T_out=max(row[-1] for row in host))
        return warped["mel"], plan["out_lengths"], [(row[:-3], row[-3], row[-1]) for row in host]

    def tts(self, text: str, sampling_rate: Optional[int] = None, diagnostics: bool = False,
            attention_window: Optional[Tuple[int, int]] = None, timings: bool = False, speed: float = 1.0,
            word_speed=None, token_speed=None, pitch: bool = False, pitch_shift: float = 0.0, word_pitch=None,
            pitch_range: float = 1.0, denoise: float = 0.0) -> Dict[str, np.ndarray]:
        """``sampling_rate`` (Hz; default: the model's): the waveform is resampled on the device before it is copied to the host,
        and ``"sampling_rate"`` of the result is the rate delivered.  ``diagnostics``: the result gains ``"alignment_stats"``
        (focus, monotonic_fraction, max_jump, coverage, first_pos, last_pos of the sentence's alignment, as Python numbers) and
        ``"stopped"`` (did the gate fire before max_decoder_steps?): a collapsed attention or a run-away decode shows without
        looking at a picture.  Every other key is what it is without them.  ``attention_window`` = (back, ahead): decode with
        the monotonic attention window of ``Tacotron2.inference`` - for a checkpoint that skips, repeats or wanders on this text;
        the result gains ``"attention_centres"`` (the token every frame attended most) and, with ``diagnostics``,
        ``"attention_window"`` records the window used (without a window the result has neither key).  ``timings``: the result
        gains ``"token_timings"`` - one ``(token, start_s, end_s)`` per input token, from a monotonic alignment search over the
        sentence's alignment (``metrics.monotonic_align``), in seconds of the delivered waveform whatever its rate, each token
        ending where the next starts and the last at the waveform's end - ``"word_timings"`` (``group_words`` of them) and
        ``"timings_status"``: ``"ok"``, or ``"infeasible"`` with both lists empty when the decode stopped with fewer frames than
        tokens.  ``speed`` (in [0.125, 8]; 2 = twice as fast), ``word_speed`` (one rate per word, or ``{word_index: rate}``: see
        ``token_rates``) and ``token_speed`` (one rate per token) set the speaking rate: token l is spoken ``speed`` times its
        word's rate times its own rate as fast.  With all three at their defaults nothing changes.  Otherwise the decoded mel is
        warped along time token by token on the device (the search of ``timings``, ``metrics.scale_durations``,
        ``metrics.time_warp``) and the waveform is vocoded from the warped mel: the result gains ``"mel_outputs_warped"``
        [n_mels, T'] and ``"speed"``, every other mel, gate and alignment key is the decode as it was, and ``timings`` are read off
        the plan's own frame counts - exact for the delivered waveform.  A decode with fewer frames than tokens is warped as a whole
        at ``speed``; a rate outside [0.125, 8] after multiplication, or a result above 32768 frames, raises ValueError.
        ``pitch``: the result gains ``"f0"`` - float32 [frames], Hz, 0 for an unvoiced frame, one value per frame of the mel that was
        vocoded (the warped one under rate control), tracked on the device on the model-rate waveform before any resampling
        (``metrics.pitch_track``, YIN) - and ``"voiced_fraction"``; with ``timings`` and an ``"ok"`` status also ``"token_pitch"``: one
        ``(token, mean_hz or None, voiced_fraction)`` per token over the token's frames (``token_pitch``).  Without ``pitch`` every
        key and every bit is what it is today.  ``pitch_shift`` (semitones; 12 = an octave up), ``word_pitch`` (semitones per word, or
        ``{word_index: semitones}``: see ``token_semitones``; on top of ``pitch_shift``, each sum within +-12) and ``pitch_range`` (>= 0:
        every voiced frame's distance from the sentence's mean log-F0 is scaled by it - 0 is monotone, 2 twice as lively) set the
        pitch.  With all three at their defaults nothing changes and no launch is added.  Otherwise the vocoded waveform is tracked
        and repitched on the device at the model's rate, before any resampling (``metrics.pitch_shift``, TD-PSOLA: the duration and
        every sample count stay, so ``timings`` are what they are without it; a word's frames are those of the search of
        ``timings``, or of the rate plan): the result gains ``"pitch_shift"`` and ``"pitch_ratio"`` - float32 [frames], the factor on
        the pitch applied to every frame of the vocoded mel, clamped to [0.5, 2] - and ``pitch`` reports the contour of the shifted
        waveform.  ``denoise`` (>= 0; needs a vocoder model, Griffin-Lim has no bias to subtract): above 0 the vocoded waveform
        goes through the vocoder's ``Denoiser`` at that strength - ``Denoiser.from_vocoder`` at its defaults, made on first use and
        kept - at the model's rate, before pitch tracking, pitch control and resampling, and the result gains ``"denoise"``: the
        strength.  A waveform of fewer than 513 samples passes through unchanged.  At 0 nothing changes and no launch is added."""
        denoise = _check_denoise(denoise, self.vocoder is not None)
        token_strs = self.text_processor.tokenize(text)
        paced = speed != 1.0 or word_speed is not None or token_speed is not None
        if paced:
            speed = self._check_speed(speed)
            rates = [self._sentence_rates(token_strs, word_speed, token_speed)]
        repitched = pitch_shift != 0.0 or word_pitch is not None or pitch_range != 1.0
        if repitched:
            pitch_shift, pitch_range = self._check_pitch_control(pitch_shift, pitch_range)
            semis = [self._sentence_semitones(token_strs, word_pitch, pitch_shift, "sentence 0")]
        by_word = repitched and word_pitch is not None
        tokens = self.text_processor.tokens_to_indices(token_strs)
        tokens = torch.IntTensor(tokens).unsqueeze(0).to(self.device)
        inputs = {"tokens": tokens}
        if attention_window is not None:
            inputs["attention_window"] = attention_window
        outputs = self.tts_model.inference(inputs=inputs)
        extra = self._diagnose(outputs, None, None)[0] if diagnostics else {}
        if diagnostics and attention_window is not None:
            extra["attention_window"] = tuple(int(v) for v in attention_window)
        mel = outputs["mel_outputs_postnet"]
        if paced:
            mel, _, plan = self._rate_control(outputs, None, None, speed, rates, ["sentence 0"])
            aligned = ([plan[0][0]], [plan[0][1]]) if timings or by_word else None
        else:
            aligned = self._align(outputs, None, None) if timings or by_word else None
        control = None
        if repitched:
            control = {"ratios": self._ratio_rows(aligned[0] if by_word else None, aligned[1] if by_word else None, mel.shape[2], semis,
                                                  pitch_shift), "range": pitch_range}
        if not timings:
            aligned = None
        wav, _, f0, ratios = self._vocode_and_track(mel, None, sampling_rate, pitch, control, denoise)  # stays on the device until the end
        result = {key: val.squeeze(0).cpu().numpy() for key, val in outputs.items()}
        result["waveform"] = wav[0].cpu().numpy()
        result["sampling_rate"] = self._out_rate(sampling_rate)
        if self.vocoder is not None:
            result["vocoder"] = self.vocoder.model_name
        result.update(extra)
        if paced:
            result["mel_outputs_warped"] = mel[0].cpu().numpy()
            result["speed"] = speed
        if aligned is not None:
            result.update(self._timings(token_strs, aligned[0][0], aligned[1][0], mel.shape[2], wav.shape[1], result["sampling_rate"]))
        if f0 is not None:
            result.update(self._pitch_keys(f0[0].cpu().numpy()))
            if aligned is not None and result["timings_status"] == "ok":
                per_token = token_pitch(aligned[0][0][:len(token_strs)], mel.shape[2], result["f0"])
                result["token_pitch"] = [(tok, hz, share) for tok, (hz, share) in zip(token_strs, per_token)]
        if ratios is not None:
            result["pitch_shift"] = pitch_shift
            result["pitch_ratio"] = ratios[0].cpu().numpy()
        if denoise > 0.0:
            result["denoise"] = denoise
        return result

    def tts_batch(self, texts: Sequence[str], batch_size: int = 32, sampling_rate: Optional[int] = None,
                  diagnostics: bool = False, attention_window: Optional[Tuple[int, int]] = None,
                  timings: bool = False, speed: float = 1.0, word_speed=None, token_speed=None,
                  pitch: bool = False, pitch_shift: float = 0.0, word_pitch=None,
                  pitch_range: float = 1.0, denoise: float = 0.0) -> List[Dict[str, np.ndarray]]:
        """Many sentences per call: one dict per sentence, in input order, with the keys, dtypes and shapes ``tts(text)`` gives
        for that sentence (every row trimmed to its own frames, tokens and samples).  Sentences are decoded as padded batches of
        at most ``batch_size`` rows of similar token length (``plan_tts_batches``) and vocoded at their own lengths in one ragged
        Griffin-Lim call per batch; the mels stay on the device in between.  A batch of one sentence is exactly the ``tts`` path,
        torch RNG draws included.  ``sampling_rate`` as in ``tts``: every row is resampled at its own sample count.
        ``diagnostics`` as in ``tts``: every sentence's alignment at its own frames and tokens.  ``attention_window`` as in
        ``tts``: every sentence is decoded with it and carries its own ``"attention_centres"``.  ``timings`` as in ``tts``: every
        sentence aligned at its own frames and tokens, timed against its own waveform.  ``speed`` as in ``tts``, for every
        sentence; ``word_speed`` and ``token_speed`` are lists with one entry per sentence, each as in ``tts`` (None: no rates
        for that sentence): every sentence is warped at its own frames, tokens and rates and vocoded at its own new length.
        ``pitch`` as in ``tts``: every sentence's waveform is tracked at its own sample count, in one call per batch.
        ``pitch_shift`` and ``pitch_range`` as in ``tts``, for every sentence; ``word_pitch`` is a list with one entry per sentence,
        each as in ``tts`` (None: no word of that sentence is named): every sentence is repitched at its own sample count, around its
        own mean pitch, in one plan and one synthesis call per batch.  ``denoise`` as in ``tts``, for every sentence: one ragged call
        per batch, every sentence at its own sample count."""
        denoise = _check_denoise(denoise, self.vocoder is not None)
        token_strs = [self.text_processor.tokenize(t) for t in texts]
        token_lists = [self.text_processor.tokens_to_indices(toks) for toks in token_strs]
        paced = speed != 1.0 or word_speed is not None or token_speed is not None
        if paced:
            speed = self._check_speed(speed)
            for what, per in (("word_speed", word_speed), ("token_speed", token_speed)):
                if per is not None and len(per) != len(token_strs):
                    raise ValueError(f"{what} has {len(per)} entries for {len(token_strs)} sentences")
            rates = [self._sentence_rates(toks, word_speed[i] if word_speed is not None else None,
                                          token_speed[i] if token_speed is not None else None) for i, toks in enumerate(token_strs)]
        repitched = pitch_shift != 0.0 or word_pitch is not None or pitch_range != 1.0
        if repitched:
            pitch_shift, pitch_range = self._check_pitch_control(pitch_shift, pitch_range)
            if word_pitch is not None and len(word_pitch) != len(token_strs):
                raise ValueError(f"word_pitch has {len(word_pitch)} entries for {len(token_strs)} sentences")
            semis = [self._sentence_semitones(toks, word_pitch[i] if word_pitch is not None else None, pitch_shift, f"sentence {i}")
                     for i, toks in enumerate(token_strs)]
        by_word = repitched and word_pitch is not None
        results: List[Dict[str, np.ndarray]] = [{} for _ in token_lists]
        for idx, tokens, lens in plan_tts_batches(token_lists, batch_size):
            inputs = {"tokens": tokens.to(self.device)}
            if len(idx) > 1:
                inputs["token_lengths"] = lens.to(self.device)
            if attention_window is not None:
                inputs["attention_window"] = attention_window
            outputs = self.tts_model.inference(inputs=inputs)
            mel = outputs["mel_outputs_postnet"]
            extras = self._diagnose(outputs, outputs.get("mel_lengths"), inputs.get("token_lengths")) if diagnostics else None
            warped = None
            if paced:
                warped, new_frames, plan = self._rate_control(outputs, outputs.get("mel_lengths"), inputs.get("token_lengths"), speed,
                                                              [rates[i] for i in idx], [f"sentence {i}" for i in idx])
                aligned = ([p[0] for p in plan], [p[1] for p in plan]) if timings or by_word else None
                new_frames_host = [p[2] for p in plan]
            else:
                aligned = self._align(outputs, outputs.get("mel_lengths"), inputs.get("token_lengths")) if timings or by_word else None
            vocoded = mel if warped is None else warped
            control = None
            if repitched:
                control = {"ratios": self._ratio_rows(aligned[0] if by_word else None, aligned[1] if by_word else None, vocoded.shape[2],
                                                      [semis[i] for i in idx], pitch_shift), "range": pitch_range}
            if not timings:
                aligned = None
            if len(idx) > 1:
                frames = outputs.pop("mel_lengths")
                wav, samples, f0, ratios = self._vocode_and_track(vocoded, frames if warped is None else new_frames, sampling_rate, pitch, control,
                                                                          denoise)
                frames = frames.tolist()
            else:
                wav, _, f0, ratios = self._vocode_and_track(vocoded, None, sampling_rate, pitch, control, denoise)
                frames, samples = [mel.shape[2]], [wav.shape[1]]
            if f0 is not None:
                f0 = f0.cpu().numpy()
            if ratios is not None:
                ratios = ratios.cpu().numpy()
            host = {key: val.cpu().numpy() for key, val in outputs.items()}
            if warped is not None:
                warped = warped.cpu().numpy()
            wav = wav.cpu().numpy()
            for r, i in enumerate(idx):
                t, n_tok = frames[r], int(lens[r])
                results[i] = {"mel_outputs": host["mel_outputs"][r, :, :t].copy(),
                              "mel_outputs_postnet": host["mel_outputs_postnet"][r, :, :t].copy(),
                              "gate_outputs": host["gate_outputs"][r, :t].copy(),
                              "alignments": host["alignments"][r, :t, :n_tok].copy(),
                              "waveform": wav[r, :samples[r]].copy(),
                              "sampling_rate": self._out_rate(sampling_rate)}
                if self.vocoder is not None:
                    results[i]["vocoder"] = self.vocoder.model_name
                if attention_window is not None:
                    results[i]["attention_centres"] = host["attention_centres"][r, :t].copy()
                if extras is not None:
                    results[i].update(extras[r])
                    if attention_window is not None:
                        results[i]["attention_window"] = tuple(int(v) for v in attention_window)
                if warped is not None:
                    t = new_frames_host[r]   # the frames of the delivered waveform
                    results[i]["mel_outputs_warped"] = warped[r, :, :t].copy()
                    results[i]["speed"] = speed
                if aligned is not None:
                    results[i].update(self._timings(token_strs[i], aligned[0][r], aligned[1][r], t, samples[r], self._out_rate(sampling_rate)))
                if f0 is not None:
                    results[i].update(self._pitch_keys(f0[r, :t]))
                    if aligned is not None and results[i]["timings_status"] == "ok":
                        per_token = token_pitch(aligned[0][r][:len(token_strs[i])], t, results[i]["f0"])
                        results[i]["token_pitch"] = [(tok, hz, share) for tok, (hz, share) in zip(token_strs[i], per_token)]
                if ratios is not None:
                    results[i]["pitch_shift"] = pitch_shift
                    results[i]["pitch_ratio"] = ratios[r, :t].copy()
                if denoise > 0.0:
                    results[i]["denoise"] = denoise
        return results
