"""Mirror of the reference's ``core.synthesizer.Synthesizer`` (core/synthesizer.py:9-45): config + checkpoint
loading, text -> tokens, autoregressive Tacotron2 on the GPU, mel -> waveform on the GPU."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

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


class Synthesizer:
    def __init__(self, tts_model_class, tts_config_path: str, tts_checkpoint_path: str, use_cuda: bool = True) -> None:
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
        starts, ends = token_times(start_frames[:len(token_strs)], ap.config.hop_length, ap.TRIM, ap.row_samples([n_frames])[0],
                                   ap.config.sampling_rate, n_delivered / out_rate)
        return {"token_timings": list(zip(token_strs, starts, ends)), "word_timings": group_words(token_strs, starts, ends),
                "timings_status": "ok"}

    def tts(self, text: str, sampling_rate: Optional[int] = None, diagnostics: bool = False,
            attention_window: Optional[Tuple[int, int]] = None, timings: bool = False) -> Dict[str, np.ndarray]:
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
        tokens."""
        token_strs = self.text_processor.tokenize(text)
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
        aligned = self._align(outputs, None, None) if timings else None
        wav = self.audio_processor.convert_mel2wav_batch(mel, out_rate=sampling_rate)  # stays on the device until the end
        result = {key: val.squeeze(0).cpu().numpy() for key, val in outputs.items()}
        result["waveform"] = wav[0].cpu().numpy()
        result["sampling_rate"] = self._out_rate(sampling_rate)
        result.update(extra)
        if aligned is not None:
            result.update(self._timings(token_strs, aligned[0][0], aligned[1][0], mel.shape[2], wav.shape[1], result["sampling_rate"]))
        return result

    def tts_batch(self, texts: Sequence[str], batch_size: int = 32, sampling_rate: Optional[int] = None,
                  diagnostics: bool = False, attention_window: Optional[Tuple[int, int]] = None,
                  timings: bool = False) -> List[Dict[str, np.ndarray]]:
        """Many sentences per call: one dict per sentence, in input order, with the keys, dtypes and shapes ``tts(text)`` gives
        for that sentence (every row trimmed to its own frames, tokens and samples).  Sentences are decoded as padded batches of
        at most ``batch_size`` rows of similar token length (``plan_tts_batches``) and vocoded at their own lengths in one ragged
        Griffin-Lim call per batch; the mels stay on the device in between.  A batch of one sentence is exactly the ``tts`` path,
        torch RNG draws included.  ``sampling_rate`` as in ``tts``: every row is resampled at its own sample count.
        ``diagnostics`` as in ``tts``: every sentence's alignment at its own frames and tokens.  ``attention_window`` as in
        ``tts``: every sentence is decoded with it and carries its own ``"attention_centres"``.  ``timings`` as in ``tts``: every
        sentence aligned at its own frames and tokens, timed against its own waveform."""
        token_strs = [self.text_processor.tokenize(t) for t in texts]
        token_lists = [self.text_processor.tokens_to_indices(toks) for toks in token_strs]
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
            aligned = self._align(outputs, outputs.get("mel_lengths"), inputs.get("token_lengths")) if timings else None
            if len(idx) > 1:
                frames = outputs.pop("mel_lengths")
                wav, samples = self.audio_processor.convert_mel2wav_batch(mel, mel_lengths=frames, out_rate=sampling_rate)
                frames = frames.tolist()
            else:
                wav = self.audio_processor.convert_mel2wav_batch(mel, out_rate=sampling_rate)
                frames, samples = [mel.shape[2]], [wav.shape[1]]
            host = {key: val.cpu().numpy() for key, val in outputs.items()}
            wav = wav.cpu().numpy()
            for r, i in enumerate(idx):
                t, n_tok = frames[r], int(lens[r])
                results[i] = {"mel_outputs": host["mel_outputs"][r, :, :t].copy(),
                              "mel_outputs_postnet": host["mel_outputs_postnet"][r, :, :t].copy(),
                              "gate_outputs": host["gate_outputs"][r, :t].copy(),
                              "alignments": host["alignments"][r, :t, :n_tok].copy(),
                              "waveform": wav[r, :samples[r]].copy(),
                              "sampling_rate": self._out_rate(sampling_rate)}
                if attention_window is not None:
                    results[i]["attention_centres"] = host["attention_centres"][r, :t].copy()
                if extras is not None:
                    results[i].update(extras[r])
                    if attention_window is not None:
                        results[i]["attention_window"] = tuple(int(v) for v in attention_window)
                if aligned is not None:
                    results[i].update(self._timings(token_strs[i], aligned[0][r], aligned[1][r], t, samples[r], self._out_rate(sampling_rate)))
        return results
