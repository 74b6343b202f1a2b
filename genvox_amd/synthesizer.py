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

    def tts(self, text: str, sampling_rate: Optional[int] = None, diagnostics: bool = False,
            attention_window: Optional[Tuple[int, int]] = None) -> Dict[str, np.ndarray]:
        """``sampling_rate`` (Hz; default: the model's): the waveform is resampled on the device before it is copied to the host,
        and ``"sampling_rate"`` of the result is the rate delivered.  ``diagnostics``: the result gains ``"alignment_stats"``
        (focus, monotonic_fraction, max_jump, coverage, first_pos, last_pos of the sentence's alignment, as Python numbers) and
        ``"stopped"`` (did the gate fire before max_decoder_steps?): a collapsed attention or a run-away decode shows without
        looking at a picture.  Every other key is what it is without them.  ``attention_window`` = (back, ahead): decode with
        the monotonic attention window of ``Tacotron2.inference`` - for a checkpoint that skips, repeats or wanders on this text;
        the result gains ``"attention_centres"`` (the token every frame attended most) and, with ``diagnostics``,
        ``"attention_window"`` records the window used (without a window the result has neither key)."""
        tokens = self.text_processor.tokens_to_indices(self.text_processor.tokenize(text))
        tokens = torch.IntTensor(tokens).unsqueeze(0).to(self.device)
        inputs = {"tokens": tokens}
        if attention_window is not None:
            inputs["attention_window"] = attention_window
        outputs = self.tts_model.inference(inputs=inputs)
        extra = self._diagnose(outputs, None, None)[0] if diagnostics else {}
        if diagnostics and attention_window is not None:
            extra["attention_window"] = tuple(int(v) for v in attention_window)
        mel = outputs["mel_outputs_postnet"]
        wav = self.audio_processor.convert_mel2wav_batch(mel, out_rate=sampling_rate)  # stays on the device until the end
        result = {key: val.squeeze(0).cpu().numpy() for key, val in outputs.items()}
        result["waveform"] = wav[0].cpu().numpy()
        result["sampling_rate"] = self._out_rate(sampling_rate)
        result.update(extra)
        return result

    def tts_batch(self, texts: Sequence[str], batch_size: int = 32, sampling_rate: Optional[int] = None,
                  diagnostics: bool = False, attention_window: Optional[Tuple[int, int]] = None) -> List[Dict[str, np.ndarray]]:
        """Many sentences per call: one dict per sentence, in input order, with the keys, dtypes and shapes ``tts(text)`` gives
        for that sentence (every row trimmed to its own frames, tokens and samples).  Sentences are decoded as padded batches of
        at most ``batch_size`` rows of similar token length (``plan_tts_batches``) and vocoded at their own lengths in one ragged
        Griffin-Lim call per batch; the mels stay on the device in between.  A batch of one sentence is exactly the ``tts`` path,
        torch RNG draws included.  ``sampling_rate`` as in ``tts``: every row is resampled at its own sample count.
        ``diagnostics`` as in ``tts``: every sentence's alignment at its own frames and tokens.  ``attention_window`` as in
        ``tts``: every sentence is decoded with it and carries its own ``"attention_centres"``."""
        token_lists = [self.text_processor.tokens_to_indices(self.text_processor.tokenize(t)) for t in texts]
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
        return results
