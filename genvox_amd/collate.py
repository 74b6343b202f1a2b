"""Mirror of the reference's ``TextMelCollateFn`` (models/tts/__init__.py:28-62): the batch layout ``Tacotron2.forward`` consumes.

Rows are sorted by token count, longest first (the reference's packed BiLSTM requires it and the kernels keep that
contract); tokens are zero padded, mels are zero padded along time, the gate target is 1 from each row's last frame on."""
from __future__ import annotations

from typing import Dict, List

import numpy as np
import torch


class TextMelCollateFn:
    def __call__(self, batch: List[Dict[str, torch.Tensor]]) -> Dict[str, torch.Tensor]:
        # same expression as the reference (models/tts/__init__.py:32) so that rows with equal token counts come out in the
        # reference's order as well
        order = [int(i) for i in np.argsort([x["tokens"].shape[0] for x in batch])[::-1]]
        n_mels = batch[0]["features"].shape[0]
        L = batch[order[0]]["tokens"].shape[0]
        T = max(x["features"].shape[1] for x in batch)
        B = len(batch)
        out = {"token_padded": torch.zeros(B, L, dtype=torch.long), "token_lengths": torch.zeros(B, dtype=torch.long),
               "mel_padded": torch.zeros(B, n_mels, T), "gate_padded": torch.zeros(B, T), "mel_lengths": torch.zeros(B, dtype=torch.long)}
        for row, i in enumerate(order):
            tok, mel = batch[i]["tokens"], batch[i]["features"]
            out["token_padded"][row, : tok.shape[0]] = tok
            out["token_lengths"][row] = tok.shape[0]
            out["mel_padded"][row, :, : mel.shape[1]] = mel
            out["gate_padded"][row, mel.shape[1] - 1:] = 1
            out["mel_lengths"][row] = mel.shape[1]
        return out


class WavTextCollateFn:
    """``TextMelCollateFn`` for items that carry the recording instead of its features: ``{"tokens", "wav"}`` (``wav`` a 1-D int16
    or floating point array) -> the same dict, same row order, dtypes and shapes.  The mel side (``mel_padded``, ``gate_padded``,
    ``mel_lengths``) comes from one ``AudioProcessor.wav_to_mel_ragged`` call - silence trimming and normalisation as the audio
    config says - and stays on the processor's device; the token side is built on the host as before.  A recording that gives no
    mel raises ``ValueError`` (the index it names is the row of the sorted batch).  An item may carry ``"wav_rate"`` (Hz) when its
    recording is not at the model's rate, and its ``wav`` may be ``(n, channels)``: such recordings are mixed down and resampled on
    the device inside the same call."""

    def __init__(self, audio_processor):
        self.audio_processor = audio_processor

    def __call__(self, batch: List[Dict]) -> Dict[str, torch.Tensor]:
        order = [int(i) for i in np.argsort([x["tokens"].shape[0] for x in batch])[::-1]]   # TextMelCollateFn's expression
        L = batch[order[0]]["tokens"].shape[0]
        B = len(batch)
        out = {"token_padded": torch.zeros(B, L, dtype=torch.long), "token_lengths": torch.zeros(B, dtype=torch.long)}
        for row, i in enumerate(order):
            tok = torch.as_tensor(batch[i]["tokens"])
            out["token_padded"][row, : tok.shape[0]] = tok
            out["token_lengths"][row] = tok.shape[0]
        rates = {}
        if any("wav_rate" in x for x in batch):
            rates["sample_rates"] = [int(batch[i].get("wav_rate", self.audio_processor.config.sampling_rate)) for i in order]
        mel, mel_lengths, gate = self.audio_processor.wav_to_mel_ragged([batch[i]["wav"] for i in order], **rates)[:3]
        out.update(mel_padded=mel, gate_padded=gate, mel_lengths=mel_lengths)
        return out
