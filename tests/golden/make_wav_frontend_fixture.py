#!/usr/bin/env python3
"""Generate tests/golden/wav_frontend.npz from the reference itself (the companion of make_fixtures.py for the ragged
wav -> mel front-end).

Runs ONLY where the reference checkout is available (the place make_fixtures.py reads it from, or $GENVOX_REFERENCE); nothing in
the product path or the tests reads it.  The reference is imported unchanged, with the same empty stand-ins for the four modules it imports but never uses on this path.  Only data is written: int16 recordings built
from audio.npz's signal with silence of different lengths in front and behind, and for each of them what the reference's
preprocessing makes of it - get_non_silent_boundary's (left, right), normalize_signal's float32 signal and the mel (dB) of the
convert_wav2mel chain.

Rows:  0 no silence            1 less than one 20 ms chunk on both sides     2 silence that is not a multiple of the chunk
       3 whole chunks          4 digital silence (zeros) around the signal   5 silence only: no chunk passes, left >= right
       6 trims to fewer than n_fft samples                                   7 all zeros
       8 trims to exactly one frame

Usage:  python tests/golden/make_wav_frontend_fixture.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("GENVOX_REFERENCE", "/root/reference")

for _name in ("yt_dlp", "inflect", "wandb", "g2p_en"):
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.modules["inflect"].engine = lambda *a, **k: None
sys.modules["g2p_en"].G2p = lambda *a, **k: None
sys.path.insert(0, REFERENCE)
sys.path.insert(1, REPO)

import configs as ref_configs  # noqa: E402  (reference)
from core.processors import AudioProcessor as RefAudioProcessor  # noqa: E402  (reference)
from utils import get_non_silent_boundary  # noqa: E402  (reference)
from utils.audio import base as ref_audio  # noqa: E402  (reference)

from tests.golden.cases import AUDIO_CASE  # noqa: E402

TRIM_DBFS = -50.0


def main():
    c = AUDIO_CASE
    ref_ac = ref_configs.AudioConfig(sampling_rate=c["fs"], filter_length=c["n_fft"], hop_length=c["hop"], n_mels=c["n_mels"],
                                     mel_fmin=c["fmin"], mel_fmax=c["fmax"], log_func=c["log_func"], ref_level_db=c["ref"],
                                     trim_dbfs=TRIM_DBFS)
    ap = RefAudioProcessor(ref_ac)
    with np.load(os.path.join(HERE, "audio.npz")) as z:
        sig = np.round(z["signal"].astype(np.float64) * 0.9 * 32767).astype(np.int16)
    rng = np.random.default_rng(c["seed"])

    def hiss(n):   # +-3 LSB: about -80 dBFS, far below the threshold
        return rng.integers(-3, 4, size=n).astype(np.int16)

    chunk = int(20 * 0.001 * c["fs"])
    rows = [
        sig,
        np.concatenate([hiss(200), sig, hiss(300)]),
        np.concatenate([hiss(1000), sig, hiss(1500)]),
        np.concatenate([hiss(2 * chunk), sig, hiss(3 * chunk)]),
        np.concatenate([np.zeros(777, np.int16), sig, np.zeros(1234, np.int16)]),
        hiss(3000),
        np.concatenate([hiss(2000), sig[4000:4500], hiss(2000)]),
        np.zeros(2500, np.int16),
        np.concatenate([hiss(2000), sig[4000:4700], hiss(2000)]),
    ]
    n_max = max(r.shape[0] for r in rows)
    out = {"fs": np.int64(c["fs"]), "trim_dbfs": np.float64(TRIM_DBFS), "pcm": np.zeros((len(rows), n_max), np.int16),
           "lengths": np.array([r.shape[0] for r in rows], np.int32), "bounds": np.zeros((len(rows), 2), np.int32),
           "has_mel": np.zeros(len(rows), np.bool_)}
    for i, r in enumerate(rows):
        out["pcm"][i, : r.shape[0]] = r
        left, right = get_non_silent_boundary(signal=r, fs=c["fs"], silence_threshold=TRIM_DBFS)
        out["bounds"][i] = (left, right)
        if right - left < c["n_fft"] or not r[left:right].any():
            continue
        norm = ref_audio.normalize_signal(r[left:right])
        spec = ref_audio.stft(norm, n_fft=c["n_fft"], hop_length=c["hop"])
        mel_db = ref_audio.amplitude_to_db(ref_audio.fft2mel(np.abs(spec), ap.mel_basis), log_func=c["log_func"], ref=c["ref"],
                                           power=False, scale=1)
        out["has_mel"][i] = True
        out[f"norm_{i}"] = norm
        out[f"mel_db_{i}"] = mel_db.astype(np.float32)
        print(f"row {i}: n {r.shape[0]} bounds ({left}, {right}) norm {norm.dtype} mel {mel_db.shape} {mel_db.dtype}")
    print("bounds", out["bounds"].tolist(), "has_mel", out["has_mel"].tolist())
    np.savez_compressed(os.path.join(HERE, "wav_frontend.npz"), **out)


if __name__ == "__main__":
    main()
