"""GPU: ``Synthesizer(tts_model_class=FastPitch, ...)`` with Griffin-Lim and with a small HiFi-GAN vocoder.  The model is a random-weight
FastPitch (d_model 32, 2 + 2 layers, 24 mels, ``min_token_frames`` 1) written by the test itself as a config and a checkpoint; the audio
and text sections are those of tests/golden/ref_exp.  The kernels themselves are held to float64 in tests/test_fastpitch_gpu.py; what is
held here is the wiring: ``tts`` and ``tts_batch`` return Tacotron2's keys, and diagnostics, timings and rate control run unchanged."""
import os

import numpy as np
import pytest
import torch

from genvox_amd import FastPitch, FastPitchConfig
from genvox_amd.configs import AudioConfig, BaseConfig, HiFiGANConfig, TextConfig
from genvox_amd.hifigan import HiFiGANGenerator
from genvox_amd.synthesizer import Synthesizer
from tests import fastpitch_ref64 as R
from tests import hifigan_ref64 as HR

pytestmark = pytest.mark.gpu
EXP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_exp", "config.yaml")
SENTENCES = ["hello there, world.", "yes!", "a batch of sentences, each of its own length."]
TACOTRON_KEYS = {"mel_outputs", "mel_outputs_postnet", "gate_outputs", "alignments", "waveform", "sampling_rate"}
OWN_KEYS = {"durations", "log_durations", "pitch_pred", "energy_pred"}
HOP = 256
CFG = dict(R.NARROW, n_tokens=33, n_mels=24)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fastpitch_syn")
    sections = BaseConfig.load_configs_from_file(EXP, {"audio_config": AudioConfig, "text_config": TextConfig})
    cfg, ckpt = str(tmp / "config.yaml"), str(tmp / "checkpoint_1.pt")
    BaseConfig.write_configs_to_file(cfg, {"model_config": FastPitchConfig(**R.model_kwargs(CFG), min_token_frames=1), **sections})
    sd = {"module." + k: v.float() for k, v in R.Model(CFG, seed=5).state_dict().items()}   # the published form
    torch.save({"state_dict": sd, "iteration": 1}, ckpt)
    vcfg, vckpt = str(tmp / "vocoder.yaml"), str(tmp / "vocoder_1.pt")
    BaseConfig.write_configs_to_file(vcfg, {"model_config": HiFiGANConfig(upsample_initial_channel=64), "audio_config": sections["audio_config"]})
    torch.save({"model_statedict": {k: v.float() for k, v in HR.random_state(dict(HR.V2, n_mels=24, c0=64), seed=21).items()}, "iteration": 1}, vckpt)
    return cfg, ckpt, vcfg, vckpt


@pytest.fixture(scope="module")
def gl(files):
    return Synthesizer(tts_model_class=FastPitch, tts_config_path=files[0], tts_checkpoint_path=files[1])


@pytest.fixture(scope="module")
def voc(files):
    return Synthesizer(tts_model_class=FastPitch, tts_config_path=files[0], tts_checkpoint_path=files[1], vocoder_model_class=HiFiGANGenerator,
                       vocoder_config_path=files[2], vocoder_checkpoint_path=files[3])


def test_tts_and_tts_batch_return_tacotron2s_keys(gl, voc):
    assert isinstance(gl.tts_model, FastPitch) and gl.tts_model.model_name == "FastPitch"
    for syn, extra in ((gl, set()), (voc, {"vocoder"})):
        res = syn.tts(SENTENCES[0])
        assert set(res) == TACOTRON_KEYS | OWN_KEYS | extra
        L = len(SENTENCES[0])
        T = int(res["durations"].sum())
        assert res["durations"].shape == (L,) and (res["durations"] >= 1).all() and T >= L
        assert res["mel_outputs_postnet"].shape == (24, T) and res["mel_outputs"].shape == (24, T) and res["mel_outputs_postnet"].dtype == np.float32
        assert res["gate_outputs"].shape == (T,) and res["alignments"].shape == (T, L) and res["alignments"].sum() == T
        assert res["waveform"].ndim == 1 and np.isfinite(res["waveform"]).all() and np.abs(res["waveform"]).max() > 0
        if extra:
            assert res["vocoder"] == "hifigan" and res["waveform"].shape == (T * HOP,)
        batch = syn.tts_batch(SENTENCES)
        assert len(batch) == 3
        for text, r in zip(SENTENCES, batch):
            assert set(r) == TACOTRON_KEYS | extra
            t = r["mel_outputs_postnet"].shape[1]
            assert r["mel_outputs_postnet"].shape == (24, t) and r["gate_outputs"].shape == (t,) and r["alignments"].shape == (t, len(text))
            if extra:
                assert r["waveform"].shape == (t * HOP,)
        # a batch row is the single call's mel, bit for bit
        assert np.array_equal(batch[0]["mel_outputs_postnet"], res["mel_outputs_postnet"])
        assert np.array_equal(batch[1]["mel_outputs_postnet"], syn.tts(SENTENCES[1])["mel_outputs_postnet"])


def test_timings_diagnostics_speed_and_the_refused_window(voc):
    plain = voc.tts(SENTENCES[0])
    timed = voc.tts(SENTENCES[0], timings=True, diagnostics=True, pitch=True)
    assert np.array_equal(timed["waveform"], plain["waveform"])
    assert timed["timings_status"] == "ok" and timed["stopped"] is True
    assert timed["alignment_stats"]["monotonic_fraction"] == 1.0 and timed["alignment_stats"]["max_jump"] <= 1
    starts = np.concatenate([[0], np.cumsum(plain["durations"])[:-1]])
    got = [round(s * 22050 / HOP) for _, s, _ in timed["token_timings"]]
    assert got == starts.tolist()   # the token frames are the durations
    assert len(timed["token_timings"]) == len(SENTENCES[0]) and timed["f0"].shape == (plain["mel_outputs"].shape[1],)
    slow = voc.tts(SENTENCES[0], speed=0.8)   # through the existing warp
    T = plain["mel_outputs"].shape[1]
    assert slow["mel_outputs_warped"].shape[1] > T and slow["waveform"].shape == (slow["mel_outputs_warped"].shape[1] * HOP,)
    assert np.array_equal(slow["mel_outputs_postnet"], plain["mel_outputs_postnet"])
    rows = voc.tts_batch(SENTENCES, timings=True, diagnostics=True, speed=0.8)
    assert all(r["timings_status"] == "ok" and r["stopped"] for r in rows)
    with pytest.raises(ValueError, match="attention_window"):
        voc.tts(SENTENCES[0], attention_window=(2, 4))
    with pytest.raises(ValueError, match="attention_window"):
        voc.tts_batch(SENTENCES, attention_window=(2, 4))
