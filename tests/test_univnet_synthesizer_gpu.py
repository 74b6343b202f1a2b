"""GPU: Synthesizer and Denoiser with a UnivNet vocoder model.  The Tacotron2 side is the reference-format experiment of
tests/golden/ref_exp (24 mels, hop 256, 12 decoder steps); the vocoder is a random-weight UnivNetGenerator (c32, hidden 32, two dilations)
saved by the test itself, in our own form and as the published ``{"model_g": ...}`` file, weight-normalised.  The kernels themselves are
held to float64 in tests/test_univnet_gpu.py; what is held here is the wiring, and the published inference's tail padding:
``inference`` and ``Synthesizer`` vocode every utterance with ``tail_pad_frames`` frames of ``tail_pad_value`` behind its own frames and
deliver ``T_b * hop`` samples."""
import os

import numpy as np
import pytest
import torch

from genvox_amd import UnivNetConfig, UnivNetGenerator
from genvox_amd.configs import AudioConfig, BaseConfig
from genvox_amd.denoiser import Denoiser
from genvox_amd.synthesizer import Synthesizer
from genvox_amd.tacotron2 import Tacotron2
from tests import univnet_ref64 as R

pytestmark = pytest.mark.gpu
EXP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_exp")
SENTENCES = ["hello there, world.", "yes!", "a batch of sentences, each of its own length."]
OLD_KEYS = {"mel_outputs", "mel_outputs_postnet", "gate_outputs", "alignments", "waveform", "sampling_rate"}
HOP = 256
TTS = dict(tts_model_class=Tacotron2, tts_config_path=os.path.join(EXP, "config.yaml"), tts_checkpoint_path=os.path.join(EXP, "checkpoint_3.pt"))
CFG = dict(n_mels=24, noise_dim=16, kpnet_hidden_channels=32, channel_size=32, dilations=(1, 3), strides=(8, 8, 4))
PAD, PAD_VALUE = 10, -11.5129


def _audio():
    return BaseConfig.load_configs_from_file(TTS["tts_config_path"], {"audio_config": AudioConfig})["audio_config"]


@pytest.fixture(scope="module")
def syn(tmp_path_factory):
    """A Synthesizer on a UnivNet checkpoint in our own form; the published form of the same weights must load to the same values."""
    tmp = tmp_path_factory.mktemp("univnet_syn")
    cfg, ours, published = str(tmp / "vocoder.yaml"), str(tmp / "vocoder_1.pt"), str(tmp / "univ_c32_0288.pt")
    BaseConfig.write_configs_to_file(cfg, {"model_config": UnivNetConfig(**R.model_kwargs(CFG)), "audio_config": _audio()})
    sd = {k: v.detach().float() for k, v in R.Generator(CFG, seed=21).state_dict().items()}
    torch.save({"model_statedict": sd, "iteration": 1}, ours)
    normed = {}
    for k, v in sd.items():   # g = ||v||: the folded weight is v itself, up to the rounding of v * (g / ||v||)
        if k.endswith(".weight"):
            normed[k[:-len("weight")] + "weight_g"] = torch.linalg.vector_norm(v.reshape(v.shape[0], -1), dim=1).reshape(-1, *([1] * (v.dim() - 1)))
            normed[k[:-len("weight")] + "weight_v"] = v
        else:
            normed[k] = v
    torch.save({"model_g": normed, "model_d": {}, "step": 288}, published)
    s = Synthesizer(**TTS, vocoder_model_class=UnivNetGenerator, vocoder_config_path=cfg, vocoder_checkpoint_path=ours)
    pub = Synthesizer(**TTS, vocoder_model_class=UnivNetGenerator, vocoder_config_path=cfg, vocoder_checkpoint_path=published)
    got = pub.vocoder.state_dict()
    assert set(got) == set(sd) and all(torch.allclose(got[k].cpu(), v, rtol=1e-6, atol=0) for k, v in sd.items())
    return s


def _padded(mel, lens):
    """The published inference's input, by hand: ``PAD`` frames of ``PAD_VALUE`` behind every row's own frames."""
    B, M, T = mel.shape
    out = torch.full((B, M, T + PAD), float("nan"), device=mel.device)
    for b, t in enumerate(lens):
        out[b, :, :t] = mel[b, :, :t]
        out[b, :, t:t + PAD] = PAD_VALUE
    return out


def test_inference_is_vocode_on_the_hand_padded_mel_cut_to_the_rows_samples(syn):
    voc = syn.vocoder
    assert (voc.model_config.tail_pad_frames, voc.model_config.tail_pad_value) == (PAD, PAD_VALUE)
    lens = (9, 4, 1, 7)
    mel = R.random_mel(CFG, 4, 9, seed=4).to("cuda:0", torch.float32)
    for b, t in enumerate(lens):
        mel[b, :, t:] = float("nan")
    voc.manual_seed(31)
    out = voc.inference({"mel": mel, "mel_lengths": lens})
    voc.manual_seed(31)
    by_hand = voc.vocode(_padded(mel, lens), [t + PAD for t in lens])
    assert out["waveform"].shape == (4, 9 * HOP) and out["lengths"].tolist() == [t * HOP for t in lens]
    for b, t in enumerate(lens):
        assert torch.equal(out["waveform"][b, :t * HOP], by_hand[b, :t * HOP]) and not out["waveform"][b, t * HOP:].any()
        assert by_hand[b, t * HOP:(t + PAD) * HOP].abs().max() > 0   # the padding's samples exist, and are dropped
    voc.manual_seed(31)
    full = voc.inference({"mel": mel[:1]})
    assert full["lengths"].tolist() == [9 * HOP] and full["lengths"].dtype == torch.int32
    voc.manual_seed(31)
    assert torch.equal(full["waveform"][0], voc.vocode(_padded(mel[:1], lens[:1]))[0, :9 * HOP])   # no lengths: every row has T frames


def test_tts_and_tts_batch_deliver_the_padded_inference(syn, monkeypatch):
    voc = syn.vocoder
    torch.manual_seed(3)
    voc.manual_seed(1)
    res = syn.tts(SENTENCES[0])
    assert set(res) == OLD_KEYS | {"vocoder"} and res["vocoder"] == "univnet" and res["sampling_rate"] == 22050
    mel = res["mel_outputs_postnet"]
    assert mel.shape == (24, 12) and res["waveform"].shape == (12 * HOP,) and res["waveform"].dtype == np.float32
    voc.manual_seed(1)
    alone = voc.vocode(_padded(torch.from_numpy(mel)[None].to("cuda:0"), [12]))[0].cpu().numpy()
    assert np.array_equal(res["waveform"], alone[:12 * HOP]) and np.abs(res["waveform"]).max() > 0
    # the batch: the one ragged vocode it makes is recorded - the batch's own width and row order decide the noise that is drawn
    calls, vocode = [], voc.vocode

    def spy(mel, mel_lengths=None, **kw):
        calls.append((mel, voc._host_lengths(mel_lengths), vocode(mel, mel_lengths, **kw)))
        return calls[-1][2]

    monkeypatch.setattr(voc, "vocode", spy)
    torch.manual_seed(5)
    batch = syn.tts_batch(SENTENCES)
    monkeypatch.undo()
    assert len(batch) == 3 and len(calls) == 1
    padded, lens, wav = calls[0]
    assert padded.shape[2] == max(lens) and wav.shape == (3, padded.shape[2] * HOP)
    rows = list(range(3))
    for i, r in enumerate(batch):
        assert set(r) == OLD_KEYS | {"vocoder"} and r["vocoder"] == "univnet"
        mel, t = torch.from_numpy(r["mel_outputs_postnet"]).to("cuda:0"), r["mel_outputs_postnet"].shape[1]
        assert r["waveform"].shape == (t * HOP,) and r["waveform"].dtype == np.float32 and np.isfinite(r["waveform"]).all(), i
        b = next(b for b in rows if lens[b] == t + PAD and torch.equal(padded[b, :, :t], mel))   # the row of the call that is this sentence
        rows.remove(b)
        assert (padded[b, :, t:t + PAD] == PAD_VALUE).all()
        assert np.array_equal(r["waveform"], wav[b, :t * HOP].cpu().numpy()), i


def test_denoise_timings_speed_and_pitch_run(syn):
    voc = syn.vocoder
    torch.manual_seed(3)
    voc.manual_seed(1)
    plain = syn.tts(SENTENCES[0])
    torch.manual_seed(3)
    on = syn.tts(SENTENCES[0], denoise=0.1)   # the first denoise takes the bias spectrum: a vocode of its own, with noise of its own
    torch.manual_seed(3)
    voc.manual_seed(1)
    on = syn.tts(SENTENCES[0], denoise=0.1)
    assert set(on) == set(plain) | {"denoise"} and on["waveform"].shape == plain["waveform"].shape
    wav = torch.from_numpy(plain["waveform"])[None].to("cuda:0")
    assert np.array_equal(on["waveform"], syn._denoiser(wav, None, 0.1)[0].cpu().numpy())
    torch.manual_seed(3)
    voc.manual_seed(1)
    timed = syn.tts(SENTENCES[0], timings=True, pitch=True)
    assert np.array_equal(timed["waveform"], plain["waveform"]) and timed["f0"].shape == (12,) and np.isfinite(timed["f0"]).all()
    torch.manual_seed(3)
    slow = syn.tts(SENTENCES[0], speed=0.5)
    frames = slow["mel_outputs_warped"].shape[1]
    assert frames > 12 and slow["waveform"].shape == (frames * HOP,)
    torch.manual_seed(5)
    for r in syn.tts_batch(SENTENCES, timings=True, pitch=True, denoise=0.05, speed=0.8):
        assert r["waveform"].shape == (r["mel_outputs_warped"].shape[1] * HOP,) and np.isfinite(r["waveform"]).all()
    dn = Denoiser.from_vocoder(voc, frames=20, mel_value=-0.5)
    assert (dn.n_fft, dn.hop_length) == (1024, 256) and float(dn.bias.abs().max()) > 0
