"""GPU: the Denoiser module and Synthesizer's ``denoise``.  The kernels are held to float64 in tests/test_denoise_gpu.py; what is held
here is the wiring: the bias ``from_vocoder`` takes from small random-weight generators (the ones of the synthesizer tests) against the
restatement's magnitudes of the same hum, and ``tts`` / ``tts_batch`` with the reference-format experiment of tests/golden/ref_exp
(24 mels, hop 256, 12 decoder steps) and a random-weight HiFi-GAN vocoder."""
import copy
import os

import numpy as np
import pytest
import torch

from genvox_amd import metrics
from genvox_amd.configs import AudioConfig, BaseConfig, HiFiGANConfig, MelGANConfig
from genvox_amd.denoiser import Denoiser
from genvox_amd.hifigan import HiFiGANGenerator
from genvox_amd.melgan import MelGANGenerator
from genvox_amd.synthesizer import Synthesizer
from genvox_amd.tacotron2 import Tacotron2
from tests import denoise_ref64 as R
from tests import hifigan_ref64 as HR
from tests import melgan_ref64 as MR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EXP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_exp")
HIFI = dict(HR.V2, n_mels=24, c0=64)
MEL = dict(n_mels=24, base_channels=64, ratios=(8, 8, 2, 2), n_res=3, dil_base=3, slope=0.2)
SENTENCES = ["hello there, world.", "yes!", "a batch of sentences, each of its own length."]
TTS = dict(tts_model_class=Tacotron2, tts_config_path=os.path.join(EXP, "config.yaml"), tts_checkpoint_path=os.path.join(EXP, "checkpoint_3.pt"))
HOP = 256


def _audio():
    return BaseConfig.load_configs_from_file(TTS["tts_config_path"], {"audio_config": AudioConfig})["audio_config"]


def _generators():
    hifi = HiFiGANGenerator(HiFiGANConfig(upsample_initial_channel=HIFI["c0"]), _audio())
    hifi.load_state_dict({k: v.float() for k, v in HR.random_state(HIFI, seed=21).items()})
    mel = MelGANGenerator(MelGANConfig(base_channels=MEL["base_channels"]), _audio())
    mel.load_state_dict({k: v.float() for k, v in MR.random_state(MEL, seed=21).items()})
    return {"hifigan": hifi.to(DEV).eval(), "melgan": mel.to(DEV).eval()}


@pytest.mark.parametrize("which", ["hifigan", "melgan"])
def test_from_vocoder_takes_the_bias_of_the_hum(which):
    voc = _generators()[which]
    frames, n_fft, hop = 20, 1024, 256
    with torch.no_grad():
        hum = voc.vocode(torch.full((1, 24, frames), -0.5, dtype=torch.float32, device=DEV)).cpu()
    assert hum.shape == (1, frames * HOP) and float(hum.abs().max()) > 0
    ref = R.reference(hum, None, n_fft, hop)
    bound = R.tol(ref["err"]["mag"][0], ref["mag"][0])
    first = Denoiser.from_vocoder(voc, frames=frames, mel_value=-0.5)
    assert (first.n_fft, first.hop_length, first.strength) == (1024, 256, 0.01) and first.bias.device.type == "cuda"
    mean = Denoiser.from_vocoder(voc, n_fft=n_fft, hop_length=hop, frames=frames, mel_value=-0.5, reduce="mean", strength=0.5)
    d_first = float((first.bias.cpu().double() - ref["mag"][0, 0]).abs().max())
    d_mean = float((mean.bias.cpu().double() - ref["mag"][0].mean(dim=0)).abs().max())
    print(f"{which}: bias of frame 0 at {d_first / bound:.3f} of its bound, mean bias at {d_mean / bound:.3f}")
    assert d_first <= bound and d_mean <= bound and mean.strength == 0.5
    assert torch.equal(first.bias.cpu(), first.magnitudes(hum.to(DEV))[0, 0].cpu())
    # hop_length None is n_fft // 4, at another size too
    assert Denoiser.from_vocoder(voc, n_fft=512, frames=8).hop_length == 128
    # the state_dict carries the bias, bit for bit; a copy makes its own plan and gives the same bits
    other = Denoiser(torch.zeros(513)).to(DEV)
    other.load_state_dict(first.state_dict())
    assert torch.equal(other.bias, first.bias)
    wav = R.noise(3, 2, 3000).to(DEV)
    want = first(wav, [3000, 2100], 0.7)
    assert torch.equal(other(wav, [3000, 2100], 0.7), want)
    twin = copy.deepcopy(first)
    assert twin._handle is None and torch.equal(twin(wav, [3000, 2100], 0.7), want) and twin._handle != first._handle
    assert bool((want[1, 2100:] == 0).all()) and not torch.equal(want, first(wav, [3000, 2100]))
    lens_dev = torch.tensor([3000, 2100], dtype=torch.int32, device=DEV)
    assert torch.equal(first(wav, lens_dev, 0.7), want)


@pytest.fixture(scope="module")
def voc(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("denoise_syn")
    cfg, ckpt = str(tmp / "vocoder.yaml"), str(tmp / "vocoder_1.pt")
    BaseConfig.write_configs_to_file(cfg, {"model_config": HiFiGANConfig(upsample_initial_channel=HIFI["c0"]), "audio_config": _audio()})
    torch.save({"model_statedict": {k: v.float() for k, v in HR.random_state(HIFI, seed=21).items()}, "iteration": 1}, ckpt)
    return Synthesizer(**TTS, vocoder_model_class=HiFiGANGenerator, vocoder_config_path=cfg, vocoder_checkpoint_path=ckpt)


def test_tts_with_denoise_off_is_tts(voc):
    before = voc._denoiser
    torch.manual_seed(3)
    plain = voc.tts(SENTENCES[0])
    torch.manual_seed(3)
    off = voc.tts(SENTENCES[0], denoise=0.0)
    assert set(plain) == set(off) and "denoise" not in off and voc._denoiser is before   # nothing was made on the way
    for k in plain:
        assert np.array_equal(plain[k], off[k]), k


def test_tts_denoise_is_the_denoiser_on_the_vocoded_waveform(voc):
    torch.manual_seed(3)
    plain = voc.tts(SENTENCES[0])
    torch.manual_seed(3)
    res = voc.tts(SENTENCES[0], denoise=0.1)
    assert set(res) == set(plain) | {"denoise"} and res["denoise"] == 0.1
    for k in set(plain) - {"waveform"}:
        assert np.array_equal(plain[k], res[k]), k
    dn = voc._denoiser
    assert isinstance(dn, Denoiser) and (dn.n_fft, dn.hop_length) == (1024, 256)
    want = dn(torch.from_numpy(plain["waveform"])[None].to(DEV), None, 0.1)[0].cpu().numpy()
    assert res["waveform"].dtype == np.float32 and np.array_equal(res["waveform"], want) and not np.array_equal(want, plain["waveform"])
    # the bias is made once per Synthesizer
    torch.manual_seed(3)
    again = voc.tts(SENTENCES[0], denoise=0.1)
    assert voc._denoiser is dn and np.array_equal(again["waveform"], res["waveform"])
    ref = Denoiser.from_vocoder(voc.vocoder)
    assert torch.equal(ref.bias, dn.bias)


def test_tts_batch_rows_are_the_rows_alone(voc):
    """The rule of the vocoder's batch tests: a batch of one sentence is the tts call bit for bit under the same seed; in a batch of
    three, every row's waveform is, bit for bit, what a tts call does with the mel that row returned - vocoded alone, then denoised."""
    torch.manual_seed(5)
    one = voc.tts(SENTENCES[1], denoise=0.1)
    torch.manual_seed(5)
    got = voc.tts_batch([SENTENCES[1]], denoise=0.1)
    assert set(got[0]) == set(one) and got[0]["denoise"] == 0.1
    for k in ("mel_outputs", "mel_outputs_postnet", "gate_outputs", "alignments", "waveform"):
        assert np.array_equal(got[0][k], one[k]), k
    torch.manual_seed(5)
    batch = voc.tts_batch(SENTENCES, denoise=0.1)
    torch.manual_seed(5)
    plain = voc.tts_batch(SENTENCES)
    for i, r in enumerate(batch):
        assert set(r) == set(plain[i]) | {"denoise"} and r["denoise"] == 0.1
        frames = r["mel_outputs_postnet"].shape[1]
        assert r["waveform"].shape == (frames * HOP,) and r["waveform"].dtype == np.float32, i
        alone = voc.vocoder.vocode(torch.from_numpy(r["mel_outputs_postnet"])[None].to(DEV))
        assert np.array_equal(plain[i]["waveform"], alone[0].cpu().numpy()), i
        assert np.array_equal(r["waveform"], voc._denoiser(alone, None, 0.1)[0].cpu().numpy()), i


def test_pitch_is_tracked_on_the_denoised_waveform(voc):
    torch.manual_seed(7)
    res = voc.tts(SENTENCES[0], denoise=0.1, pitch=True)
    T = res["mel_outputs_postnet"].shape[1]
    wav = torch.from_numpy(res["waveform"])[None].to(DEV)
    f0 = metrics.pitch_track(wav, None, sampling_rate=22050, hop_length=HOP)["f0"][0, :T].cpu().numpy()
    assert res["f0"].shape == (T,) and np.array_equal(res["f0"], f0) and res["denoise"] == 0.1


def test_short_rows_pass_through(voc):
    dn_min = 513
    wav = R.noise(2, 3, 1024).to(DEV)
    counts = [1024, 512, 768]   # 2 frames of 256 are below n_fft / 2 + 1
    assert counts[1] < dn_min
    out = voc._denoise(wav, counts, 0.5)
    keep = voc._denoiser(wav[[0, 2]], [1024, 768], 0.5)
    assert torch.equal(out[1], wav[1]) and torch.equal(out[0], keep[0]) and torch.equal(out[2], keep[1])
    short = wav[:, :512].contiguous()
    assert torch.equal(voc._denoise(short, None, 0.5), short) and torch.equal(voc._denoise(short, [512, 256, 512], 0.5), short)


def test_denoise_needs_a_vocoder_model():
    plain = Synthesizer(**TTS)
    with pytest.raises(ValueError, match="Griffin-Lim has no bias"):
        plain.tts(SENTENCES[1], denoise=0.01)
    with pytest.raises(ValueError, match="Griffin-Lim has no bias"):
        plain.tts_batch(SENTENCES[:2], denoise=0.01)
    with pytest.raises(ValueError, match="denoise must be"):
        plain.tts(SENTENCES[1], denoise=True)
    torch.manual_seed(1)
    assert "denoise" not in plain.tts(SENTENCES[1], denoise=0.0)
