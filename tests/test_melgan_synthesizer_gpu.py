"""GPU: Synthesizer with a MelGAN vocoder model.  The Tacotron2 side is the reference-format experiment of tests/golden/ref_exp (24
mels, hop 256, 12 decoder steps); the vocoder is a random-weight MelGANGenerator saved to a temporary checkpoint in weight-normalised
form.  Waveforms are held to the float64 restatement (tests/melgan_ref64.py) of the mel the call itself returned, within 8 times the
restatement's own float32 error (the rule of tests/test_melgan_gpu.py)."""
import os

import numpy as np
import pytest
import torch

from genvox_amd import resample as rs
from genvox_amd.configs import AudioConfig, BaseConfig, MelGANConfig
from genvox_amd.melgan import MelGANGenerator
from genvox_amd.synthesizer import Synthesizer
from genvox_amd.tacotron2 import Tacotron2
from tests import melgan_ref64 as R

pytestmark = pytest.mark.gpu
EXP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_exp")
CFG = dict(n_mels=24, base_channels=64, ratios=(8, 8, 2, 2), n_res=3, dil_base=3, slope=0.2)
SENTENCES = ["hello there, world.", "yes!", "a batch of sentences, each of its own length."]
OLD_KEYS = {"mel_outputs", "mel_outputs_postnet", "gate_outputs", "alignments", "waveform", "sampling_rate"}
HOP = 256


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """(Synthesizer without a vocoder, Synthesizer with one, the vocoder's folded weights in float64)."""
    tmp = tmp_path_factory.mktemp("melgan_syn")
    tts = dict(tts_model_class=Tacotron2, tts_config_path=os.path.join(EXP, "config.yaml"), tts_checkpoint_path=os.path.join(EXP, "checkpoint_3.pt"))
    ac = BaseConfig.load_configs_from_file(tts["tts_config_path"], {"audio_config": AudioConfig})["audio_config"]
    cfg, ckpt = str(tmp / "vocoder.yaml"), str(tmp / "vocoder_1.pt")
    BaseConfig.write_configs_to_file(cfg, {"model_config": MelGANConfig(base_channels=CFG["base_channels"]), "audio_config": ac})
    sd, normed = R.random_state(CFG, seed=21), {}
    for k, v in sd.items():
        v = v.float()
        if k.endswith(".weight"):   # weight-normalised: a direction of twice the length and the weight's own norm over all axes but the first
            normed[k + "_v"] = 2.0 * v
            normed[k + "_g"] = v.reshape(v.shape[0], -1).norm(dim=1).reshape(-1, 1, 1)
        else:
            normed[k] = v
    torch.save({"model_statedict": normed, "iteration": 1}, ckpt)
    plain = Synthesizer(**tts)
    voc = Synthesizer(**tts, vocoder_model_class=MelGANGenerator, vocoder_config_path=cfg, vocoder_checkpoint_path=ckpt)
    folded = {k: v.detach().cpu().double() for k, v in voc.vocoder.state_dict().items()}
    for k in sd:
        assert (folded[k] - sd[k]).abs().max() < 1e-6   # the fold gives the weights back
    with pytest.raises(ValueError, match="all three"):
        Synthesizer(**tts, vocoder_model_class=MelGANGenerator)
    return plain, voc, folded


def _hold_to_restatement(wav, mel, folded, what):
    """wav [n] float32 from the device against the restatement of mel [M, T] (numpy)."""
    m = torch.from_numpy(np.ascontiguousarray(mel)).double()[None]
    (want, _), errs = R.reference_pair(folded, m, None, CFG)
    assert wav.shape == (mel.shape[1] * HOP,) and wav.dtype == np.float32, (what, wav.shape, wav.dtype)
    d = np.abs(wav.astype(np.float64) - want[0].numpy()).max()
    print(f"{what}: device error {d:.3e}, float32 restatement error {errs[0]:.3e}")
    assert d <= 8.0 * errs[0], f"{what}: {d:.3e} above 8 x {errs[0]:.3e}"
    assert np.abs(wav).max() < 1.0 and np.abs(wav).max() > 0


def test_tts_vocodes_the_postnet_mel(pair):
    plain, voc, folded = pair
    torch.manual_seed(3)
    res = voc.tts(SENTENCES[0])
    after_voc = torch.rand(1)
    assert set(res) == OLD_KEYS | {"vocoder"} and res["vocoder"] == "melgan" and res["sampling_rate"] == 22050
    assert res["mel_outputs_postnet"].shape == (24, 12)
    _hold_to_restatement(res["waveform"], res["mel_outputs_postnet"], folded, "tts")
    # without the vocoder arguments: the keys and the Griffin-Lim waveform of before, and the same decode and RNG draws with and without
    torch.manual_seed(3)
    old = plain.tts(SENTENCES[0])
    after_plain = torch.rand(1)
    assert set(old) == OLD_KEYS and torch.equal(after_voc, after_plain)
    for k in OLD_KEYS - {"waveform", "sampling_rate"}:
        assert np.array_equal(old[k], res[k]), k
    griffin_lim = plain.audio_processor.convert_mel2wav_batch(torch.from_numpy(old["mel_outputs_postnet"])[None])[0].cpu().numpy()
    assert old["waveform"].dtype == np.float64 and old["waveform"].shape == (1024 + 11 * HOP - 1000,)
    assert np.array_equal(old["waveform"], griffin_lim)


def test_tts_batch_rows_are_the_rows_alone(pair):
    """A batch of one sentence is the tts call, bit for bit, under the same seed.  In a batch of three sentences of different token
    lengths a padded row's mel depends on its padding and on the batch's dropout draws (as in the reference), so what is held is
    the hand-over: every row has the keys and shapes of tts, and its waveform is, bit for bit, the vocoder run alone on the mel that
    row returned - what a tts call does with that mel - and within tolerance of the restatement."""
    _, voc, folded = pair
    torch.manual_seed(5)
    one = voc.tts(SENTENCES[1])
    torch.manual_seed(5)
    got = voc.tts_batch([SENTENCES[1]])
    assert set(got[0]) == set(one)
    for k in OLD_KEYS - {"sampling_rate"}:
        assert np.array_equal(got[0][k], one[k]), k
    torch.manual_seed(5)
    batch = voc.tts_batch(SENTENCES)
    assert len(batch) == 3
    for i, r in enumerate(batch):
        assert set(r) == OLD_KEYS | {"vocoder"} and r["vocoder"] == "melgan"
        mel = torch.from_numpy(r["mel_outputs_postnet"])[None].to("cuda:0")
        alone = voc.vocoder.vocode(mel)[0].cpu().numpy()
        assert np.array_equal(r["waveform"], alone), i
        _hold_to_restatement(r["waveform"], r["mel_outputs_postnet"], folded, f"tts_batch row {i}")


def test_timings_on_the_untrimmed_waveform(pair):
    _, voc, _ = pair
    for rate in (None, 16000):
        torch.manual_seed(7)
        res = voc.tts("hi there.", timings=True, sampling_rate=rate)
        assert res["timings_status"] == "ok"
        out_rate = 22050 if rate is None else rate
        assert res["token_timings"][-1][2] == len(res["waveform"]) / out_rate
        from genvox_amd import metrics

        a = torch.from_numpy(res["alignments"])[None].to("cuda:0")
        starts = metrics.monotonic_align(a, None, None)["starts"][0].tolist()
        assert [t[1] for t in res["token_timings"]] == [f * HOP / 22050 for f in starts[:len(res["token_timings"])]]
        assert res["token_timings"][0][1] == 0.0
    torch.manual_seed(7)
    rows = voc.tts_batch(["hi there.", "yes!"], timings=True)
    for r in rows:
        assert r["timings_status"] == "ok" and r["token_timings"][-1][2] == len(r["waveform"]) / 22050


def test_speed_vocodes_the_warped_mel(pair):
    _, voc, folded = pair
    torch.manual_seed(9)
    res = voc.tts(SENTENCES[0], speed=0.8)
    warped = res["mel_outputs_warped"]
    assert warped.shape == (24, 15) and res["speed"] == 0.8 and res["vocoder"] == "melgan"
    _hold_to_restatement(res["waveform"], warped, folded, "speed 0.8")
    torch.manual_seed(9)
    rows = voc.tts_batch(SENTENCES[:2], speed=0.8)
    for i, r in enumerate(rows):
        _hold_to_restatement(r["waveform"], r["mel_outputs_warped"], folded, f"speed 0.8 row {i}")


def test_sampling_rate_delivers_the_resampled_length(pair):
    _, voc, _ = pair
    up, down = rs.resample_ratio(22050, 16000)
    torch.manual_seed(3)
    res = voc.tts(SENTENCES[0], sampling_rate=16000)
    assert res["sampling_rate"] == 16000 and res["waveform"].shape == (rs.resampled_length(12 * HOP, up, down),)
    assert res["waveform"].dtype == np.float32 and np.isfinite(res["waveform"]).all() and np.abs(res["waveform"]).max() > 0
    torch.manual_seed(3)
    rows = voc.tts_batch(SENTENCES, sampling_rate=16000)
    for r in rows:
        assert r["waveform"].shape == (rs.resampled_length(r["mel_outputs_postnet"].shape[1] * HOP, up, down),)
