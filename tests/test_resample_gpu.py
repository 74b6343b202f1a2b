"""The resampler and the mix-down on the MI355X: every output sample against the float64 restatement (tests/resample_ref64.py)
under a rounding bound of its own, the edges of rows and blocks, bit-stability across batches, tones, and the Python surface
(``resample``, ``convert_wav2mel_batch`` / ``WavTextCollateFn`` with foreign rates, ``tts`` at a requested rate)."""
import numpy as np
import pytest
import scipy.io.wavfile
import torch

from genvox_amd import _lib
from genvox_amd import resample as rs
from genvox_amd.audio import AudioProcessor
from genvox_amd.collate import WavTextCollateFn
from genvox_amd.configs import AudioConfig
from oracle import audio_ref
from tests import resample_ref64 as ref
from tests.golden.cases import AUDIO_CASE
from tests.test_tts_batch_gpu import TEXTS, syn  # noqa: F401  (the module's Synthesizer fixture)
from tests.test_wav_frontend_cpu import peak_normalise, silence_bounds

pytestmark = pytest.mark.gpu

KINDS = {"int16": (np.int16, 0, 2.0 ** -24), "float32": (np.float32, 1, 2.0 ** -24), "float64": (np.float64, 2, 2.0 ** -53)}
SOURCES = rs.RATES


def processor(fs=AUDIO_CASE["fs"], **kw):
    c = AUDIO_CASE
    return AudioProcessor(AudioConfig(sampling_rate=fs, filter_length=c["n_fft"], hop_length=c["hop"], n_mels=c["n_mels"], mel_fmin=c["fmin"],
                                      mel_fmax=c["fmax"], log_func=c["log_func"], ref_level_db=c["ref"], **kw))


@pytest.fixture(scope="module")
def ap():
    return processor()


def signal(rng, n, kind):
    if kind == "int16":
        return rng.integers(-30000, 30001, size=n).astype(np.int16)
    return rng.uniform(-1.0, 1.0, size=n).astype(KINDS[kind][0])


def check_row(got, lengths_b, x, src, dst, kind, what):
    """Every sample of one output row: |got - want| <= (K + 2) * u * sum_k |h_k x_k| - K fused multiply-adds in ascending order
    (gamma_K), one rounding of each tap to the table's type and none of the input - then exact zeros behind the row's length."""
    up, down = rs.resample_ratio(src, dst)
    h = rs.resample_filter(up, down)
    K = rs.taps_per_phase(len(h), up)
    want, mag = ref.resample(x, h, up, down)
    n_out = rs.resampled_length(len(x), up, down)
    assert lengths_b == n_out == len(want), what
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), what
    bound = (K + 2) * KINDS[kind][2] * mag + 1e-300
    worst = np.abs(got[:n_out] - want) - bound
    assert (worst <= 0).all(), (what, int(worst.argmax()), float(worst.max()))
    assert not got[n_out:].any(), what


# ---- 6. every instantiation, every pair that reaches a model rate, both table paths -------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("dst", [16000, 22050, 44100])
def test_every_sample_against_the_restatement(kind, dst):
    ap, lib, rng = processor(dst), _lib.load(), np.random.default_rng(dst)
    paths = set()
    for src in SOURCES:
        if src == dst:
            continue
        up, down = rs.resample_ratio(src, dst)
        K = rs.taps_per_phase(len(rs.resample_filter(up, down)), up)
        staged = lib.gvx_resample_uses_lds_table(up, K, KINDS[kind][1])
        table_bytes = up * K * (8 if kind == "float64" else 4)
        assert staged in (0, 1) and (staged == 1 or table_bytes > 100 * 1024) and (staged == 0 or table_bytes < 160 * 1024)
        paths.add(staged)
        rows = [signal(rng, n, kind) for n in (1500, 1, 377)]
        out, lengths = ap.resample(rows, src)
        assert out.dtype == (torch.float64 if kind == "float64" else torch.float32) and lengths.dtype == torch.int32
        assert out.shape == (3, rs.resampled_length(1500, up, down))
        host, lens = out.cpu().numpy(), lengths.tolist()
        for b, x in enumerate(rows):
            check_row(host[b], lens[b], x, src, dst, kind, (src, dst, b))
    # 11025 -> 16000 (up = 640), 32000 / 96000 -> 22050 (100 and 296 taps per phase) and every big float64 table are read from global
    # memory; all float32 tables that reach 44 100 Hz fit the LDS
    assert paths == ({1} if dst == 44100 and kind != "float64" else {0, 1}), paths


# ---- 7. edges ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_row_and_block_edges_bounds_and_poison(ap, kind):
    """48000 -> 22050 (K = 148 taps per phase, output blocks of 4 * 294 = 1176 samples): rows of 1, K - 1, K samples, rows that end
    one output before / on / one output behind a block's end and behind two blocks, very different lengths in one call, bounds
    inside the rows, poison outside the bounds and NaN in the output buffer beforehand."""
    src, dst = 48000, 22050
    up, down, K, table = ap._resample_table(src, dst, kind == "float64")
    assert (up, down, K) == (147, 320, 148)
    block = 1176
    n_for = lambda n_out: (n_out * down) // up      # noqa: E731  the largest n with ceil(n * up / down) == n_out
    sizes = [1, K - 1, K, n_for(block - 1), n_for(block), n_for(block + 1), n_for(2 * block + 1), 7, 30000]
    assert [rs.resampled_length(n, up, down) for n in sizes[3:7]] == [block - 1, block, block + 1, 2 * block + 1]
    rng = np.random.default_rng(3)
    dtype, kind_id, _ = KINDS[kind]
    lefts = [0, 3, 0, 17, 0, 1, 250, 2, 1000]
    n_max = max(l + n for l, n in zip(lefts, sizes)) + 64
    poison = (lambda shape: np.where(rng.random(shape) < 0.5, 32767, -32767).astype(np.int16)) if kind == "int16" else (lambda shape: np.full(shape, np.nan, dtype))
    pcm = poison((len(sizes), n_max))
    rows = [signal(rng, n, kind) for n in sizes]
    for b, x in enumerate(rows):
        pcm[b, lefts[b]: lefts[b] + len(x)] = x
    bounds = torch.tensor([[l, l + n] for l, n in zip(lefts, sizes)], dtype=torch.int32, device=ap.device)
    stride = rs.resampled_length(n_max, up, down) + 5
    odt = torch.float64 if kind == "float64" else torch.float32
    out = torch.full((len(sizes), stride), float("nan"), dtype=odt, device=ap.device)
    lengths = torch.full((len(sizes),), -1, dtype=torch.int32, device=ap.device)
    x_dev = torch.from_numpy(pcm).to(ap.device)
    lib = _lib.load()
    call = lambda o, l: _lib.check(lib.gvx_wav_resample_ragged(x_dev.data_ptr(), kind_id, len(sizes), n_max, bounds.data_ptr(), up, down,  # noqa: E731
                                                                table.data_ptr(), K, o.data_ptr(), stride, l.data_ptr(), ap._stream()))
    call(out, lengths)
    host, lens = out.cpu().numpy(), lengths.tolist()
    for b, x in enumerate(rows):
        check_row(host[b], lens[b], x, src, dst, kind, (kind, b, sizes[b]))
    # 8. the call repeated, and every row alone, give the same bits
    again, l2 = torch.full_like(out, float("nan")), torch.empty_like(lengths)
    call(again, l2)
    assert torch.equal(out, again) and torch.equal(lengths, l2)
    for b, x in enumerate(rows):
        alone, la = ap.resample([x], src)
        assert la.tolist() == [lens[b]] and torch.equal(alone[0], out[b, : alone.shape[1]]), (kind, b)
    # the same rows through the Python surface with bounds
    via, lv = ap.resample(x_dev, src, sample_lengths=[n_max] * len(sizes), bounds=bounds)
    assert torch.equal(via, out[:, : via.shape[1]]) and torch.equal(lv, lengths)
    # what the call refuses, before anything is launched
    bad = lambda *a: lib.gvx_wav_resample_ragged(*a)   # noqa: E731
    args = [x_dev.data_ptr(), kind_id, len(sizes), n_max, bounds.data_ptr(), up, down, table.data_ptr(), K, out.data_ptr(), stride, lengths.data_ptr(), ap._stream()]
    for pos, val, rc in [(10, rs.resampled_length(n_max, up, down) - 1, -1), (0, None, -1), (7, None, -1), (1, 7, -1), (8, 150, -1), (8, 1028, -1),
                         (5, rs.MAX_UP + 1, -2), (6, rs.MAX_DOWN + 1, -2), (5, 0, -1)]:
        a = list(args)
        a[pos] = val
        assert bad(*a) == rc, (pos, val)
    with pytest.raises(ValueError, match="up = 22050"):
        ap.resample(rows[:1], 22051)
    torch.cuda.synchronize()
    assert torch.equal(out, again)   # none of the refused calls wrote


# ---- 9. tones -------------------------------------------------------------------------------------------------------------------------
def test_tones_keep_their_level_below_and_vanish_above_the_new_nyquist(ap):
    src, dst, n = 48000, 22050, 48000
    t = np.arange(n) / src
    low, high = np.sin(2 * np.pi * 1000.0 * t).astype(np.float32), np.sin(2 * np.pi * 15000.0 * t).astype(np.float32)
    out, lengths = ap.resample([low, high], src)
    y = out.cpu().numpy().astype(np.float64)
    assert lengths.tolist() == [22050, 22050]
    mid = slice(1000, 21000)
    m = np.arange(22050)[mid]
    assert np.abs(y[0][mid] - np.sin(2 * np.pi * 1000.0 * m / dst)).max() <= 1e-3
    assert np.abs(y[1][mid]).max() <= 10.0 ** (-90.0 / 20.0)


# ---- 10. mix-down --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["int16", "float32", "float64"])
@pytest.mark.parametrize("channels", [2, 4, 5])
def test_mixdown_is_the_float64_mean_rounded_once(ap, kind, channels):
    rng = np.random.default_rng(channels)
    frames = np.stack([signal(rng, 3001, kind) for _ in range(channels)], axis=1)
    if kind == "int16":
        frames[:4] = [[32767] * channels, [-32768] * channels, [32767, -32768] + [1] * (channels - 2), [1, 2] + [0] * (channels - 2)]
    mono, lengths = ap.resample([frames, frames[:100]], ap.config.sampling_rate)    # same rate: the mix-down alone
    assert mono.dtype == torch.float32 and lengths.tolist() == [3001, 100]
    assert np.array_equal(mono[0].cpu().numpy(), ref.mixdown(frames))
    assert np.array_equal(mono[1, :100].cpu().numpy(), ref.mixdown(frames[:100]))
    lib = _lib.load()
    x = torch.from_numpy(frames).to(ap.device)
    for c in (1, 9):
        assert lib.gvx_wav_mixdown(x.data_ptr(), KINDS[kind][1], 1, 3001, c, mono.data_ptr(), ap._stream()) == -1


# ---- 11. front-end: a mixed batch ---------------------------------------------------------------------------------------------------
def mixed_batch(rng):
    loud = lambda n: rng.integers(-20000, 20001, size=n).astype(np.int16)      # noqa: E731
    hiss = lambda n: rng.integers(-3, 4, size=n).astype(np.int16)              # noqa: E731
    a = np.concatenate([hiss(3 * 960), loud(20000), hiss(2 * 960)])                                # 48 kHz mono int16, silence at both ends
    b = np.concatenate([hiss(441), loud(6000)])                                                     # 22 050 Hz mono int16
    c = rng.uniform(-0.5, 0.5, size=(15000, 2)).astype(np.float32)                                  # 44.1 kHz stereo float32
    d = np.zeros(9000, np.int16)                                                                    # silent
    e = loud(1500)                                                                                  # 48 kHz: 690 samples at 22 050 Hz, too short
    f = np.stack([loud(12000), loud(12000)], axis=1)                                                # 48 kHz stereo int16
    return [a, b, c, d, e, f], [48000, 22050, 44100, 48000, 48000, 48000]


def expected_mel(ap, rec, rate):
    """(float64 mel of the restatement's resampling, duration, the device's own resampled signal) of one good recording."""
    mono = rec if rec.ndim == 1 else ref.mixdown(rec)
    scale = 32767.0 if rec.dtype == np.int16 else 1.0
    left, right = silence_bounds(mono if rec.ndim == 1 else (mono * np.float32(1.0 / 32767.0) if rec.dtype == np.int16 else mono), rate, ap.config.trim_dbfs,
                                 scale if rec.ndim == 1 else 1.0)
    kept = mono[left:right]
    if rate == ap.config.sampling_rate:
        y64, dev = kept.astype(np.float64), kept.astype(np.float32)
    else:
        up, down = rs.resample_ratio(rate, ap.config.sampling_rate)
        y64, _ = ref.resample(kept, rs.resample_filter(up, down), up, down)
        dev = ap.resample([mono], rate, bounds=[[left, right]])
        dev = dev[0][0, : dev[1][0].item()].cpu().numpy()
    c = AUDIO_CASE
    basis = audio_ref.mel_filter(c["fs"], c["n_fft"], c["n_mels"], c["fmin"], c["fmax"])
    return audio_ref.wav_to_mel((y64 / np.abs(y64).max()).astype(np.float32), basis, c["n_fft"], c["hop"], c["log_func"], c["ref"]), (right - left) / rate, dev


def test_mixed_batch_through_convert_wav2mel_batch_and_collate(ap, tmp_path):
    recs, rates = mixed_batch(np.random.default_rng(11))
    path = str(tmp_path / "a48k.wav")
    scipy.io.wavfile.write(path, 48000, recs[0])
    inputs = [path] + recs[1:]
    with pytest.raises(ValueError, match=r"\[3, 4\]"):
        ap.convert_wav2mel_batch(inputs, sample_rates=rates)
    mels, durations = ap.convert_wav2mel_batch(inputs, sample_rates=[0] + rates[1:], drop_bad=True)   # a path carries its own rate
    assert [m is None for m in mels] == [False, False, False, True, True, False]
    for i in (0, 1, 2, 5):
        want, duration, dev = expected_mel(ap, recs[i], rates[i])
        assert durations[i] == duration, i
        assert mels[i].shape == want.shape and np.abs(mels[i] - want).max() <= 1e-4, (i, np.abs(mels[i] - want).max())
        own = ap.wav_to_mel_ragged([dev], trim=False)[0][0]         # wav_to_mel_ragged fed with resample()'s own output: the same bits
        assert np.array_equal(mels[i], own.cpu().numpy()), i
    assert durations[3] <= 0.02 and durations[4] == 1500 / 48000
    # bad rows keep their meaning
    with pytest.raises(ValueError, match="row 3 of the batch gives no mel: .*zero"):
        ap.wav_to_mel_ragged(recs, sample_rates=rates, trim=False)
    mel, mel_lengths, gate, dropped = ap.wav_to_mel_ragged(recs, sample_rates=rates, drop_bad=True)
    assert dropped == [3, 4] and mel.shape[0] == 4 and mel_lengths.tolist() == [m.shape[1] for m in mels if m is not None]
    for k, i in enumerate((0, 1, 2, 5)):
        assert np.array_equal(mel[k, :, : mels[i].shape[1]].cpu().numpy(), mels[i]) and mel[k, :, mels[i].shape[1]:].eq(0).all()
        assert gate[k].tolist() == [0.0] * (mels[i].shape[1] - 1) + [1.0] * (mel.shape[2] - mels[i].shape[1] + 1)
    # the collate: items with "wav_rate", sorted by token count
    good = [0, 1, 2, 5]
    items = [{"tokens": torch.arange(3 + 2 * k), "wav": recs[i], "wav_rate": rates[i]} for k, i in enumerate(good)]
    del items[1]["wav_rate"]                                          # the 22 050 Hz recording: the model's rate is the default
    batch = WavTextCollateFn(ap)(items)
    assert batch["token_lengths"].tolist() == [9, 7, 5, 3]
    for row, i in enumerate(reversed(good)):
        t = mels[i].shape[1]
        assert batch["mel_lengths"][row].item() == t and np.array_equal(batch["mel_padded"][row, :, :t].cpu().numpy(), mels[i])


def test_format_audio2wav_writes_16_bit_mono_at_the_models_rate(ap, tmp_path):
    rng = np.random.default_rng(5)
    stereo = np.stack([rng.integers(-32768, 32768, size=9600).astype(np.int16)] * 2, axis=1)
    src, dst = str(tmp_path / "in.wav"), str(tmp_path / "out.wav")
    scipy.io.wavfile.write(src, 48000, stereo)
    ap.format_audio2wav(src, dst)
    fs, got = scipy.io.wavfile.read(dst)
    y, _ = ap.resample([stereo], 48000)
    assert fs == 22050 and got.dtype == np.int16 and got.shape == (4410,)
    assert np.array_equal(got, np.clip(np.round(y[0].cpu().numpy()), -32768, 32767).astype(np.int16))
    assert got.max() == 32767 or got.min() == -32768 or np.abs(got).max() > 20000          # loud noise: the rounding saturates, it does not wrap
    with open(str(tmp_path / "not.wav"), "wb") as fh:
        fh.write(b"ID3 this is no RIFF file")
    with pytest.raises(ValueError, match="not a wav file"):
        ap.format_audio2wav(str(tmp_path / "not.wav"), dst)


# ---- 12. nothing moved ----------------------------------------------------------------------------------------------------------------
def test_calls_without_the_new_arguments_are_unchanged(ap):
    rng = np.random.default_rng(12)
    rows = [rng.integers(-20000, 20001, size=n).astype(np.int16) for n in (5000, 3000, 9000)]
    base = ap.wav_to_mel_ragged(rows)
    for kw in ({"sample_rates": None}, {"sample_rates": 22050}, {"sample_rates": [22050] * 3}):
        again = ap.wav_to_mel_ragged(rows, **kw)
        assert all(torch.equal(a, b) for a, b in zip(base, again)), kw
    m0, d0 = ap.convert_wav2mel_batch(rows)
    m1, d1 = ap.convert_wav2mel_batch(rows, sample_rates=22050)
    assert d0 == d1 and all(np.array_equal(a, b) for a, b in zip(m0, m1))
    same, lengths = ap.resample(rows, 22050)
    assert lengths.tolist() == [5000, 3000, 9000] and same.dtype == torch.float32
    assert all(np.array_equal(same[b, :len(r)].cpu().numpy(), r.astype(np.float32)) for b, r in enumerate(rows))
    mel = torch.randn(2, ap.config.n_mels, 12, device=ap.device)
    w0 = ap.convert_mel2wav_batch(mel)
    assert torch.equal(w0, ap.convert_mel2wav_batch(mel, out_rate=None)) and torch.equal(w0, ap.convert_mel2wav_batch(mel, out_rate=22050))


# ---- 13. synthesis at a requested rate ------------------------------------------------------------------------------------------------
def test_tts_delivers_the_rate_asked_for(syn):  # noqa: F811
    syn.tts_model.model_config.gate_threshold = 1.0
    ap, rate = syn.audio_processor, syn.audio_processor.config.sampling_rate

    def seeded(call, *a, **kw):
        torch.manual_seed(11)
        return call(*a, **kw)

    one = seeded(syn.tts, TEXTS[1])
    for kw in ({"sampling_rate": None}, {"sampling_rate": rate}):
        same = seeded(syn.tts, TEXTS[1], **kw)
        assert same["sampling_rate"] == rate and np.array_equal(same["waveform"], one["waveform"])
    hi = seeded(syn.tts, TEXTS[1], sampling_rate=48000)
    up, down = rs.resample_ratio(rate, 48000)
    assert hi["sampling_rate"] == 48000 and hi["waveform"].dtype == np.float64
    assert hi["waveform"].shape == (rs.resampled_length(len(one["waveform"]), up, down),)
    want, _ = ap.resample([one["waveform"]], rate, 48000)
    assert want.dtype == torch.float64 and np.array_equal(hi["waveform"], want[0].cpu().numpy())
    assert np.array_equal(hi["mel_outputs_postnet"], one["mel_outputs_postnet"])
    texts = [TEXTS[0], TEXTS[3], TEXTS[1]]
    base = seeded(syn.tts_batch, texts)
    low = seeded(syn.tts_batch, texts, sampling_rate=16000)
    up, down = rs.resample_ratio(rate, 16000)
    for b, l in zip(base, low):
        assert b["sampling_rate"] == rate and l["sampling_rate"] == 16000 and l["waveform"].dtype == np.float64
        assert l["waveform"].shape == (rs.resampled_length(len(b["waveform"]), up, down),)
        want, _ = ap.resample([b["waveform"]], rate, 16000)
        assert np.array_equal(l["waveform"], want[0].cpu().numpy())
    assert all(np.array_equal(a["waveform"], b["waveform"]) for a, b in zip(base, seeded(syn.tts_batch, texts, sampling_rate=rate)))
