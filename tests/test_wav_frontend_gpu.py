"""The ragged wav -> mel front-end on the MI355X: silence bounds, peak normalisation fused into the STFT, mel, dB and the batch
tail (zero padding, gate target, frame counts) of many recordings in one call - against the reference-generated fixture
tests/golden/wav_frontend.npz, against ``wav_to_mel`` on every row alone (bit for bit), and through ``WavTextCollateFn`` into
``Tacotron2.forward`` / ``train_step``."""
import numpy as np
import pytest
import torch

from genvox_amd import weights as gw
from genvox_amd.audio import AudioProcessor, keep_by_duration
from genvox_amd.collate import TextMelCollateFn, WavTextCollateFn
from genvox_amd.configs import AudioConfig
from genvox_amd.tacotron2 import Tacotron2
from tests.golden.cases import AUDIO_CASE, TRAIN_CASE, case_configs
from tests.helpers import load_fixture
from tests.test_wav_frontend_cpu import frames_of, peak_normalise, silence_bounds

pytestmark = pytest.mark.gpu

CHUNK = int(20 * 0.001 * AUDIO_CASE["fs"])


def processor(n_fft=AUDIO_CASE["n_fft"], hop=AUDIO_CASE["hop"], n_mels=AUDIO_CASE["n_mels"], **kw):
    c = AUDIO_CASE
    return AudioProcessor(AudioConfig(sampling_rate=c["fs"], filter_length=n_fft, hop_length=hop, n_mels=n_mels, mel_fmin=c["fmin"],
                                      mel_fmax=c["fmax"], log_func=c["log_func"], ref_level_db=c["ref"], **kw))


@pytest.fixture(scope="module")
def ap():
    return processor()


@pytest.fixture(scope="module")
def fx():
    return load_fixture("wav_frontend")


def alone(ap, signal: np.ndarray) -> torch.Tensor:
    """``wav_to_mel`` on one normalised signal, as one row (however short: the padded mel basis has a workspace region of its own)."""
    return ap.wav_to_mel(torch.from_numpy(signal)[None])[0]


def recording(rng, frames, n_fft, hop, front_chunks=0, back_chunks=0, extra=0):
    """int16: whole chunks of faint hiss, `frames` frames (+ extra samples, less than a hop) of loud noise, whole chunks of hiss."""
    loud = rng.integers(-20000, 20001, size=n_fft + (frames - 1) * hop + extra).astype(np.int16)
    hiss = lambda n: rng.integers(-3, 4, size=n).astype(np.int16)   # noqa: E731
    return np.concatenate([hiss(front_chunks * CHUNK), loud, hiss(back_chunks * CHUNK)])


# ---- 1. bounds ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["int16", "float32"])
def test_trim_bounds_equal_the_reference(ap, fx, kind):
    rng = np.random.default_rng(1)
    pcm = rng.integers(-30000, 30001, size=fx["pcm"].shape).astype(np.int16)     # loud garbage behind every row's end
    for i, n in enumerate(fx["lengths"]):
        pcm[i, :n] = fx["pcm"][i, :n]
    batch = pcm if kind == "int16" else (pcm.astype(np.float64) / 32767.0).astype(np.float32)
    got = ap.trim_bounds(batch, fx["lengths"])
    assert got.dtype == torch.int32 and got.is_cuda
    assert got.cpu().numpy().tolist() == fx["bounds"].tolist()
    assert all(got[i, 0] >= got[i, 1] for i in (5, 7))                           # nothing passes: the caller's "empty row"
    as_list = ap.trim_bounds([batch[i, :n] for i, n in enumerate(fx["lengths"])])
    assert torch.equal(as_list, got)


def test_trim_bounds_follow_the_restatement_on_odd_lengths(ap):
    """Rows shorter than a chunk, one sample long, empty, ending inside a chunk, loud only in the very last short chunk."""
    rng = np.random.default_rng(2)
    rows = [rng.integers(-3, 4, size=n).astype(np.int16) for n in (1, 100, CHUNK, CHUNK + 1, 5 * CHUNK + 17, 9 * CHUNK - 1)]
    rows[4][-5:] = 20000
    rows[5][0] = 30000
    rows.append(recording(rng, 3, 1024, 256, front_chunks=2, back_chunks=1, extra=100))
    want = [list(silence_bounds(r, AUDIO_CASE["fs"], ap.config.trim_dbfs, 32767.0)) for r in rows]
    assert ap.trim_bounds(rows).cpu().numpy().tolist() == want
    padded = np.zeros((2, 50), np.int16)
    assert ap.trim_bounds(padded, [0, 50]).cpu().numpy().tolist()[0] == [0, 0]   # an empty row


# ---- 2. ragged == single row, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop", [(1024, 256), (512, 128)])
def test_ragged_rows_equal_single_row_calls(n_fft, hop):
    ap = processor(n_fft, hop)
    rng = np.random.default_rng(7)
    T = 37
    counts = [T, T - 1, 9, 8, 5, 4, 3, 1]      # ends inside a four-frame workgroup, exactly on its edge, one frame only
    rows = [recording(rng, t, n_fft, hop, front_chunks=b % 3, back_chunks=(b + 1) % 4, extra=(31 * b) % hop) for b, t in enumerate(counts)]
    n_max = max(r.shape[0] for r in rows)
    pcm = rng.integers(-30000, 30001, size=(len(rows), n_max)).astype(np.int16)   # garbage behind the rows
    for b, r in enumerate(rows):
        pcm[b, : r.shape[0]] = r
    lengths = [r.shape[0] for r in rows]
    for trim in (True, False):
        mel, mel_lengths, gate = ap.wav_to_mel_ragged(pcm, lengths, trim=trim, normalize=True)
        want_counts = counts if trim else [frames_of(n, n_fft, hop) for n in lengths]
        assert mel_lengths.dtype == torch.int64 and mel_lengths.tolist() == want_counts
        assert tuple(mel.shape) == (len(rows), ap.config.n_mels, max(want_counts)) and tuple(gate.shape) == (len(rows), max(want_counts))
        for b, r in enumerate(rows):
            left, right = silence_bounds(r, AUDIO_CASE["fs"], ap.config.trim_dbfs, 32767.0) if trim else (0, r.shape[0])
            Tb = want_counts[b]
            assert torch.equal(mel[b, :, :Tb], alone(ap, peak_normalise(r[left:right]))), (trim, b)
            assert mel[b, :, Tb:].eq(0).all(), (trim, b)
            assert gate[b, : Tb - 1].eq(0).all() and gate[b, Tb - 1:].eq(1).all(), (trim, b)
    # float32 recordings (full scale 1.0), without normalisation: the samples as they are
    as_float = [(r.astype(np.float64) / 32767.0).astype(np.float32) for r in rows]
    mel, mel_lengths, _ = ap.wav_to_mel_ragged(as_float, trim=True, normalize=False)
    assert mel_lengths.tolist() == counts
    for b, r in enumerate(as_float):
        left, right = silence_bounds(r, AUDIO_CASE["fs"], ap.config.trim_dbfs, 1.0)
        assert torch.equal(mel[b, :, : counts[b]], alone(ap, r[left:right])), b
    mel_n, _, _ = ap.wav_to_mel_ragged(as_float, trim=True, normalize=True)
    for b, r in enumerate(as_float):
        left, right = silence_bounds(r, AUDIO_CASE["fs"], ap.config.trim_dbfs, 1.0)
        assert torch.equal(mel_n[b, :, : counts[b]], alone(ap, r[left:right] / np.abs(r[left:right]).max())), b


def test_one_row_alone_equals_the_first_of_identical_rows(ap):
    """Rows of a uniform batch do not see each other: a short signal alone (one frame, and 3 frames - fewer than a workgroup of the
    fused STFT takes) equals the first of several identical rows bit for bit, also where the frames of two rows share a workgroup."""
    rng = np.random.default_rng(12)
    for frames, reps in ((1, 41), (3, 14), (5, 9), (40, 2)):
        sig = (rng.standard_normal(1024 + (frames - 1) * 256 + 7) * 0.2).astype(np.float32)
        one = alone(ap, sig)
        many = ap.wav_to_mel(torch.from_numpy(sig)[None].repeat(reps, 1))
        assert one.shape == (ap.config.n_mels, frames)
        for r in range(reps):
            assert torch.equal(many[r], one), (frames, r)


def test_rows_of_a_large_batch_equal_single_row_calls(ap):
    """Above 4096 frames the mel GEMM takes another tile shape: a row's result still does not depend on its batch."""
    rng = np.random.default_rng(8)
    counts = [700, 640, 700, 511, 700, 699, 650]
    rows = [recording(rng, t, 1024, 256, front_chunks=1, back_chunks=2, extra=11 * b) for b, t in enumerate(counts)]
    mel, mel_lengths, _ = ap.wav_to_mel_ragged(rows)
    assert mel_lengths.tolist() == counts and len(rows) * max(counts) > 4096
    for b in (1, 3, 6):
        left, right = silence_bounds(rows[b], AUDIO_CASE["fs"], ap.config.trim_dbfs, 32767.0)
        assert torch.equal(mel[b, :, : counts[b]], alone(ap, peak_normalise(rows[b][left:right]))), b
        assert mel[b, :, counts[b]:].eq(0).all()


# ---- 3. reference parity --------------------------------------------------------------------------------------------------------
def test_fixture_rows_match_the_reference(ap, fx):
    good = [int(i) for i in np.flatnonzero(fx["has_mel"])]
    rows = [fx["pcm"][i, : fx["lengths"][i]] for i in good]
    mel, mel_lengths, gate = ap.wav_to_mel_ragged(rows)          # the config's defaults: trim at -50 dBFS, normalise
    assert ap.config.trim_silence and ap.config.normalize and ap.config.trim_dbfs == float(fx["trim_dbfs"])
    for k, i in enumerate(good):
        want = fx[f"mel_db_{i}"]
        assert mel_lengths[k].item() == want.shape[1]
        assert np.abs(mel[k, :, : want.shape[1]].cpu().numpy() - want).max() <= 1e-4, i
        # the samples the kernel normalises in its loads are the reference's float32 samples to the bit: the same frames through
        # the uniform call, fed the reference's own normalised signal, give the same bits
        assert torch.equal(mel[k, :, : want.shape[1]], alone(ap, fx[f"norm_{i}"])), i
    assert not torch.isnan(mel).any() and not torch.isnan(gate).any()


def test_convert_wav2mel_batch_writes_what_convert_wav2mel_writes(ap, fx, tmp_path):
    import scipy.io.wavfile

    good = [int(i) for i in np.flatnonzero(fx["has_mel"])]
    paths, want = [], []
    for i in good:
        left, right = fx["bounds"][i]
        paths.append(str(tmp_path / f"trimmed_{i}.wav"))          # the reference trims into a file, then converts that file
        scipy.io.wavfile.write(paths[-1], int(fx["fs"]), fx["pcm"][i, left:right])
        if fx[f"mel_db_{i}"].shape[1] > 40:
            ap.convert_wav2mel(paths[-1], str(tmp_path / f"single_{i}.npy"))
            want.append(np.load(str(tmp_path / f"single_{i}.npy")))
        else:                                                     # (the single-file call refuses recordings of 40 frames and fewer)
            want.append(alone(ap, fx[f"norm_{i}"]).cpu().numpy())
    batch_outs = [str(tmp_path / f"batch_{i}.npy") for i in good]
    mels, durations = ap.convert_wav2mel_batch([fx["pcm"][i, : fx["lengths"][i]] for i in good], batch_outs)
    for k, i in enumerate(good):
        assert mels[k].dtype == np.float32 and np.array_equal(np.load(batch_outs[k]), want[k]) and np.array_equal(mels[k], want[k]), i
        assert durations[k] == (fx["bounds"][i, 1] - fx["bounds"][i, 0]) / int(fx["fs"])
    from_files, _ = ap.convert_wav2mel_batch(paths, trim=False)   # paths are read like convert_wav2mel reads them
    assert all(np.array_equal(a, b) for a, b in zip(from_files, mels))
    limits = AudioConfig(min_wav_duration=0.5, max_wav_duration=10)
    assert keep_by_duration(durations, limits) == [k for k, d in enumerate(durations) if d >= 0.5]


# ---- 4. batch dict --------------------------------------------------------------------------------------------------------------
def small_model():
    mc, ac, tc = case_configs(TRAIN_CASE)
    m = Tacotron2(mc, ac, tc)
    m.load_state_dict(gw.generate_state_dict(mc, ac, tc, seed=TRAIN_CASE["weight_seed"], peaky_attention=True))
    return m.to("cuda:0"), (mc, ac, tc)


def wav_items(rng, tc):
    token_counts, frame_counts = [6, 9, 6, 4, 9], [12, 7, 10, 5, 9]      # tied token counts
    return [{"tokens": torch.from_numpy(rng.integers(1, tc.n_tokens, size=n)),
             "wav": recording(rng, t, 1024, 256, front_chunks=b % 2, back_chunks=1, extra=7 * b)}
            for b, (n, t) in enumerate(zip(token_counts, frame_counts))], frame_counts


def test_wav_collate_equals_text_mel_collate_and_feeds_the_model():
    model, (mc, ac, tc) = small_model()
    wav_ap = AudioProcessor(ac)
    rng = np.random.default_rng(11)
    items, frame_counts = wav_items(rng, tc)
    got = WavTextCollateFn(wav_ap)(items)
    mels, _ = wav_ap.convert_wav2mel_batch([x["wav"] for x in items])
    assert [m.shape[1] for m in mels] == frame_counts
    want = TextMelCollateFn()([{"tokens": x["tokens"], "features": torch.from_numpy(m)} for x, m in zip(items, mels)])
    assert list(got) == list(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and torch.equal(got[k].cpu(), want[k]), k
    for k in ("mel_padded", "gate_padded", "mel_lengths"):
        assert got[k].is_cuda, k
    for row in range(len(items)):
        Tb = int(want["mel_lengths"][row])
        assert got["gate_padded"][row, : Tb - 1].eq(0).all() and got["gate_padded"][row, Tb - 1:].eq(1).all()
    B, T = want["mel_padded"].shape[0], want["mel_padded"].shape[2]
    masks = torch.from_numpy(gw.prenet_keep_masks((T + 1) * B, mc.prenet_dim))
    out_wav = model.forward({**got, "prenet_keep_masks": masks})
    out_npy = model.forward({**want, "prenet_keep_masks": masks})
    for k in out_npy:
        assert torch.equal(out_wav[k], out_npy[k]), k
    model.check_status()


def test_train_step_from_a_wav_batch_equals_the_npy_route():
    losses = []
    for route in ("wav", "npy"):
        model, (mc, ac, tc) = small_model()
        wav_ap = AudioProcessor(ac)
        items, _ = wav_items(np.random.default_rng(12), tc)
        if route == "wav":
            batch = WavTextCollateFn(wav_ap)(items)
        else:
            mels, _ = wav_ap.convert_wav2mel_batch([x["wav"] for x in items])
            batch = TextMelCollateFn()([{"tokens": x["tokens"], "features": torch.from_numpy(m)} for x, m in zip(items, mels)])
        torch.manual_seed(99)                                   # the dropout masks of the step are drawn from torch's generator
        model.train_step(batch, model.get_criterion(), model.get_optimizer())
        model.check_status()
        assert all(np.isfinite(v) for v in model.loss_items.values())
        losses.append((dict(model.loss_items), model.grad_norm_val))
    assert losses[0] == losses[1]


# ---- 5. bad rows ----------------------------------------------------------------------------------------------------------------
def test_bad_rows_raise_or_are_dropped_and_never_give_nan(ap, fx):
    rng = np.random.default_rng(13)
    ok = recording(rng, 6, 1024, 256, front_chunks=1, back_chunks=1)
    rows = [ok, fx["pcm"][5, : fx["lengths"][5]], fx["pcm"][6, : fx["lengths"][6]], np.zeros(3000, np.int16), ok[CHUNK:-CHUNK][:1023], ok]
    with pytest.raises(ValueError, match=r"row 1 .*after trimming.*rows \[2, 3, 4\]"):
        ap.wav_to_mel_ragged(rows)
    with pytest.raises(ValueError, match="row 0 .*shorter than one frame"):
        ap.wav_to_mel_ragged([rows[2], ok])
    with pytest.raises(ValueError, match="row 1 .*every sample of it is zero"):
        ap.wav_to_mel_ragged([ok, rows[3]], trim=False)
    mel, mel_lengths, gate, dropped = ap.wav_to_mel_ragged(rows, drop_bad=True)
    assert dropped == [1, 2, 3, 4] and mel_lengths.tolist() == [6, 6] and tuple(mel.shape) == (2, ap.config.n_mels, 6)
    assert torch.equal(mel[0], mel[1]) and not torch.isnan(mel).any()
    assert torch.equal(mel[0], ap.wav_to_mel_ragged([ok])[0][0])
    mels, durations = ap.convert_wav2mel_batch(rows, drop_bad=True)
    assert [m is None for m in mels] == [False, True, True, True, True, False] and len(durations) == 6
    with pytest.raises(ValueError, match=r"\[1, 2, 3, 4\]"):
        ap.convert_wav2mel_batch(rows)
    # through the collate function: the error comes before any model sees the batch
    with pytest.raises(ValueError, match="gives no mel"):
        WavTextCollateFn(ap)([{"tokens": torch.arange(1, 4), "wav": rows[3]}, {"tokens": torch.arange(1, 6), "wav": ok}])
    none_left = ap.wav_to_mel_ragged([rows[3], rows[1]], drop_bad=True)
    assert none_left[3] == [0, 1] and none_left[0].shape[0] == 0 and none_left[1].numel() == 0


def test_status_words_and_clamped_bounds_of_the_c_call(ap):
    """The C call on its own: bounds outside the row are clamped on the device, a row with more frames than T_out is cut."""
    from genvox_amd import _lib

    lib = ap._ensure()
    rng = np.random.default_rng(14)
    n_max, T_out, c = 1024 + 9 * 256, 6, ap.config
    pcm = torch.from_numpy(rng.integers(-9000, 9001, size=(3, n_max)).astype(np.int16)).cuda()
    bounds = torch.tensor([[-50, 10 ** 6], [100, 100 + 1024 + 3 * 256 + 5], [700, 300]], dtype=torch.int32).cuda()
    need = lib.gvx_wav_to_mel_ragged_workspace_bytes(ap._plan, 3, 1024 + (T_out - 1) * 256, c.n_mels)   # what T_out frames per row take
    assert 0 < need <= lib.gvx_wav_to_mel_ragged_workspace_bytes(ap._plan, 3, n_max, c.n_mels)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    mel = torch.full((3, c.n_mels, T_out), float("nan"), device="cuda")
    frames, status = torch.zeros(3, dtype=torch.int32).cuda(), torch.zeros(3, dtype=torch.int32).cuda()
    args = [ap._plan, pcm.data_ptr(), 0, ap._window_dev.data_ptr(), ap._mel_basis_dev.data_ptr(), 3, n_max, bounds.data_ptr(), 1, c.n_mels,
            0, 1.0, T_out, mel.data_ptr(), None, frames.data_ptr(), status.data_ptr(), ws.data_ptr()]
    assert lib.gvx_wav_to_mel_ragged(*args, need - 256, ap._stream()) == -5          # GVX_ERR_WORKSPACE, nothing launched
    assert torch.isnan(mel).all()
    _lib.check(lib.gvx_wav_to_mel_ragged(*args, need, ap._stream()))
    assert frames.tolist() == [6, 4, 0] and status.tolist() == [ap.ROW_CUT, 0, ap.ROW_EMPTY]
    assert not torch.isnan(mel).any() and mel[2].eq(0).all() and mel[1, :, 4:].eq(0).all()
    sig = pcm[0].cpu().numpy()
    assert torch.equal(mel[0], alone(ap, peak_normalise(sig))[:, :6])
    sig = pcm[1].cpu().numpy()[100: 100 + 1024 + 3 * 256 + 5]
    assert torch.equal(mel[1, :, :4], alone(ap, peak_normalise(sig)))
