"""The ragged wav -> mel front-end without a GPU: a NumPy restatement of the reference's preprocessing decisions (silence walk,
threshold, peak normalisation, convert_wav2mel chain) held to the reference-generated fixture tests/golden/wav_frontend.npz, the
argument checks of the new C-ABI calls and of the Python surface, keep_by_duration, and WavTextCollateFn's layout with a stub
processor.  The GPU tests (tests/test_wav_frontend_gpu.py) hold the kernels to the same fixture and to this restatement."""
import ctypes as C

import numpy as np
import pytest
import torch

from genvox_amd import _lib
from genvox_amd.audio import AudioProcessor, keep_by_duration
from genvox_amd.collate import TextMelCollateFn, WavTextCollateFn
from genvox_amd.configs import AudioConfig
from oracle import audio_ref
from tests.golden.cases import AUDIO_CASE
from tests.helpers import load_fixture


# ---- the restatement (also imported by the GPU tests) ---------------------------------------------------------------------------
def silence_bounds(x: np.ndarray, fs: int, trim_dbfs: float, full_scale: float):
    """(left, right) of the samples to keep.  A 20 ms chunk counts as sound when its mean square reaches full_scale^2 *
    10^(dbfs/10).  The first such chunk from the front gives left; the walk from the back uses chunks aligned to the last sample
    and gives right.  A walk that finds nothing stops on its last chunk, so a silent recording comes back with left >= right."""
    chunk = int(20 * 0.001 * fs)
    n = x.shape[0]
    thr = full_scale ** 2 * 10.0 ** (trim_dbfs / 10.0)

    def first_sound(sig):
        start = 0
        for start in range(0, n, chunk):
            seg = sig[start: start + chunk]
            sq = int((seg.astype(np.int64) ** 2).sum()) if seg.dtype.kind == "i" else float((seg.astype(np.float64) ** 2).sum())
            if sq >= seg.shape[0] * thr:
                break
        return start

    return first_sound(x), n - first_sound(x[::-1])


def peak_normalise(x: np.ndarray) -> np.ndarray:
    """float32(double(sample) / double(peak)), peak = the largest magnitude (of the widened samples: no int16 wrap)."""
    wide = x.astype(np.float64)
    return (wide / np.abs(wide).max()).astype(np.float32)


def frames_of(n: int, n_fft: int, hop: int) -> int:
    return (n - n_fft) // hop + 1 if n >= n_fft else 0


@pytest.fixture(scope="module")
def fx():
    return load_fixture("wav_frontend")


def test_fixture_covers_the_corners(fx):
    chunk = int(20 * 0.001 * int(fx["fs"]))
    left, right = fx["bounds"][:, 0], fx["bounds"][:, 1]
    span = right - left
    assert (left[0], right[0]) == (0, fx["lengths"][0])                       # nothing to trim
    assert (left[1], right[1]) == (0, fx["lengths"][1])                       # less than a chunk of silence stays
    assert left[2] % chunk == 0 and (fx["lengths"][2] - right[2]) % chunk == 0 and right[2] != fx["lengths"][2]
    assert left[5] >= right[5] and left[7] >= right[7]                        # silence only / all zeros: nothing passes
    assert 0 < span[6] < AUDIO_CASE["n_fft"]                                  # trims to less than a frame
    assert frames_of(int(span[8]), AUDIO_CASE["n_fft"], AUDIO_CASE["hop"]) == 1
    assert fx["has_mel"].tolist() == [True, True, True, True, True, False, False, False, True]


def test_restated_bounds_equal_the_reference(fx):
    for i, n in enumerate(fx["lengths"]):
        row = fx["pcm"][i, :n]
        assert silence_bounds(row, int(fx["fs"]), float(fx["trim_dbfs"]), 32767.0) == tuple(fx["bounds"][i]), i
        as_float = (row.astype(np.float64) / 32767.0).astype(np.float32)      # the same recording at full scale 1.0
        assert silence_bounds(as_float, int(fx["fs"]), float(fx["trim_dbfs"]), 1.0) == tuple(fx["bounds"][i]), i


def test_restated_normalisation_and_mel_equal_the_reference(fx):
    c = AUDIO_CASE
    basis = load_fixture("audio")["mel_basis"]
    for i in np.flatnonzero(fx["has_mel"]):
        left, right = fx["bounds"][i]
        norm = peak_normalise(fx["pcm"][i, left:right])
        assert norm.dtype == np.float32 and np.array_equal(norm, fx[f"norm_{i}"]), i
        mel = audio_ref.wav_to_mel(norm, basis, c["n_fft"], c["hop"], c["log_func"], c["ref"])
        assert mel.shape == fx[f"mel_db_{i}"].shape == (c["n_mels"], frames_of(right - left, c["n_fft"], c["hop"]))
        assert np.abs(mel - fx[f"mel_db_{i}"]).max() <= 1e-4, i


def test_peak_of_int16_minimum_does_not_wrap():
    x = np.array([-32768, 16384, 0], np.int16)
    assert np.array_equal(peak_normalise(x), np.array([-1.0, 0.5, 0.0], np.float32))


# ---- C ABI: bad arguments are refused before anything is launched -----------------------------------------------------------------
def test_c_abi_refuses_bad_arguments():
    lib = _lib.load()
    p = C.c_void_p(0x1000)   # never dereferenced: every call below fails its checks first
    assert lib.gvx_wav_trim_bounds(None, 0, 2, 100, p, 22050, -50.0, p, None) == -1
    assert lib.gvx_wav_trim_bounds(p, 2, 2, 100, p, 22050, -50.0, p, None) == -1          # pcm_kind
    assert b"pcm_kind" in lib.gvx_last_error()
    assert lib.gvx_wav_trim_bounds(p, 0, 0, 100, p, 22050, -50.0, p, None) == -1          # B
    assert lib.gvx_wav_trim_bounds(p, 0, 2, 0, p, 22050, -50.0, p, None) == -1            # n_max
    assert lib.gvx_wav_trim_bounds(p, 0, 2, 100, None, 22050, -50.0, p, None) == -1
    assert lib.gvx_wav_trim_bounds(p, 0, 2, 100, p, 22050, -50.0, None, None) == -1
    assert lib.gvx_wav_trim_bounds(p, 0, 2, 100, p, 40, -50.0, p, None) == -1             # no 20 ms chunk
    assert lib.gvx_wav_trim_bounds(p, 0, 2, 100, p, 22050, 3.0, p, None) == -1            # above full scale
    assert lib.gvx_wav_trim_bounds(C.c_void_p(0x1001), 0, 2, 100, p, 22050, -50.0, p, None) == -1   # misaligned int16
    assert lib.gvx_wav_to_mel_ragged_workspace_bytes(None, 2, 100, 80) == 0
    assert lib.gvx_wav_to_mel_ragged(None, p, 0, p, p, 2, 100, p, 1, 80, 0, 1.0, 4, p, None, p, p, p, 1 << 20, None) == -1
    assert b"null" in lib.gvx_last_error()


# ---- Python surface -----------------------------------------------------------------------------------------------------------
def cpu_processor():
    c = AUDIO_CASE
    return AudioProcessor(AudioConfig(sampling_rate=c["fs"], filter_length=c["n_fft"], hop_length=c["hop"], n_mels=c["n_mels"],
                                      log_func=c["log_func"]), device="cpu")


def test_pcm_batch_checks():
    ap = cpu_processor()
    x, lengths = ap._pcm_batch([np.zeros(5, np.int16), np.ones(9, np.int16)])
    assert x.dtype == torch.int16 and tuple(x.shape) == (2, 9) and lengths == [5, 9] and x[0, 5:].eq(0).all()
    x, lengths = ap._pcm_batch(np.zeros((2, 7), np.float64), [7, 3])
    assert x.dtype == torch.float32 and lengths == [7, 3]
    with pytest.raises(ValueError, match="all be int16 or all be floating point"):
        ap._pcm_batch([np.zeros(5, np.int16), np.zeros(5, np.float32)])
    with pytest.raises(ValueError, match="int16 or all"):
        ap._pcm_batch([np.zeros(5, np.int32)])
    with pytest.raises(ValueError, match="row 1"):
        ap._pcm_batch([np.zeros(5, np.int16), np.zeros((5, 2), np.int16)])
    with pytest.raises(ValueError, match="needs sample_lengths"):
        ap._pcm_batch(np.zeros((2, 7), np.int16))
    with pytest.raises(ValueError, match="row 1"):
        ap._pcm_batch(np.zeros((2, 7), np.int16), [7, 8])
    with pytest.raises(ValueError, match="3 sample lengths"):
        ap._pcm_batch(np.zeros((2, 7), np.int16), [7, 7, 7])
    with pytest.raises(ValueError, match="empty batch"):
        ap._pcm_batch([])


def test_no_cpu_fallback():
    ap = cpu_processor()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ap.wav_to_mel_ragged([np.zeros(5000, np.int16)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ap.trim_bounds([np.zeros(5000, np.int16)])


def test_keep_by_duration():
    c = AudioConfig(min_wav_duration=0.5, max_wav_duration=10)
    assert keep_by_duration([0.49, 0.5, 3.0, 10.0, 10.01], c) == [1, 2, 3]
    assert keep_by_duration([], c) == []


class StubProcessor:
    """Stands in for AudioProcessor: the 'mel' of a recording of n samples is n // 100 frames filled with its first sample."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def features(wav):
        return torch.full((4, wav.shape[0] // 100), float(wav[0]))

    def wav_to_mel_ragged(self, rows):
        self.calls.append([int(r[0]) for r in rows])
        feats = [self.features(r) for r in rows]
        T = max(f.shape[1] for f in feats)
        mel, gate = torch.zeros(len(rows), 4, T), torch.zeros(len(rows), T)
        for b, f in enumerate(feats):
            mel[b, :, : f.shape[1]] = f
            gate[b, f.shape[1] - 1:] = 1
        return mel, torch.tensor([f.shape[1] for f in feats], dtype=torch.long), gate


def test_wav_collate_lays_rows_out_like_text_mel_collate():
    rng = np.random.default_rng(3)
    token_counts = [5, 9, 5, 7, 9, 2]                 # ties: the order among equals is the reference's argsort order
    items = [{"tokens": torch.from_numpy(rng.integers(1, 30, size=n)), "wav": np.full(100 * (3 + i), i + 1, np.int16)}
             for i, n in enumerate(token_counts)]
    stub = StubProcessor()
    got = WavTextCollateFn(stub)(items)
    want = TextMelCollateFn()([{"tokens": x["tokens"], "features": StubProcessor.features(x["wav"])} for x in items])
    assert len(stub.calls) == 1                       # one ragged call per batch
    assert list(got) == list(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
