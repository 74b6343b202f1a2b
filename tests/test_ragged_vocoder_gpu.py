"""GPU: the ragged vocoder path (gvx_griffin_lim_ragged / gvx_wav_finalize_ragged behind AudioProcessor's `frame_lengths` /
`mel_lengths` arguments).  A padded batch whose rows have their own frame counts must give, row by row and bit for bit, what the
uniform call gives for that row alone at its own length - whatever the padding holds - and match the NumPy oracle run on the
trimmed row.  Lengths are chosen so that a row ends inside a workgroup's tile, exactly at a tile edge of the two-frames-per-wave
kernel (T_b + 3 = 29) and of the one-frame kernel (T_b + 3 = 13), and is shorter than the four-frame overlap."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from genvox_amd import _lib
from genvox_amd.audio import AudioProcessor
from genvox_amd.configs import AudioConfig
from oracle import audio_ref
from tests.golden.cases import AUDIO_CASE
from tests.helpers import load_fixture

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_FIX = AUDIO_CASE["frames"]
LENS = [T_FIX, T_FIX - 1, 27, 26, 17, 10, 3, 2, 1]


def make_ap(n_fft=AUDIO_CASE["n_fft"], hop=AUDIO_CASE["hop"]):
    c = AUDIO_CASE
    return AudioProcessor(AudioConfig(sampling_rate=c["fs"], filter_length=n_fft, hop_length=hop, n_mels=c["n_mels"],
                                      mel_fmin=c["fmin"], mel_fmax=c["fmax"], log_func=c["log_func"], ref_level_db=c["ref"]))


@pytest.fixture(scope="module")
def ap():
    return make_ap()


def mel_rows(n):
    """n different mels [n, 80, T] from the fixture's one: shifted in level, flipped and rolled in time."""
    mel = torch.from_numpy(load_fixture("audio")["mel_db"])
    rows = [mel, mel - 0.5, mel.flip(1), mel.roll(7, 1) + 0.25]
    return torch.stack([rows[i % 4] - 0.1 * (i // 4) for i in range(n)])


def pad_fill(x, lens, value):
    """x [B, C, T] with the frames past each row's length set to `value`."""
    x = x.clone()
    for b, t in enumerate(lens):
        x[b, :, t:] = value
    return x


def samples(ap, t):
    return ap.config.filter_length + (t - 1) * ap.config.hop_length


def test_ragged_rows_equal_single_rows_bit_for_bit(ap):
    batch = pad_fill(mel_rows(len(LENS)), LENS, 0.0)
    wav, counts = ap.convert_mel2wav_batch(batch, n_iter=8, mel_lengths=LENS)
    assert wav.dtype == torch.float64 and wav.shape == (len(LENS), samples(ap, T_FIX) - 2 * ap.TRIM)
    assert counts == [samples(ap, t) - 2 * ap.TRIM for t in LENS]
    for b, t in enumerate(LENS):
        alone = ap.convert_mel2wav_batch(batch[b:b + 1, :, :t].contiguous(), n_iter=8)
        assert alone.shape == (1, counts[b])
        assert torch.equal(wav[b, :counts[b]], alone[0]), (b, t)
        assert torch.all(wav[b, counts[b]:] == 0), (b, t)
    # device int32 lengths (what Tacotron2.inference hands over) take the same path
    wav2, counts2 = ap.convert_mel2wav_batch(batch, n_iter=8, mel_lengths=torch.tensor(LENS, dtype=torch.int32, device="cuda"))
    assert counts2 == counts and torch.equal(wav2, wav)
    # without lengths: today's call, today's return value
    assert isinstance(ap.convert_mel2wav_batch(batch[:2], n_iter=1), torch.Tensor)


@pytest.mark.parametrize("n_iter", [0, 1, 5])
def test_ragged_griffin_lim_phase_and_raw_waveform_equal_single_rows(ap, n_iter):
    mag = ap.mel_to_magnitude(mel_rows(len(LENS)))
    phase, wav = ap.griffin_lim(mag, n_iter=n_iter, frame_lengths=LENS)
    assert phase.shape == mag.shape and wav.shape == (len(LENS), samples(ap, T_FIX))
    for b, t in enumerate(LENS):
        ph1, w1 = ap.griffin_lim(mag[b:b + 1, :, :t].contiguous(), n_iter=n_iter)
        assert torch.equal(phase[b, :, :t], ph1[0]) and torch.all(phase[b, :, t:] == 0), (b, t)
        assert torch.equal(wav[b, :samples(ap, t)], w1[0]) and torch.all(wav[b, samples(ap, t):] == 0), (b, t)
    # one output only
    ph_only, none = ap.griffin_lim(mag, n_iter=n_iter, frame_lengths=LENS, want_wav=False)
    assert none is None and torch.equal(ph_only, phase)


def test_nothing_leaks_from_the_padding(ap):
    """The same calls with the padded frames full of large finite values (their magnitudes overflow to inf) instead of 0."""
    rows = mel_rows(len(LENS))
    clean, counts = ap.convert_mel2wav_batch(pad_fill(rows, LENS, 0.0), n_iter=8, mel_lengths=LENS)
    dirty, _ = ap.convert_mel2wav_batch(pad_fill(rows, LENS, 90.0), n_iter=8, mel_lengths=LENS)
    assert torch.isfinite(dirty).all() and torch.equal(clean, dirty)
    mag = ap.mel_to_magnitude(rows)
    bad = pad_fill(mag, LENS, 3.0e38)
    bad[0::2] = pad_fill(mag[0::2], LENS[0::2], float("nan"))
    ph_a, wav_a = ap.griffin_lim(mag, n_iter=3, frame_lengths=LENS)
    ph_b, wav_b = ap.griffin_lim(bad, n_iter=3, frame_lengths=LENS)
    assert torch.equal(ph_a, ph_b) and torch.equal(wav_a, wav_b) and torch.isfinite(wav_b).all()
    # the tail alone: garbage behind a row's samples changes nothing either
    raw = wav_a.clone()
    for b, t in enumerate(LENS):
        raw[b, samples(ap, t):] = 0.9 * (-1) ** b
    assert torch.equal(ap.finalize(wav_a, frame_lengths=LENS), ap.finalize(raw, frame_lengths=LENS))


def weighted_phase_diff(phase_a, phase_b, mag):
    w = np.abs(mag) / np.abs(mag).sum()
    return float((np.abs(np.exp(1j * phase_a) - np.exp(1j * phase_b)) * w).sum())


@pytest.mark.parametrize("n_iter", [1, 2])
def test_ragged_rows_match_the_oracle_on_trimmed_rows(ap, n_iter):
    c = AUDIO_CASE
    fx = load_fixture("audio")
    lens = [T_FIX, 26, 17, 3, 1]
    mags = np.stack([fx["mag"], 0.5 * fx["mag"][:, ::-1], np.roll(fx["mag"], 5, axis=1), fx["mag"], fx["mag"][:, ::-1]]).astype(np.float32)
    phase, _ = ap.griffin_lim(torch.from_numpy(mags.copy()), n_iter=n_iter, frame_lengths=lens)
    phase = phase.cpu().numpy()
    for b, t in enumerate(lens):
        m = np.ascontiguousarray(mags[b, :, :t])
        want = audio_ref.griffin_lim(m, c["n_fft"], c["hop"], n_iter=n_iter)
        assert weighted_phase_diff(phase[b, :, :t], want, m) <= 1e-3, (b, t)


def test_ragged_tail_matches_the_oracle_tail(ap):
    """clip / trim / normalise / low-pass of every row of a padded raw-signal batch against the reference's tail
    (core/processors.py:91-95) on the trimmed raw signal."""
    import scipy.signal

    c = AUDIO_CASE
    fx = load_fixture("audio")
    ph = fx["gl_phase_32"]
    lens = [T_FIX, 39, 17, 3, 1]
    n = samples(ap, T_FIX)
    raws, batch = [], np.full((len(lens), n), 0.7, np.float32)     # padding that would move the peak if it were read
    for b, t in enumerate(lens):
        spec = ((1.0 - 0.1 * b) * fx["mag"][:, :t] * (np.cos(ph[:, :t]) + 1j * np.sin(ph[:, :t]))).astype(np.complex64)
        raws.append(audio_ref.istft(spec, c["n_fft"], c["hop"]))
        batch[b, :raws[b].shape[0]] = raws[b]
    got = ap.finalize(torch.from_numpy(batch), frame_lengths=lens).cpu().numpy()
    bb, aa = scipy.signal.butter(6, 6000, fs=c["fs"], btype="low", analog=False)
    for b, t in enumerate(lens):
        sig = raws[b].copy()
        sig[(sig > 1) | (sig < -1)] = 0
        sig = sig[500:-500]
        sig = (sig / max(np.abs(np.min(sig)), np.abs(np.max(sig)))).astype(np.float32)
        want = scipy.signal.lfilter(bb, aa, sig)
        assert np.abs(got[b, :want.shape[0]] - want).max() <= 1e-5, (b, t)
        assert np.all(got[b, want.shape[0]:] == 0)
    assert np.abs(got[0] - fx["wav"]).max() <= 1e-5            # row 0 is the fixture's own signal


def test_ragged_finalize_long_rows_chunked_and_sequential_filter(ap):
    """Rows long enough for many filter chunks, ending in different chunks and before the end of the first: equal to the
    one-row call; and the sequential kernel (a filter too slow for overlap-discard) through the C ABI."""
    rng = np.random.default_rng(11)
    hop, n_fft = ap.config.hop_length, ap.config.filter_length
    lens = [130, 129, 61, 9, 4, 1]
    n = n_fft + (lens[0] - 1) * hop
    wav = (rng.standard_normal((len(lens), n)) * 0.4).astype(np.float32)
    wav[1, 2000:2010] = 3.0
    y = torch.from_numpy(wav)
    got = ap.finalize(y, frame_lengths=lens)
    for b, t in enumerate(lens):
        nb = n_fft + (t - 1) * hop
        alone = ap.finalize(y[b:b + 1, :nb].contiguous())
        assert torch.equal(got[b, :nb - 2 * ap.TRIM], alone[0]) and torch.all(got[b, nb - 2 * ap.TRIM:] == 0), (b, t)
    lib = _lib.load()
    trim = 10
    bc, ac = (C.c_double * 2)(1.0, 0.0), (C.c_double * 2)(1.0, -0.9999)     # pole at 0.9999: the sequential kernel
    yd = y.cuda()
    out = torch.empty(len(lens), n - 2 * trim, dtype=torch.float64, device="cuda")
    scratch = torch.empty(len(lens), dtype=torch.int32, device="cuda")
    ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.gvx_wav_finalize_ragged(yd.data_ptr(), len(lens), n, ld.data_ptr(), n_fft, hop, trim, bc, ac, 1, out.data_ptr(),
                                           scratch.data_ptr(), s))
    for b, t in enumerate(lens):
        nb = n_fft + (t - 1) * hop
        one = torch.empty(1, nb - 2 * trim, dtype=torch.float64, device="cuda")
        row = yd[b:b + 1, :nb].contiguous()
        _lib.check(lib.gvx_wav_finalize(row.data_ptr(), 1, nb, trim, bc, ac, 1, one.data_ptr(), scratch.data_ptr(), s))
        assert torch.equal(out[b, :nb - 2 * trim], one[0]) and torch.all(out[b, nb - 2 * trim:] == 0), (b, t)


CHILD = r"""
import sys
import torch
sys.path.insert(0, {repo!r})
from tests.test_ragged_vocoder_gpu import LENS, make_ap, mel_rows, pad_fill, samples
ap = make_ap({n_fft}, {hop})
lens = {lens!r}
T = max(lens)
mag = ap.mel_to_magnitude(mel_rows(len(lens))[:, :, :T].contiguous()) if {n_fft} == 1024 else \
    (torch.rand(len(lens), {n_fft} // 2 + 1, T, generator=torch.Generator().manual_seed(3)) * 2.0)
mag = pad_fill(mag, lens, 1.0e30)
for n_iter in (0, 3):
    phase, wav = ap.griffin_lim(mag, n_iter=n_iter, frame_lengths=lens)
    for b, t in enumerate(lens):
        ph1, w1 = ap.griffin_lim(mag[b:b + 1, :, :t].contiguous(), n_iter=n_iter)
        nb = samples(ap, t)
        assert torch.equal(phase[b, :, :t], ph1[0]) and torch.all(phase[b, :, t:] == 0), ("phase", n_iter, b, t)
        assert torch.equal(wav[b, :nb], w1[0]) and torch.all(wav[b, nb:] == 0), ("wav", n_iter, b, t)
torch.cuda.synchronize()
print("ragged child ok")
"""


@pytest.mark.parametrize("n_fft,hop,rocfft", [(1024, 256, True), (512, 128, False)])
def test_ragged_rows_on_the_rocfft_path_in_a_child_process(n_fft, hop, rocfft):
    """The rocFFT pipeline (every size other than 1024 / 256, or GVX_GL_ROCFFT=1) transforms the padded frames too; its
    overlap-add skips them and divides by the row's own window sums.  Run in a fresh process of its own."""
    env = {**os.environ, "PYTHONNOUSERSITE": "1"}
    env.pop("GVX_GL_ROCFFT", None)
    if rocfft:
        env["GVX_GL_ROCFFT"] = "1"
    lens = LENS if n_fft == 1024 else [24, 23, 9, 4, 3, 2, 1]
    r = subprocess.run([sys.executable, "-c", CHILD.format(repo=REPO, n_fft=n_fft, hop=hop, lens=lens)], env=env, cwd=REPO,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ragged child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_bad_arguments_are_refused_and_launch_nothing(ap):
    mel = mel_rows(3)
    for bad in ([T_FIX, 0, 5], [T_FIX, T_FIX + 1, 5], [T_FIX, 5], [T_FIX, -3, 5]):
        with pytest.raises(ValueError):
            ap.convert_mel2wav_batch(mel, n_iter=1, mel_lengths=bad)
        with pytest.raises(ValueError):
            ap.griffin_lim(torch.ones(3, 513, T_FIX), n_iter=1, frame_lengths=bad)
    with pytest.raises(ValueError):
        ap.finalize(torch.zeros(3, samples(ap, T_FIX)), frame_lengths=[T_FIX, T_FIX + 1, 5])
    with pytest.raises(ValueError):
        ap.finalize(torch.zeros(3, samples(ap, T_FIX) + 1), frame_lengths=[T_FIX, 4, 5])      # not a whole number of frames
    short = make_ap(512, 128)
    with pytest.raises(ValueError, match="too short"):
        short.convert_mel2wav_batch(mel, n_iter=1, mel_lengths=[T_FIX, 4, 5])                  # 512 + 3*128 = 896 samples < 2*500
    # C ABI: null lengths, workspace of the uniform call (too small by the per-row divisors)
    lib = ap._ensure()
    B, T = 3, T_FIX
    mag = ap.mel_to_magnitude(mel)
    wav = torch.full((B, samples(ap, T)), 7.0, device="cuda")
    lens = torch.tensor([T, 4, 5], dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.gvx_gl_workspace_bytes_ragged(ap._plan, B, T, 80), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    small = lib.gvx_gl_workspace_bytes(ap._plan, B, T, 0)       # what the uniform Griffin-Lim call needs: no room for the divisors
    assert 0 < small < lib.gvx_gl_workspace_bytes_ragged(ap._plan, B, T, 0) <= ws.numel()
    win = ap._window_dev.data_ptr()
    assert lib.gvx_griffin_lim_ragged(ap._plan, mag.data_ptr(), win, B, T, None, 1, 0.99, None, wav.data_ptr(), ws.data_ptr(),
                                      ws.numel(), s) == -1
    assert b"frame_lengths" in lib.gvx_last_error()
    assert lib.gvx_griffin_lim_ragged(ap._plan, mag.data_ptr(), win, B, T, lens.data_ptr(), 1, 0.99, None, wav.data_ptr(), ws.data_ptr(),
                                      small, s) == -5
    assert b"workspace too small" in lib.gvx_last_error()
    out = torch.full((B, wav.shape[1] - 1000), 7.0, dtype=torch.float64, device="cuda")
    scratch = torch.zeros(B, dtype=torch.int32, device="cuda")
    one = (C.c_double * 2)(1.0, 0.0)
    assert lib.gvx_wav_finalize_ragged(wav.data_ptr(), B, wav.shape[1], None, 1024, 256, 500, one, one, 1, out.data_ptr(),
                                       scratch.data_ptr(), s) == -1
    torch.cuda.synchronize()
    assert torch.all(wav == 7.0) and torch.all(out == 7.0)      # nothing ran
    # lengths the C ABI cannot trust are clamped, a row of length 0 is zeros: no fault, no out-of-range access
    wild = torch.tensor([T + 1000, 0, -5], dtype=torch.int32, device="cuda")
    ph = torch.full_like(mag, 7.0)
    _lib.check(lib.gvx_griffin_lim_ragged(ap._plan, mag.data_ptr(), win, B, T, wild.data_ptr(), 2, 0.99, ph.data_ptr(), wav.data_ptr(),
                                          ws.data_ptr(), ws.numel(), s))
    ph1, w1 = ap.griffin_lim(mag[:1], n_iter=2)
    assert torch.equal(wav[0], w1[0]) and torch.equal(ph[0], ph1[0])
    assert torch.all(wav[1:] == 0) and torch.all(ph[1:] == 0)
    bb, aa = ap._b, ap._a
    nb = len(bb)
    _lib.check(lib.gvx_wav_finalize_ragged(wav.data_ptr(), B, wav.shape[1], wild.data_ptr(), 1024, 256, 500,
                                           (C.c_double * nb)(*bb), (C.c_double * nb)(*aa), nb - 1, out.data_ptr(), scratch.data_ptr(), s))
    assert torch.isfinite(out[0]).all() and torch.equal(out[0], ap.finalize(w1)[0]) and torch.all(out[1:] == 0)
