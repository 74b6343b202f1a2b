"""The vocoder's HIP kernels (genvox_amd/csrc/griffinlim.hip, wav_to_mel.hip; the real-transform pieces they share are
csrc/fft512_lds.h, the waveform tail is wav_finalize.hip) against the float64 restatement tests/audio_ref64.py, element by
element, at the edges of their workgroups.

tests/test_audio_gpu.py holds the same calls to the reference's fixture with aggregates (one number per call); here every bin,
sample and mel element is checked on its own with the metrics of tests/audio_ref64.py, and the assertion message names the worst
element.  tests/test_vocoder_metric_cpu.py shows on the CPU that these metrics, at the tolerances below, catch the mistakes such
kernels make (a halo frame left out of one hop block, a bin taken from the wrong place, the previous spectrum of the wrong buffer,
a tail not divided, one twiddle off by 1e-4) and measures the float32 noise floor the tolerances start from.

Edges.  A workgroup of gl_inverse_ola_kernel and of gl_iteration_kernel<1> completes 13 hop blocks, one of gl_iteration_kernel<2>
29; a row of T frames has T + 3 hop blocks and takes two frames per wave when T + 3 > 13.  So T = 10 | 11, 23 | 24, 26 | 27 and
55 | 56 are where a workgroup is added, T = 1 .. 4 are rows with fewer frames than overlap in one hop block, and 13, 14, 59 sit
inside.  Four paths run every T: the one-launch iteration (default), GVX_GL_ONE_FRAME=1 (gl_iteration_kernel<1> with halo frames
from a neighbour), GVX_GL_TWO_KERNELS=1 (gl_inverse_ola_kernel + gl_forward_update_kernel) and GVX_GL_ROCFFT=1.  The flags are
read per call.

Pruning.  The full product path x T x B x n_iter x momentum has 1 536 members.  Kept: on every path and every T one call with
B = 3, three iterations, momentum 0.99 (first-iteration branch, momentum branch, both buffer parities, the iteration with and
without the inverse half) and B = 1 with 0, 1 and 2 iterations (the tolerances tighten with fewer iterations); momentum 0 and 0.5
at T = 4, 24, 56 only.  The float64 steps of a (T, B, momentum) are computed once and shared by all paths and iteration counts.

Calls go through ctypes with buffers of this module: every output has a sentinel border (checked after the call) and is
pre-filled with finite junk.  WORST collects the largest error / tolerance ratio per kernel and path; the last test prints it.
"""
import functools

import numpy as np
import pytest
import torch

from genvox_amd import _lib
from genvox_amd.audio import AudioProcessor
from genvox_amd.configs import AudioConfig
from tests import audio_ref64 as r64
from tests.test_bptt_gpu import SENTINEL, _Out

pytestmark = pytest.mark.gpu

T_EDGES = (1, 2, 3, 4, 5, 10, 11, 13, 14, 23, 24, 26, 27, 55, 56, 59)
PATHS = {"one_launch": None, "one_frame": "GVX_GL_ONE_FRAME", "two_kernels": "GVX_GL_TWO_KERNELS", "rocfft": "GVX_GL_ROCFFT"}
WORST = {}   # (kernel, path, quantity) -> (error, tolerance, where)


def note(kernel, path, quantity, err, tol, where):
    key = (kernel, path, quantity)
    if key not in WORST or err / tol > WORST[key][0] / WORST[key][1]:
        WORST[key] = (err, tol, where)


def use_path(monkeypatch, path):
    for flag in PATHS.values():
        if flag:
            monkeypatch.delenv(flag, raising=False)
    if PATHS[path]:
        monkeypatch.setenv(PATHS[path], "1")


def processor(n_fft=1024, hop=256, n_mels=80, log_func="np.log", ref=1.0):
    return AudioProcessor(AudioConfig(sampling_rate=22050, filter_length=n_fft, hop_length=hop, n_mels=n_mels, mel_fmin=0.0,
                                      mel_fmax=8000.0, log_func=log_func, ref_level_db=ref))


@pytest.fixture(scope="module")
def ap():
    return processor()


@pytest.fixture(scope="module")
def ap512():
    return processor(512, 128)


class Call:
    """The C ABI of the vocoder on buffers with sentinel borders."""

    def __init__(self, ap):
        self.ap, self.lib = ap, ap._ensure()
        self.c = ap.config
        self.bins = self.c.filter_length // 2 + 1
        self.window = ap._window_dev
        self.stream = torch.cuda.current_stream().cuda_stream

    def samples(self, T):
        return self.c.filter_length + (T - 1) * self.c.hop_length

    @staticmethod
    def done(what, *outs):
        torch.cuda.synchronize()
        for o in outs:
            assert o is None or o.border_intact(), f"{what}: the call wrote outside an output"

    def griffin_lim(self, mag, n_iter, momentum=0.99, lens=None, want_phase=True, want_wav=True):
        B, bins, T = mag.shape
        m = torch.from_numpy(np.ascontiguousarray(mag, np.float32)).cuda()
        phase = _Out((B, bins, T), junk=True) if want_phase else None
        wav = _Out((B, self.samples(T)), junk=True) if want_wav else None
        ws = self.ap._workspace(B, T, ragged=lens is not None)
        pp, pw = (phase.t.data_ptr() if phase else None), (wav.t.data_ptr() if wav else None)
        if lens is None:
            rc = self.lib.gvx_griffin_lim(self.ap._plan, m.data_ptr(), self.window.data_ptr(), B, T, n_iter, float(momentum), pp, pw,
                                          ws.data_ptr(), ws.numel(), self.stream)
        else:
            lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
            rc = self.lib.gvx_griffin_lim_ragged(self.ap._plan, m.data_ptr(), self.window.data_ptr(), B, T, lens_d.data_ptr(), n_iter,
                                                 float(momentum), pp, pw, ws.data_ptr(), ws.numel(), self.stream)
        _lib.check(rc)
        self.done(f"griffin_lim B={B} T={T} n_iter={n_iter}", phase, wav)
        return (phase.t.cpu().numpy() if phase else None), (wav.t.cpu().numpy() if wav else None)

    def stft(self, signal):
        B, n = signal.shape
        T = r64.frame_count(n, self.c.filter_length, self.c.hop_length)
        x = torch.from_numpy(np.ascontiguousarray(signal, np.float32)).cuda()
        out = _Out((B, self.bins, T, 2), junk=True)
        ws = self.ap._workspace(B, T)
        _lib.check(self.lib.gvx_stft(self.ap._plan, x.data_ptr(), self.window.data_ptr(), B, n, out.t.data_ptr(), ws.data_ptr(), ws.numel(),
                                     self.stream))
        self.done(f"stft B={B} n={n}", out)
        z = out.t.cpu().numpy().astype(np.float64)
        return z[..., 0] + 1j * z[..., 1]

    def istft(self, spec):
        B, bins, T = spec.shape
        z = torch.from_numpy(np.ascontiguousarray(np.stack([spec.real, spec.imag], axis=-1), np.float32)).cuda()
        out = _Out((B, self.samples(T)), junk=True)
        ws = self.ap._workspace(B, T)
        _lib.check(self.lib.gvx_istft(self.ap._plan, z.data_ptr(), self.window.data_ptr(), B, T, out.t.data_ptr(), ws.data_ptr(), ws.numel(),
                                      self.stream))
        self.done(f"istft B={B} T={T}", out)
        return out.t.cpu().numpy()

    def wav_to_mel(self, signal):
        B, n = signal.shape
        T = r64.frame_count(n, self.c.filter_length, self.c.hop_length)
        x = torch.from_numpy(np.ascontiguousarray(signal, np.float32)).cuda()
        basis = torch.from_numpy(np.ascontiguousarray(self.ap.mel_basis)).cuda()
        out = _Out((B, self.c.n_mels, T), junk=True)
        ws = self.ap._workspace(B, T)
        _lib.check(self.lib.gvx_wav_to_mel(self.ap._plan, x.data_ptr(), self.window.data_ptr(), basis.data_ptr(), B, n, self.c.n_mels,
                                           0 if self.c.log_func == "np.log" else 1, float(self.c.ref_level_db), out.t.data_ptr(),
                                           ws.data_ptr(), ws.numel(), self.stream))
        self.done(f"wav_to_mel B={B} n={n}", out)
        return out.t.cpu().numpy()

    def mel_to_magnitude(self, mel_db, n_mels=None, check=True):
        B, M, T = mel_db.shape
        x = torch.from_numpy(np.ascontiguousarray(mel_db, np.float32)).cuda()
        out = _Out((B, self.bins, T))
        ws = self.ap._workspace(B, T)
        rc = self.lib.gvx_mel_to_magnitude(self.ap._plan, x.data_ptr(), self.ap._inv_basis_dev.data_ptr(), B, n_mels or M, T,
                                           0 if self.c.log_func == "np.log" else 1, float(self.c.ref_level_db), out.t.data_ptr(),
                                           ws.data_ptr(), ws.numel(), self.stream)
        if check:
            _lib.check(rc)
        self.done(f"mel_to_magnitude B={B} T={T}", out)
        return rc, out


def window64(ap):
    return ap.window.astype(np.float64)


@functools.lru_cache(maxsize=None)
def steps64(kind, n_fft, hop, T, B, momentum):
    """(mag [B, bins, T] float32, per row the float64 Griffin-Lim records of 0 .. 3 iterations)."""
    bins = n_fft // 2 + 1
    mk = r64.random_magnitudes if kind == "random" else r64.speech_like_magnitudes
    mag = mk(1000 * T + B, B, bins, T)
    import scipy.signal
    win = scipy.signal.get_window("hann", n_fft, fftbins=True).astype(np.float32).astype(np.float64)
    return mag, [r64.griffin_lim_steps(mag[b], win, hop, 1 if kind == "speech" else 3, momentum) for b in range(B)]


def check_griffin_lim(call, path, kind, T, B, n_iter, momentum, phase, wav, kernel="griffin_lim"):
    """phase / wav of one call against the float64 records: every bin, every sample."""
    c = call.c
    mag, rows = steps64(kind, c.filter_length, c.hop_length, T, B, momentum)
    win = window64(call.ap)
    a = np.stack([rows[b][n_iter]["a"] for b in range(B)])
    tag = f"{kernel} {path} {kind} T={T} B={B} n_iter={n_iter} momentum={momentum}"
    tol_p = r64.TOL_PHASE[kind][n_iter]
    err, where = r64.phase_error(phase, a, mag)
    note(kernel, path, f"phase {kind} n_iter={n_iter}", err, tol_p, where)
    assert err <= tol_p, f"{tag}: phase error {err:.3e} > {tol_p:.1e} at (row, bin, frame) {where}"
    for b in range(B):
        want, wss = r64.final_signal(mag[b], r64.final_phase(rows[b][n_iter]["angles"]), win, c.hop_length)
        tol_s = r64.TOL_SIGNAL[kind][n_iter]
        err, where = r64.signal_error(wav[b], want, wss, c.hop_length)
        note(kernel, path, f"signal {kind} n_iter={n_iter}", err, tol_s, (b,) + where[1:])
        assert err <= tol_s, f"{tag}: signal error {err:.3e} > {tol_s:.1e} at row {b}, (sample, hop block) {where[1:]}"
        own, wss = r64.final_signal(mag[b], phase[b], win, c.hop_length)   # the inverse STFT alone, from the phases the call returned
        err, where = r64.signal_error(wav[b], own, wss, c.hop_length)
        tol_o = r64.TOL_SIGNAL_OWN if kind == "random" else r64.TOL_SIGNAL_OWN_SPEECH
        note(kernel, path, f"signal of the returned phases, {kind}", err, tol_o, (b,) + where[1:])
        assert err <= tol_o, f"{tag}: final inverse STFT error {err:.3e} at row {b}, (sample, hop block) {where[1:]}"


def combos(T):
    out = [(3, 3, 0.99), (1, 0, 0.99), (1, 1, 0.99), (1, 2, 0.99)]
    if T in (4, 24, 56):
        out += [(1, 3, 0.0), (3, 2, 0.5)]
    return out


# ---- 1. Griffin-Lim, every path, against float64 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("T", T_EDGES)
@pytest.mark.parametrize("path", list(PATHS))
def test_griffin_lim_every_bin_and_sample(ap, monkeypatch, path, T):
    call = Call(ap)
    use_path(monkeypatch, path)
    for B, n_iter, momentum in combos(T):
        mag, _ = steps64("random", 1024, 256, T, B, momentum)
        phase, wav = call.griffin_lim(mag, n_iter, momentum)
        check_griffin_lim(call, path, "random", T, B, n_iter, momentum, phase, wav)
        if (B, n_iter) == (3, 3):   # an output that is not asked for changes nothing in the other
            only_phase, none = call.griffin_lim(mag, n_iter, momentum, want_wav=False)
            assert none is None and np.array_equal(only_phase, phase), f"{path} T={T}: want_wav=False changed the phases"
            none, only_wav = call.griffin_lim(mag, n_iter, momentum, want_phase=False)
            assert none is None and np.array_equal(only_wav, wav), f"{path} T={T}: want_phase=False changed the waveform"


@pytest.mark.parametrize("T", (4, 24, 56))
@pytest.mark.parametrize("path", list(PATHS))
def test_griffin_lim_speech_like_magnitudes(ap, monkeypatch, path, T):
    """Low-rank magnitudes with negative entries (the pseudo-inverse mel basis produces them): most bins are quiet, the sign of mag
    turns the returned phase by pi.  Zero and one iteration only: a smooth spectrum at zero phase is a pulse where the Hann window
    vanishes, the rebuilt spectrum is a small difference of large numbers, and from the second iteration on float32 itself is
    O(1) from float64 in the new metric (tests/test_vocoder_metric_cpu.py measures it)."""
    call = Call(ap)
    use_path(monkeypatch, path)
    for n_iter in (0, 1):
        mag, _ = steps64("speech", 1024, 256, T, 3, 0.99)
        assert (mag < 0).any() and (mag > 0).any()
        phase, wav = call.griffin_lim(mag, n_iter)
        check_griffin_lim(call, path, "speech", T, 3, n_iter, 0.99, phase, wav)


# ---- 2. the fused paths against each other -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", (10, 11, 23, 24, 26, 27, 55, 56, 59))
def test_fused_paths_against_each_other(ap, monkeypatch, T):
    """gl_iteration_kernel<1> and <2> are one body: the same operations in the same order on every frame and hop block, whichever
    workgroup computes them (halo or owned) - bit equality.  The two-launch iteration shares the FFT and the formulas but scales
    the unit vector as a * (rcp * mag) where the one-launch kernel computes (a * rcp) * mag: one rounding apart per bin and
    iteration, so it is held to the float64 bound (section 1) and to a few ulp of the one-launch result after one iteration."""
    call = Call(ap)
    mag, _ = steps64("random", 1024, 256, T, 3, 0.99)
    got = {}
    for path in ("one_launch", "one_frame", "two_kernels"):
        use_path(monkeypatch, path)
        got[path] = {n: call.griffin_lim(mag, n) for n in (1, 3)}
    for n in (1, 3):
        for k, name in enumerate(("phase", "waveform")):
            assert np.array_equal(got["one_launch"][n][k], got["one_frame"][n][k]), f"T={T} n_iter={n}: {name} of GVX_GL_ONE_FRAME differs"
    d = np.abs(np.exp(1j * got["two_kernels"][1][0].astype(np.float64)) - np.exp(1j * got["one_launch"][1][0].astype(np.float64))).max()
    note("griffin_lim", "two_kernels", "phase vs one_launch, 1 iteration", float(d), 2e-6, (T,))
    assert d <= 2e-6, f"T={T}: the two-launch iteration is {d:.2e} from the one-launch one after one iteration"


# ---- 3. ragged rows at the same edges --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ("one_launch", "one_frame", "rocfft"))
@pytest.mark.parametrize("T,lens", [(56, (56, 55, 27, 26, 24, 11, 10, 4, 1)), (59, (24, 10, 1))])
def test_ragged_rows_equal_single_row_calls(ap, monkeypatch, path, T, lens):
    """Workgroups wholly behind a row's end, rows ending on a workgroup's last hop block and on its first: each row bit-equal to its
    own uniform call (which section 1 ties to float64), zeros behind its end."""
    call = Call(ap)
    use_path(monkeypatch, path)
    B = len(lens)
    rng = np.random.default_rng(T)
    mag = (np.abs(rng.standard_normal((B, 513, T))) * 3.0).astype(np.float32)
    for b, Tb in enumerate(lens):
        mag[b, :, Tb:] = 1e30 * (1 + b)           # what lies behind a row's end must reach nothing
    phase, wav = call.griffin_lim(mag, 3, lens=list(lens))
    for b, Tb in enumerate(lens):
        p1, w1 = call.griffin_lim(mag[b:b + 1, :, :Tb], 3)
        nb = call.samples(Tb)
        assert np.array_equal(phase[b, :, :Tb], p1[0]), f"{path} T={T}: phases of row {b} ({Tb} frames) differ from its own call"
        assert np.array_equal(wav[b, :nb], w1[0]), f"{path} T={T}: waveform of row {b} ({Tb} frames) differs from its own call"
        assert not phase[b, :, Tb:].any() and not wav[b, nb:].any(), f"{path} T={T}: row {b} is not zero behind its end"


# ---- 4. another FFT size: the rocFFT pipeline alone ----------------------------------------------------------------------------------
@pytest.mark.parametrize("T", (1, 3, 4, 37))
def test_other_fft_size_every_bin_and_sample(ap, ap512, T):
    """n_fft 512 / hop 128 has no fused kernels.  A plan of this size lives beside the 1024 plan in one process (`ap` is created
    first on purpose), uniform and ragged."""
    Call(ap)
    call = Call(ap512)
    for B, n_iter in ((3, 3), (1, 1)):
        mag, _ = steps64("random", 512, 128, T, B, 0.99)
        phase, wav = call.griffin_lim(mag, n_iter)
        check_griffin_lim(call, "rocfft 512/128", "random", T, B, n_iter, 0.99, phase, wav)
    lens = [T, max(1, T // 2), 1]
    mag, _ = steps64("random", 512, 128, T, 3, 0.99)
    phase, wav = call.griffin_lim(mag, 3, lens=lens)
    for b, Tb in enumerate(lens):
        p1, w1 = call.griffin_lim(mag[b:b + 1, :, :Tb], 3)
        assert np.array_equal(phase[b, :, :Tb], p1[0]) and np.array_equal(wav[b, :call.samples(Tb)], w1[0]), (T, b)
        assert not phase[b, :, Tb:].any() and not wav[b, call.samples(Tb):].any(), (T, b)


# ---- 5. gvx_stft / gvx_istft -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("n", (1024, 1279, 1280, 1281, 5001, 1024 + 55 * 256 + 3))
def test_stft_every_bin(ap, n, B):
    """Odd lengths put rows 1 and 2 on odd offsets (the scalar framing path); per element against the frame's largest bin."""
    call = Call(ap)
    rng = np.random.default_rng(n + B)
    sig = (rng.standard_normal((B, n)) * 0.3).astype(np.float32)
    sig[:, n // 2: n // 2 + 40] = 0.0
    got = call.stft(sig)
    for b in range(B):
        want = r64.stft(sig[b], window64(ap), 256)
        assert got[b].shape == want.shape
        err, where = r64._worst(np.abs(got[b] - want) / np.abs(want).max(axis=0, keepdims=True))
        note("gvx_stft", "rocfft", "spectrum", err, r64.TOL_STFT, (b,) + where)
        assert err <= r64.TOL_STFT, f"stft n={n} B={B}: {err:.3e} at row {b}, (bin, frame) {where}"


@pytest.mark.parametrize("T", T_EDGES)
def test_istft_every_sample(ap, T):
    """Random complex spectra.  The imaginary parts of the DC and Nyquist bins are not zero here: a real signal has none, the
    reference's irfft drops them, and so must the call (a c2r transform that let them in would add a constant and an alternating
    term to every frame)."""
    call = Call(ap)
    rng = np.random.default_rng(T)
    spec = (rng.standard_normal((2, 513, T)) + 1j * rng.standard_normal((2, 513, T))).astype(np.complex64)
    assert np.abs(spec[:, 0].imag).min() > 0 and np.abs(spec[:, 512].imag).min() > 0
    got = call.istft(spec)
    for b in range(2):
        want, wss = r64.istft(spec[b], window64(ap), 256)
        err, where = r64.signal_error(got[b], want, wss, 256)
        note("gvx_istft", "rocfft", "signal", err, r64.TOL_ISTFT, (b,) + where[1:])
        assert err <= r64.TOL_ISTFT, f"istft T={T}: {err:.3e} at row {b}, (sample, hop block) {where[1:]}"


# ---- 6. gvx_wav_to_mel ----------------------------------------------------------------------------------------------------------------
MEL_CONFIGS = [(80, "np.log", 1.0), (80, "np.log10", 20.0), (12, "np.log10", 1.0), (128, "np.log", 20.0)]


@pytest.mark.parametrize("path", ("one_launch", "rocfft"))
@pytest.mark.parametrize("n_mels,log_func,ref", MEL_CONFIGS)
def test_wav_to_mel_every_element(monkeypatch, path, n_mels, log_func, ref):
    """stft_magnitude_kernel puts four frames on a workgroup and numbers them across rows: B*T = 1, 2, 3, 5, 41 and 4k + 1, and
    B = 3 with T = 5 and 7 (a workgroup spans two rows).  Every call here has fewer than n_mels * 516 / 1026 frames or more: the
    padded basis has room of its own.  An all-zero stretch covers whole frames (the amin clamp)."""
    call = Call(processor(n_mels=n_mels, log_func=log_func, ref=ref))
    use_path(monkeypatch, path)
    for B, T, extra in ((1, 1, 0), (1, 2, 3), (1, 3, 255), (1, 5, 1), (1, 41, 0), (3, 5, 2), (3, 7, 0), (1, 45, 0), (2, 1, 0)):
        n = 1024 + (T - 1) * 256 + extra
        rng = np.random.default_rng(100 * B + T)
        sig = (rng.standard_normal((B, n)) * 0.3).astype(np.float32)
        if T >= 3:
            sig[:, 256: 256 + 1024 + 256 * (T >= 5)] = 0.0
        got = call.wav_to_mel(sig)
        for b in range(B):
            want, amp = r64.wav_to_mel(sig[b], window64(call.ap), 256, call.ap.mel_basis, log_func, ref)
            if T >= 3:
                assert (amp[:, 1] == 0).all()
            err, where = r64.mel_error(got[b], want, amp, amp, log_func)
            note("gvx_wav_to_mel", path, f"mel {log_func}", err, r64.TOL_MEL, (B, T, b) + where)
            assert err <= r64.TOL_MEL, f"wav_to_mel {path} n_mels={n_mels} {log_func} ref={ref} B={B} T={T}: {err:.3e} at row {b}, (mel, frame) {where}"


def test_wav_to_mel_one_row_of_one_frame(ap):
    """What `AudioProcessor.convert_wav2mel` sends for a 1 024-sample file: B = 1, T = 1 (the call once refused every batch of fewer
    than n_mels * 516 / 1026 frames)."""
    rng = np.random.default_rng(3)
    sig = (rng.standard_normal((1, 1024)) * 0.3).astype(np.float32)
    got = ap.wav_to_mel(torch.from_numpy(sig)).cpu().numpy()
    want, amp = r64.wav_to_mel(sig[0], window64(ap), 256, ap.mel_basis, ap.config.log_func, ap.config.ref_level_db)
    assert got.shape == (1, 80, 1)
    err, where = r64.mel_error(got[0], want, amp, amp, ap.config.log_func)
    assert err <= r64.TOL_MEL, (err, where)


def test_convert_wav2mel_on_a_file_of_one_frame(tmp_path):
    """The reference's own signature on a recording of 1 024 samples, with the config's default log10."""
    import scipy.io.wavfile

    apx = processor(log_func="np.log10")
    rng = np.random.default_rng(4)
    pcm = rng.integers(-20000, 20001, size=1024).astype(np.int16)
    scipy.io.wavfile.write(str(tmp_path / "one.wav"), 22050, pcm)
    apx.convert_wav2mel(str(tmp_path / "one.wav"), str(tmp_path / "one.npy"))
    got = np.load(str(tmp_path / "one.npy"))
    sig = (pcm / max(np.abs(np.min(pcm)), np.abs(np.max(pcm)))).astype(np.float32)
    want, amp = r64.wav_to_mel(sig, window64(apx), 256, apx.mel_basis, "np.log10", 1.0)
    assert got.shape == (80, 1)
    err, where = r64.mel_error(got, want, amp, amp, "np.log10")
    assert err <= r64.TOL_MEL, (err, where)


# ---- 7. gvx_mel_to_magnitude ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels,log_func,ref", MEL_CONFIGS)
def test_mel_to_magnitude_every_element(n_mels, log_func, ref):
    """B*T around the 32-frame tile of db_to_amp_transpose_kernel; inputs down to the floor of amplitude_to_db (log(1e-5))."""
    call = Call(processor(n_mels=n_mels, log_func=log_func, ref=ref))
    lo, hi = (-11.5, 2.0) if log_func == "np.log" else (-5.0, 1.0)
    inv = np.ascontiguousarray(call.ap.inverse_mel_basis, dtype=np.float32)
    negatives = 0
    for B, T in ((1, 1), (1, 31), (1, 32), (1, 33), (3, 37)):
        rng = np.random.default_rng(10 * T + B)
        mel = rng.uniform(lo, hi, (B, n_mels, T)).astype(np.float32)
        mel[:, :, 0] = lo
        _, out = call.mel_to_magnitude(mel)
        got = out.t.cpu().numpy()
        for b in range(B):
            want, yard = r64.mel_to_magnitude(mel[b], inv, log_func, ref)
            err, where = r64.magnitude_error(got[b], want, yard)
            note("gvx_mel_to_magnitude", "gemm", f"magnitude {log_func}", err, r64.TOL_MAGNITUDE, (B, T, b) + where)
            assert err <= r64.TOL_MAGNITUDE, f"mel_to_magnitude n_mels={n_mels} {log_func} ref={ref} B={B} T={T}: {err:.3e} at row {b}, (bin, frame) {where}"
            clearly = np.abs(want) > 100 * r64.TOL_MAGNITUDE * yard      # the pseudo-inverse gives negative magnitudes: signs kept
            negatives += int((want[clearly] < 0).sum())
            assert np.array_equal(got[b][clearly] < 0, want[clearly] < 0), f"mel_to_magnitude n_mels={n_mels} B={B} T={T}: a sign differs"
    assert negatives > 0


def test_mel_to_magnitude_refuses_mels_not_a_multiple_of_four(ap):
    call = Call(ap)
    mel = np.zeros((2, 80, 5), np.float32)
    rc, out = call.mel_to_magnitude(mel, n_mels=14, check=False)
    assert rc == -2, rc                                    # GVX_ERR_UNSUPPORTED, before any launch
    assert b"multiple of 4" in call.lib.gvx_last_error()
    assert bool((out.buf.view(torch.int32) == SENTINEL).all()), "a refused call wrote to its output"


def test_zz_report():
    """The measured worst errors per kernel and path of the tests that ran before (run with -rP or -s to see them)."""
    for (kernel, path, quantity), (err, tol, where) in sorted(WORST.items()):
        print(f"WORST {kernel:22s} {path:16s} {quantity:40s} {err:.3e}  tol {tol:.1e}  ratio {err / tol:5.2f}  at {where}")
