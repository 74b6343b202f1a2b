"""Plain float64 restatement of the vocoder (STFT / inverse STFT / dB <-> amplitude / mel projections / fast Griffin-Lim) with every
intermediate kept, and the element-wise metrics that hold the HIP kernels to it: what tests/test_vocoder_kernels_gpu.py asserts
and what tests/test_vocoder_metric_cpu.py shows to bite.

Written from the formulas in oracle/audio_ref.py and the comments of genvox_amd/csrc/griffinlim.hip, wav_to_mel.hip and
fft512_lds.h, not from their code:
NumPy, float64 / complex128 throughout.  Every input (signal, window, mel basis, magnitudes) is an fp32 number converted to
float64 once; nothing is rounded on the way.  oracle/audio_ref.py - the reference's own float32 arithmetic - stays the parity
oracle; this file is the yardstick that says how far a float32 computation may be from the exact one.

  stft / istft            Hann frames without centring or padding; istft also returns the window sum of squares it divided by
  db_to_amplitude / amplitude_to_db   both log kinds, any ref, the reference's amin clamp
  mel_to_magnitude / wav_to_mel       with the yardstick of each element's dot product, sum_k |w_k| |x_k|
  griffin_lim_steps       per iteration the pre-normalisation value a = rebuilt - c * prev, the projected spectrum and its signal
  final_phase / final_signal          phase = angle(angles) and istft(mag * exp(i phase)), which differ from `angles` where mag < 0
  phase_error / signal_error / mel_error / magnitude_error   worst element and where it is
"""
import numpy as np

TINY32 = float(np.finfo(np.float32).tiny)
AMIN = 1e-5


def frame_count(n_samples, n_fft, hop):
    return (n_samples - n_fft) // hop + 1


def stft(y, window, hop):
    """y [n] -> complex128 [bins, T]: frame t is window * y[t*hop : t*hop + n_fft]."""
    y, window = np.asarray(y, np.float64), np.asarray(window, np.float64)
    n_fft = window.shape[0]
    T = frame_count(y.shape[0], n_fft, hop)
    frames = np.stack([y[t * hop: t * hop + n_fft] for t in range(T)])
    return np.fft.rfft(frames * window, axis=1).T


def window_sum_of_squares(window, hop, T):
    window = np.asarray(window, np.float64)
    n_fft = window.shape[0]
    wss = np.zeros(n_fft + (T - 1) * hop)
    for t in range(T):
        wss[t * hop: t * hop + n_fft] += window ** 2
    return wss


def istft(spec, window, hop, skip=None):
    """spec complex [bins, T] -> (y [n_fft + (T-1)*hop], wss): overlap-add of window * irfft(column), divided by the summed squared
    window where that exceeds float32's smallest normal number (elsewhere - sample 0 of a Hann window - the sum is left as it is).
    The imaginary parts of the DC and Nyquist bins do not enter (irfft drops them).  `skip`: (frame, first sample, one past the
    last) triples whose contribution is left out, for the seeded defects of the CPU tests."""
    spec, window = np.asarray(spec, np.complex128), np.asarray(window, np.float64)
    n_fft = window.shape[0]
    T = spec.shape[1]
    seg = np.fft.irfft(spec.T, n_fft, axis=1) * window
    for t, lo, hi in (skip or ()):
        seg[t, max(0, lo - t * hop): max(0, hi - t * hop)] = 0.0
    y = np.zeros(n_fft + (T - 1) * hop)
    for t in range(T):
        y[t * hop: t * hop + n_fft] += seg[t]
    wss = window_sum_of_squares(window, hop, T)
    nz = wss > TINY32
    y[nz] /= wss[nz]
    return y, wss


def _log_ref(log_func, ref):
    return (np.log if log_func == "np.log" else np.log10)(max(AMIN, float(ref)))


def db_to_amplitude(db, log_func="np.log10", ref=1.0):
    x = np.asarray(db, np.float64) + _log_ref(log_func, ref)
    return np.exp(x) if log_func == "np.log" else np.power(10.0, x)


def amplitude_to_db(amp, log_func="np.log10", ref=1.0):
    lf = np.log if log_func == "np.log" else np.log10
    return lf(np.maximum(AMIN, np.abs(np.asarray(amp, np.float64)))) - _log_ref(log_func, ref)


def mel_to_magnitude(mel_db, inv_basis, log_func, ref):
    """mel_db [M, T], inv_basis [bins, M] -> (mag [bins, T], yardstick [bins, T] = sum_m |inv_basis| * amp)."""
    amp = db_to_amplitude(mel_db, log_func, ref)
    w = np.asarray(inv_basis, np.float64)
    return w @ amp, np.abs(w) @ amp


def wav_to_mel(signal, window, hop, mel_basis, log_func, ref):
    """signal [n] -> (mel_db [M, T], mel amplitude before the clamp [M, T])."""
    amp = np.asarray(mel_basis, np.float64) @ np.abs(stft(signal, window, hop))
    return amplitude_to_db(amp, log_func, ref), amp


def griffin_lim_steps(mag, window, hop, n_iter, momentum=0.99):
    """mag [bins, T] -> list of n_iter + 1 records.  Record 0 is the start (angles = mag + 0i, a = 1); record k the state behind
    iteration k: `rebuilt` = stft(istft(angles of k-1)), `a` = rebuilt - c * rebuilt of k-1 (c = momentum / (1 + momentum); the first
    iteration has no previous one), `angles` = a / (|a| + tiny) * mag, `signal` = istft(angles)."""
    mag = np.asarray(mag, np.float64)
    c = float(momentum) / (1.0 + float(momentum))
    angles = mag.astype(np.complex128)
    steps = [{"a": np.ones_like(angles), "angles": angles, "signal": istft(angles, window, hop)[0], "rebuilt": None}]
    prev = None
    for _ in range(n_iter):
        rebuilt = stft(steps[-1]["signal"], window, hop)
        a = rebuilt if prev is None else rebuilt - c * prev
        angles = a / (np.abs(a) + TINY32) * mag
        prev = rebuilt
        steps.append({"a": a, "angles": angles, "signal": istft(angles, window, hop)[0], "rebuilt": rebuilt})
    return steps


def final_phase(angles):
    return np.angle(angles)


def final_signal(mag, phase, window, hop):
    """The synthesis output: istft(mag * exp(i phase)) and its window sum of squares."""
    return istft(np.asarray(mag, np.float64) * np.exp(1j * np.asarray(phase, np.float64)), window, hop)


# ---- metrics: the worst element and where it is ---------------------------------------------------------------------------------
def _worst(err):
    idx = np.unravel_index(int(np.argmax(err)), err.shape)
    return float(err[idx]), tuple(int(i) for i in idx)


def phase_error(phase_got, a_want, mag):
    """phase_got, mag [B, bins, T] (or [bins, T]); a_want the float64 pre-normalisation value.  Per bin
    |e^{i got} - sign(mag) a/|a|| * |a| / scale, scale = RMS of |a| over the bin's frame: the distance on the unit circle weighted by
    how well conditioned the bin's phase is (an fp32 error d in `a` turns the phase by d / |a|, so the product is the error in `a`
    relative to its frame).  The sign: the kernels return angle(a / |a| * mag), which is turned by pi where mag < 0; bins with mag = 0
    or a = 0 have no defined phase and weigh nothing.  Returns (worst value, (row, bin, frame))."""
    got, a, mag = (np.asarray(x) for x in (phase_got, a_want, mag))
    if got.ndim == 2:
        got, a, mag = got[None], a[None], mag[None]
    mod = np.abs(a)
    scale = np.sqrt((mod ** 2).mean(axis=1, keepdims=True))
    unit = np.where(mod > 0, a / np.where(mod > 0, mod, 1.0), 0.0) * np.sign(mag)
    err = np.abs(np.exp(1j * got.astype(np.float64)) - unit) * mod / np.where(scale > 0, scale, 1.0)
    return _worst(np.where((mod > 0) & (mag != 0), err, 0.0))


def signal_error(got, want, wss, hop):
    """got, want [B, n] (or [n]); per sample |got - want| * min(1, wss) / scale, scale = the row's largest |want| * min(1, wss).  The
    first and last samples of the un-centred inverse STFT are divided by a window sum down to 1e-10, which amplifies any rounding by its
    inverse (the product path trims 500 samples at both ends before use); the weight takes that amplification out and leaves every
    sample checked.  Returns (worst value, (row, sample, hop block))."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.ndim == 1:
        got, want = got[None], want[None]
    wgt = np.minimum(1.0, np.asarray(wss, np.float64))
    scale = np.maximum((np.abs(want) * wgt).max(axis=1, keepdims=True), 1e-30)
    v, (b, i) = _worst(np.abs(got - want) * wgt / scale)
    return v, (b, i, i // hop)


def mel_error(got_db, want_db, want_amp, yard, log_func):
    """Per element of a mel (dB): the difference of the logarithms turned back into a relative error of the amplitude, against the
    element's yardstick sum_k basis[m][k] |X[k]| (the mel basis is non-negative, so that is the amplitude itself) - except where
    the amplitude lies under the amin clamp, where the result must be the clamp's value: there the plain difference counts."""
    got, want = np.asarray(got_db, np.float64), np.asarray(want_db, np.float64)
    per_db = 1.0 if log_func == "np.log" else np.log(10.0)
    clamped = np.asarray(want_amp) < AMIN * (1 + 1e-4)
    near = np.asarray(want_amp) < AMIN * (1 + 1e-3)        # an amplitude within fp32 rounding of the clamp may land on either side
    rel = np.abs(np.expm1((got - want) * per_db)) * np.asarray(want_amp) / np.maximum(np.asarray(yard), AMIN)
    return _worst(np.where(clamped, np.abs(got - want) * per_db, np.where(near, np.minimum(rel, np.abs(got - want) * per_db), rel)))


def magnitude_error(got, want, yard):
    """Per element |got - want| / sum_m |inv_basis[k][m]| amp[m]: the pseudo-inverse basis has entries of both signs, so a result may
    be small against the terms it is the sum of."""
    return _worst(np.abs(np.asarray(got, np.float64) - want) / np.maximum(yard, 1e-300))


def weighted_phase_diff(phase_a, phase_b, mag):
    """The aggregate tests/test_audio_gpu.py compares phases with: one number per call."""
    w = np.abs(mag) / np.abs(mag).sum()
    return float((np.abs(np.exp(1j * np.asarray(phase_a, np.float64)) - np.exp(1j * np.asarray(phase_b, np.float64))) * w).sum())


# ---- tolerances of tests/test_vocoder_kernels_gpu.py (here so that the CPU module can show what they catch) ----------------------
# Beside each: the float32 floor (oracle/audio_ref.py against this file, tests/test_vocoder_metric_cpu.py; the oracle is float64 in
# places, so it is a lower bound), the worst error measured on an MI355X over every path and T of the GPU module, and the factor
# between that and the tolerance.  Errors of an iteration enter the next through the bins whose |a| is small (their phase turns by
# d / |a|, a heavy-tailed amplification), which is why two and three iterations share a tolerance.
TOL_PHASE = {
    "random": {0: 5e-7,      # floor 0 (phases are 0 or pi: 8.7e-8 from float32 pi); measured 8.7e-8; x 6
               1: 8e-6,      # floor 5.4e-7; measured 1.0e-6 (rocFFT), 9.3e-7 (fused); x 8
               2: 1e-3,      # floor 7.3e-6; measured 2.2e-4 (fused, first frame), 1.0e-4 (rocFFT); x 4.5
               3: 1e-3},     # floor 1.4e-5; measured 7.2e-5 (1024 / 256), 1.6e-4 (512 / 128); x 6
    "speech": {0: 5e-7,      # as above
               1: 4e-3},     # floor 3.5e-4 (the cancellation described at TOL_SIGNAL); measured 5.5e-4 (rocFFT), 4.8e-4 (fused); x 7
}
TOL_SIGNAL = {               # against the float64 signal of the float64 phases, relative to the row's largest weighted sample
    "random": {0: 5e-6,      # measured 9.8e-7; x 5
               1: 3e-5,      # floor 6.7e-7; measured 4.7e-6; x 6.4
               2: 3e-5,      # floor 6.6e-7; measured 1.9e-6 (the tolerance of one iteration: errors do not shrink)
               3: 1e-4},     # floor 6.7e-7; measured 6.1e-6 (1024 / 256), 1.3e-5 (512 / 128); x 7.4
    "speech": {0: 2e-3,      # measured 3.4e-4 (fused), 2.6e-4 (rocFFT): the signal of a smooth zero-phase spectrum is what is left of a
                             # pulse where the window vanishes, small against the float32 rounding of the pulse; x 6
               1: 2e-1},     # floor 3.1e-3; measured 2.8e-2 on every path; x 7.  Loose: the phases of the quiet bins carry this signal.
                             # What the inverse STFT itself does is held by TOL_SIGNAL_OWN_SPEECH
}
TOL_SIGNAL_OWN = 5e-6        # the returned waveform against the float64 inverse STFT of the returned phases: floor 1.7e-7; measured 9.8e-7; x 5
TOL_SIGNAL_OWN_SPEECH = 2e-3 # the same on the speech-like magnitudes: measured 3.4e-4 (fused), 2.6e-4 (rocFFT); x 6
TOL_ISTFT = 1.5e-6           # gvx_istft on random spectra: measured 2.2e-7; x 7
TOL_STFT = 2e-6              # gvx_stft, per element against the frame's largest bin: measured 2.6e-7; x 8
TOL_MEL = 2e-5               # gvx_wav_to_mel, relative error of the mel amplitude: measured 2.6e-6 (fused), 1.5e-6 (rocFFT); x 8
TOL_MAGNITUDE = 5e-6         # gvx_mel_to_magnitude against sum |w| |x|: measured 6.4e-7; x 8


# ---- inputs shared by the CPU and the GPU module ---------------------------------------------------------------------------------
def random_magnitudes(seed, B, bins, T):
    """|N(0,1)| * 3 with one quiet frame per row and one quiet band."""
    rng = np.random.default_rng(seed)
    mag = np.abs(rng.standard_normal((B, bins, T))) * 3.0
    mag[:, :, T // 2] *= 1e-3
    mag[:, bins // 3: bins // 3 + 9, :] *= 1e-3
    return mag.astype(np.float32)


def speech_like_magnitudes(seed, B, bins, T):
    """Low rank: a few smooth spectral envelopes with slowly varying gains, minus a small offset so that - like the output of the
    pseudo-inverse mel basis - some entries are negative and most bins are far from loud."""
    rng = np.random.default_rng(seed)
    k = np.arange(bins)[:, None]
    centres, widths = rng.uniform(0.02, 0.7, 4) * bins, rng.uniform(0.01, 0.08, 4) * bins
    env = np.exp(-0.5 * ((k - centres) / widths) ** 2)                                       # [bins, 4]
    gains = np.abs(rng.standard_normal((B, 4, T))).cumsum(axis=2) / np.sqrt(np.arange(1, T + 1))
    return (np.einsum("kr,brt->bkt", env, gains) * 2.0 - 0.02).astype(np.float32)
