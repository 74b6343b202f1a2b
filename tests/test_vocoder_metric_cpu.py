"""The element-wise vocoder metrics of tests/audio_ref64.py, on the CPU: what float32 itself costs in them (the floor the GPU
tolerances of tests/test_vocoder_kernels_gpu.py start from), and that each catches the mistakes a Griffin-Lim kernel can make
while the aggregate the suite used so far (`weighted_phase_diff`, one number per call) mostly does not.

Noise floor.  oracle/audio_ref.py is the reference's float32 arithmetic (NumPy's FFT keeps float32).  Not all of it is float32:
the first momentum update promotes `angles` to complex128 (its `prev` starts as float64 zeros) and irfft of a complex128
spectrum is float64, so from the second iteration on only the overlap-add buffer and the forward STFT round to float32.  The floor
measured here is therefore a lower bound for an all-float32 kernel; the errors measured on the GPU decide the tolerances, and
both are quoted beside them in tests/audio_ref64.py.

Seeded defects.  Applied in NumPy to the float64 computation (no kernel is touched): each must exceed the GPU tolerance of its
quantity by 10x at least.  What the aggregate makes of them, measured at T = 56 with momentum 0.99:
  defect                                         new metric (tolerance)          aggregate (today's tolerance)
  (a) halo frame left out of one hop block       phase 2.1e-1 at 2 iterations    2.3e-3 at 2 (1e-3: noticed), 7.7e-3 at 4 (1e-2: missed)
  (b) bin 512 of every frame taken from bin 0    phase 5.0 at 1 iteration        9.1e-4 at 1 (1e-3: missed), 2.5e-3 at 4 (1e-2: missed)
  (c) prev of the wrong parity, one workgroup    phase 4.2e-1 at 3 iterations    1.6e-2 at 3 (1e-2: noticed; the 32-iteration 0.1: missed)
  (d) last hop block not divided by its tail sum signal 1.8e-1                   0 (phases only; the waveform check of the suite sees it)
  (e) one twiddle off by 1e-4                    phase 1.2e-4 at 1 iteration     1.0e-7 at 1, 2.5e-6 at 4 (missed everywhere)
Today's tolerances are those of tests/test_audio_gpu.py: 1e-3 for 1 and 2 iterations, `tol * 50` = 1e-2 for the 4 iterations of
the fused-vs-rocFFT test (the only one that runs more than one workgroup per row beyond 2 iterations), 0.1 for 32.  So the
aggregate misses (a) beyond two iterations, (b) and (e); it notices (c) at the tighter tolerances and cannot see (d).
"""
import numpy as np
import pytest

from oracle import audio_ref
from tests import audio_ref64 as r64

N_FFT, HOP = 1024, 256
WIN = audio_ref.hann_window(N_FFT).astype(np.float64)


# ---- the restatement against the oracle, and the float32 floor ---------------------------------------------------------------------
def test_restatement_agrees_with_the_oracle_on_one_frame_chain():
    rng = np.random.default_rng(0)
    sig = (rng.standard_normal(N_FFT + 9 * HOP + 5) * 0.3).astype(np.float32)
    spec = r64.stft(sig, WIN, HOP)
    want = audio_ref.stft(sig, N_FFT, HOP)
    assert spec.shape == want.shape and np.abs(spec - want).max() <= 2e-6 * np.abs(want).max()
    back, wss = r64.istft(spec, WIN, HOP)
    assert r64.signal_error(audio_ref.istft(want, N_FFT, HOP), back, wss, HOP)[0] <= 1e-6
    assert np.abs(back[N_FFT:-N_FFT] - sig[N_FFT: back.shape[0] - N_FFT]).max() <= 1e-12      # perfect reconstruction inside
    for log_func in ("np.log", "np.log10"):
        for ref in (1.0, 20.0):
            x = rng.uniform(-5, 2, (7, 5)).astype(np.float32)
            assert np.abs(r64.db_to_amplitude(x, log_func, ref) / audio_ref.db_to_amplitude(x, log_func, ref) - 1).max() <= 1e-5
            a = np.abs(rng.standard_normal((7, 5))).astype(np.float32)
            a[0, 0] = 0.0                                                                     # the amin clamp
            assert np.abs(r64.amplitude_to_db(a, log_func, ref) - audio_ref.amplitude_to_db(a, log_func, ref)).max() <= 1e-5


@pytest.mark.parametrize("kind,T", [("random", 4), ("random", 11), ("random", 24), ("random", 56), ("speech", 24)])
def test_float32_noise_floor(kind, T):
    """oracle (float32) against float64 after 1, 2 and 3 iterations, in the new metrics.  Measured (phase / signal):
    random T=56: 5.4e-7 / 2e-7, 7.3e-6 / 2e-7, 1.4e-5 / 3e-7; speech-like T=24: 3.5e-4, 3.3e-2, 1.9e-1 - a smooth spectrum at zero
    phase is a pulse where the Hann window vanishes, its rebuilt spectrum a small difference of large numbers, which is why the GPU
    module runs the speech-like case for 0 and 1 iterations only."""
    mk = r64.random_magnitudes if kind == "random" else r64.speech_like_magnitudes
    mag = mk(T, 1, N_FFT // 2 + 1, T)[0]
    steps = r64.griffin_lim_steps(mag, WIN, HOP, 3)
    for n_iter in (1, 2, 3):
        ph32 = audio_ref.griffin_lim(mag, N_FFT, HOP, momentum=0.99, n_iter=n_iter)
        perr, pwhere = r64.phase_error(ph32, steps[n_iter]["a"], mag)
        want, wss = r64.final_signal(mag, r64.final_phase(steps[n_iter]["angles"]), WIN, HOP)
        y32 = audio_ref.istft((mag * (np.cos(ph32) + 1j * np.sin(ph32))).astype(np.complex64), N_FFT, HOP)
        serr, swhere = r64.signal_error(y32, want, wss, HOP)
        own, _ = r64.final_signal(mag, ph32, WIN, HOP)
        oerr, _ = r64.signal_error(y32, own, wss, HOP)
        print(f"FLOOR {kind} T={T} n_iter={n_iter}: phase {perr:.2e} at {pwhere}, signal {serr:.2e} at {swhere}, signal of own phases {oerr:.2e}")
        if kind == "random" or n_iter == 1:      # float32 stays within the GPU tolerance: the tolerance is not below the floor
            assert perr <= r64.TOL_PHASE[kind][n_iter] and serr <= r64.TOL_SIGNAL[kind][n_iter], (perr, serr)
        assert oerr <= r64.TOL_SIGNAL_OWN


# ---- seeded defects --------------------------------------------------------------------------------------------------------------
def defective_griffin_lim(mag, n_iter, defect=None, momentum=0.99, workgroup=(13, 26)):
    """The float64 Griffin-Lim with one of the mistakes a kernel could make.  `workgroup`: the hop blocks (= owned frames) of the second
    workgroup of gl_iteration_kernel<1>.
      halo     the iteration's overlap-add leaves the oldest of the four frames out of the workgroup's first hop block
      nyquist  bin 512 of the rebuilt spectrum is a copy of bin 0
      parity   the third iteration reads the rebuilt spectrum of the first as `prev` for the workgroup's frames (wrong buffer of the ping-pong)
      tail     the last hop block of the final signal (the last frame alone) is windowed but not divided by the window sum
      twiddle  e^{-2 pi i k / 1024} of the real-FFT split is off by 1e-4 at k = 100"""
    mag = np.asarray(mag, np.float64)
    T = mag.shape[1]
    c = momentum / (1 + momentum)
    lo, hi = workgroup
    angles = mag.astype(np.complex128)
    y = r64.istft(angles, WIN, HOP)[0]
    rebuilt = []
    for it in range(n_iter):
        reb = r64.stft(y, WIN, HOP)
        if defect == "nyquist":
            reb[512] = reb[0]
        if defect == "twiddle":   # X[k] = (Z[k] + conj Z[512-k]) / 2 - i W^k (Z[k] - conj Z[512-k]) / 2, Z the FFT of even + i odd samples
            fr = np.stack([y[t * HOP: t * HOP + N_FFT] for t in range(T)]) * WIN
            Z = np.fft.fft(fr[:, 0::2] + 1j * fr[:, 1::2], axis=1)
            reb[100] += -0.5j * 1e-4 * (Z[:, 100] - np.conj(Z[:, 412]))
        rebuilt.append(reb)
        a = reb
        if it > 0:
            prev = rebuilt[it - 1].copy()
            if defect == "parity" and it == 2:
                prev[:, lo:hi] = rebuilt[0][:, lo:hi]
            a = reb - c * prev
        angles = a / (np.abs(a) + r64.TINY32) * mag
        if it < n_iter - 1:
            y = r64.istft(angles, WIN, HOP, skip=[(lo - 3, lo * HOP, (lo + 1) * HOP)] if defect == "halo" else None)[0]
    phase = np.angle(angles)
    wav, wss = r64.final_signal(mag, phase, WIN, HOP)
    if defect == "tail":
        wav[(T + 2) * HOP:] *= wss[(T + 2) * HOP:]
    return phase, wav


TODAY = {1: 1e-3, 2: 1e-3, 3: 1e-2, 4: 1e-2}   # tests/test_audio_gpu.py: 1e-3 (1, 2 iterations), tol * 50 = 1e-2 (4; taken for 3 as well)


def measure(T, n_iter, defect):
    mag = r64.random_magnitudes(T, 1, N_FFT // 2 + 1, T)[0]
    steps = r64.griffin_lim_steps(mag, WIN, HOP, n_iter)
    clean_phase = r64.final_phase(steps[n_iter]["angles"])
    want, wss = r64.final_signal(mag, clean_phase, WIN, HOP)
    phase, wav = defective_griffin_lim(mag, n_iter, defect)
    own, _ = r64.final_signal(mag, phase, WIN, HOP)
    return {"phase": r64.phase_error(phase, steps[n_iter]["a"], mag), "signal": r64.signal_error(wav, want, wss, HOP),
            "own": r64.signal_error(wav, own, wss, HOP), "aggregate": r64.weighted_phase_diff(phase, clean_phase, mag)}


def test_the_clean_computation_has_no_error_in_the_new_metrics():
    for n_iter in (1, 3):
        m = measure(24, n_iter, None)
        assert m["phase"][0] <= 1e-12 and m["signal"][0] <= 1e-12 and m["own"][0] <= 1e-12 and m["aggregate"] <= 1e-12


@pytest.mark.parametrize("defect,T,n_iter,quantity,where", [
    ("halo", 24, 2, "phase", lambda w: 10 <= w[2] <= 13),                  # T = 24: block 13 opens the second workgroup; frames 10 .. 13 read it
    ("halo", 56, 3, "phase", lambda w: True),
    ("nyquist", 56, 1, "phase", lambda w: w[1] == 512),
    ("parity", 56, 3, "phase", lambda w: 13 <= w[2] < 26),
    ("tail", 56, 1, "own", lambda w: w[2] == 58),
    ("tail", 24, 3, "signal", lambda w: w[2] == 26),
    ("twiddle", 56, 1, "phase", lambda w: w[1] == 100),
])
def test_seeded_defect_exceeds_the_gpu_tolerance_tenfold(defect, T, n_iter, quantity, where):
    m = measure(T, n_iter, defect)
    tol = {"phase": r64.TOL_PHASE["random"][n_iter], "signal": r64.TOL_SIGNAL["random"][n_iter], "own": r64.TOL_SIGNAL_OWN}[quantity]
    err, at = m[quantity]
    print(f"DEFECT {defect} T={T} n_iter={n_iter}: {quantity} {err:.2e} at {at} (tolerance {tol:.1e}), aggregate {m['aggregate']:.2e} (today {TODAY[n_iter]:.0e})")
    assert err >= 10 * tol, f"{defect}: {quantity} error {err:.2e} is not 10x the tolerance {tol:.1e}"
    assert where(at), f"{defect}: the worst element {at} is not where the defect was put"


@pytest.mark.parametrize("defect,n_iter", [("halo", 4), ("nyquist", 1), ("nyquist", 4), ("twiddle", 1)])
def test_the_aggregate_at_todays_tolerance_misses_the_defect(defect, n_iter):
    """weighted_phase_diff averages a local error over the call: a wrong hop block (a), a wrong bin per frame (b) and a wrong twiddle
    (e) stay under the tolerance the suite applied at that iteration count, while the element-wise phase error is far above its own."""
    m = measure(56, n_iter, defect)
    tol_new = r64.TOL_PHASE["random"][min(n_iter, 3)]
    print(f"MISSED {defect} n_iter={n_iter}: aggregate {m['aggregate']:.2e} <= {TODAY[n_iter]:.0e}; phase error {m['phase'][0]:.2e} vs {tol_new:.1e}")
    assert m["aggregate"] <= TODAY[n_iter]
    assert m["phase"][0] >= 10 * tol_new


def test_the_aggregate_notices_the_wrong_parity_only_at_the_tighter_tolerances():
    """(c) turns the phases of 13 frames of 56 by O(1): 1.6e-2 in the aggregate - above 1e-2, far below the 0.1 of the 32-iteration test."""
    m = measure(56, 3, "parity")
    assert 1e-2 < m["aggregate"] < 0.1
