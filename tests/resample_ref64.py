"""Float64 restatement of the resampler's definition (NumPy only), written from the definition and not from the kernel:

    a row x of n samples is zero outside [0, n); with h the prototype centred on index 0 (h[t] = 0 for |t| > half),
    y[m] = sum_j x[j] * h[m * down - j * up]       for 0 <= m < ceil(n * up / down).

``resample`` also returns sum_j |x[j] * h[m * down - j * up]| per output, the scale of a rounding bound.
"""
import numpy as np


def resampled_length(n: int, up: int, down: int) -> int:
    return (n * up + down - 1) // down


def resample(x: np.ndarray, h: np.ndarray, up: int, down: int):
    """(y, sum of magnitudes) in float64; ``h`` has odd length with its centre tap in the middle."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    half = h.shape[0] // 2
    assert h.shape[0] == 2 * half + 1
    n = x.shape[0]
    n_out = resampled_length(n, up, down)
    y, mag = np.zeros(n_out), np.zeros(n_out)
    for m in range(n_out):
        t = m * down
        lo = max(0, -((half - t) // up))          # smallest j with t - j * up <= half
        hi = min(n - 1, (t + half) // up)         # largest j with t - j * up >= -half
        if hi < lo:
            continue
        j = np.arange(lo, hi + 1)
        terms = x[j] * h[t - j * up + half]
        y[m], mag[m] = terms.sum(), np.abs(terms).sum()
    return y, mag


def resample_vec(x: np.ndarray, h: np.ndarray, up: int, down: int, wide: bool = False):
    """``resample`` without a Python loop per output: the same definition from the same centred prototype, the same (y, sum of
    magnitudes).  ``wide``: products and sums in the platform's long double (64 significant bits on x86-64), rounded to float64
    once - what a float64 kernel is held against, so that the restatement's own rounding takes nothing out of the kernel's bound.

    Outputs m = r, r + up, r + 2 up, ... share their prototype taps h[r * down - a * up - k * up] (k = 0 .. taps - 1, a the smallest j
    they can reach, less the multiple of down that m adds) and their first input moves on by ``down`` each, so one class is a strided
    gather of windows out of the zero-extended row times one tap vector, summed per output by NumPy's pairwise sum.  The terms
    outside the row and outside the prototype are exact zeros: the sums differ from the loop form's only in their order, by a few
    ulp of the magnitude sum (tests/test_resample_cpu.py pins both forms within 1e-15 * mag)."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    half = h.shape[0] // 2
    assert x.ndim == 1 and h.shape[0] == 2 * half + 1
    n = x.shape[0]
    n_out = resampled_length(n, up, down)
    y, mag = np.zeros(n_out), np.zeros(n_out)
    if n_out == 0:
        return y, mag
    taps = 2 * half // up + 1                                   # the most j with |t - j * up| <= half
    pad = half // up + 1                                        # the smallest j of any output is >= -(half // up)
    j_last = -((half - (n_out - 1) * down) // up)               # smallest j of the last output
    dt = np.longdouble if wide else np.float64
    xp = np.zeros(max(pad + n, pad + j_last + taps), dt)
    xp[pad: pad + n] = x
    windows = np.lib.stride_tricks.sliding_window_view(xp, taps)
    hp = np.concatenate([np.zeros(taps * up), h]).astype(dt)              # index i of h sits at taps * up + i: what falls below the prototype is 0
    for r in range(min(up, n_out)):
        t = r * down
        a = -((half - t) // up)                                 # smallest j with t - j * up <= half
        count = len(range(r, n_out, up))
        xs = windows[pad + a:: down][:count]                    # [count][taps]: inputs j = a + i * down + k of output r + i * up
        hr = hp[taps * up + (t - a * up + half) - np.arange(taps) * up]
        terms = xs * hr
        y[r::up], mag[r::up] = terms.sum(axis=1), np.abs(terms).sum(axis=1)
    return y, mag


def prototype(table: np.ndarray) -> np.ndarray:
    """A full ``[up][K]`` table (every tap in use) as the centred prototype it is the polyphase form of: (K / 2) * up taps on each
    side of the centre, ``h[t] = table[t mod up][K / 2 - 1 - floor(t / up)]`` for t in [-(K / 2) * up, (K / 2) * up - 1], and a zero
    at t = (K / 2) * up, the one tap of that length the table has no place for."""
    table = np.asarray(table, dtype=np.float64)
    up, K = table.shape
    half = (K // 2) * up
    t = np.arange(-half, half)
    return np.concatenate([table[t % up, K // 2 - 1 - t // up], [0.0]])


def mixdown(frames: np.ndarray) -> np.ndarray:
    """(n, channels) -> float32 mono: the mean of the channels, summed in float64 in channel order and rounded once."""
    s = np.zeros(frames.shape[0], dtype=np.float64)
    for c in range(frames.shape[1]):
        s = s + frames[:, c].astype(np.float64)
    return (s / frames.shape[1]).astype(np.float32)
