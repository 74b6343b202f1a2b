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


def mixdown(frames: np.ndarray) -> np.ndarray:
    """(n, channels) -> float32 mono: the mean of the channels, summed in float64 in channel order and rounded once."""
    s = np.zeros(frames.shape[0], dtype=np.float64)
    for c in range(frames.shape[1]):
        s = s + frames[:, c].astype(np.float64)
    return (s / frames.shape[1]).astype(np.float32)
