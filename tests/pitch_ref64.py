"""The pitch tracker and the contour comparison of include/genvox_amd.h (gvx_pitch_yin, gvx_f0_compare) restated in numpy, written
from the definitions there.  Every function takes a dtype: float64 is the reference the kernels are held to, float32 the same code
at the kernels' precision, whose distance from float64 is the rounding scale of a quantity.

Besides the outputs, ``yin`` returns per frame the decision margin: the smallest relative distance of any comparison the scan
actually performed from a tie.  A frame whose margin is not above the table's relative error bound may decide differently in
float32 without being wrong."""
import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

EPS32 = 2.0 ** -24


def table_bound(window: int, lag_max: int) -> float:
    """|c32 - c| <= this * c, for fp32 arithmetic in any summation order, eps = 2^-24.
      d    every term is a rounded difference, squared - (1 + e)^2 - and then goes through at most W roundings of additions (a fused
           multiply-add rounds once; a separate product once more): a factor (1 + e)^(W + 2) at most on a non-negative term, so
           the sum of the W non-negative terms is off by (W + 2) eps relative, at first order.
      sum  at most lag_max such numbers, all non-negative, through at most lag_max - 1 additions: (W + lag_max + 1) eps.
      c    = d * tau / sum: tau is exact, the product and the quotient round once each, the relative errors of d and of the sum add:
           (W + 2) + (W + lag_max + 1) + 2 = (2 W + lag_max + 5) eps.
    The remaining 3 eps of 2 W + lag_max + 8 hold the second-order terms: n^2 eps^2 for n = 2 W + lag_max + 5 <= 5125 is below
    1.6 eps.  At W = 1024, lag_max = 368: 2424 * 2^-24 = 1.45e-4."""
    return (2 * window + lag_max + 8) * EPS32


def frames_of(n: int, hop: int) -> int:
    return 0 if n <= 0 else -(-n // hop)


def frame_window(x: np.ndarray, n: int, s: int, length: int, dtype) -> np.ndarray:
    """x[s .. s + length) of a row of n samples, zeros outside [0, n); nothing at or behind n is touched."""
    out = np.zeros(length, dtype=dtype)
    lo, hi = max(s, 0), min(s + length, n)
    if hi > lo:
        out[lo - s:hi - s] = x[lo:hi].astype(dtype)
    return out


def cmnd(xw: np.ndarray, window: int, lag_max: int, dtype):
    """(d, c) of one frame from its W + lag_max samples."""
    A = sliding_window_view(xw, window)[:lag_max + 1]          # A[tau][j] = x[s + j + tau]
    e = (A[0][None, :] - A).astype(dtype)
    d = (e * e).sum(axis=1, dtype=dtype)
    run = np.cumsum(d[1:], dtype=dtype)
    c = np.ones(lag_max + 1, dtype=dtype)
    tau = np.arange(1, lag_max + 1).astype(dtype)
    pos = run > 0
    c[1:][pos] = (d[1:][pos] * tau[pos] / run[pos]).astype(dtype)
    return d, c


def decide(c: np.ndarray, lag_min: int, lag_max: int, threshold: float):
    """(lag or -1, margin): the scan of the definition, and the smallest relative distance from a tie among its comparisons."""
    margin = math.inf

    def rel(a, b, scale):
        return math.inf if scale == 0 else abs(float(a) - float(b)) / float(scale)

    lag = -1
    for tau in range(lag_min, lag_max):
        margin = min(margin, rel(c[tau], threshold, c[tau]))
        if c[tau] < threshold:
            lag = tau
            break
    if lag < 0:
        return -1, margin
    while lag + 1 <= lag_max - 1:
        margin = min(margin, rel(c[lag + 1], c[lag], c[lag + 1] + c[lag]))
        if not c[lag + 1] < c[lag]:
            break
        lag += 1
    return lag, margin


def refine(c: np.ndarray, lag: int, sampling_rate: int, dtype):
    """(f0, shift, den) of a voiced frame."""
    cm, c0, cp = dtype(c[lag - 1]), dtype(c[lag]), dtype(c[lag + 1])
    den = dtype(dtype(cm - dtype(2) * c0) + cp)
    shift = dtype(0)
    if den > 0:
        shift = dtype(min(1.0, max(-1.0, dtype(cm - cp) / dtype(dtype(2) * den))))
    return dtype(dtype(sampling_rate) / dtype(dtype(lag) + shift)), shift, den


def yin(wav: np.ndarray, lengths, *, sampling_rate: int, hop: int, window: int, lag_min: int, lag_max: int, threshold: float,
        first_centre: int = 0, dtype=np.float64):
    """wav [B, N] (anything at and behind lengths[b], NaN included), lengths [B] or None.  Returns a dict of arrays over [B, F]:
    f0, lag, aperiodicity, cmnd [B, F, lag_max + 1], d (same shape), margin, den (NaN for an unvoiced frame), shift, and frames [B].
    Behind a row's frames: f0 0, lag -1, aperiodicity 1, cmnd NaN."""
    wav = np.asarray(wav)
    B, N = wav.shape
    F = frames_of(N, hop)
    lengths = [N] * B if lengths is None else [min(max(int(n), 0), N) for n in lengths]
    out = {"f0": np.zeros((B, F), dtype), "lag": np.full((B, F), -1, np.int32), "aperiodicity": np.ones((B, F), dtype),
           "cmnd": np.full((B, F, lag_max + 1), np.nan, dtype), "d": np.full((B, F, lag_max + 1), np.nan, dtype),
           "margin": np.full((B, F), np.inf), "den": np.full((B, F), np.nan), "shift": np.zeros((B, F), dtype),
           "frames": np.array([frames_of(n, hop) for n in lengths], np.int32)}
    thr = dtype(threshold)
    for b in range(B):
        n = lengths[b]
        for f in range(frames_of(n, hop)):
            s = first_centre + f * hop - (window + lag_max) // 2
            d, c = cmnd(frame_window(wav[b], n, s, window + lag_max, dtype), window, lag_max, dtype)
            out["d"][b, f], out["cmnd"][b, f] = d, c
            lag, out["margin"][b, f] = decide(c, lag_min, lag_max, thr)
            out["lag"][b, f] = lag
            if lag < 0:
                out["aperiodicity"][b, f] = c[lag_min:lag_max].min()
            else:
                out["f0"][b, f], out["shift"][b, f], out["den"][b, f] = refine(c, lag, sampling_rate, dtype)
                out["aperiodicity"][b, f] = c[lag]
    return out


def f0_tolerance(c: np.ndarray, lag: int, sampling_rate: int, rel: float):
    """(tolerance of f0 in Hz or None, den): the table's bound carried through the parabola's quotient, on the float64 table c.
    Each of c(lag-1), c(lag), c(lag+1) is off by at most A = (rel + 4 eps) max of the three (the 4 eps: the parabola's own fp32
    subtractions, product and quotient, each at most one rounding of a number no larger than that maximum's small multiple).  The
    numerator n = c(lag-1) - c(lag+1) is then off by at most 2 A and den by at most 4 A; for den >= 16 A
        |shift' - shift| <= (2 A + 2 |shift| 4 A) / (2 (den - 4 A))
    (the clamp to [-1, 1] does not stretch), and f0 = rate / (lag + shift) moves by at most rate * ds / (lag + shift - ds)^2 plus
    two roundings of its own.  den < 16 A: None - the quotient is not determined to a useful width, the frame is held on lag only."""
    cm, c0, cp = float(c[lag - 1]), float(c[lag]), float(c[lag + 1])
    A = (rel + 4 * EPS32) * max(cm, c0, cp)
    den = cm - 2 * c0 + cp
    if den < 16 * A:
        return None, den
    shift = min(1.0, max(-1.0, (cm - cp) / (2 * den)))
    ds = (2 * A + 8 * abs(shift) * A) / (2 * (den - 4 * A))
    f0 = sampling_rate / (lag + shift)
    return sampling_rate * ds / (lag + shift - ds) ** 2 + 4 * EPS32 * f0, den


def f0_compare(fa: np.ndarray, fb: np.ndarray, frames_a=None, frames_b=None, dtype=np.float64):
    """Contours [B, F].  Returns counts int32 [B, 4] (frames, voiced in both, voiced in exactly one, gross) and vde, gpe, rmse_cents
    [B] in dtype; NaN where a denominator is 0.  The voicing and gross decisions are taken in float64 whatever the dtype (they are
    exact in the definition); dtype governs the cents, their squares, the mean and the root."""
    fa, fb = np.asarray(fa), np.asarray(fb)
    B, F = fa.shape
    counts = np.zeros((B, 4), np.int32)
    vde, gpe, rmse = (np.full(B, np.nan, dtype) for _ in range(3))
    for b in range(B):
        na = F if frames_a is None else min(max(int(frames_a[b]), 0), F)
        nb = F if frames_b is None else min(max(int(frames_b[b]), 0), F)
        n = min(na, nb)
        a, c = fa[b, :n], fb[b, :n]
        va, vc = a > 0, c > 0
        both = va & vc
        with np.errstate(all="ignore"):
            r = a[both].astype(np.float64) / c[both].astype(np.float64)
        gross = np.abs(r - 1.0) > 0.2
        counts[b] = (n, both.sum(), (va != vc).sum(), gross.sum())
        if n:
            vde[b] = dtype(counts[b, 2]) / dtype(n)
        if counts[b, 1]:
            gpe[b] = dtype(counts[b, 3]) / dtype(counts[b, 1])
        keep = ~gross
        if keep.sum():
            ratio = (a[both][keep].astype(dtype) / c[both][keep].astype(dtype)).astype(dtype)
            cents = (dtype(1200) * np.log2(ratio)).astype(dtype)
            rmse[b] = np.sqrt((cents * cents).sum(dtype=dtype) / dtype(keep.sum()))
    return counts, vde, gpe, rmse
